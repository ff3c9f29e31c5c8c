// Included by smcounter_hip.hip (after k_bp_emit2.inc: it uses bp2_resolve, the walk's own CIGAR rules).
// ------------------------------------------------------------------------------------------
// --dsAF: which barcodes of a run cover / carry a listed allele (smc_allele_carriers)
// ------------------------------------------------------------------------------------------
// A run's alignments, CIGAR words and (letter, quality) pairs are in HBM before the plane builder runs.  For every listed variant
// (a locus of the run and an allele key: a letter, an insertion start, a deletion start - smCounter.py:371-460) two counters per
// run-wide barcode id are summed over the pileup of the variant's locus:
//   reads  the barcode's alignments with pos <= p < end - the loc[].n reads the plane builder puts there, deleted positions
//          included, no quality or mapping filter;
//   alt    those whose allele key at p is the variant's, by the rule the walk's exact path assigns keys (bp2_resolve; the key's
//          letters are the read's own, the deleted letters the reference's - the host lists a deletion only by its length and
//          lists one whose letters are not the reference's as SMC_AF_NONE).
// Then a bit per barcode: covers (reads > 0), carries (2 x alt > reads).  Two launches:
//   k_af_count   a lane per alignment of the locus's window [w0, w1), a row of blocks per variant: the CIGAR walked to p, the two
//                counters by returnless atomics (most lanes of a wavefront hit different barcodes: the file is position-sorted);
//   k_af_bits    a lane per barcode, a row of blocks per variant: a ballot per predicate, 64 barcodes' bits one 8-byte store.
// A few windows per file, before the first batch: not on the per-locus hot path, not tuned.
#define AF_BLOCK 256

__device__ __forceinline__ bool af_shows(const smc_af_variant& V, const smc_dev_aln& a, const uint32_t* __restrict__ cig,
                                         const uint8_t* __restrict__ bq, const uint8_t* __restrict__ ins, int p) {
    const BpRes r = bp2_resolve(cig + a.cig_off, (int)a.n_cig, a.pos, p, (int)a.l_seq);
    if ((r.isdel && r.indel == 0) || r.qpos < 0 || r.qpos >= (int)a.l_seq) return false;     // 'DEL' (inside a deletion): no listed shape
    const uint8_t* s = bq + 2ull * a.seq_off;                                                // (the letter of base k: byte 2k)
    if ((uint32_t)s[2 * r.qpos] != V.letter) return false;
    if (V.kind == SMC_AF_SNV) return r.indel == 0;
    if (V.kind == SMC_AF_DEL) return r.indel < 0 && (uint32_t)(-r.indel) == V.len;
    if (V.kind != SMC_AF_INS || r.indel <= 0) return false;
    // the inserted letters as the host's slice clamps them: query [qpos + 1, min(l_seq, qpos + 1 + indel))
    const int n = min((int)a.l_seq - (r.qpos + 1), r.indel);
    if ((uint32_t)n != V.len) return false;
    for (int k = 0; k < n; ++k)
        if (s[2 * (r.qpos + 1 + k)] != ins[V.ins_off + (uint32_t)k]) return false;
    return true;
}

__global__ __launch_bounds__(AF_BLOCK) void k_af_count(const smc_dev_aln* __restrict__ aln, uint32_t n_aln, const uint32_t* __restrict__ cig,
                                                       const uint8_t* __restrict__ bq, const smc_dev_locus* __restrict__ loc, int32_t start0,
                                                       const smc_af_variant* __restrict__ var, const uint8_t* __restrict__ ins,
                                                       uint32_t n_bc, uint32_t* __restrict__ counts) {
    const smc_af_variant V = var[blockIdx.y];
    const smc_dev_locus L = loc[V.locus];
    const uint32_t w1 = min(L.w1, n_aln);
    const int p = start0 + (int)V.locus;
    uint32_t* const c = counts + 2ull * n_bc * blockIdx.y;
    for (uint32_t i = L.w0 + blockIdx.x * AF_BLOCK + threadIdx.x; i < w1; i += gridDim.x * AF_BLOCK) {
        const smc_dev_aln a = aln[i];
        if (a.pos > p || p >= a.end || a.bc_gid >= n_bc) continue;
        atomicAdd(&c[2ull * a.bc_gid], 1u);
        if (af_shows(V, a, cig, bq, ins, p)) atomicAdd(&c[2ull * a.bc_gid + 1], 1u);
    }
}

// (n_words64: 64-bit words per mask; every wavefront of the grid writes one, the lanes beyond n_bc vote 0)
__global__ __launch_bounds__(AF_BLOCK) void k_af_bits(const uint32_t* __restrict__ counts, uint32_t n_bc, uint32_t n_words64,
                                                      unsigned long long* __restrict__ covers, unsigned long long* __restrict__ carries) {
    const uint32_t g = blockIdx.x * AF_BLOCK + threadIdx.x;
    uint32_t reads = 0, alt = 0;
    if (g < n_bc) {
        const uint2 c = *(const uint2*)(counts + 2ull * n_bc * blockIdx.y + 2ull * g);
        reads = c.x; alt = c.y;
    }
    const unsigned long long m_cov = __ballot(reads > 0u), m_car = __ballot(2ull * alt > (unsigned long long)reads);
    const uint32_t w = g / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0 && w < n_words64) {
        covers[(size_t)n_words64 * blockIdx.y + w] = m_cov;
        carries[(size_t)n_words64 * blockIdx.y + w] = m_car;
    }
}
