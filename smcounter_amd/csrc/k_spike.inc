// Included by smcounter_hip.hip (after k_bp_emit2.inc: it uses bp2_resolve, the walk's own CIGAR rules; after k_philox_marks.inc:
// smc_philox4x32_10).
// ------------------------------------------------------------------------------------------
// --spikeAF, --spikeReps: listed SNVs planted in copies of a run's bases, whole barcodes at a time (smc_spike_alleles: one copy, every
// variant at its own threshold; smc_spike_alleles_reps: B copies from one call, each with a seed and one threshold of its own)
// ------------------------------------------------------------------------------------------
// A run's alignments and (letter, quality) pairs are in HBM before the plane builder runs.  The host hands over room for COPIES of the
// alignment records' array and of the pair pool; the kernels write into those, the run itself is only read.  Replicate j of --spikeAF
// is the same spike-in with seed s_j: the run, the variants and the rewrite rule stay, only the draws move.
//   k_spike_pool      the pair pool read ONCE, stored B times: a lane per 16-byte chunk (uint4 load, B uint4 stores - every wave's access
//                     is 1 KiB of consecutive bytes), the bytes behind the last whole chunk by one lane, one at a time, so that nothing
//                     beyond a copy's 2 * n_pairs bytes is written.  A launch of its own: the rewrite behind it, on the same stream, finds
//                     every copy complete.  (smc_spike_alleles copies its one pool with hipMemcpyAsync: no alignment asked of it.)
//                     smc_spike_indels_reps (k_spike_indel.inc) sends the pair pool AND the CIGAR pool through it, one launch each.
//   k_spike_rewrite   blockIdx.y = copy c, a lane per alignment; the copies' seeds and thresholds come by value (at most
//                     SMC_SPIKE_MAX_COPIES of each).  Per listed variant v whose 0-based position lies in the alignment's [pos, end) (the
//                     variants are sorted by position: a binary search for the first, then along the array):
//   draw     u_v(b) = word 0 of Philox4x32-10(counter = (identity lo, identity hi, "spAF", (pos0 + 1) mod 2^32), key = seed_c lo, hi)
//            of the alignment's barcode b; b is spiked at v when u_v(b) < thr (in [0, 2^32]): the variant's own V.thr with `own_thr`
//            (uniform), else the copy's, and V.thr is not read.  --spikePhase: a member of a phase set (V.lead != 0) draws with the
//            position of its set's leader, var[k - V.lead] - one load more, for such records only (the host checked lead <= k); every
//            member of a set then makes the same draw: all of them are hit or none
//   column   bp2_resolve at pos0, only behind a draw that hits; the record is rewritten when its allele key there is a single letter: a
//            base (not inside a deletion) with no insertion or deletion starting behind it
//   store    ALT into the letter byte of that base (the quality byte next to it stays); NM + 1 when the old letter was REF
// and at the end, for EVERY alignment of every copy, the SMC_DA_MMOK bit as the decoder computes it (smc_bam_alignments) from the new
// NM.  stats[c][v][0] counts the records rewritten at v (one that showed ALT already is rewritten with the same letter and counted),
// stats[c][v][1] those that took an NM increment.  Positions are reference positions: a listed position need not be a locus of the run.
// A handful of launches per file and stage: not on the per-locus hot path, not tuned.
#define SPK_BLOCK 256
#define SPR_BLOCK 256
#define SPK_DOMAIN 0x73704146u               // counter word 2 of the draw ("spAF")

struct SpkCopies {
    unsigned long long seed[SMC_SPIKE_MAX_COPIES];
    unsigned long long thr[SMC_SPIKE_MAX_COPIES];     // floor(t * 2^32), in [0, 2^32]
};
struct SpkThr {
    unsigned long long t[SMC_SPIKE_REP_MAX_TARGETS];
};

// src: 16-byte aligned, n_bytes = 2 * n_pairs; copy c at dst + c * stride (dst and stride 16-byte aligned)
__global__ __launch_bounds__(SPR_BLOCK) void k_spike_pool(const uint8_t* __restrict__ src, unsigned long long n_bytes, uint8_t* __restrict__ dst,
                                                          unsigned long long stride, int n_copies) {
    const unsigned long long n_chunks = n_bytes >> 4;
    const unsigned long long step = (unsigned long long)gridDim.x * SPR_BLOCK;
    for (unsigned long long k = (unsigned long long)blockIdx.x * SPR_BLOCK + threadIdx.x; k < n_chunks; k += step) {
        const uint4 v = reinterpret_cast<const uint4*>(src)[k];
        for (int c = 0; c < n_copies; ++c) reinterpret_cast<uint4*>(dst + (unsigned long long)c * stride)[k] = v;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0)
        for (unsigned long long b = n_chunks << 4; b < n_bytes; ++b) {
            const uint8_t x = src[b];
            for (int c = 0; c < n_copies; ++c) dst[(unsigned long long)c * stride + b] = x;
        }
}

// copy c: records at aln_out + c * aln_stride (4-byte aligned), pool at bq_out + c * bq_stride, statistics at stats + 2 * c * n_var
__global__ __launch_bounds__(SPK_BLOCK) void k_spike_rewrite(const smc_dev_aln* __restrict__ aln, uint32_t n_aln, const uint32_t* __restrict__ cig,
                                                             unsigned long long n_pairs, const smc_spike_variant* __restrict__ var, int n_var,
                                                             const unsigned long long* __restrict__ ident, uint32_t n_bc, SpkCopies C, int own_thr,
                                                             double mismatch_thr, const int32_t* __restrict__ nm, const int32_t* __restrict__ n_indel,
                                                             uint8_t* __restrict__ aln_out, unsigned long long aln_stride,
                                                             uint8_t* __restrict__ bq_out, unsigned long long bq_stride, uint32_t* __restrict__ stats) {
    const uint32_t i = blockIdx.x * SPK_BLOCK + threadIdx.x;
    if (i >= n_aln) return;
    const uint32_t c = blockIdx.y;
    const unsigned long long seed = C.seed[c];
    uint8_t* const bq_c = bq_out + (unsigned long long)c * bq_stride;
    uint32_t* const stats_c = stats + 2ull * c * (unsigned long long)n_var;
    smc_dev_aln a = aln[i];
    int lo = 0, hi = n_var;                                      // first variant with pos0 >= a.pos
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (var[mid].pos0 < a.pos) lo = mid + 1; else hi = mid; }
    long long new_nm = (long long)nm[i];
    if (a.bc_gid < n_bc) {
        const unsigned long long id = ident[a.bc_gid];
        for (int k = lo; k < n_var; ++k) {
            const smc_spike_variant V = var[k];
            if (V.pos0 >= a.end) break;
            uint32_t x[4];
            smc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), SPK_DOMAIN, (uint32_t)(V.lead ? var[k - (int)V.lead].pos0 : V.pos0) + 1u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
            if (!((unsigned long long)x[0] < (own_thr ? V.thr : C.thr[c]))) continue;
            const BpRes r = bp2_resolve(cig + a.cig_off, (int)a.n_cig, a.pos, V.pos0, (int)a.l_seq);
            if (r.isdel || r.indel != 0 || r.qpos < 0 || r.qpos >= (int)a.l_seq) continue;
            const unsigned long long at = (unsigned long long)a.seq_off + (unsigned long long)r.qpos;
            if (at >= n_pairs) continue;                         // (a record that points beyond the pool: nothing is written)
            uint8_t* const s = bq_c + 2ull * at;
            const uint8_t old = s[0];
            s[0] = V.alt;
            atomicAdd(&stats_c[2 * k], 1u);
            if (old == V.ref) { ++new_nm; atomicAdd(&stats_c[2 * k + 1], 1u); }
        }
    }
    const long long mm = max(0ll, new_nm - (long long)n_indel[i]);
    const double mm100 = a.l_seq > 0 ? 100.0 * (double)mm / (double)a.l_seq : 0.0;     // smCounter.py:352-356
    a.oflag = (uint8_t)((a.oflag & ~SMC_DA_MMOK) | (mm100 <= mismatch_thr ? SMC_DA_MMOK : 0u));
    reinterpret_cast<smc_dev_aln*>(aln_out + (unsigned long long)c * aln_stride)[i] = a;
}
