// Included by smcounter_hip.hip (after k_bp_emit2.inc: it uses bp2_resolve, the walk's own CIGAR rules; after k_philox_marks.inc:
// smc_philox4x32_10).
// ------------------------------------------------------------------------------------------
// --spikeAF: listed SNVs planted in a run's bases, whole barcodes at a time (smc_spike_alleles)
// ------------------------------------------------------------------------------------------
// A run's alignments and (letter, quality) pairs are in HBM before the plane builder runs.  The host hands over COPIES of the
// alignment records' array and of the pair pool; this kernel writes into those, the run itself is only read.  Per alignment (one
// lane each) and per listed variant v whose 0-based position lies in the alignment's [pos, end) (the variants are sorted by
// position: a binary search for the first, then along the array):
//   draw     u_v(b) = word 0 of Philox4x32-10(counter = (identity lo, identity hi, "spAF", (pos0 + 1) mod 2^32), key = seed lo, hi)
//            of the alignment's barcode b; b is spiked at v when u_v(b) < thr_v (thr in [0, 2^32]).  --spikePhase: a member of a phase
//            set (V.lead != 0) draws with the position of its set's leader, var[k - V.lead] - one load more, for such records only
//            (the host checked lead <= k); every member of a set then makes the same draw: all of them are hit or none
//   column   bp2_resolve at pos0; the record is rewritten when its allele key there is a single letter: a base (not inside a
//            deletion) with no insertion or deletion starting behind it
//   store    ALT into the letter byte of that base (the quality byte next to it stays); NM + 1 when the old letter was REF
// and at the end, for EVERY alignment, the SMC_DA_MMOK bit as the decoder computes it (smc_bam_alignments) from the new NM.
// stats[v][0] counts the records rewritten at v (one that showed ALT already is rewritten with the same letter and counted),
// stats[v][1] those that took an NM increment.  Positions are reference positions: a listed position need not be a locus of the run.
// A handful of launches per file: not on the per-locus hot path, not tuned.
#define SPK_BLOCK 256
#define SPK_DOMAIN 0x73704146u               // counter word 2 of the draw ("spAF")

__global__ __launch_bounds__(SPK_BLOCK) void k_spike(const smc_dev_aln* __restrict__ aln, uint32_t n_aln, const uint32_t* __restrict__ cig,
                                                     unsigned long long n_pairs, const smc_spike_variant* __restrict__ var, int n_var,
                                                     const unsigned long long* __restrict__ ident, uint32_t n_bc, unsigned long long seed,
                                                     double mismatch_thr, const int32_t* __restrict__ nm, const int32_t* __restrict__ n_indel,
                                                     smc_dev_aln* __restrict__ aln_out, uint8_t* __restrict__ bq_out, uint32_t* __restrict__ stats) {
    const uint32_t i = blockIdx.x * SPK_BLOCK + threadIdx.x;
    if (i >= n_aln) return;
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
            if (!((unsigned long long)x[0] < V.thr)) continue;
            const BpRes r = bp2_resolve(cig + a.cig_off, (int)a.n_cig, a.pos, V.pos0, (int)a.l_seq);
            if (r.isdel || r.indel != 0 || r.qpos < 0 || r.qpos >= (int)a.l_seq) continue;
            const unsigned long long at = (unsigned long long)a.seq_off + (unsigned long long)r.qpos;
            if (at >= n_pairs) continue;                         // (a record that points beyond the pool: nothing is written)
            uint8_t* const s = bq_out + 2ull * at;
            const uint8_t old = s[0];
            s[0] = V.alt;
            atomicAdd(&stats[2 * k], 1u);
            if (old == V.ref) { ++new_nm; atomicAdd(&stats[2 * k + 1], 1u); }
        }
    }
    const long long mm = max(0ll, new_nm - (long long)n_indel[i]);
    const double mm100 = a.l_seq > 0 ? 100.0 * (double)mm / (double)a.l_seq : 0.0;     // smCounter.py:352-356
    a.oflag = (uint8_t)((a.oflag & ~SMC_DA_MMOK) | (mm100 <= mismatch_thr ? SMC_DA_MMOK : 0u));
    aln_out[i] = a;
}
