// Included by smcounter_hip.hip (after k_spike.inc: the same draw, the same rewrite rule).
// ------------------------------------------------------------------------------------------
// --spikeReps: B spiked copies of a run from one call (smc_spike_alleles_reps), and (S, READS, V1) of every listed variant,
// replicate and target without any spiked copy (smc_spike_rep_counts)
// ------------------------------------------------------------------------------------------
// Replicate j of --spikeAF is the same spike-in with seed s_j: the run, the variants and the rewrite rule stay, only the draws move.
//   k_spike_pool   the pair pool read ONCE, stored B times: a lane per 16-byte chunk (uint4 load, B uint4 stores - every wave's access
//                  is 1 KiB of consecutive bytes), the bytes behind the last whole chunk by one lane, one at a time, so that nothing
//                  beyond a copy's 2 * n_pairs bytes is written.  A launch of its own: the rewrite behind it, on the same stream, finds
//                  every copy complete.
//   k_spike_reps   k_spike with blockIdx.y = copy: a lane per alignment, the copy's seed and threshold from the argument block (at most
//                  SMC_SPIKE_MAX_COPIES of each travel by value), one draw per (lane, variant in span, copy), bp2_resolve only behind a
//                  draw that hits, SMC_DA_MMOK recomputed for every alignment of every copy.  A member of a phase set draws with its
//                  leader's position, as in k_spike.
//   k_spike_counts a lane per covering barcode of a listed variant (blockIdx.y = variant, blockIdx.z strides over the replicates): ONE
//                  Philox per (barcode, variant, replicate), compared against all T thresholds; per target the three sums over the
//                  wavefront (ballot + popcount for S and V1, a DPP sum for READS), the workgroup's four wavefronts added in LDS, then
//                  one atomic add per workgroup, replicate, target and counter that is not 0.
// V1 NEEDS NO SPIKED COPY: what the rewrite does to a barcode at a listed position is fixed by three numbers the run itself gives -
// `reads` (its pileup reads there), `alt0` (those that show ALT as they are) and `single` (those whose allele key there is a single
// letter: exactly the reads a hit rewrites to ALT, every other read of the barcode keeps a key that is not ALT).  So a barcode that is
// hit shows ALT in `single` of its reads, one that is not in `alt0`, and it carries the variant when twice that exceeds `reads`.
// `single` depends on the CIGAR alone - not on any letter - so a neighbouring listed variant that is written into the same reads does
// not change it.
// A handful of launches per file and stage: not on the per-locus hot path.
#define SPR_BLOCK 256

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

__global__ __launch_bounds__(SPK_BLOCK) void k_spike_reps(const smc_dev_aln* __restrict__ aln, uint32_t n_aln, const uint32_t* __restrict__ cig,
                                                          unsigned long long n_pairs, const smc_spike_variant* __restrict__ var, int n_var,
                                                          const unsigned long long* __restrict__ ident, uint32_t n_bc, SpkCopies C,
                                                          double mismatch_thr, const int32_t* __restrict__ nm, const int32_t* __restrict__ n_indel,
                                                          uint8_t* __restrict__ aln_out, unsigned long long aln_stride,
                                                          uint8_t* __restrict__ bq_out, unsigned long long bq_stride, uint32_t* __restrict__ stats) {
    const uint32_t i = blockIdx.x * SPK_BLOCK + threadIdx.x;
    if (i >= n_aln) return;
    const uint32_t c = blockIdx.y;
    const unsigned long long seed = C.seed[c], thr = C.thr[c];
    uint8_t* const bq_c = bq_out + (unsigned long long)c * bq_stride;
    uint32_t* const stats_c = stats + 2ull * c * (unsigned long long)n_var;
    smc_dev_aln a = aln[i];
    int lo = 0, hi = n_var;                                      // first variant with pos0 >= a.pos
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (var[mid].pos0 < a.pos) lo = mid + 1; else hi = mid; }
    long long new_nm = (long long)nm[i];
    if (a.bc_gid < n_bc) {
        const unsigned long long id = ident[a.bc_gid];
        for (int k = lo; k < n_var; ++k) {
            const smc_spike_variant V = var[k];                  // (V.thr is not read: the copy's threshold holds for every variant)
            if (V.pos0 >= a.end) break;
            uint32_t x[4];
            smc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), SPK_DOMAIN, (uint32_t)(V.lead ? var[k - (int)V.lead].pos0 : V.pos0) + 1u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
            if (!((unsigned long long)x[0] < thr)) continue;
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

// out[((v * n_reps + j) * n_tgt + t) * 3 + {0, 1, 2}] += (S, READS, V1) of variant v (zeroed before the launch).  cov_ident / cov_cnt:
// the covering barcodes of all variants one behind the other, variant v's at [cov_off[v], cov_off[v + 1]); cov_cnt[e][3] = (reads,
// alt0, single) of barcode e at its variant's position.
__global__ __launch_bounds__(SPR_BLOCK) void k_spike_counts(const unsigned long long* __restrict__ cov_ident, const uint32_t* __restrict__ cov_cnt,
                                                            const uint32_t* __restrict__ cov_off, const uint32_t* __restrict__ pos1, SpkThr T,
                                                            int n_tgt, const unsigned long long* __restrict__ seeds, int n_reps,
                                                            uint32_t* __restrict__ out) {
    __shared__ uint32_t part[SPR_BLOCK / WAVE][SMC_SPIKE_REP_MAX_TARGETS][3];
    const uint32_t v = blockIdx.y;
    const uint32_t e0 = cov_off[v], e1 = cov_off[v + 1], pos = pos1[v];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const uint32_t stride = gridDim.x * SPR_BLOCK;
    for (uint32_t base = e0 + blockIdx.x * SPR_BLOCK; base < e1; base += stride) {     // (whole workgroups: the barriers below)
        const uint32_t e = base + threadIdx.x;
        const bool live = e < e1;
        unsigned long long id = 0;
        uint32_t reads = 0, alt0 = 0, single = 0;
        if (live) { id = cov_ident[e]; reads = cov_cnt[3ull * e]; alt0 = cov_cnt[3ull * e + 1]; single = cov_cnt[3ull * e + 2]; }
        for (int j = blockIdx.z; j < n_reps; j += gridDim.z) {
            const unsigned long long seed = seeds[j];
            uint32_t x[4];
            smc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), SPK_DOMAIN, pos, (uint32_t)seed, (uint32_t)(seed >> 32), x);
            for (int t = 0; t < n_tgt; ++t) {
                const bool hit = live && (unsigned long long)x[0] < T.t[t];
                const unsigned long long m_s = __ballot(hit);
                const unsigned long long m_v = __ballot(live && 2ull * (hit ? single : alt0) > (unsigned long long)reads);
                const int rd = wave_add((int)(hit ? single : 0u));       // (a run holds fewer than 2^32 - 256 alignments: no wrap that matters)
                if (lane == 0) { part[wave][t][0] = (uint32_t)__popcll(m_s); part[wave][t][1] = (uint32_t)rd; part[wave][t][2] = (uint32_t)__popcll(m_v); }
            }
            __syncthreads();
            if ((int)threadIdx.x < 3 * n_tgt) {
                const int t = threadIdx.x / 3, k = threadIdx.x % 3;
                uint32_t sum = 0;
                for (int w = 0; w < SPR_BLOCK / WAVE; ++w) sum += part[w][t][k];
                if (sum) atomicAdd(&out[(((size_t)v * n_reps + j) * n_tgt + t) * 3 + k], sum);
            }
            __syncthreads();
        }
    }
}
