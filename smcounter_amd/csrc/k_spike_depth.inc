// Included by smcounter_hip.hip (after k_spike_reps.inc: the spike draw's domain and SpkThr; after k_select_aln.inc: sel_draw; after
// k_af_depth.inc: AfdThr and afd_keep_depth).
// ------------------------------------------------------------------------------------------
// --spikeDepth: what every cell (target t, barcode fraction f) of R replicate spike-ins achieves, with no spiked copy and no
// selection at all (smc_spike_depth_counts)
// ------------------------------------------------------------------------------------------
// A cell of --spikeDepth is the --spikeAF spike-in at t, then the --dsMT philox selection at f, both drawn with the key s_j, each a
// stream of its own:
//   the spike rule at t    hit  = u_v(b) = k_spike's draw (domain "spAF", counter word 3 the variant's 1-based position) < thr[t];
//   the --dsMT rule at f   keep = d(b) = sel_draw (domain "dsMT": k_select_aln.inc's philox rule) < floor(f * 2^32), 2^32 at f = 1.
// The selection keeps or drops whole barcodes, so of k_spike_counts' sums only the barcodes with `keep` remain; N' and V0' are the
// cover and the carriers before spiking that remain.  At one fraction of 2^32 (S', READS', V1') are k_spike_counts' (S, READS, V1).
//   k_spike_depth_counts   a lane per covering barcode of a listed variant (blockIdx.y = variant, blockIdx.z strides over the
//                  replicates): TWO Philox calls per (barcode, variant, replicate) - one when no fraction is below 2^32 (`with_depth`
//                  = 0, from the host, the same for all lanes) - whose T + F compares become two small bit sets per lane; a cell's
//                  vote is one bit of each.  Per cell four ballots + popcounts and a DPP sum for READS', the workgroup's four
//                  wavefronts added in LDS, then one atomic add per workgroup, replicate, cell and counter that is not 0.
// Once per run / once per file: not on the per-locus hot path.
#define SPD_COUNTERS 5

// bit t: the spike draw hits the barcode at target t
__device__ __forceinline__ uint32_t spd_hits(const SpkThr& T, uint32_t u, int n_tgt) {
    uint32_t hit = 0u;
    for (int t = 0; t < n_tgt; ++t) hit |= (uint32_t)((unsigned long long)u < T.t[t]) << t;
    return hit;
}

// out[((((v * n_reps + j) * n_tgt + t) * n_frac + f) * 5 + {0 .. 4}] += (N', V0', S', READS', V1') of variant v (zeroed before the
// launch); n_tgt * n_frac <= SMC_AF_DEPTH_MAX_CELLS.  cov_ident / cov_cnt / cov_off / pos1: as k_spike_counts takes them.
__global__ __launch_bounds__(SPR_BLOCK) void k_spike_depth_counts(const unsigned long long* __restrict__ cov_ident, const uint32_t* __restrict__ cov_cnt,
                                                                  const uint32_t* __restrict__ cov_off, const uint32_t* __restrict__ pos1, SpkThr T,
                                                                  int n_tgt, AfdThr D, int n_frac, int with_depth,
                                                                  const unsigned long long* __restrict__ seeds, int n_reps,
                                                                  uint32_t* __restrict__ out) {
    __shared__ uint32_t part[SPR_BLOCK / WAVE][SMC_AF_DEPTH_MAX_CELLS][SPD_COUNTERS];
    const uint32_t v = blockIdx.y;
    const uint32_t e0 = cov_off[v], e1 = cov_off[v + 1], pos = pos1[v];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int n_cells = n_tgt * n_frac;
    const uint32_t stride = gridDim.x * SPR_BLOCK;
    for (uint32_t base = e0 + blockIdx.x * SPR_BLOCK; base < e1; base += stride) {     // (whole workgroups: the barriers below)
        const uint32_t e = base + threadIdx.x;
        const bool live = e < e1;
        unsigned long long id = 0;
        uint32_t reads = 0, alt0 = 0, single = 0;
        if (live) { id = cov_ident[e]; reads = cov_cnt[3ull * e]; alt0 = cov_cnt[3ull * e + 1]; single = cov_cnt[3ull * e + 2]; }
        const bool car0 = 2ull * alt0 > (unsigned long long)reads, car1 = 2ull * single > (unsigned long long)reads;
        for (int j = blockIdx.z; j < n_reps; j += gridDim.z) {
            const unsigned long long seed = seeds[j];
            uint32_t x[4];
            smc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), SPK_DOMAIN, pos, (uint32_t)seed, (uint32_t)(seed >> 32), x);
            const uint32_t d = with_depth ? sel_draw(id, seed) : 0u;                   // (0 passes 2^32: all there is without the draw)
            const uint32_t k_hit = spd_hits(T, x[0], n_tgt), k_d = live ? afd_keep_depth(D, d, n_frac) : 0u;
            for (int t = 0; t < n_tgt; ++t) {
                const bool hit = ((k_hit >> t) & 1u) != 0u;
                for (int f = 0; f < n_frac; ++f) {
                    const bool keep = ((k_d >> f) & 1u) != 0u;
                    const unsigned long long m_n = __ballot(keep), m_v0 = __ballot(keep && car0), m_s = __ballot(keep && hit);
                    const unsigned long long m_v1 = __ballot(keep && (hit ? car1 : car0));
                    const int rd = wave_add((int)((keep && hit) ? single : 0u));       // (a run holds fewer than 2^32 - 256 alignments: no wrap that matters)
                    if (lane == 0) {
                        uint32_t* const p = part[wave][t * n_frac + f];
                        p[0] = (uint32_t)__popcll(m_n); p[1] = (uint32_t)__popcll(m_v0); p[2] = (uint32_t)__popcll(m_s);
                        p[3] = (uint32_t)rd; p[4] = (uint32_t)__popcll(m_v1);
                    }
                }
            }
            __syncthreads();
            if ((int)threadIdx.x < SPD_COUNTERS * n_cells) {                           // (5 * 32 = 160 < SPR_BLOCK)
                const int c = threadIdx.x / SPD_COUNTERS, k = threadIdx.x % SPD_COUNTERS;
                uint32_t sum = 0;
                for (int w = 0; w < SPR_BLOCK / WAVE; ++w) sum += part[w][c][k];
                if (sum) atomicAdd(&out[(((size_t)v * n_reps + j) * n_cells + c) * SPD_COUNTERS + k], sum);
            }
            __syncthreads();
        }
    }
}
