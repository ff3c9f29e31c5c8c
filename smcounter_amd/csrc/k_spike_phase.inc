// Included by smcounter_hip.hip (after k_spike_depth.inc: SpkThr, AfdThr, spd_hits, afd_keep_depth and sel_draw).
// ------------------------------------------------------------------------------------------
// --spikePhase: what every cell (target t, barcode fraction f) of R replicate spike-ins achieves for a whole PHASE SET - how many
// molecules carry every member of the haplotype - with no spiked copy and no selection (smc_spike_phase_counts)
// ------------------------------------------------------------------------------------------
// A phase set is a group of listed SNVs that share ONE draw per barcode: counter word 3 is the 1-based position of the set's leader
// (k_spike.inc reads it through smc_spike_variant.lead), so a barcode is spiked at every member or at none.  The JOINT barcodes of a
// set are those that cover every member; per joint barcode and member the host gives k_spike_counts' three numbers (reads, alt0,
// single).  A joint barcode carries the whole set before spiking when 2 * alt0 > reads at EVERY member, and after spiking when 2 *
// (hit ? single : alt0) > reads at every member - `hit` is the same for all members, so the two conjunctions are made once per lane,
// outside the loops over the replicates and the cells.
//   k_spike_phase_counts   k_spike_depth_counts' layout: a lane per joint barcode (blockIdx.y = set, blockIdx.z strides over the
//                  replicates); one spike draw per (barcode, set, replicate), the depth draw only with `with_depth`; per cell four
//                  ballots + popcounts, the workgroup's four wavefronts added in LDS, then one atomic add per workgroup, replicate,
//                  cell and counter that is not 0.
// Once per run: not on the per-locus hot path.
#define SPP_COUNTERS 4

// out[((((g * n_reps + j) * n_tgt + t) * n_frac + f) * 4 + {0 .. 3}] += (N_ALL', V0_ALL', S_ALL', V1_ALL') of set g (zeroed before the
// launch); n_tgt * n_frac <= SMC_AF_DEPTH_MAX_CELLS.  Set g: joint barcodes [joint_off[g], joint_off[g + 1]) of joint_ident, M =
// set_m[g] members (1 .. SMC_SPIKE_PHASE_MAX_MEMBERS, checked by the host), counters joint_cnt[cnt_off[g] + (e - joint_off[g]) * 3 * M
// + 3 * m + {0, 1, 2}].
__global__ __launch_bounds__(SPR_BLOCK) void k_spike_phase_counts(const unsigned long long* __restrict__ joint_ident, const uint32_t* __restrict__ joint_cnt,
                                                                  const uint32_t* __restrict__ joint_off, const uint32_t* __restrict__ set_m,
                                                                  const uint32_t* __restrict__ cnt_off, const uint32_t* __restrict__ pos1, SpkThr T,
                                                                  int n_tgt, AfdThr D, int n_frac, int with_depth,
                                                                  const unsigned long long* __restrict__ seeds, int n_reps,
                                                                  uint32_t* __restrict__ out) {
    __shared__ uint32_t part[SPR_BLOCK / WAVE][SMC_AF_DEPTH_MAX_CELLS][SPP_COUNTERS];
    const uint32_t g = blockIdx.y;
    const uint32_t e0 = joint_off[g], e1 = joint_off[g + 1], pos = pos1[g], M = set_m[g];
    const uint32_t* const cnt_g = joint_cnt + cnt_off[g];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int n_cells = n_tgt * n_frac;
    const uint32_t stride = gridDim.x * SPR_BLOCK;
    for (uint32_t base = e0 + blockIdx.x * SPR_BLOCK; base < e1; base += stride) {     // (whole workgroups: the barriers below)
        const uint32_t e = base + threadIdx.x;
        const bool live = e < e1;
        unsigned long long id = 0;
        bool car0 = live, car1 = live;                                                 // carries EVERY member before / when hit
        if (live) {
            id = joint_ident[e];
            const uint32_t* const row = cnt_g + (size_t)(e - e0) * 3u * M;
            for (uint32_t m = 0; m < M; ++m) {
                const unsigned long long reads = row[3 * m], alt0 = row[3 * m + 1], single = row[3 * m + 2];
                car0 = car0 && 2ull * alt0 > reads;
                car1 = car1 && 2ull * single > reads;
            }
        }
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
                    if (lane == 0) {
                        uint32_t* const p = part[wave][t * n_frac + f];
                        p[0] = (uint32_t)__popcll(m_n); p[1] = (uint32_t)__popcll(m_v0); p[2] = (uint32_t)__popcll(m_s);
                        p[3] = (uint32_t)__popcll(m_v1);
                    }
                }
            }
            __syncthreads();
            if ((int)threadIdx.x < SPP_COUNTERS * n_cells) {                           // (4 * 32 = 128 < SPR_BLOCK)
                const int c = threadIdx.x / SPP_COUNTERS, k = threadIdx.x % SPP_COUNTERS;
                uint32_t sum = 0;
                for (int w = 0; w < SPR_BLOCK / WAVE; ++w) sum += part[w][c][k];
                if (sum) atomicAdd(&out[(((size_t)g * n_reps + j) * n_cells + c) * SPP_COUNTERS + k], sum);
            }
            __syncthreads();
        }
    }
}
