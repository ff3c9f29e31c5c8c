// Included by smcounter_hip.hip (after k_spike.inc: the spike draw's domain, SpkThr and SPR_BLOCK; after k_select_aln.inc: sel_draw;
// after k_af_depth.inc: AfdThr and afd_keep_depth).
// ------------------------------------------------------------------------------------------
// --spikeReps, --spikeDepth, --spikePhase: what every cell (target t, barcode fraction f) of R replicate spike-ins achieves, per
// listed variant or per whole PHASE SET, with no spiked copy and no selection at all (smc_spike_rep_counts, smc_spike_depth_counts,
// smc_spike_phase_counts)
// ------------------------------------------------------------------------------------------
// A cell is the --spikeAF spike-in at t, then the --dsMT philox selection at f, both drawn with the key s_j, each a stream of its own:
//   the spike rule at t    hit  = u(b) = k_spike_rewrite's draw (domain "spAF", counter word 3 the row's 1-based position) < thr[t];
//   the --dsMT rule at f   keep = d(b) = sel_draw (domain "dsMT": k_select_aln.inc's philox rule) < floor(f * 2^32), 2^32 at f = 1.
// A ROW g is a listed variant (M = 1) or a phase set of M members, which share ONE draw per barcode - counter word 3 is the position
// of the set's leader, so a barcode is spiked at every member or at none.  Its barcodes are those that cover every member; per
// barcode and member the host gives three numbers the run itself fixes: `reads` (its pileup reads there), `alt0` (those that show ALT
// as they are) and `single` (those whose allele key there is a single letter: exactly the reads a hit rewrites to ALT, every other
// read of the barcode keeps a key that is not ALT).  NO SPIKED COPY IS NEEDED: a barcode that is hit shows ALT in `single` of its
// reads, one that is not in `alt0`, and it carries a member when twice that exceeds `reads`.  `single` depends on the CIGAR alone - not
// on any letter - so a neighbouring listed variant that is written into the same reads does not change it.  A barcode carries the row
// before spiking when 2 * alt0 > reads at EVERY member (car0), when hit when 2 * single > reads at every member (car1): `hit` is the
// same for all members, so the two conjunctions are made once per lane, outside the loops over the replicates and the cells.  The
// selection keeps or drops whole barcodes.  Per cell, over the row's barcodes:
//   N' = keep    V0' = keep && car0    S' = keep && hit    READS' = sum of `single` over keep && hit (M = 1)    V1' = keep && (hit ? car1 : car0)
// The replicate entry is the cells of ONE fraction of 2^32, which keeps every barcode whatever it draws: when no fraction is below
// 2^32 the host says so (`with_depth` = 0, the same for all lanes) and the depth draw is not made.
//   k_spike_cells  a lane per barcode of a row (blockIdx.y = row, blockIdx.z strides over the replicates): one spike draw per (barcode,
//                  row, replicate) and the depth draw with `with_depth`, whose T + F compares become two small bit sets per lane; a
//                  cell's vote is one bit of each.  Per cell four ballots + popcounts and, where READS' is wanted, a DPP sum; the
//                  workgroup's four wavefronts added in LDS, then one atomic add per workgroup, replicate, cell and WANTED counter that
//                  is not 0.  `want` (uniform): bit k = counter k of (N', V0', S', READS', V1') is stored, the stored ones one behind
//                  the other in that order - 0b11100 for the replicates, 0b11111 for the depths, 0b10111 for the phase sets.
// --spikeIndelReps, --spikeIndelDepth (smc_spike_indel_counts): for an insertion or a deletion `single` is two numbers - the reads
// that show ALT when the barcode is hit (`alt1`: those that show it already, and the rewritten ones whose anchor letter is REF's) and
// the records the rewrite changes (`touch`: an eligible record whose anchor holds another letter is rewritten, and shows another key).
// The host then gives FOUR numbers per barcode, (reads, alt0, alt1, touch), and the kernel takes the row's stride `cs` and the two
// columns as uniform arguments: car1 from column `i_alt1`, READS' from column `i_touch`.  cs = 3 with both columns 2 is the kernel of
// the three entries above.
// Once per run / once per file: not on the per-locus hot path.
#define SPC_COUNTERS 5
static_assert(SMC_SPIKE_REP_MAX_TARGETS <= SMC_AF_DEPTH_MAX_CELLS && SPC_COUNTERS * SMC_AF_DEPTH_MAX_CELLS <= SPR_BLOCK,
              "k_spike_cells: a cell per target fits the LDS tile, a lane per cell and counter the workgroup");

// bit t: the spike draw hits the barcode at target t
__device__ __forceinline__ uint32_t spd_hits(const SpkThr& T, uint32_t u, int n_tgt) {
    uint32_t hit = 0u;
    for (int t = 0; t < n_tgt; ++t) hit |= (uint32_t)((unsigned long long)u < T.t[t]) << t;
    return hit;
}

// out[((g * n_reps + j) * n_tgt * n_frac + t * n_frac + f) * popcount(want) + k] += the k-th wanted counter of row g (zeroed before
// the launch); n_tgt * n_frac <= SMC_AF_DEPTH_MAX_CELLS.  Row g: barcodes [off[g], off[g + 1]) of `ident`, M = set_m[g] members (1 ..
// SMC_SPIKE_PHASE_MAX_MEMBERS, checked by the host; 1 when set_m is NULL), counters cnt[base + (e - off[g]) * cs * M + cs * m + {0, 1,
// i_alt1, i_touch}] = (reads, alt0, alt1, touch) with base = cnt_off[g], or cs * off[g] when cnt_off is NULL (every row has one member).
__global__ __launch_bounds__(SPR_BLOCK) void k_spike_cells(const unsigned long long* __restrict__ ident, const uint32_t* __restrict__ cnt,
                                                           uint32_t cs, uint32_t i_alt1, uint32_t i_touch,
                                                           const uint32_t* __restrict__ off, const uint32_t* __restrict__ set_m,
                                                           const uint32_t* __restrict__ cnt_off, const uint32_t* __restrict__ pos1, SpkThr T,
                                                           int n_tgt, AfdThr D, int n_frac, int with_depth,
                                                           const unsigned long long* __restrict__ seeds, int n_reps, uint32_t want,
                                                           uint32_t* __restrict__ out) {
    __shared__ uint32_t part[SPR_BLOCK / WAVE][SMC_AF_DEPTH_MAX_CELLS][SPC_COUNTERS];
    const uint32_t g = blockIdx.y;
    const uint32_t e0 = off[g], e1 = off[g + 1], pos = pos1[g], M = set_m ? set_m[g] : 1u;
    const uint32_t* const cnt_g = cnt + (cnt_off ? (size_t)cnt_off[g] : (size_t)cs * e0);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int n_cells = n_tgt * n_frac, n_want = __popc(want);
    const uint32_t stride = gridDim.x * SPR_BLOCK;
    for (uint32_t base = e0 + blockIdx.x * SPR_BLOCK; base < e1; base += stride) {     // (whole workgroups: the barriers below)
        const uint32_t e = base + threadIdx.x;
        const bool live = e < e1;
        unsigned long long id = 0;
        uint32_t single = 0;
        bool car0 = live, car1 = live;                                                 // carries EVERY member before / when hit
        if (live) {
            id = ident[e];
            const uint32_t* const row = cnt_g + (size_t)(e - e0) * cs * M;
            for (uint32_t m = 0; m < M; ++m) {
                const unsigned long long reads = row[cs * m], alt0 = row[cs * m + 1], sgl = row[cs * m + i_alt1];
                car0 = car0 && 2ull * alt0 > reads;
                car1 = car1 && 2ull * sgl > reads;
            }
            if (M == 1u) single = row[i_touch];
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
                    // (a run holds fewer than 2^32 - 256 alignments: no wrap that matters)
                    const int rd = (want & 8u) ? wave_add((int)((keep && hit) ? single : 0u)) : 0;
                    if (lane == 0) {
                        uint32_t* const p = part[wave][t * n_frac + f];
                        p[0] = (uint32_t)__popcll(m_n); p[1] = (uint32_t)__popcll(m_v0); p[2] = (uint32_t)__popcll(m_s);
                        p[3] = (uint32_t)rd; p[4] = (uint32_t)__popcll(m_v1);
                    }
                }
            }
            __syncthreads();
            if ((int)threadIdx.x < SPC_COUNTERS * n_cells) {                           // (5 * 32 = 160 < SPR_BLOCK)
                const int c = threadIdx.x / SPC_COUNTERS, q = threadIdx.x % SPC_COUNTERS;
                uint32_t sum = 0;
                for (int w = 0; w < SPR_BLOCK / WAVE; ++w) sum += part[w][c][q];
                if (sum && ((want >> q) & 1u))                                         // (its place: the wanted counters in front of q)
                    atomicAdd(&out[(((size_t)g * n_reps + j) * n_cells + c) * n_want + __popc(want & ((1u << q) - 1u))], sum);
            }
            __syncthreads();
        }
    }
}
