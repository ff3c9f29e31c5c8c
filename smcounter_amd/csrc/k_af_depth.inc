// Included by smcounter_hip.hip (after k_select_aln.inc and k_af_reps.inc: it uses sel_draw, afr_draw and afr_find).
// ------------------------------------------------------------------------------------------
// --dsAFDepth: the keep masks and the achieved counts of the cells (target t, barcode fraction f) (smc_af_depth_masks, smc_af_depth_counts)
// ------------------------------------------------------------------------------------------
// A barcode b stays in cell (t, f) of replicate j when BOTH draws keep it, each a stream of its own with the key s_j:
//   the --dsAF rule at t   b is no carrier, or u_j(b) = afr_draw (domain "dsAF") < the carrier table's threshold at t;
//   the --dsMT rule at f   d_j(b) = sel_draw (domain "dsMT": k_select_aln.inc's philox rule) < floor(f * 2^32), 2^32 at f = 1.
// So a cell is the .dsMT<f> output of a --dsMT f --dsSampler philox run on the BAM tools/ds_allele_fraction.py --af t writes, the kept
// sets are nested in t and in f, and f = 1 gives k_afr_masks' masks bit for bit.  The AF draw is made for carriers only (one binary
// search per lane, as in k_af_reps.inc); the depth draw for EVERY barcode, once per replicate; the T + F compares become two small
// bit sets per lane, and a cell's vote is one bit of each.
//   k_afd_masks   a lane per run-wide barcode id of one decoded run; a wave's ballot is two mask words per cell; all R x T x F masks
//                 of a run in one launch (blockIdx.y strides over the replicates), in the layout smc_select_alignments takes.
//   k_afd_counts  a lane per covering barcode of a listed variant (blockIdx.y = variant, blockIdx.z strides over the replicates):
//                 N' / V' per cell by ballot + popcount, one atomic add per wave, replicate, cell and counter.
// The depth thresholds come by value (at most SMC_AF_DEPTH_MAX_CELLS of them: T x F is bounded by it).  Once per run / once per
// file: not on the per-locus hot path.
struct AfdThr {
    unsigned long long f[SMC_AF_DEPTH_MAX_CELLS];   // per fraction: floor(f * 2^32), 2^32 at f >= 1 (sel_keep's thr)
};

// bit t: the --dsAF rule keeps the barcode at target t (c: its place in the carrier table, AFR_NONE for a non-carrier)
__device__ __forceinline__ uint32_t afd_keep_af(const unsigned long long* __restrict__ thr, uint32_t c, uint32_t u, int n_tgt) {
    uint32_t keep = 0u;
    for (int t = 0; t < n_tgt; ++t) keep |= (uint32_t)(c == AFR_NONE || (unsigned long long)u < thr[t]) << t;
    return keep;
}

// bit f: the --dsMT draw keeps the barcode at fraction f
__device__ __forceinline__ uint32_t afd_keep_depth(const AfdThr& D, uint32_t d, int n_frac) {
    uint32_t keep = 0u;
    for (int f = 0; f < n_frac; ++f) keep |= (uint32_t)((unsigned long long)d < D.f[f]) << f;
    return keep;
}

// masks[((j * n_tgt + t) * n_frac + f) * n_words + (g >> 5)] bit (g & 31): barcode id g is kept in replicate j in cell (t, f).  The
// grid covers n_words words (two per wave); the lanes at and beyond n_ids vote 0, so the padding words are written as zeros.
__global__ __launch_bounds__(AFR_BLOCK) void k_afd_masks(const unsigned long long* __restrict__ ident, uint32_t n_ids,
                                                         const unsigned long long* __restrict__ car, const unsigned long long* __restrict__ car_thr,
                                                         uint32_t n_car, int n_tgt, AfdThr D, int n_frac, const unsigned long long* __restrict__ seeds,
                                                         int n_reps, uint32_t* __restrict__ masks, uint32_t n_words, uint32_t* __restrict__ draws) {
    const uint32_t g = blockIdx.x * AFR_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    const bool live = g < n_ids;
    unsigned long long id = 0;
    uint32_t c = AFR_NONE;
    if (live) { id = ident[g]; c = afr_find(car, n_car, id); }
    const unsigned long long* const thr = car_thr + (size_t)(c == AFR_NONE ? 0u : c) * (size_t)n_tgt;
    const uint32_t word = (g - lane) >> 5;             // the wave's first word
    for (int j = blockIdx.y; j < n_reps; j += gridDim.y) {
        const unsigned long long seed = seeds[j];
        const uint32_t u = c != AFR_NONE ? afr_draw(id, seed) : 0u;
        const uint32_t d = live ? sel_draw(id, seed) : 0u;
        if (draws && live) draws[(size_t)j * n_ids + g] = d;
        const uint32_t k_af = live ? afd_keep_af(thr, c, u, n_tgt) : 0u, k_d = live ? afd_keep_depth(D, d, n_frac) : 0u;
        for (int t = 0; t < n_tgt; ++t) {
            for (int f = 0; f < n_frac; ++f) {
                const unsigned long long m = __ballot((((k_af >> t) & (k_d >> f)) & 1u) != 0u);
                if (lane == 0) {
                    uint32_t* const row = masks + (((size_t)j * n_tgt + t) * n_frac + f) * n_words;
                    if (word < n_words) row[word] = (uint32_t)m;
                    if (word + 1 < n_words) row[word + 1] = (uint32_t)(m >> 32);
                }
            }
        }
    }
}

// out[(((v * n_reps + j) * n_tgt + t) * n_frac + f) * 2 + {0, 1}] += kept covering barcodes / kept carriers of variant v (zeroed
// before the launch).  cov_ident / cov_carry / cov_off: as k_afr_counts takes them.
__global__ __launch_bounds__(AFR_BLOCK) void k_afd_counts(const unsigned long long* __restrict__ cov_ident, const uint8_t* __restrict__ cov_carry,
                                                          const uint32_t* __restrict__ cov_off, const unsigned long long* __restrict__ car,
                                                          const unsigned long long* __restrict__ car_thr, uint32_t n_car, int n_tgt, AfdThr D,
                                                          int n_frac, const unsigned long long* __restrict__ seeds, int n_reps,
                                                          uint32_t* __restrict__ out) {
    const uint32_t v = blockIdx.y;
    const uint32_t e0 = cov_off[v], e1 = cov_off[v + 1];
    const int lane = threadIdx.x & (WAVE - 1);
    const uint32_t stride = gridDim.x * AFR_BLOCK;
    for (uint32_t w = e0 + (blockIdx.x * AFR_BLOCK + threadIdx.x) - lane; w < e1; w += stride) {       // (whole waves: the ballots)
        const uint32_t e = w + lane;
        const bool live = e < e1;
        unsigned long long id = 0;
        uint32_t c = AFR_NONE;
        bool carries = false;
        if (live) { id = cov_ident[e]; carries = cov_carry[e] != 0; c = afr_find(car, n_car, id); }
        const unsigned long long* const thr = car_thr + (size_t)(c == AFR_NONE ? 0u : c) * (size_t)n_tgt;
        for (int j = blockIdx.z; j < n_reps; j += gridDim.z) {
            const unsigned long long seed = seeds[j];
            const uint32_t u = c != AFR_NONE ? afr_draw(id, seed) : 0u;
            const uint32_t d = live ? sel_draw(id, seed) : 0u;
            const uint32_t k_af = live ? afd_keep_af(thr, c, u, n_tgt) : 0u, k_d = live ? afd_keep_depth(D, d, n_frac) : 0u;
            for (int t = 0; t < n_tgt; ++t) {
                for (int f = 0; f < n_frac; ++f) {
                    const bool keep = (((k_af >> t) & (k_d >> f)) & 1u) != 0u;
                    const unsigned long long m_n = __ballot(keep), m_v = __ballot(keep && carries);
                    if (lane == 0) {
                        uint32_t* const o = out + ((((size_t)v * n_reps + j) * n_tgt + t) * n_frac + f) * 2;
                        if (m_n) atomicAdd(&o[0], (uint32_t)__popcll(m_n));
                        if (m_v) atomicAdd(&o[1], (uint32_t)__popcll(m_v));
                    }
                }
            }
        }
    }
}
