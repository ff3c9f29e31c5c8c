// Included by smcounter_hip.hip (after k_philox_marks.inc and k_select_aln.inc: it uses smc_philox4x32_10 and sel_draw).
// ------------------------------------------------------------------------------------------
// --dsAFReps / --dsAFDepth: the keep masks and the achieved counts of the cells (target t, barcode fraction f) of R replicate
// dilutions (smc_af_rep_masks, smc_af_rep_counts, smc_af_depth_masks, smc_af_depth_counts)
// ------------------------------------------------------------------------------------------
// Replicate j of --dsAF is the same dilution with seed s_j: the carriers, N, V and the thresholds do not depend on the seed, only
// the draws do.  The host builds the CARRIER TABLE once - the sorted identities of the barcodes that carry a listed variant and,
// per carrier and target, the smallest threshold among the variants it carries (a barcode goes when any carried variant draws it
// out: u >= min thr) - and both kernels look a barcode up in it by binary search.  A barcode b stays in cell (t, f) of replicate j
// when BOTH draws keep it, each a stream of its own with the key s_j:
//   the --dsAF rule at t   b is no carrier, or u_j(b) = afr_draw (domain "dsAF") < the carrier table's threshold at t;
//   the --dsMT rule at f   d_j(b) = sel_draw (domain "dsMT": k_select_aln.inc's philox rule) < floor(f * 2^32), 2^32 at f = 1.
// So a cell is the .dsMT<f> output of a --dsMT f --dsSampler philox run on the BAM tools/ds_allele_fraction.py --af t writes, and
// the kept sets are nested in t and in f.  The replicate entries are the depth entries at ONE fraction of 2^32, which keeps every
// barcode whatever it draws: when no fraction is below 2^32 and nobody asked for the depth draws, the host says so (`with_depth`
// = 0, wave-uniform) and the depth draw is not made.  The AF draw is made for carriers only (one binary search per lane); the
// T + F compares become two small bit sets per lane, and a cell's vote is one bit of each.
//   k_afd_masks   a lane per run-wide barcode id of one decoded run; a wave's ballot is two mask words per cell; all R x T x F masks
//                 of a run in one launch (blockIdx.y strides over the replicates), in the layout smc_select_alignments takes.
//   k_afd_counts  a lane per covering barcode of a listed variant (blockIdx.y = variant, blockIdx.z strides over the replicates):
//                 N' = kept covering barcodes, V' = kept carriers of THAT variant, per cell by ballot + popcount, one atomic add
//                 per wave, replicate, cell and counter.
// The carrier table's thresholds reach 2^32 (k = 1: never dropped), so they are 64-bit words.  The depth thresholds come by value
// (at most SMC_AF_DEPTH_MAX_CELLS of them: T x F is bounded by it).  Once per run / once per file: not on the per-locus hot path.
#define AFR_BLOCK 256
#define AFR_DOMAIN 0x64734146u               // counter word 2 ("dsAF": tools/ds_allele_fraction.py AF_DOMAIN)
#define AFR_NONE 0xFFFFFFFFu

struct AfdThr {
    unsigned long long f[SMC_AF_DEPTH_MAX_CELLS];   // per fraction: floor(f * 2^32), 2^32 at f >= 1 (sel_keep's thr)
};

__device__ __forceinline__ uint32_t afr_draw(unsigned long long id, unsigned long long seed) {
    uint32_t x[4];
    smc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), AFR_DOMAIN, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
    return x[0];
}

// index of `id` in the ascending table, AFR_NONE when it is not there
__device__ __forceinline__ uint32_t afr_find(const unsigned long long* __restrict__ tab, uint32_t n, unsigned long long id) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (tab[mid] < id) lo = mid + 1; else hi = mid;
    }
    return (lo < n && tab[lo] == id) ? lo : AFR_NONE;
}

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
// draws_af / draws_depth (each may be NULL): [n_reps][n_ids] the AF draw of every carrier (0 for the others) / the depth draw of
// every id.
__global__ __launch_bounds__(AFR_BLOCK) void k_afd_masks(const unsigned long long* __restrict__ ident, uint32_t n_ids,
                                                         const unsigned long long* __restrict__ car, const unsigned long long* __restrict__ car_thr,
                                                         uint32_t n_car, int n_tgt, AfdThr D, int n_frac, int with_depth,
                                                         const unsigned long long* __restrict__ seeds, int n_reps, uint32_t* __restrict__ masks,
                                                         uint32_t n_words, uint32_t* __restrict__ draws_af, uint32_t* __restrict__ draws_depth) {
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
        const uint32_t d = (with_depth && live) ? sel_draw(id, seed) : 0u;        // (0 passes 2^32: all there is without the draw)
        if (draws_af && live) draws_af[(size_t)j * n_ids + g] = u;
        if (draws_depth && live) draws_depth[(size_t)j * n_ids + g] = d;
        const uint32_t k_af = live ? afd_keep_af(thr, c, u, n_tgt) : 0u, k_d = afd_keep_depth(D, d, n_frac);
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
// before the launch).  cov_ident / cov_carry: the covering barcodes of all variants one behind the other, variant v's at
// [cov_off[v], cov_off[v + 1]).
__global__ __launch_bounds__(AFR_BLOCK) void k_afd_counts(const unsigned long long* __restrict__ cov_ident, const uint8_t* __restrict__ cov_carry,
                                                          const uint32_t* __restrict__ cov_off, const unsigned long long* __restrict__ car,
                                                          const unsigned long long* __restrict__ car_thr, uint32_t n_car, int n_tgt, AfdThr D,
                                                          int n_frac, int with_depth, const unsigned long long* __restrict__ seeds, int n_reps,
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
            const uint32_t d = (with_depth && live) ? sel_draw(id, seed) : 0u;
            const uint32_t k_af = live ? afd_keep_af(thr, c, u, n_tgt) : 0u, k_d = afd_keep_depth(D, d, n_frac);
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
