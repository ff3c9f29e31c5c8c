// Included by smcounter_hip.hip (after k_philox_marks.inc: it uses smc_philox4x32_10).
// ------------------------------------------------------------------------------------------
// --dsAFReps: the keep masks and the achieved counts of R replicate dilutions (smc_af_rep_masks, smc_af_rep_counts)
// ------------------------------------------------------------------------------------------
// Replicate j of --dsAF is the same dilution with seed s_j: the carriers, N, V and the thresholds do not depend on the seed, only
// the draw u_j(b) = word 0 of Philox4x32-10(counter = (ident lo, ident hi, "dsAF", 0), key = s_j) of every carrier b does.  The host
// builds the CARRIER TABLE once - the sorted identities of the barcodes that carry a listed variant and, per carrier and target,
// the smallest threshold among the variants it carries (a barcode goes when any carried variant draws it out: u >= min thr) - and
// both kernels look a barcode up in it by binary search:
//   k_afr_masks   a lane per run-wide barcode id of one decoded run: non-carriers are kept in every mask, a carrier draws once per
//                 replicate and compares with its T thresholds; a wave's ballot is two mask words.  All R x T masks of a run in
//                 one launch (blockIdx.y strides over the replicates), in the layout smc_select_alignments takes.
//   k_afr_counts  a lane per covering barcode of a listed variant (blockIdx.y = variant, blockIdx.z strides over the replicates):
//                 N' = kept covering barcodes, V' = kept carriers of THAT variant, summed per wave by ballot + popcount, one
//                 atomic add per wave, replicate, target and counter.
// Thresholds reach 2^32 (k = 1: never dropped), so they are 64-bit words.  Once per run / once per file: not on the per-locus hot path.
#define AFR_BLOCK 256
#define AFR_DOMAIN 0x64734146u               // counter word 2 ("dsAF": tools/ds_allele_fraction.py AF_DOMAIN)
#define AFR_NONE 0xFFFFFFFFu

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

// masks[(j * n_tgt + t) * n_words + (g >> 5)] bit (g & 31): barcode id g is kept in replicate j at target t.  The grid covers
// n_words words (two per wave); the lanes at and beyond n_ids vote 0, so the padding words are written as zeros.
__global__ __launch_bounds__(AFR_BLOCK) void k_afr_masks(const unsigned long long* __restrict__ ident, uint32_t n_ids,
                                                         const unsigned long long* __restrict__ car, const unsigned long long* __restrict__ car_thr,
                                                         uint32_t n_car, int n_tgt, const unsigned long long* __restrict__ seeds, int n_reps,
                                                         uint32_t* __restrict__ masks, uint32_t n_words, uint32_t* __restrict__ draws) {
    const uint32_t g = blockIdx.x * AFR_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    const bool live = g < n_ids;
    unsigned long long id = 0;
    uint32_t c = AFR_NONE;
    if (live) { id = ident[g]; c = afr_find(car, n_car, id); }
    const unsigned long long* const thr = car_thr + (size_t)(c == AFR_NONE ? 0u : c) * (size_t)n_tgt;
    const uint32_t word = (g - lane) >> 5;             // the wave's first word
    for (int j = blockIdx.y; j < n_reps; j += gridDim.y) {
        const uint32_t u = c != AFR_NONE ? afr_draw(id, seeds[j]) : 0u;
        if (draws && live) draws[(size_t)j * n_ids + g] = u;
        for (int t = 0; t < n_tgt; ++t) {
            const bool keep = live && (c == AFR_NONE || (unsigned long long)u < thr[t]);
            const unsigned long long m = __ballot(keep);
            if (lane == 0) {
                uint32_t* const row = masks + ((size_t)j * n_tgt + t) * n_words;
                if (word < n_words) row[word] = (uint32_t)m;
                if (word + 1 < n_words) row[word + 1] = (uint32_t)(m >> 32);
            }
        }
    }
}

// out[((v * n_reps + j) * n_tgt + t) * 2 + {0, 1}] += kept covering barcodes / kept carriers of variant v (zeroed before the launch).
// cov_ident / cov_carry: the covering barcodes of all variants one behind the other, variant v's at [cov_off[v], cov_off[v + 1]).
__global__ __launch_bounds__(AFR_BLOCK) void k_afr_counts(const unsigned long long* __restrict__ cov_ident, const uint8_t* __restrict__ cov_carry,
                                                          const uint32_t* __restrict__ cov_off, const unsigned long long* __restrict__ car,
                                                          const unsigned long long* __restrict__ car_thr, uint32_t n_car, int n_tgt,
                                                          const unsigned long long* __restrict__ seeds, int n_reps, uint32_t* __restrict__ out) {
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
            const uint32_t u = c != AFR_NONE ? afr_draw(id, seeds[j]) : 0u;
            for (int t = 0; t < n_tgt; ++t) {
                const bool keep = live && (c == AFR_NONE || (unsigned long long)u < thr[t]);
                const unsigned long long m_n = __ballot(keep), m_v = __ballot(keep && carries);
                if (lane == 0) {
                    uint32_t* const o = out + (((size_t)v * n_reps + j) * n_tgt + t) * 2;
                    if (m_n) atomicAdd(&o[0], (uint32_t)__popcll(m_n));
                    if (m_v) atomicAdd(&o[1], (uint32_t)__popcll(m_v));
                }
            }
        }
    }
}
