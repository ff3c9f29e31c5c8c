// Included by smcounter_hip.hip.
// ------------------------------------------------------------------------------------------
// kernel 2: filterVariants (smCounter.py:182-269), one workgroup per locus (a wavefront per Fisher test), only where it applies
// ------------------------------------------------------------------------------------------
// log(n!) for an integer-valued n >= 0: Stirling's series on x = n + 1 >= 9 (truncation < 1e-12), exact constants
// below (one log either way, unlike the general lgamma of the device library, which is several hundred instructions)
__device__ __forceinline__ double d_lfact(double n) {
    const double x = n + 1.0;
    const double r = 1.0 / x, r2 = r * r;
    const double series = r * (8.33333333333333333e-2 + r2 * (-2.77777777777777778e-3 + r2 * (7.93650793650793651e-4 +
                          r2 * (-5.95238095238095238e-4 + r2 * 8.41750841750841751e-4))));
    const double st = (x - 0.5) * log(x) - x + 0.918938533204672742 + series;
    // n = 0..7: log of 1, 1, 2, 6, 24, 120, 720, 5040
    double small = 0.0;
    small = n == 2.0 ? 0.693147180559945309 : small;
    small = n == 3.0 ? 1.79175946922805500 : small;
    small = n == 4.0 ? 3.17805383034794562 : small;
    small = n == 5.0 ? 4.78749174278204599 : small;
    small = n == 6.0 ? 6.57925121201010100 : small;
    small = n == 7.0 ? 8.52516136106541430 : small;
    return n < 8.0 ? small : st;
}

// log(n!) for n < SMC_LFACT_N from the per-context table (k_lfact_table: the values d_lfact computes, so a lookup changes
// no bit); beyond it computed.  A Fisher test asks for five of them per lane: the logarithm in each was most of the kernel.
#define SMC_LFACT_N 65536
__global__ void k_lfact_table(double* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n < SMC_LFACT_N) out[n] = d_lfact((double)n);
}
__device__ __forceinline__ double t_lfact(const double* __restrict__ tab, long long n) {
    return n < SMC_LFACT_N ? tab[n] : d_lfact((double)n);
}

// scipy.stats.fisher_exact(table) two-sided, evaluated by one wavefront: the support is cut into
// 64 contiguous chunks, each lane anchors its chunk with one log-factorial-based pmf and walks it with the
// exact ratio pmf(k+1)/pmf(k) = (n1-k)(n-k) / ((k+1)(n2-n+k+1)).  The nine log-factorials every lane needs
// (margins, the observed table) are evaluated once, one per lane, and broadcast.
__device__ void wave_fisher(const double* __restrict__ lft, long long a, long long b, long long c, long long d, double* orat, double* pval) {
    const int lane = threadIdx.x & 63;
    if (a + b == 0 || c + d == 0 || a + c == 0 || b + d == 0) { *orat = NAN; *pval = 1.0; return; }
    *orat = (c > 0 && b > 0) ? ((double)(a * d)) / ((double)(c * b)) : INFINITY;
    const long long n1 = a + b, n2 = c + d, n = a + c;
    const long long lo = n - n2 > 0 ? n - n2 : 0, hi = n < n1 ? n : n1;
    // uniform terms: lane i evaluates argument i
    const long long args[9] = {n1, n2, n1 + n2, n, n1 + n2 - n, a, n1 - a, n - a, n2 - n + a};
    long long mine = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) mine = lane == i ? args[i] : mine;
    const double lf_mine = t_lfact(lft, mine);
    double u[9];
#pragma unroll
    for (int i = 0; i < 9; ++i)
        u[i] = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(lf_mine), i), __builtin_amdgcn_readlane(__double2loint(lf_mine), i));
    const double lden = u[2] - u[3] - u[4];                              // log C(n1 + n2, n)
    const double lnum0 = u[0] + u[1] - lden;                             // log(n1!) + log(n2!) - log C(n1 + n2, n)
    const double pexact = exp(lnum0 - u[5] - u[6] - u[7] - u[8]);
    const double thr = pexact * (1.0 + 1e-7);
    const long long len = hi - lo + 1, chunk = (len + 63) / 64;
    const long long k0 = lo + chunk * lane, k1 = (k0 + chunk - 1 < hi) ? k0 + chunk - 1 : hi;
    double p = 0.0;
    if (k0 <= hi) {
        double pk = exp(lnum0 - t_lfact(lft, k0) - t_lfact(lft, n1 - k0) - t_lfact(lft, n - k0) - t_lfact(lft, n2 - n + k0));
        for (long long k = k0;; ++k) {
            if (pk <= thr) p += pk;
            if (k == k1) break;
            // (reciprocal + Newton steps instead of the IEEE division sequence: the quotient is within an ulp, the walk is ~ 50 terms)
            pk *= fast_div((double)(n1 - k) * (double)(n - k), (double)(k + 1) * (double)(n2 - n + k + 1));
        }
    }
    p += dpp_f64<DPP_XOR1>(p); p += dpp_f64<DPP_XOR2>(p); p += dpp_f64<DPP_HALF_MIRROR>(p); p += dpp_f64<DPP_MIRROR>(p);
    p = __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(p), 0), __builtin_amdgcn_readlane(__double2loint(p), 0)) +
        __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(p), 16), __builtin_amdgcn_readlane(__double2loint(p), 16)) +
        __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(p), 32), __builtin_amdgcn_readlane(__double2loint(p), 32)) +
        __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(p), 48), __builtin_amdgcn_readlane(__double2loint(p), 48));
    *pval = p < 1.0 ? p : 1.0;
}

// filterVariants for one queued locus.  SPLIT: by the four wavefronts of a workgroup - wavefront t takes the t-th of the four Fisher
// tests (strand bias, R1 / R2 / primer end clustering: each a chain of table look-ups, an exponential and a walk over its share of
// the support), the integer / ratio tests ride with wavefront 0, flags are ORed in LDS.  Not SPLIT: by one wavefront, the tests one
// after the other (`t` unused, no barrier).
template <bool SPLIT>
__device__ __forceinline__ void flt_locus(const smc_locus* __restrict__ loci, smc_row* __restrict__ rows, int li,
                                          const double* __restrict__ lft, int t, int lane, uint32_t* s_f) {
    smc_row* R = rows + li;
    if ((R->status & 0xff) != SMC_ST_OK) return;                                  // (uniform over the locus's threads)
    const smc_locus L = loci[li];
    for (int ci = 0; ci < 2; ++ci) {
        smc_cand* C = &R->cand[ci];
        if (C->allele < 0 || !C->flt_applied) continue;                           // (uniform)
        const int alt = C->allele;
        const bool snp = (L.snp_mask >> alt) & 1ull;
        const int* ta = C->tal;
        const int* tr = R->ref_tal;
        if (SPLIT) {
            __syncthreads();                                                      // (the previous candidate's flags have been read)
            if (threadIdx.x == 0) *s_f = 0u;
            __syncthreads();
        }
        uint32_t f = 0;
        const double af_alt = 100.0 * ta[SMC_T_CNT] / R->cvg;                     // :206
        double orat, p;
        if (!SPLIT || t == 0) {
            if (R->used_mt < 5) f |= SMC_F_LM;                                    // :187
            if (C->vsm < 2) f |= SMC_F_LSM;                                       // :191
            const int vmf = (1.0 * C->vmt / R->used_mt < 0.99);                   // :198,:202
            const int pairs = ta[SMC_T_DISCORD] + ta[SMC_T_CONCORD];              // :207
            double p_sb = NAN;
            if (pairs >= 1000 && 1.0 * ta[SMC_T_DISCORD] / pairs >= 0.5) {
                f |= SMC_F_DP;                                                    // :208-209
            } else if (af_alt <= 60.0) {
                wave_fisher(lft, tr[SMC_T_REV], tr[SMC_T_FWD], ta[SMC_T_REV], ta[SMC_T_FWD], &orat, &p);   // :211-215
                p_sb = p;
                if (p < 0.00001 && (orat >= 50 || orat <= 1.0 / 50)) f |= SMC_F_SB;
            }
            double bq_alt = 0.0;                                                  // :222-227
            if (snp && ta[SMC_T_LOWQ] > 0) bq_alt = 1.0 * ta[SMC_T_LOWQ] / ta[SMC_T_CNT];
            if (bq_alt > 0.4) f |= SMC_F_LOWQ;
            if (lane == 0) { C->vmf_lt_099 = vmf; C->p_sb = p_sb; }
        }
        // :230-266: the end-distance tests are the SNPs'
        if (!SPLIT || t == 1) {
            p = NAN;
            if (snp) {
                wave_fisher(lft, tr[SMC_T_R1LE], tr[SMC_T_R1N] - tr[SMC_T_R1LE], ta[SMC_T_R1LE], ta[SMC_T_R1N] - ta[SMC_T_R1LE], &orat, &p);
                if (p < 0.001 && orat < 0.05 && af_alt <= 60.0) f |= SMC_F_R1CP;
            }
            if (lane == 0) C->p_r1 = p;
        }
        if (!SPLIT || t == 2) {
            p = NAN;
            if (snp) {
                wave_fisher(lft, tr[SMC_T_R2BCLE], tr[SMC_T_R2N] - tr[SMC_T_R2BCLE], ta[SMC_T_R2BCLE], ta[SMC_T_R2N] - ta[SMC_T_R2BCLE], &orat, &p);
                if (p < 0.001 && orat < 0.05 && af_alt <= 60.0) f |= SMC_F_R2CP;
            }
            if (lane == 0) C->p_r2 = p;
        }
        if (!SPLIT || t == 3) {
            p = NAN;
            if (snp) {
                const int alt_le = ta[SMC_T_R2PRLE], alt_gt = ta[SMC_T_R2N] - ta[SMC_T_R2PRLE];
                wave_fisher(lft, tr[SMC_T_R2PRLE], tr[SMC_T_R2N] - tr[SMC_T_R2PRLE], alt_le, alt_gt, &orat, &p);
                if (alt_le + alt_gt > 0)
                    if (1.0 * alt_le / (alt_le + alt_gt) >= 0.98 || (p < 0.001 && orat < 1.0 / 20)) f |= SMC_F_PRIMERCP;
            }
            if (lane == 0) C->p_pr = p;
        }
        if (SPLIT) {
            if (lane == 0 && f) atomicOr(s_f, f);
            __syncthreads();
            if (threadIdx.x == 0) C->flt = *s_f;
        } else if (lane == 0) {
            C->flt = f;
        }
    }
}

// A fixed grid of four-wavefront workgroups walks the worklist.  A short list (fewer loci than the grid has wavefronts: the
// deep shapes - a few hundred loci whose tests run over supports of thousands) is taken a locus per WORKGROUP, the four tests side
// by side: the kernel is then as long as one test, not four.  A long list (X3: 12,000 shallow loci, short tests) is taken a
// locus per WAVEFRONT: there the chain before the tests (list entry, row, descriptor) is what takes the time, and 8192 of them
// in flight beat 2048.  (Round 4; before: always a locus per wavefront.)
#define SMC_FLT_BLOCK 256
__global__ __launch_bounds__(SMC_FLT_BLOCK) void k_filter_loci(KParams P, const smc_locus* __restrict__ loci, smc_row* __restrict__ rows,
                                                               const uint32_t* __restrict__ flt_list, uint32_t* __restrict__ other_count, const double* __restrict__ lft) {
    __shared__ uint32_t s_f;
    const uint32_t n_work = flt_list[0];
    const int lane = threadIdx.x & 63;
    const int t = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    constexpr uint32_t NWV = SMC_FLT_BLOCK / WAVE;
    if (n_work <= gridDim.x * NWV) {                                              // (grid-uniform)
        for (uint32_t w = blockIdx.x; w < n_work; w += gridDim.x)
            flt_locus<true>(loci, rows, (int)flt_list[1 + w], lft, t, lane, &s_f);
    } else {
        for (uint32_t w = blockIdx.x * NWV + (uint32_t)t; w < n_work; w += gridDim.x * NWV)
            flt_locus<false>(loci, rows, (int)flt_list[1 + w], lft, t, lane, &s_f);
    }
    // (the plan's two worklists are used in turn: the count of the one this run does not use is zeroed for the next run - whoever
    // filled it has finished long ago)
    if (blockIdx.x == 0 && threadIdx.x == 0) *other_count = 0u;
}

// Checking entries (smc_fisher_tables, smc_lfact_values): the device functions above on arguments a test chooses - k_filter_loci only
// ever sees the tallies k_call_v2 wrote.  A wavefront per table, the SAME wave_fisher with the context's table; lane 0 stores.
#define SMC_FISHER_BLOCK 256
__global__ __launch_bounds__(SMC_FISHER_BLOCK) void k_fisher_tables(const long long* __restrict__ tables, long long n, const double* __restrict__ lft,
                                                                    double* __restrict__ orat, double* __restrict__ pval) {
    const long long w = (long long)blockIdx.x * (SMC_FISHER_BLOCK / WAVE) + (threadIdx.x >> 6);
    if (w >= n) return;                                                           // (uniform over the wavefront)
    const long long* T = tables + 4 * w;
    double o, p;
    wave_fisher(lft, T[0], T[1], T[2], T[3], &o, &p);
    if ((threadIdx.x & 63) == 0) { orat[w] = o; pval[w] = p; }
}
// v >= 0: what a Fisher test gets for log(v!) - t_lfact; v < 0: d_lfact(~v), computed whatever the size (the table's entries against
// the series at the same argument)
__global__ void k_lfact_values(const long long* __restrict__ v, long long n, const double* __restrict__ lft, double* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = v[i] >= 0 ? t_lfact(lft, v[i]) : d_lfact((double)~v[i]);
}
