// Included by smcounter_hip.hip.
// ------------------------------------------------------------------------------------------
// the limit-of-detection table of --lod (reference: mt_depths_lod.R:24-39; host restatement: smcounter_amd/tools/mt_depths_lod.py)
// ------------------------------------------------------------------------------------------
// LOD(needed, d) = the root on [0, 1] of f(p) = pbinom(needed - 1, d, p) - 0.05, found the way R's uniroot finds it: R_zeroin2
// (Brent) at tol = DBL_EPSILON^0.25 = 2^-13, maxit 1000.  The value depends on (needed, d) alone, both integers: a table over
// d = 0 .. max_depth per `needed`, one lane per depth.  R then rounds to 4 decimals, so which of the finder's iterates is returned
// matters: lod_zeroin follows tools.mt_depths_lod.zeroin operation for operation (same swaps, same comparisons, same order of the
// arithmetic; the library is built with -ffp-contract=off and no fast-math, FP64 division is IEEE), and the rounding is left to
// the host so that device and tool can differ through the root only.
//
// pbinom(k, n, p) for the small k of this use (k = needed - 1 <= a few dozen) is the direct sum of the first k + 1 terms,
// t_0 = (1 - p)^n = exp(n log1p(-p)), t_(i+1) = t_i (n - i) / (i + 1) p / (1 - p): k multiply-divide steps, no incomplete beta.
// Every term is positive, so the sum loses nothing to cancellation; against scipy's incomplete-beta binom.cdf it differs at the
// 1e-13 level (tests/test_lod.py pins the rounded LODs equal).
//
// Lanes of a wavefront stop after different numbers of iterations (6-12 for the depths of a run): accepted - a table is a few
// thousand lanes, nothing here is bandwidth- or issue-bound.  Workgroups of one wavefront, so that a table of 16,000 depths spreads
// over the device's compute units instead of filling 63 of them.
#define LOD_BLOCK 64
#define LOD_MAXIT 1000

__device__ static double lod_pbinom(int k, int n, double p) {
    if (p <= 0.0) return 1.0;
    if (p >= 1.0) return k >= n ? 1.0 : 0.0;
    double t = exp((double)n * log1p(-p));
    double s = t;
    const double r = p / (1.0 - p);
    for (int i = 0; i < k; ++i) {
        t = t * (double)(n - i) / (double)(i + 1) * r;
        s += t;
    }
    return s;
}

// R_zeroin2 as tools.mt_depths_lod.zeroin has it; *iters: passes of the loop begun (LOD_MAXIT + 1: no convergence, root 1.0)
__device__ static double lod_zeroin(int k, int n, double ax, double bx, double fa, double fb, double tol, int* iters) {
    const double EPS = 2.220446049250313e-16;
    double a = ax, b = bx, c = ax, fc = fa;
    *iters = 0;
    if (fa == 0.0) return a;
    if (fb == 0.0) return b;
    for (int it = 1; it <= LOD_MAXIT + 1; ++it) {
        *iters = it;
        const double prev_step = b - a;
        if (fabs(fc) < fabs(fb)) {          // swap so that b is the best approximation
            a = b; b = c; c = a;
            fa = fb; fb = fc; fc = fa;
        }
        const double tol_act = 2 * EPS * fabs(b) + tol / 2;
        double new_step = (c - b) / 2;
        if (fabs(new_step) <= tol_act || fb == 0.0) return b;
        if (fabs(prev_step) >= tol_act && fabs(fa) > fabs(fb)) {
            const double cb = c - b;
            double p, q;
            if (a == c) {                   // linear interpolation
                const double t1 = fb / fa;
                p = cb * t1;
                q = 1.0 - t1;
            } else {                        // inverse quadratic interpolation
                q = fa / fc;
                const double t1 = fb / fc;
                const double t2 = fb / fa;
                p = t2 * (cb * q * (q - t1) - (b - a) * (t1 - 1.0));
                q = (q - 1.0) * (t1 - 1.0) * (t2 - 1.0);
            }
            if (p > 0) q = -q;
            else p = -p;
            if (p < (0.75 * cb * q - fabs(tol_act * q) / 2) && p < fabs(prev_step * q / 2)) new_step = p / q;
        }
        if (fabs(new_step) < tol_act) new_step = new_step > 0 ? tol_act : -tol_act;
        a = b; fa = fb;
        b += new_step;
        fb = lod_pbinom(k, n, b) - 0.05;
        if ((fb > 0 && fc > 0) || (fb < 0 && fc < 0)) { c = a; fc = fa; }
    }
    return 1.0;                             // "no convergence" -> try-error -> 1 (mt_depths_lod.R:34-37)
}

// roots[d], iters[d] for d = 0 .. max_depth: tools.mt_depths_lod.find_lod(d, needed) without its final round(., 4)
__global__ __launch_bounds__(LOD_BLOCK) void k_lod_table(int needed, int max_depth, double* __restrict__ roots, int32_t* __restrict__ iters) {
    const int d = (int)(blockIdx.x * LOD_BLOCK + threadIdx.x);
    if (d > max_depth) return;
    const int k = needed - 1;
    double root = 1.0;
    int it = 0;
    if (d >= 5) {
        const double f_lo = lod_pbinom(k, d, 0.0) - 0.05, f_hi = lod_pbinom(k, d, 1.0) - 0.05;
        if (f_lo * f_hi <= 0) root = lod_zeroin(k, d, 0.0, 1.0, f_lo, f_hi, 0x1p-13 /* DBL_EPSILON^0.25 */, &it);
    }
    roots[d] = root;
    iters[d] = it;
}
