// Included by smcounter_hip.hip: LDS header, DPP reductions, read-class / state encodings, the per-count posterior and
// PCR-term table kernels, the epilogue arithmetic and the E stage (finish_row) of the locus kernel.
// ------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------
struct KParams {
    int min_bq, min_mq, mt_drop, primer_dist, ds;
    double smt;
    int lite_from;   // reference-allele fragments from which a barcode's other alleles get no sequencing-error term (k_call_v2, general path)
    int use_alt;     // k_call_v2: one-allele barcodes of the locus's major OTHER allele are scored from the table too (0: SMC_NO_ALT)
    int tallies_later;   // k_call_v2 leaves the filter-only tallies of the loci it queues to k_filter_tallies (batches with loci of the deep class)
    int simple_to;   // k_call_v2: fragment count from which no barcode takes a shortcut that never forms rightP (the per-count table, `lite`):
                     // <= SMC_SIMPLE_N, lower where rightP can leave the normal double range before that (host_abi.inc, simple_to_for)
};

// header of the per-block LDS image; the tables follow it
struct Hdr {
    uint32_t misc[32];
    uint32_t scan_tmp[32];
};
enum {
    M_NINC = 0,   // some read is included
    M_ERR2,       // barcode read / slot ranges out of order (found after the scan)
    M_ERR,
    M_NBC,        // barcodes with an included read
    M_ALLMT,
    M_TOTFRAG,
    M_MT3, M_MT5, M_MT7, M_MT10,
    M_USEDFRAG,
    M_TOUCH_LO, M_TOUCH_HI,
    M_CVG,
    M_NEEDFIX,
    M_NCOMPLEX,   // barcodes deferred to the general calProb path
    M_NKEPT,      // bcDict keys the host's down-sampling kept (SMC_LF_SAMPLED loci)
    M_SEGFIT,     // (k_call_v2 uses this slot as M_NKEYS_BEFORE)
    M_UNDERFLOW,  // barcodes whose calProb products left the normal double range (SMC_ST_UNDERFLOW)
};

#define NT_K1 11  // tallies kept per allele in LDS: the SMC_T_* of the header, without the pad

__device__ __forceinline__ uint32_t lds_hdr_bytes(int a_cap) {
    // Hdr + tal[a_cap][SMC_NT] + pifx[a_cap] (u64) + mtc[a_cap] + strong[a_cap] + lut[LUT_N] doubles
    // (the row is staged over the LUT, which is dead by then)
    return (uint32_t)(sizeof(Hdr) + a_cap * SMC_NT * 4 + a_cap * 8 + a_cap * 4 + a_cap * 4 + 128 * 8 + 32 * 8);
}

// ---- reductions through DPP (one VALU instruction per step, no LDS round trip, unlike __shfl = ds_bpermute).
// Callers keep whole 8-lane groups (grp8_*) or the whole wavefront (wave_*) active.
#define DPP_XOR1 0xB1          // quad_perm:[1,0,3,2]
#define DPP_XOR2 0x4E          // quad_perm:[2,3,0,1]
#define DPP_HALF_MIRROR 0x141  // lane i <- lane 7-i of its 8
#define DPP_MIRROR 0x140       // lane i <- lane 15-i of its row
template <int CTRL>
__device__ __forceinline__ int dpp_i32(int v) { return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xF, 0xF, false); }
template <int CTRL>
__device__ __forceinline__ double dpp_f64(double v) {
    return __hiloint2double(dpp_i32<CTRL>(__double2hiint(v)), dpp_i32<CTRL>(__double2loint(v)));
}
template <int CTRL>
__device__ __forceinline__ long long dpp_i64(long long v) {
    return (long long)(((unsigned long long)(uint32_t)dpp_i32<CTRL>((int)(v >> 32)) << 32) | (uint32_t)dpp_i32<CTRL>((int)v));
}
__device__ __forceinline__ int grp8_add(int v) { v += dpp_i32<DPP_XOR1>(v); v += dpp_i32<DPP_XOR2>(v); v += dpp_i32<DPP_HALF_MIRROR>(v); return v; }
__device__ __forceinline__ uint32_t grp8_or(uint32_t v) {
    v |= (uint32_t)dpp_i32<DPP_XOR1>((int)v); v |= (uint32_t)dpp_i32<DPP_XOR2>((int)v); v |= (uint32_t)dpp_i32<DPP_HALF_MIRROR>((int)v);
    return v;
}
__device__ __forceinline__ double grp8_mul(double v) { v *= dpp_f64<DPP_XOR1>(v); v *= dpp_f64<DPP_XOR2>(v); v *= dpp_f64<DPP_HALF_MIRROR>(v); return v; }
// whole-wavefront totals, returned wave-uniform (row totals by DPP, the four rows added on the scalar unit)
__device__ __forceinline__ int wave_add(int v) {
    v = grp8_add(v); v += dpp_i32<DPP_MIRROR>(v);
    return __builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16) + __builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48);
}
__device__ __forceinline__ uint32_t wave_or(uint32_t v) {
    v = grp8_or(v); v |= (uint32_t)dpp_i32<DPP_MIRROR>((int)v);
    return (uint32_t)(__builtin_amdgcn_readlane((int)v, 0) | __builtin_amdgcn_readlane((int)v, 16) | __builtin_amdgcn_readlane((int)v, 32) | __builtin_amdgcn_readlane((int)v, 48));
}
__device__ __forceinline__ long long wave_add64(long long v) {
    v += dpp_i64<DPP_XOR1>(v); v += dpp_i64<DPP_XOR2>(v); v += dpp_i64<DPP_HALF_MIRROR>(v); v += dpp_i64<DPP_MIRROR>(v);
    long long t = 0;
#pragma unroll
    for (int r = 0; r < 64; r += 16)
        t += (long long)(((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(v >> 32), r) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)v, r));
    return t;
}

#define KEY_ALLELE(k) (((k) >> 8) & 63u)
// read-class table entry (two words): nine 5-bit tally increments in SMC_T_* order (six in .x, three in .y),
// .y bit 31 = the read enters bcDict (incCond), bit 30 = the class exists.  (In-deletion reads need nothing special
// here: the batch carries minBQ as their quality, smCounter.py:418.)
#define CLS_INC 0x80000000u
// fragment state word handed to the calProb code: present | paired | allele << 8 | probability index.  The index is the
// merged quality of a 'Paired' fragment (error prob 10^(-q/10)) or PIDX_UNPAIRED for a single read (prob forced to 0.1,
// smCounter.py:67-68); qualities are <= 126 by the batch contract (a BAM holds 0..93) and clamped to that.
#define PIDX_UNPAIRED 127u
#define XS_PRESENT 0x20000000u
#define XS_PAIRED 0x10000000u
__device__ __forceinline__ uint32_t make_xstate(int allele, int bq, bool paired) {
    return XS_PRESENT | (paired ? XS_PAIRED : 0u) | ((uint32_t)allele << 8) | (uint32_t)bq;
}

// 10^x in double.  The LUT of 10^(-q/10) is computed on the host with the same libm the CPU restatement uses; the
// PCR-error terms use the device library's exp10 (tabulated once per context, k_pcr_table), the final -log10 the routine
// below (a few ulp from glibc's pow/log10: invisible at the 1e-6 tolerance on PI, and symmetric across alleles so exact
// ties between alleles stay exact).
__device__ __forceinline__ double pcr_of(int cnt, double denom) { return exp10(-6.0 * ((cnt + 0.5) / denom)); }

// a / b for normal, positive b without the IEEE division's scaling and fix-up steps (~ 8 instructions instead of ~ 35):
// hardware reciprocal seed, two Newton steps, one residual correction - within an ulp or so of the quotient, far inside
// the 1e-6 budget on PI; every lane runs the same sequence, so equal inputs still give bit-equal outputs (the exact-tie
// test of smCounter.py:514 stays symmetric across alleles).
__device__ __forceinline__ double fast_div(double a, double b) {
    double r = __builtin_amdgcn_rcp(b);
    r = fma(fma(-b, r, 1.0), r, r);
    r = fma(fma(-b, r, 1.0), r, r);
    const double q = a * r;
    return fma(fma(-b, q, a), r, q);
}
// -log10(x) for a normal x in (0, 1] (what 1 - posterior is, smCounter.py:508-510): the classic reduction
// x = m 2^e, m in [sqrt(1/2), sqrt(2)), log m = f - (f^2/2 - s (f^2/2 + R(s^2))) with s = f / (2 + f), f = m - 1 and the
// degree-14 odd remainder R (coefficients of the public fdlibm e_log.c minimax fit, error < 2^-58) - about 45
// instructions instead of the device library's general log10 (~ 110: it also serves zero, infinities, subnormals and
// negative arguments, none of which can come here).
__device__ __forceinline__ double neg_log10_unit(double x) {
    double m = __builtin_amdgcn_frexp_mant(x);                       // [0.5, 1)
    int e = __builtin_amdgcn_frexp_exp(x);
    const bool low = m < 0.70710678118654752440;
    m = low ? m + m : m;
    e = low ? e - 1 : e;
    const double f = m - 1.0;
    const double s = fast_div(f, 2.0 + f);
    const double z = s * s, w = z * z;
    const double t1 = w * (3.999999999940941908e-01 + w * (2.222219843214978396e-01 + w * 1.531383769920937332e-01));
    const double t2 = z * (6.666666666666735130e-01 + w * (2.857142874366239149e-01 + w * (1.818357216161805012e-01 + w * 1.479819860511658591e-01)));
    const double hfsq = 0.5 * f * f;
    const double logm = f - (hfsq - s * (hfsq + (t2 + t1)));
    // -(e ln 2 + log m) / ln 10, the exponent part split so that e * (high part) is exact
    return -(fma((double)e, 3.01029995663611771306e-01, (double)e * 3.69423907715893078616e-13) + logm * 4.34294481903251827651e-01);
}

#define LUT_N 128
// Predicates are kept as 64-bit lane masks: a ballot of a single compare is one v_cmp into an SGPR
// pair, combinations are scalar ANDs, "counter += predicate" is one v_addc_co_u32 with the mask as
// carry-in, and a branch on a mask is s_and_saveexec (inverse ballot) - no per-lane 0/1 integers.
typedef unsigned long long lmask;
#define BAL(x) __builtin_amdgcn_ballot_w64(x)
#define LANES(m) __builtin_amdgcn_inverse_ballot_w64(m)


// calProb for a barcode whose fragments all show ONE allele (the common case) depends only on the fragment
// count nf: prodP[allele] == rightP bit for bit (same factors, same order), so rightP cancels in the posterior
// (smCounter.py:83-96) and   post(allele) = (pne + pcr(0)) / (pne + pcr(0) + 3 pcr(nf)),  post(pad) = pcr(nf) / (same)
// with pcr(c) = 10^(-6 (c + .5) / (nf + 2))  (:79-81, |uniqBase| = 4).  The two -log10(1 - post) values are
// tabulated once per context for nf < SMC_SIMPLE_N by the device code below; larger barcodes take the general path.
// (The cancellation holds while rightP is a normal double: where minBQ is so low that rightP can underflow below SMC_SIMPLE_N
// fragments, KParams.simple_to sends such barcodes to the general path too, which follows the products down and flags the row.)
#define SMC_SIMPLE_N 4096
__global__ void k_simple_table(double* __restrict__ out, int n) {
    const int nf = blockIdx.x * blockDim.x + threadIdx.x;
    if (nf >= n) return;
    const double pne = 1.0 - 3e-5;
    double pred0 = 0.0, predpad = 0.0;
    if (nf > 0) {
        const double denom = nf + 2.0;
        const double pcr_self = pcr_of(nf, denom), pcr_zero = pcr_of(0, denom);
        const double tmp0 = pne + pcr_zero, padOut = pcr_self;
        double sumP = tmp0;
        sumP += padOut; sumP += padOut; sumP += padOut;
        const double post0 = tmp0 / sumP, postp = padOut / sumP;
        const double x0 = 1.0 - post0;
        pred0 = x0 > 0.0 ? -log10(x0) : 16.0;                         // :508-510
        // -log10(1 - t) for the padded keys: t is tiny, the series is exact to < 1e-19 below 1e-6
        if (postp < 1e-6) predpad = postp * (1.0 + postp * (0.5 + postp * (1.0 / 3.0))) * 0.43429448190325182765;
        else { const double xp = 1.0 - postp; predpad = xp > 0.0 ? -log10(xp) : 16.0; }
    }
    out[2 * nf] = pred0;
    out[2 * nf + 1] = predpad;
}

// PCR-error term 10^(-6 (c + .5) / (nf + 2)) (smCounter.py:79-81 with |uniqBase| = 4, the case of every barcode with at
// most four alleles) for nf, c < SMC_PCR_N, tabulated once per context by the same device code that computes it on the
// fly (pcr_of): a lookup gives the bit-identical value and spares the general path its exp10 (~ 90 FP64 instructions).
#define SMC_PCR_N 128
__global__ void k_pcr_table(double* __restrict__ out) {
    const int nf = blockIdx.x, c = threadIdx.x;
    out[nf * SMC_PCR_N + c] = pcr_of(c, nf + 2.0);
}

// ---- fixed-point PI sums: value * 2^shift as 64-bit integers (order-independent adds).  Conversions are spelled
// out (5 / 3 instructions) instead of the generic 64-bit casts (~ 50 each).
__device__ __forceinline__ long long to_fx(double pred, double fxscale) {
    const double t = pred * fxscale + 0.5;                   // in [0, 2^53): pred <= 16, shift <= 48
    const double hi_d = floor(t * 0x1p-32);
    const uint32_t hi = (uint32_t)hi_d, lo = (uint32_t)fma(hi_d, -0x1p32, t);
    return (long long)(((unsigned long long)hi << 32) | lo);
}
__device__ __forceinline__ double from_fx(unsigned long long v, double inv /* 2^-shift */) {
    return fma((double)(uint32_t)(v >> 32), 0x1p32, (double)(uint32_t)v) * inv;   // one rounding, like the cast
}

// ---- E stage shared by both locus kernels: ranking and candidates (smCounter.py:534-555), one thread.
// R points at a zeroed row staged in LDS; misc[] holds the M_* counters.
// Called either by one thread (lane 0, step 1) or by every lane of one wavefront (lane, step 64): the scalar logic
// is then computed redundantly by all lanes (same instructions, same values) and the tally copies are spread over
// the lanes.
__device__ __forceinline__ void finish_row(smc_row* R, const smc_locus& L, int li, int n, int nF, int used, bool downsampled,
                                           double fxscale, const uint32_t* misc, const uint32_t* tal,
                                           const unsigned long long* pifx, const uint32_t* mtc, const uint32_t* strong,
                                           uint32_t* flt_list, int lane, int step) {
    const int nA = L.n_alleles;
    const unsigned long long touched = ((unsigned long long)misc[M_TOUCH_HI] << 32) | misc[M_TOUCH_LO];
    const int nkeys = __popcll(touched);
    const double inv = __longlong_as_double((2046ll << 52) - __double_as_longlong(fxscale));   // 1 / fxscale, a power of two
    auto PI = [&](int a) { return from_fx(pifx[a], inv); };
    // py2 dict slot order of the fixed keys A,T,G,C,N,DEL: 8-slot table (<= 5 keys) / 32-slot table (py2compat.py)
    auto rank = [&](int a) {
        return a < 6 ? (int)(((nkeys <= 5 ? 0x040702060500ull : 0x140F02061500ull) >> (8 * a)) & 0xffull) : 64 + a;
    };
    // top two by (PI desc, rank asc): one pass (a strict total order, so this equals two argmax passes)
    int best = -1, second = -1;
    double vb = 0.0, vs = 0.0;
    int rb = 0, rs = 0;
    for (int a = 0; a < nA; ++a) {
        if (!((touched >> a) & 1ull)) continue;
        const double v = PI(a);
        const int r = rank(a);
        if (best < 0 || v > vb || (v == vb && r < rb)) { second = best; vs = vb; rs = rb; best = a; vb = v; rb = r; }
        else if (second < 0 || v > vs || (v == vs && r < rs)) { second = a; vs = v; rs = r; }
    }
    R->status = (downsampled ? SMC_ST_DOWNSAMPLED : SMC_ST_OK) | (misc[M_UNDERFLOW] ? SMC_ST_UNDERFLOW : 0);
    R->n_touched = nkeys;
    R->cvg = n;
    R->all_frag = nF;
    R->all_mt = misc[M_ALLMT];
    R->used_frag = misc[M_USEDFRAG];
    R->used_mt = used;
    R->mt3 = misc[M_MT3]; R->mt5 = misc[M_MT5]; R->mt7 = misc[M_MT7]; R->mt10 = misc[M_MT10];
    R->max_allele = best; R->second_allele = second;
    R->touched_mask = touched;
    for (int k = lane; k < 4; k += step) {
        R->dp[k] = tal[k * SMC_NT + SMC_T_CNT];
        R->umt[k] = mtc[k];
        R->vsm[k] = strong[k];
        R->pi[k] = PI(k);
    }
    const int ref = L.ref_allele;
    if (ref < nA) for (int k = lane; k < SMC_NT; k += step) R->ref_tal[k] = tal[ref * SMC_NT + k];
    auto fill = [&](smc_cand& C, int a, double pia) {
        C.allele = a;
        C.p_sb = C.p_r1 = C.p_r2 = C.p_pr = NAN;
        if (a < 0) return;
        C.pi = pia;
        C.vdp = tal[a * SMC_NT + SMC_T_CNT];
        C.vmt = mtc[a];
        C.vsm = strong[a];
        for (int k = lane; k < SMC_NT; k += step) C.tal[k] = tal[a * SMC_NT + k];
    };
    auto filterable = [&](int a) { return ((L.snp_mask >> a) & 1ull) || a != GAP_ID; };  // SNP or INDEL
    const int alt = best == ref ? second : best;                                   // :541
    const double pi_alt = best == ref ? vs : vb;
    fill(R->cand[0], alt, pi_alt);
    const bool flt0 = alt >= 0 && pi_alt >= 5 && filterable(alt);                 // :549
    bool flt1 = false;
    if (flt0) R->cand[0].flt_applied = 1;
    if (best >= 0 && second >= 0 && best != ref && second != ref && 1.0 * mtc[best] / used >= 0.45 &&
        1.0 * mtc[second] / used >= 0.45) {                                        // :553-555
        R->biallelic = 1;
        fill(R->cand[1], second, vs);
        flt1 = vs >= 5 && filterable(second);                                      // :563
        if (flt1) R->cand[1].flt_applied = 1;
    } else {
        fill(R->cand[1], -1, 0.0);
    }
    // loci whose candidate(s) go through filterVariants are queued for k_filter_loci
    if ((flt0 || flt1) && lane == 0) flt_list[1 + atomicAdd(&flt_list[0], 1u)] = (uint32_t)li;
}

