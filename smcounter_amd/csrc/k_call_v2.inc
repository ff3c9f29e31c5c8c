// Included by smcounter_hip.hip.
// ------------------------------------------------------------------------------------------
// kernel 1 (round 2): scan + group + score + rank WITHOUT per-fragment tables
// ------------------------------------------------------------------------------------------
// What the batch contract gives (include/smcounter_hip.h): a locus's reads are barcode-major, one word each (allele,
// quality, "starts a fragment", read class) - a barcode is a contiguous read range [umi_start[u], umi_start[u+1]) and a
// fragment is a run of reads from one fragment-start bit to the next (the dense ascending slot numbers that bit stands
// for are checked where they exist: smc_pack_words).  Nothing has to be looked up by slot: the mate merge (smCounter.py:468-479) of a run is decided from the run's own reads, which
// sit in the same lane's 4-read quad or in the neighbour lane's (DPP wavefront shift).
//
// Per read ONE byte of flags is left in LDS (4 reads = one dword per lane and step, a coalesced ds_write_b32):
//   bit 7 LIVE  the run that ENDS right before this read is a fragment that survives in bcDict (:468-479)
//   bit 6 LREF  ... and it shows the locus's reference allele
//   bit 5 INC   this read is included (incCond, :378)        bit 4 NF   this read starts a new fragment
//   bit 3 L3    the run that ends before this read has >= 3 reads (re-created fragment): replayed sequentially
//   bit 2 PAIR  the surviving fragment is a merged pair (both reads included, :472-476): its quality is the smaller one
// (a run's verdict is written at the position AFTER it: everything it needs lies behind, nothing ahead.)
// The predicates are evaluated four reads at a time as BYTE LANES of one 32-bit register (bit 7 of byte k = read k
// of the quad; the other bits are don't-care until the final mask): gathers by v_perm_b32, look-back by
// v_alignbyte_b32 over the neighbour lane's register, equality by the carry-free zero-byte test
// (x + 0x7f7f7f7f, bytes < 0x80), combinations by plain bitwise VALU - no compare, no scalar mask work per read.
// Round 1's kernel spent ~50 vector and ~27 scalar instructions per read on the same decisions (one LDS atomicMax per
// read into a 4-byte-per-fragment table, a second pass over that table); this one ~33 and ~5, and the table, its
// zeroing and the pass over it are gone.
//
// A barcode is then scored by one lane: live fragments = popcount of LIVE over its positions, "all show the reference
// allele" = the same count of LREF -> the per-count posterior table (device_common.inc, k_simple_table); the others
// (15 % on C3) are queued and walked by 8 lanes each, the fragment states rebuilt from the flag bytes + the words
// of the one or two reads that define them.
//
// Deep loci: a workgroup takes its share of the locus's barcodes ("part") in CHUNKS of whole barcodes whose flag bytes
// fit the LDS; everything a chunk produces is additive (tallies, fixed-point PI sums, consensus counts, counters), so
// parts of one locus add their headers into a global accumulator (integer atomics, order-free -> bit-identical rows)
// and the last part to arrive ranks and writes the row.  1000 loci x 58 k reads no longer run as two rounds of 512
// resident workgroups.
// ------------------------------------------------------------------------------------------
#ifndef SMC_ABLATE
#define SMC_ABLATE 0   // diagnostic builds: return after phase N (instruction counts only, rows are garbage)
#endif
#ifndef SMC_ALT_FROM_READS
#define SMC_ALT_FROM_READS 24576  // loci of more reads than this - the deep class - look for their major other allele (k_call_v2); measured at
                                   // 8192: the 64 sampled lines cost loci of 12-20 k reads without a variant 3 %
#endif
#ifndef SMC_GC
#define SMC_GC 8         // lanes per queued barcode in the general calProb path (4: measured below)
#endif
#ifndef SMC_V2_WAVES
#define SMC_V2_WAVES 6
#endif
#define FLB_LIVE 0x80u
#define FLB_LREF 0x40u
#define FLB_INC 0x20u
#define FLB_NF 0x10u
#define FLB_L3 0x08u
#define FLB_PAIR 0x04u
#define FLB_LALT 0x02u   // ... and it shows the locus's major other allele (guessed from a sample of the locus: `alta` below)
#define CLS_VALID 0x40000000u      // class table, second word bit 30: the class exists
#define M_NKEYS_BEFORE M_SEGFIT    // (misc slot) bcDict keys counted in the chunks before this one (down-sampling stand-in)

struct V2Part {
    int32_t li;      // locus (batch index)
    int32_t part;    // this workgroup's share: barcodes [nU * part / nparts, nU * (part + 1) / nparts)
    int32_t nparts;
    int32_t acc;     // nparts > 1: index of the locus's global accumulator
};

// accumulator of a multi-part locus in global memory: the additive part of the LDS header, then a ticket
__host__ __device__ inline size_t v2_acc_words(int a_cap) { return 32 + (size_t)a_cap * (SMC_NT + 2 + 1 + 1) + 2; }

__device__ __forceinline__ uint32_t gather_b0(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
    const uint32_t t01 = __builtin_amdgcn_perm(x1, x0, 0x0c0c0400u), t23 = __builtin_amdgcn_perm(x3, x2, 0x0c0c0400u);
    return __builtin_amdgcn_perm(t23, t01, 0x05040100u);
}
__device__ __forceinline__ uint32_t gather_b3(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
    const uint32_t t01 = __builtin_amdgcn_perm(x1, x0, 0x0c0c0703u), t23 = __builtin_amdgcn_perm(x3, x2, 0x0c0c0703u);
    return __builtin_amdgcn_perm(t23, t01, 0x05040100u);
}
__device__ __forceinline__ uint32_t gather_b2(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
    const uint32_t t01 = __builtin_amdgcn_perm(x1, x0, 0x0c0c0602u), t23 = __builtin_amdgcn_perm(x3, x2, 0x0c0c0602u);
    return __builtin_amdgcn_perm(t23, t01, 0x05040100u);
}
__device__ __forceinline__ uint32_t gather_b1(uint32_t x0, uint32_t x1, uint32_t x2, uint32_t x3) {
    const uint32_t t01 = __builtin_amdgcn_perm(x1, x0, 0x0c0c0501u), t23 = __builtin_amdgcn_perm(x3, x2, 0x0c0c0501u);
    return __builtin_amdgcn_perm(t23, t01, 0x05040100u);
}
// value of the neighbour lane (lane - 1); lane 0 keeps `old`
__device__ __forceinline__ uint32_t lane_before(uint32_t old, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp((int)old, (int)v, 0x138, 0xF, 0xF, false);
}
// bytes k of a quad with lo <= k < hi as 0xFF
__device__ __forceinline__ uint32_t byte_range(int lo, int hi) {
    const int l = lo < 0 ? 0 : (lo > 4 ? 4 : lo), h = hi < 0 ? 0 : (hi > 4 ? 4 : hi);
    const uint32_t mh = h >= 4 ? 0xFFFFFFFFu : ((1u << (8 * h)) - 1u), ml = l >= 4 ? 0xFFFFFFFFu : ((1u << (8 * l)) - 1u);
    return mh & ~ml;
}

template <int G> __device__ __forceinline__ int grpN_add(int v) {
    v += dpp_i32<DPP_XOR1>(v); v += dpp_i32<DPP_XOR2>(v);
    if (G == 8) v += dpp_i32<DPP_HALF_MIRROR>(v);
    return v;
}
template <int G> __device__ __forceinline__ uint32_t grpN_or(uint32_t v) {
    v |= (uint32_t)dpp_i32<DPP_XOR1>((int)v); v |= (uint32_t)dpp_i32<DPP_XOR2>((int)v);
    if (G == 8) v |= (uint32_t)dpp_i32<DPP_HALF_MIRROR>((int)v);
    return v;
}
template <int G> __device__ __forceinline__ double grpN_mul(double v) {
    v *= dpp_f64<DPP_XOR1>(v); v *= dpp_f64<DPP_XOR2>(v);
    if (G == 8) v *= dpp_f64<DPP_HALF_MIRROR>(v);
    return v;
}

// Flag bytes of a chunk live in LDS, or - for ONE barcode with more reads than the LDS holds flags for - in global scratch.  Explicit
// branches on the (uniform) switch: a merged pointer would turn every access into a flat_ one.
typedef __attribute__((address_space(3))) unsigned char lds_u8;
typedef __attribute__((address_space(3))) uint32_t lds_u32;
struct FlagBytes {
    lds_u32* lds;        // [fcap] flag dwords (typed as LDS: ds_ instructions, not flat_)
    uint32_t* glob;      // nullptr: LDS; else the flag dwords of the chunk in global scratch
    int fbase;           // position of byte 0 (4 * first quad of the chunk)
    __device__ __forceinline__ uint32_t byte_at(uint32_t i) const {
        if (__builtin_expect(glob != nullptr, 0)) return (uint32_t)((const unsigned char*)glob)[i - (uint32_t)fbase];
        return (uint32_t)((const lds_u8*)lds)[i - (uint32_t)fbase];
    }
    __device__ __forceinline__ uint32_t word_at(int d) const {
        if (__builtin_expect(glob != nullptr, 0)) return glob[d];
        return lds[d];
    }
    __device__ __forceinline__ void store_word(int d, uint32_t fw) const {
        if (__builtin_expect(glob != nullptr, 0)) glob[d] = fw; else lds[d] = fw;
    }
    __device__ __forceinline__ void store_byte(uint32_t i, uint32_t v) const {
        if (__builtin_expect(glob != nullptr, 0)) ((unsigned char*)glob)[i - (uint32_t)fbase] = (unsigned char)v; else ((lds_u8*)lds)[i - (uint32_t)fbase] = (unsigned char)v;
    }
};

// The run that ends before position i, replayed read by read in pileup order (smCounter.py:468-479): the exact path for a
// read name with three or more alignments on the locus (rare; kept out of line).  Returns the fragment's state word.
// (allele, quality) of read x in the low half of a 32-bit word, whichever form the read words have
__device__ __forceinline__ uint32_t v2_word_aq(const uint32_t* __restrict__ meta, uint32_t x, bool w16) {
    if (!w16) return meta[x];
    const uint32_t h = ((const uint16_t*)meta)[x];
    return (h & 15u) | ((h >> 8) & 63u) << 8;
}
__device__ __noinline__ uint32_t v2_replay_run(FlagBytes fb, const uint32_t* __restrict__ meta, bool w16, uint32_t rc0, uint32_t i, uint32_t* tal /* or null */) {
    uint32_t j = i - 1;
    while (j > rc0 && !(fb.byte_at(j) & FLB_NF)) --j;
    bool present = false, paired = false;
    uint32_t sa = 0, sq = 0;
    for (uint32_t x = j; x < i; ++x) {
        if (!(fb.byte_at(x) & FLB_INC)) continue;
        const uint32_t mw = v2_word_aq(meta, x, w16);
        const uint32_t a = mw & 0xffu;
        uint32_t q = (mw >> 8) & 0xffu;
        q = q < PIDX_UNPAIRED ? q : PIDX_UNPAIRED - 1u;
        if (!present) { present = true; paired = false; sa = a; sq = q; }
        else if (a == sa || a == (uint32_t)N_ID) {
            sq = q < sq ? q : sq; paired = true;
            if (a == sa && tal) atomicAdd(&tal[a * SMC_NT + SMC_T_CONCORD], 1u);
        } else {
            present = false;
            if (tal) atomicAdd(&tal[a * SMC_NT + SMC_T_DISCORD], 1u);
        }
    }
    return present ? make_xstate((int)sa, paired ? (int)sq : (int)PIDX_UNPAIRED, paired) : 0u;
}

// The eight per-allele tallies that only filterVariants reads (forwardCnt / reverseCnt, lowQReads, the end-distance counts:
// smCounter.py:386-389, :408-411, :428-457 - SMC_T_FWD .. SMC_T_R2PRLE) for the reference allele and the locus's candidate(s):
// taken by the workgroup that has just ranked the locus, in one more pass over its reads (from L2 / the infinity cache: it has
// just streamed them), and only when a candidate goes on to the filters (altPI >= 5, :549) - the scan does not count them
// for the loci that never get there.  Every read of the pileup counts (the tallies precede UMI grouping and down-sampling).
// want[s] < 0: nobody.  Adds into tal[want[s]][1..8] (LDS).  Packed like the scan's own counts used to be: nine 5-bit
// fields per read in two words, widened after every step of 16 reads into 10-bit fields, summed over the wavefront when those fill.
// (The function is not inlined and its pointer parameters are generic: left so, every load below is a flat_ one with a full
// s_waitcnt behind it - the class table's sixteen look-ups per step one after the other, the quads' loads not in flight together.
// The pointers are re-typed to their address spaces on entry: global_load / ds_read, and the loads of a step overlap.  Measured:
// no difference on any shape, nor from asking for the next step's quads before counting this step's - by timestamps the pass
// is 5 us of a 3,000-read locus's 58 and 11 us of a 58,000-read locus's 57.)
typedef uint32_t v2_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t v2_u32x2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) const v2_u32x4 glb_cu32x4;
typedef __attribute__((address_space(3))) const v2_u32x2 lds_cu32x2;
template <int BLOCK, int NS /* alleles wanted: 2 (reference + candidate) or 3 */, bool W16 /* 16-bit read words; cls_lut is then indexed by smc_class16's code */,
          bool LATER /* called by k_filter_tallies: an instantiation of its own - a function is compiled for the loosest register budget among its
                        callers, and the locus kernel's copy must fit the locus kernel's (shared, it took k_call_v2<64> from 80 to 99 registers) */>
__device__ __noinline__ void v2_filter_tallies(const int tid /* 0 .. BLOCK - 1: the thread's place among those that share the pass */,
                                               const uint32_t* __restrict__ meta /* the read words (global) */, int n, int qa, int qb /* quads [qa, qb) of the locus */,
                                               int w0, int w1, int w2, const uint2* cls_lut_generic /* LDS */, uint32_t* tal /* LDS: [3][SMC_NT], one set per wanted allele */) {
    glb_cu32x4* const meta4 = (glb_cu32x4*)meta;
    typedef __attribute__((address_space(1))) const v2_u32x2 glb_cu32x2;
    glb_cu32x2* const meta2 = (glb_cu32x2*)meta;                      // (16-bit words: a quad of reads is 8 bytes)
    lds_cu32x2* const cls_lut = (lds_cu32x2*)cls_lut_generic;
    const int lane = tid & 63;
    const int want[3] = {w0, w1, w2};
    uint32_t a0[3] = {0, 0, 0}, a1[3] = {0, 0, 0}, wa[3] = {0, 0, 0}, wb[3] = {0, 0, 0}, wc[3] = {0, 0, 0};
    int widenings = 0;
    auto widen = [&]() {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            wa[s] += a0[s] & 0x01F07C1Fu;                              // fields 0, 2, 4 at bits 0, 10, 20
            wb[s] += (a0[s] >> 5) & 0x01F07C1Fu;                       // fields 1, 3, 5
            wc[s] += (a1[s] & 0x00007C1Fu) + (((a1[s] >> 5) & 31u) << 20);   // fields 6, 8 at bits 0, 10; field 7 at bit 20
            a0[s] = a1[s] = 0u;
        }
    };
    auto flush = [&]() {
        widen();
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (want[s] < 0) continue;                                 // (block-uniform)
            const uint32_t p01 = (wa[s] & 1023u) | ((wb[s] & 1023u) << 16), p23 = ((wa[s] >> 10) & 1023u) | (((wb[s] >> 10) & 1023u) << 16),
                           p45 = ((wa[s] >> 20) & 1023u) | (((wb[s] >> 20) & 1023u) << 16), p67 = (wc[s] & 1023u) | (((wc[s] >> 20) & 1023u) << 16),
                           p8 = (wc[s] >> 10) & 1023u;
            const uint32_t sv[5] = {(uint32_t)wave_add((int)p01), (uint32_t)wave_add((int)p23), (uint32_t)wave_add((int)p45),
                                    (uint32_t)wave_add((int)p67), (uint32_t)wave_add((int)p8)};
            if (lane == 0) {
                unsigned long long* t64 = (unsigned long long*)(tal + s * SMC_NT);
#pragma unroll
                for (int j = 0; j < 5; ++j) {
                    const unsigned long long v = ((unsigned long long)(sv[j] >> 16) << 32) | (sv[j] & 0xFFFFu);
                    if (v) atomicAdd(&t64[j], v);
                }
            }
            wa[s] = wb[s] = wc[s] = 0u;
        }
        widenings = 0;
    };
    // (the trip count is the WAVE's: the in-loop flush reduces over the wavefront with DPP / readlane, which want every lane
    // there - a lane whose own reads are exhausted keeps stepping with the loads guarded below)
    // Sixteen reads in flight per thread, as four quads (the rows are quad-aligned: the scan's own loads): the pass is a chain of
    // round trips by ONE workgroup - with four single words per step a 58,000-read locus took 28 of them (~ 100 us at the tail
    // of the locus, a fifth of the launch on the example run's shape), a 3,000-read locus 12.
    const int n4 = qb;
    constexpr int NQ = 4;
    for (int q0 = qa + tid; q0 - lane < n4; q0 += NQ * BLOCK) {
        v2_u32x4 mq[NQ];
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int q = q0 + j * BLOCK;
            if (W16) { const v2_u32x2 h = q < n4 ? meta2[q] : (v2_u32x2){0u, 0u}; mq[j] = (v2_u32x4){h.x, h.y, q < n4 ? 1u : 0u, 0u}; }
            else mq[j] = q < n4 ? meta4[q] : (v2_u32x4){0xFFu, 0xFFu, 0xFFu, 0xFFu};   // (allele 255: nobody's)
        }
#pragma unroll
        for (int j = 0; j < NQ; ++j) {
            const int i = 4 * (q0 + j * BLOCK);
            uint32_t mw[4];                                                 // (the row's last quad may run past n)
            if (W16) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {                                 // -> allele in bits 0-7, smc_class16's code where the class is
                    const uint32_t h = ((k < 2 ? mq[j].x : mq[j].y) >> (16 * (k & 1))) & 0xFFFFu;
                    mw[k] = (mq[j].z && i + k < n) ? (h & 15u) | (((h >> 5) & 1u) << 4 | ((h >> 6) & 3u) | ((h >> 14) & 3u) << 2) << SMC_RW_CLASS_SHIFT : 0xFFu;
                }
            } else { mw[0] = mq[j].x; mw[1] = i + 1 < n ? mq[j].y : 0xFFu; mw[2] = i + 2 < n ? mq[j].z : 0xFFu; mw[3] = i + 3 < n ? mq[j].w : 0xFFu; }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int a = (int)(mw[k] & 0xffu);
                const v2_u32x2 cw = cls_lut[mw[k] >> SMC_RW_CLASS_SHIFT];
#pragma unroll
                for (int s = 0; s < NS; ++s) {
                    const uint32_t m = a == want[s] ? 0xFFFFFFFFu : 0u;
                    a0[s] += cw.x & 0xFFFFFFE0u & m;                   // (field 0, alleleCnt, is the scan's)
                    a1[s] += cw.y & 0x7FFFu & m;
                }
            }
        }
        if (++widenings == 63) flush(); else widen();                  // (16 reads a step: the 5-bit fields hold them, the 10-bit ones 63 steps)
    }
    flush();
}

template <int BLOCK, bool W16 /* g_words holds 16-bit read words (smc_read_word16) */>
// (wavefronts per SIMD the register budget is set for: 6 for the one-wavefront workgroup, 7 for two wavefronts - measured:
// C5 5 % faster at 7, C3 1 % slower; 8 costs 10 % in spills everywhere)
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(BLOCK == 128 ? SMC_V2_WAVES + 1 : SMC_V2_WAVES, 8))) void k_call_v2(
    KParams P, const smc_locus* __restrict__ desc /* the loci's descriptors in launch order: one per workgroup */,
    const V2Part* __restrict__ parts, int a_cap, int fcap /* flag dwords */,
    int ucap /* barcodes per chunk */, const uint32_t* __restrict__ g_words, const uint32_t* __restrict__ g_umi_start,
    const double* __restrict__ g_lut, const double* __restrict__ g_simple,
    const double* __restrict__ g_pcr,
    smc_row* __restrict__ rows, uint32_t* __restrict__ g_acc, uint32_t* __restrict__ g_flags, const int64_t* __restrict__ g_flags_off,

    uint32_t* __restrict__ flt_list,
    const uint32_t* __restrict__ launch_n /* a plan made without the host (smc_plan_create_dev_spec): the workgroups of this launch that have
                                            work - the grid is an upper bound; else null */) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (launch_n != nullptr && blockIdx.x >= *launch_n) return;
    constexpr int NW = BLOCK / WAVE;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);      // wave-uniform, and the compiler should know it
    // ---- carve LDS: header + accumulators (live across chunks), LUTs, then the chunk's tables
    Hdr* H = (Hdr*)smem;
    uint32_t* tal = (uint32_t*)(smem + sizeof(Hdr));                 // [a_cap][SMC_NT]
    unsigned long long* pifx = (unsigned long long*)(tal + a_cap * SMC_NT);
    uint32_t* mtc = (uint32_t*)(pifx + a_cap);
    uint32_t* strong = mtc + a_cap;
    double* lut = (double*)(strong + a_cap);                         // [LUT_N]
    smc_row* rowst = (smc_row*)lut;                                   // row stage: over the LUT once it is dead
    uint2* cls_lut = (uint2*)(lut + LUT_N);                           // [32] read class -> tally increments / flags
    uint32_t* fl_lds = (uint32_t*)(smem + lds_hdr_bytes(a_cap));      // [fcap] one flag dword per quad of the chunk
    uint32_t* ur = fl_lds + fcap;                                 // [ucap + 1] first read of each barcode of the chunk (umi_start)
    uint16_t* worklist = (uint16_t*)(ur + (ucap + 1));                // [ucap] barcodes queued for the general calProb path
    uint16_t* bcinfo = worklist + ucap;                               // [ucap] fragment count of a one-allele barcode still to score
    unsigned char* umi_flag = (unsigned char*)(bcinfo + ucap);        // [ucap] bit 0: kept key of bcDict

    // The tables first: their loads depend on nothing and are in flight with the list entry's and the descriptor's; they go to
    // LDS while the descriptor is still on its way.  (Left below the first use of the descriptor they were issued after it had
    // arrived: two round trips at the head of every workgroup instead of one.)
    constexpr int LUT_PER = (LUT_N + BLOCK - 1) / BLOCK;
    double lutv[LUT_PER];
    uint2 clsv = make_uint2(0u, 0u);
#pragma unroll
    for (int k = 0; k < LUT_PER; ++k) { const int i = tid + k * BLOCK; lutv[k] = i < LUT_N ? g_lut[i] : 0.0; }
    if (tid < 32) clsv = ((const uint2*)(g_lut + (W16 ? 288 : 256)))[tid];   // (the class table in smc_read_class's numbering, then in smc_class16's)
    const V2Part pt = parts[blockIdx.x];
    const int li = pt.li;
    const smc_locus L = desc[blockIdx.x];                            // (a copy in launch order: no load that waits for the load of `li`)
#pragma unroll
    for (int k = 0; k < LUT_PER; ++k) { const int i = tid + k * BLOCK; if (i < LUT_N) lut[i] = i == (int)PIDX_UNPAIRED ? 0.1 : lutv[k]; }
    if (tid < 32) cls_lut[tid] = clsv;
    const int n = L.n_reads, nU = L.n_umi, nF = L.n_frag, nA = L.n_alleles;
    // one word per read (smc_read_word / smc_read_word16): allele, quality, fragment start, class
    const uint32_t* meta = W16 ? (const uint32_t*)((const uint16_t*)g_words + 4ll * L.read_off4) : g_words + 4ll * L.read_off4;
    const uint32_t* ustart = g_umi_start + L.umi_off;
    const uint4* meta4 = (const uint4*)meta;
    const uint2* meta2 = (const uint2*)meta;                         // (16-bit words: a quad of reads)

    const bool sampled = (L.flags & SMC_LF_SAMPLED) != 0;
    // More barcodes than ds without the host's marks: the (non-parity) stand-in keeps the ds lowest barcode ids that are
    // keys of bcDict - a running count over the WHOLE locus, so one workgroup takes it alone, chunk after chunk.
    const bool standin = nU > P.ds && !sampled;
    int u0 = (int)((long long)nU * pt.part / pt.nparts), u1 = (int)((long long)nU * (pt.part + 1) / pt.nparts);
    const bool solo = pt.nparts == 1 || standin;
    if (pt.nparts > 1 && standin) {
        if (pt.part != 0) return;
        u0 = 0; u1 = nU;
    }
    smc_row* out = rows + li;

    // ---- the locus's major OTHER allele, guessed from 64 reads spread over the locus (every part and chunk of a deep locus
    // samples the same reads): barcodes whose live fragments all show it are one-allele barcodes like the reference's - calProb's
    // posteriors of a one-allele barcode depend on its fragment count only, whatever the allele (rightP cancels, :83-96) - and
    // are scored from the same table.  At a locus with a 10-30 % variant that is most of what the general path would otherwise
    // walk.  A wrong or missing guess costs nothing but the shortcut.  (Requested here, beside the table loads.)
    // Only for deep loci: the sampled reads are one 128-byte line each - 8 KB more per locus, nothing beside the 230 KB of a
    // 58,000-read locus but two thirds of a 3,000-read locus's own bytes (measured: + 4 % on C3 with 64 samples everywhere,
    // + 3 % on 12,000-20,000-read loci without a variant).
    uint32_t alt_w = 0xFFFFFFFFu;
    constexpr bool ALT_OK = BLOCK >= 512;                            // (loci of that depth run in workgroups of 512 threads: the other
                                                                     // instantiations carry none of this)
    const int n_samp = (ALT_OK && P.use_alt && n > SMC_ALT_FROM_READS) ? (n / 256 < 64 ? n / 256 : 64) : 0;
    if (ALT_OK && lane < n_samp) alt_w = v2_word_aq(meta, (uint32_t)((long long)lane * n / (n_samp > 0 ? n_samp : 1)), W16);
    // ---- S0 (once): zero the header and the accumulators, load the LUTs
    {
        uint32_t* z = (uint32_t*)smem;
        const int nz = (int)((sizeof(Hdr) + a_cap * 64) / 4);
        for (int i = tid; i < nz; i += BLOCK) z[i] = 0;
    }
    __syncthreads();
    if (tid == 0 && nU == 0 && n != 0) H->misc[M_ERR2] = 1;
    uint32_t alta = 255u;                                            // (wave-uniform; the same in every wavefront and part)
    if (ALT_OK) {
        const uint32_t a = alt_w & 0xFFu;
        const bool cand = alt_w != 0xFFFFFFFFu && a != L.ref_allele && a < (uint32_t)nA;
        int best_c = 0;
        for (lmask m = BAL(cand); m; ) {
            const uint32_t a0 = (uint32_t)__builtin_amdgcn_readlane((int)a, __builtin_ctzll(m));
            const lmask same = BAL(cand && a == a0);
            const int c = __popcll(same);
            if (c > best_c || (c == best_c && a0 < alta)) { best_c = c; alta = a0; }
            m &= ~same;
        }
    }
    const bool has_alt = ALT_OK && alta != 255u;

    // bad input, or no read enters bcDict: the Zero_Coverage row (smCounter.py:489-494).  Called by every thread.
    auto special_row = [&](uint32_t status) {
        __syncthreads();
        for (int i = tid; i < (int)(sizeof(smc_row) / 4); i += BLOCK) ((uint32_t*)rowst)[i] = 0u;
        __syncthreads();
        if (tid == 0) {
            smc_row* R = rowst;
            R->status = status;
            R->cvg = n;
            R->all_mt = (uint32_t)nU;
            R->all_frag = nF;
            R->max_allele = R->second_allele = -1;
            for (int k = 0; k < 4; ++k) R->dp[k] = tal[k * SMC_NT + SMC_T_CNT];
            for (int c = 0; c < 2; ++c) {
                R->cand[c].allele = -1;
                R->cand[c].p_sb = R->cand[c].p_r1 = R->cand[c].p_r2 = R->cand[c].p_pr = NAN;
            }
        }
        __syncthreads();
        const uint32_t* src = (const uint32_t*)rowst;
        uint32_t* dst = (uint32_t*)out;
        for (int i = tid; i < (int)(sizeof(smc_row) / 4); i += BLOCK) dst[i] = src[i];
    };

    // fixed-point scale of the PI sums: order-independent, hence bit-reproducible (sized for the most barcodes the locus
    // can use; the same in every part of a locus)
    const int ubound = nU < P.ds ? nU : P.ds;
    int fxbits = 32 - __clz(ubound);
    int fxshift = 58 - fxbits; if (fxshift > 48) fxshift = 48;
    const double fxscale = __longlong_as_double((long long)(1023 + fxshift) << 52);   // 2^shift
    const uint32_t refa = L.ref_allele;
    const double pne = 1.0 - 3e-5;                                 // pcr_no_error, :20
    auto R_of = [&](int u) -> uint32_t { return ustart[u] & ~SMC_USTART_DROPPED; };

    // =====================================================================================================
    // chunks of whole barcodes [cu0, cu1) of this part; reads [rc0, rc1)
    // =====================================================================================================
    const uint32_t cap_reads = 4u * (uint32_t)(fcap - 2);
    for (int cu0 = u0; cu0 < u1;) {
        // ---- chunk bounds (block-uniform): as many whole barcodes as fit the flag array and the per-barcode tables
        const int cand = u1 < cu0 + ucap ? u1 : cu0 + ucap;
        const uint32_t rc0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)R_of(cu0));
        int cu1 = cand;
        uint32_t rc1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)R_of(cand));
        uint32_t* fl_glob = nullptr;
        bool fl_bad = false;
        if (__builtin_expect(rc1 - rc0 > cap_reads && rc0 <= rc1, 0)) {
            // the largest end whose reads still fit: every thread probes candidates, two rounds (umi_start is ascending)
            __syncthreads();
            if (tid == 0) H->scan_tmp[0] = 0u;
            __syncthreads();
            const int span = cand - cu0;                            // candidates cu0 + 1 .. cand
            const int stride = (span + BLOCK - 1) / BLOCK;
            {
                const int c = cu0 + 1 + tid * stride;
                if (c <= cand && R_of(c) - rc0 <= cap_reads) atomicMax(&H->scan_tmp[0], (uint32_t)(c - cu0));
            }
            __syncthreads();
            const int base = (int)H->scan_tmp[0];                   // fits; base + stride does not (or is beyond)
            __syncthreads();
            if (tid < stride) {
                const int c = cu0 + base + tid;
                if (c > cu0 && c <= cand && R_of(c) - rc0 <= cap_reads) atomicMax(&H->scan_tmp[0], (uint32_t)(c - cu0));
            }
            __syncthreads();
            const int fit = (int)H->scan_tmp[0];
            if (fit == 0) {
                // ONE barcode with more reads than the LDS holds flags for: its flag bytes go to the locus's global
                // scratch (1 byte per read, indexed by the absolute quad; same code, L1/L2 instead of LDS)
                cu1 = cu0 + 1;
                if (g_flags) fl_glob = g_flags + g_flags_off[blockIdx.x] + (rc0 >> 2); else fl_bad = true;
            } else {
                cu1 = cu0 + fit;
            }
            rc1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)R_of(cu1));
        }
        if (!(rc0 < rc1 && rc1 <= (uint32_t)n) || (cu0 == 0 && rc0 != 0) || (cu1 == nU && rc1 != (uint32_t)n) || fl_bad ||
            (!fl_glob && rc1 - rc0 > cap_reads)) {
            if (tid == 0) H->misc[M_ERR2] = 1;                       // barcode read ranges out of order / not covering
            break;
        }
        const int qlo = (int)(rc0 >> 2), qend = (int)(rc1 >> 2);    // quads of the chunk, incl. the one holding position rc1
        const int n4 = (n + 3) >> 2;
        const FlagBytes fb{(lds_u32*)fl_lds, fl_glob, 4 * qlo};   // flag byte of read i: fb.byte_at(i)

        // ---- P1: ONE pass over the chunk's reads.  A wavefront step covers 63 new quads; lane 0 re-reads the quad
        // before them (the previous step's last) so that every other lane finds its look-back in the lane before it.
        {
            // the chunk's barcode boundaries are requested now and parked in LDS after the scan (their latency hides behind it)
            const int ncb1 = cu1 - cu0 + 1;
            uint32_t upre[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) upre[j] = tid + j * BLOCK < ncb1 ? ustart[cu0 + tid + j * BLOCK] : 0u;
            // Of the reference's per-allele tallies (smCounter.py:379-459) only alleleCnt is part of every row (DP_x, VDP); the
            // strand / quality / end-distance counts feed filterVariants alone and are taken by k_filter_loci for the loci - and
            // the two or three alleles - that get there.  Here: the reads that show the reference allele are counted per lane,
            // every other read adds one to its own allele's count.
            uint32_t cnt_ref = 0;
            uint32_t errv = 0, incany = 0;
            // (a reference allele that is not a key of the locus, 255, never matches: 64 is no allele id and keeps the
            // zero-byte test carry-free)
            const uint32_t refa4 = (refa < 64u ? refa : 64u) * 0x01010101u;
            const uint32_t alt4 = (has_alt ? alta : 64u) * 0x01010101u;
            const uint32_t KnA = (uint32_t)(0x80 - nA) * 0x01010101u;   // byte + (0x80 - nA) has bit 7 iff byte >= nA (bytes < 0x80)
            const uint32_t K7 = lane ? 0x80808080u : 0u;               // lane 0's quad is counted by the lane that owns it

            auto load_quad = [&](int Q, uint4& M) {
                if (Q >= 0 && Q < n4 && Q <= qend) { if (W16) { const uint2 h = meta2[Q]; M = make_uint4(h.x, h.y, 0u, 0u); } else M = meta4[Q]; }
                else M = make_uint4(0, 0, 0, 0);
            };
            uint4 M;
            load_quad(qlo - 1 + wid * 63 + lane, M);
            for (int Qb = qlo + wid * 63; Qb <= qend; Qb += 63 * NW) {   // Qb: first NEW quad of this wavefront step
                const int Qc = Qb - 1 + lane;
                const uint4 cM = M;
                if (Qb + 63 * NW <= qend) load_quad(Qc + 63 * NW, M);      // prefetch the next step (two ahead: measured, no gain - the scan is VALU-bound)
                const uint32_t m[4] = {cM.x, cM.y, cM.z, cM.w};
                // byte 2 of a word: bit 0 the read starts a new fragment, bit 1 it is included, bit 2 its class is a known one
                // (SMC_RW_NF / _INC / _OK: the class looked up for the scan by whoever made the word)
                uint32_t NF, A, Y;
                if (W16) {                                           // the four low bytes: allele | NF << 4 | INC << 5 (every class exists)
                    const uint32_t lo4 = __builtin_amdgcn_perm(m[1], m[0], 0x06040200u);
                    NF = (lo4 & 0x10101010u) << 3; A = lo4 & 0x0F0F0F0Fu; Y = ((lo4 & 0x20202020u) << 2) | 0x40404040u;
                } else {
                    const uint32_t G2 = gather_b2(m[0], m[1], m[2], m[3]);
                    NF = (G2 & 0x01010101u) << 7;                    // bit 7 of byte k: read k starts a new fragment
                    A = gather_b0(m[0], m[1], m[2], m[3]);           // allele ids
                    Y = ((G2 & 0x02020202u) << 6) | ((G2 & 0x04040404u) << 4);   // bit 7: included, bit 6: class exists
                }
                // interior step: every quad of it lies inside the chunk, behind its first read and before its end
                const bool fast = Qb >= 1 && 4u * (uint32_t)Qb > rc0 && 4u * (uint32_t)(Qb + 62) + 3u < rc1;
                uint32_t IM = 0xFFFFFFFFu, cm = K7;                  // bytes inside the chunk / bit 7 of the positions counted
                if (!fast) {
                    const int i0 = 4 * Qc;
                    const uint32_t RM = byte_range(-i0, n - i0);                          // real reads of the locus
                    IM = byte_range((int)rc0 - i0, (int)rc1 - i0);                        // reads of this chunk
                    const uint32_t EM = byte_range((int)rc0 + 1 - i0, (int)rc1 + 1 - i0); // positions whose verdict is this chunk's
                    cm = K7 & EM;
                    // read 0 and the positions behind the locus's last read start a "new fragment" by definition
                    NF = (NF & RM) | ~RM | (Qc == 0 ? 0xFFu : 0u);
                    Y &= RM;
                    A &= RM;
                }
                // look-back: the same vectors one and two reads earlier (bytes of the lane before fill in from the left)
                const uint32_t NFd = lane_before(NF, NF), Ad = lane_before(A, A), Yd = lane_before(Y, Y);
                const uint32_t n1 = __builtin_amdgcn_alignbyte(NF, NFd, 3), n2 = __builtin_amdgcn_alignbyte(NF, NFd, 2);
                const uint32_t Ap = __builtin_amdgcn_alignbyte(A, Ad, 3), App = __builtin_amdgcn_alignbyte(A, Ad, 2);
                const uint32_t ip = __builtin_amdgcn_alignbyte(Y, Yd, 3), ipp = __builtin_amdgcn_alignbyte(Y, Yd, 2);
                // bit 7 set = NOT equal (x + 0x7f.. carries into bit 7 of a byte iff the byte is non-zero)
                const uint32_t nrefp = (Ap ^ refa4) + 0x7F7F7F7Fu, nrefpp = (App ^ refa4) + 0x7F7F7F7Fu;
                const uint32_t nconc = (Ap ^ App) + 0x7F7F7F7Fu, nisn = (Ap ^ (N_ID * 0x01010101u)) + 0x7F7F7F7Fu;
                // the run that ends before read i (p = i - 1, pp = i - 2), smCounter.py:468-479
                const uint32_t len2 = ~n1 & n2;                      // exactly two reads
                const uint32_t both = ip & ipp;
                const uint32_t bad = both & nconc & nisn;            // second read disagrees and is not 'N': fragment deleted
                const uint32_t pairlive = (ip | ipp) & ~bad;
                const uint32_t firstref = (ipp & ~nrefpp) | (~ipp & ~nrefp);   // the fragment's allele (first included read) is the reference
                uint32_t live = NF & ((n1 & ip) | (len2 & pairlive));
                uint32_t liveref = NF & ((n1 & ip & ~nrefp) | (len2 & pairlive & firstref));
                const uint32_t concT = NF & len2 & both & ~nconc;    // concordPairCnt[a_p] (:475-476)
                const uint32_t discT = NF & len2 & bad;              // discordPairCnt[a_p] (:479)
                const uint32_t l3 = NF & ~n1 & ~n2;                  // three or more reads in the run
                uint32_t OUT = (live & 0x80808080u) | ((liveref >> 1) & 0x40404040u) | ((Y >> 2) & 0x20202020u) | ((NF >> 3) & 0x10101010u) |
                               (((NF & len2 & both & ~bad) >> 5) & 0x04040404u);
                if (has_alt) {                                       // (block-uniform) LALT, as LREF with the other allele
                    const uint32_t naltp = (Ap ^ alt4) + 0x7F7F7F7Fu, naltpp = (App ^ alt4) + 0x7F7F7F7Fu;
                    const uint32_t firstalt = (ipp & ~naltpp) | (~ipp & ~naltp);
                    const uint32_t livealt = NF & ((n1 & ip & ~naltp) | (len2 & pairlive & firstalt));
                    OUT |= (livealt >> 6) & 0x02020202u;
                }
                // (the pair counts are read by the DP filter for a CANDIDATE allele only, :207: the pairs of the reference allele -
                // nearly all - are not counted; those of any other allele go to its tallies below)
                const uint32_t rare = (((concT | discT) & nrefp) | l3) & cm;
                if (__builtin_expect(rare != 0u, 0)) {
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const uint32_t bit = 0x80u << (8 * k);
                        if (rare & bit) {
                            const uint32_t a = (Ap >> (8 * k)) & 0xffu;
                            if (l3 & bit) { OUT |= (uint32_t)FLB_L3 << (8 * k); H->misc[M_NEEDFIX] = 1u; }
                            else if (a < (uint32_t)nA) atomicAdd(&tal[a * SMC_NT + ((concT & bit) ? SMC_T_CONCORD : SMC_T_DISCORD)], 1u);
                        }
                    }
                }
                if (lane && Qc >= qlo && Qc <= qend) fb.store_word(Qc - qlo, OUT);
                errv |= ((A | (A + KnA)) | ~(Y << 1)) & IM;
                incany |= Y & IM;
                // alleleCnt (:379,401,459): bit 7 of byte k of `other` = read k of this chunk shows another allele than the reference's
                const uint32_t other = (A ^ refa4) + 0x7F7F7F7Fu;
                cnt_ref += (uint32_t)__popc(~other & K7 & IM);
                // (a step of 252 reads nearly always has a few such reads, in a few lanes: the lanes that have one take their
                // lowest, until none is left - one short block per round instead of four predicated ones per step)
                for (uint32_t stray = other & K7 & IM; BAL(stray != 0u); stray &= stray - 1u) {
                    if (stray) {
                        const uint32_t a = (A >> ((uint32_t)__builtin_ctz(stray) & 24u)) & 0xffu;
                        if (a < (uint32_t)nA) atomicAdd(&tal[a * SMC_NT + SMC_T_CNT], 1u);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
                if (tid + j * BLOCK < ncb1) ur[tid + j * BLOCK] = upre[j];
            for (int k = tid + 2 * BLOCK; k < ncb1; k += BLOCK) ur[k] = ustart[cu0 + k];
            const uint32_t nref = (uint32_t)wave_add((int)cnt_ref);
            const lmask e_any = BAL((errv & 0x80808080u) != 0u);
            const lmask i_any = BAL((incany & 0x80808080u) != 0u);
            if (lane == 0) {
                if (refa < (uint32_t)nA) {
                    if (nref) atomicAdd(&tal[refa * SMC_NT + SMC_T_CNT], nref);
                }
                if (e_any) H->misc[M_ERR] = 1u;
                if (i_any) H->misc[M_NINC] = 1u;
            }
        }
        if (fl_glob) __threadfence_block();
        __syncthreads();
        if (SMC_ABLATE == 1) return;
        if (H->misc[M_ERR]) break;                                   // (block-uniform)

        if (__builtin_expect(H->misc[M_NEEDFIX] != 0u, 0)) {
            // (rare) verdicts of the runs with >= 3 reads: replayed, their LIVE / LREF bits patched in
            for (uint32_t i = rc0 + 1 + (uint32_t)tid; i <= rc1; i += BLOCK) {
                const uint32_t b = fb.byte_at(i);
                if (!(b & FLB_L3)) continue;
                const uint32_t st = v2_replay_run(fb, meta, W16, rc0, i, tal);
                uint32_t nb = b & ~(FLB_LIVE | FLB_LREF | FLB_LALT);
                if (st & XS_PRESENT) nb |= FLB_LIVE | (KEY_ALLELE(st) == refa ? FLB_LREF : 0u) | (has_alt && KEY_ALLELE(st) == alta ? FLB_LALT : 0u);
                fb.store_byte(i, nb);
            }
            if (fl_glob) __threadfence_block();
            __syncthreads();
        }
        // state of the fragment whose run ends before position i (0: none): from the flag bytes; a merged pair's error
        // probability (min quality = max probability, :473) comes from the two reads' words; the allele is the
        // reference's (LREF) or, for the few others, read from the word of the read that defines it
        auto frag_state = [&](uint32_t i) -> uint32_t {
            const uint32_t b = fb.byte_at(i);
            if (__builtin_expect((b & FLB_L3) != 0u, 0)) return (b & FLB_LIVE) ? v2_replay_run(fb, meta, W16, rc0, i, nullptr) : 0u;      // (rare)
            // one read, or a pair with one included read: 'unpaired' (error probability 0.1, :65-68)
            uint32_t st = XS_PRESENT | PIDX_UNPAIRED, a = refa;
            if ((b & FLB_LIVE) && (b & (FLB_LREF | FLB_PAIR)) != FLB_LREF) {
                // a merged pair (its quality) or a fragment of another allele (its allele): the two reads before i
                const uint32_t mp = v2_word_aq(meta, i - 1, W16), mpp = i >= 2 ? v2_word_aq(meta, i - 2, W16) : 0u;
                uint32_t def = mpp;                                                             // a merged pair: the first read's allele
                if (b & FLB_PAIR) {
                    uint32_t qp = (mp >> 8) & 0xffu, qpp = (mpp >> 8) & 0xffu;
                    qp = qp < qpp ? qp : qpp;
                    st = XS_PRESENT | XS_PAIRED | (qp < PIDX_UNPAIRED ? qp : PIDX_UNPAIRED - 1u);
                } else {
                    // (rare) not the reference allele and not merged: the included read of the run defines it
                    const uint32_t bp = fb.byte_at(i - 1);
                    const bool second = (bp & FLB_NF) || !(i >= 2 + (uint32_t)fb.fbase && (fb.byte_at(i - 2) & FLB_INC));
                    def = second ? mp : mpp;
                }
                a = (b & FLB_LREF) ? refa : (def & 0xffu);
            }
            return (b & FLB_LIVE) ? (st | (a << 8)) : 0u;
        };

        // ---- U: per-barcode posterior (calProb, :26-98) and PI / consensus accumulation (:506-532)
        {
            long long acc_fx0 = 0, acc_fxp = 0;
            int acc_mt = 0, acc_st = 0;
            int c3 = 0, c5 = 0, c7 = 0, c10 = 0, ufrag = 0;
            uint32_t touch_lo = 0, touch_hi = 0;
            auto prob_of = [&](uint32_t st) -> double { return lut[st & (LUT_N - 1)]; };
            const int ncb = cu1 - cu0;                               // barcodes of the chunk

            // live fragments / of those the reference allele / included reads of barcode u, from the flag bytes: verdicts
            // sit at positions (r0, r1], inclusion at [r0, r1)
            auto barcode_counts = [&](int u, int& nf, int& cr, int& ca, uint32_t& r0, uint32_t& r1) -> bool {
                r0 = ur[u - cu0] & ~SMC_USTART_DROPPED; r1 = ur[u - cu0 + 1] & ~SMC_USTART_DROPPED;
                nf = 0; cr = 0; ca = 0;
                if (!(r0 < r1 && r0 >= rc0 && r1 <= rc1)) { H->misc[M_ERR2] = 1; return false; }
                // a barcode starts a fragment (a fragment never spans two barcodes)
                if (!(fb.byte_at(r0) & FLB_NF)) { H->misc[M_ERR2] = 1; return false; }
                // first and last dword masked to the barcode's positions, the dwords between taken whole
                const int dA = (int)(r0 >> 2) - qlo, dB = (int)(r1 >> 2) - qlo;
                const uint32_t geA = 0xFFFFFFFFu << (8 * (r0 & 3u)), gtA = 0xFFFFFF00u << (8 * (r0 & 3u));   // bytes >= / > r0's
                const uint32_t geB = 0xFFFFFFFFu << (8 * (r1 & 3u)), gtB = 0xFFFFFF00u << (8 * (r1 & 3u));   // bytes >= / > r1's
                uint32_t w = fb.word_at(dA);
                uint32_t ninc;
                if (dA == dB) {
                    nf = __popc(w & 0x80808080u & gtA & ~gtB);
                    cr = __popc(w & 0x40404040u & gtA & ~gtB);
                    if (ALT_OK) ca = __popc(w & 0x02020202u & gtA & ~gtB);
                    ninc = w & 0x20202020u & geA & ~geB;
                } else {
                    nf = __popc(w & 0x80808080u & gtA);
                    cr = __popc(w & 0x40404040u & gtA);
                    if (ALT_OK) ca = __popc(w & 0x02020202u & gtA);
                    ninc = w & geA;
                    for (int d = dA + 1; d < dB; ++d) {
                        w = fb.word_at(d);
                        nf += __popc(w & 0x80808080u);
                        cr += __popc(w & 0x40404040u);
                        if (ALT_OK) ca += __popc(w & 0x02020202u);
                        ninc |= w;
                    }
                    w = fb.word_at(dB);
                    nf += __popc(w & 0x80808080u & ~gtB);
                    cr += __popc(w & 0x40404040u & ~gtB);
                    if (ALT_OK) ca += __popc(w & 0x02020202u & ~gtB);
                    ninc = (ninc | (w & ~geB)) & 0x20202020u;
                }
                return ninc != 0u;                                   // a key of bcDict: has an included read (:467-468)
            };
            const bool two_pass = nU > P.ds || sampled;
            if (__builtin_expect(two_pass, 0)) {
                uint32_t nb = 0, nkeep = 0;
                for (int k = tid; k < ncb; k += BLOCK) {
                    int nf, cr, ca; uint32_t r0, r1;
                    const bool key = barcode_counts(cu0 + k, nf, cr, ca, r0, r1);
                    const bool keep = key && !(sampled && (ur[k] >> 31));
                    umi_flag[k] = keep;
                    nb += key;
                    nkeep += keep;
                }
                nb = (uint32_t)wave_add((int)nb);
                nkeep = (uint32_t)wave_add((int)nkeep);
                if (tid == 0) H->scan_tmp[1] = 0u;
                __syncthreads();
                if (lane == 0 && nb) { atomicAdd(&H->scan_tmp[1], nb); atomicAdd(&H->misc[M_NKEPT], nkeep); }
                __syncthreads();
                if (!sampled) {
                    // the stand-in: bcDict's keys in barcode order, the first ds of the locus stay
                    const int before = (int)H->misc[M_NKEYS_BEFORE];
                    if (before + (int)H->scan_tmp[1] > P.ds) {
                        if (tid == 0) {
                            int k = before;
                            for (int x = 0; x < ncb; ++x)
                                if (umi_flag[x]) { if (k >= P.ds) umi_flag[x] = 0; ++k; }
                        }
                    }
                    __syncthreads();
                    if (tid == 0) H->misc[M_NKEYS_BEFORE] = (uint32_t)before + H->scan_tmp[1];
                }
                if (tid == 0) H->misc[M_NBC] += H->scan_tmp[1];
                __syncthreads();
            }
            if (tid == 0) H->misc[M_NCOMPLEX] = 0u;
            __syncthreads();
            uint32_t nb1 = 0;
            for (int k = tid; k < ncb; k += BLOCK) {
                int nf, cr, ca; uint32_t r0, r1;
                const bool key = barcode_counts(cu0 + k, nf, cr, ca, r0, r1);
                bcinfo[k] = 0xFFFFu;                                   // nothing to score in pass B (default)
                if (two_pass ? !umi_flag[k] : !key) continue;          // not a (kept) key of bcDict
                ++nb1;
                ufrag += nf; c3 += nf >= 3; c5 += nf >= 5; c7 += nf >= 7; c10 += nf >= 10;
                if (nf <= P.mt_drop) {                                 // :28-32 -> all four posteriors 0
                    touch_lo |= 0xFu;                                  // finalDict gets A,T,G,C (+ -0.0)
                    if (nf == 1) {                                     // tie -> single-fragment rule, :521-523
                        for (uint32_t i = r0 + 1; i <= r1; ++i) {
                            const uint32_t st = frag_state(i);
                            if (st & XS_PRESENT) { const uint32_t a = KEY_ALLELE(st); if (a < (uint32_t)nA) atomicAdd(&mtc[a], 1u); break; }
                        }
                    }
                    continue;
                }
                if (ALT_OK && ca == nf && nf < P.simple_to && nf > 0) {          // every live fragment shows the major other allele (ca > 0 only where has_alt)
                    bcinfo[k] = (uint16_t)(0x8000 | nf);
                    continue;
                }
                if (!(refa < 64u && cr == nf && nf < P.simple_to)) {
                    // bit 15: enough reference fragments that the other alleles' sequencing-error terms vanish (`lite`, below)
                    // (not for a barcode of thousands of fragments OF ANY ALLELE - the gate is on nf, not on cr: there the reference's
                    // products underflow - rightP = 0.9^n leaves the double range near n = 6,700, with merged pairs of a quality below
                    // 9 earlier: P.simple_to - and the full walk follows them down)
                    worklist[atomicAdd(&H->misc[M_NCOMPLEX], 1u)] = (uint16_t)(k | (refa < 64u && cr >= P.lite_from && nf < P.simple_to ? 0x8000 : 0));
                    continue;
                }
                bcinfo[k] = (uint16_t)nf;                              // (< P.simple_to <= SMC_SIMPLE_N = 4096)
            }
            // (nb1, the wave's keys of bcDict, is summed over the wavefront further down, packed with the other small counts)
            __syncthreads();                                           // the queue of the general path is complete
            if (SMC_ABLATE == 2) return;
            if (H->misc[M_ERR2]) break;
            // From here every wavefront works on its own, no barrier until the end of U: pass B scores the one-allele
            // barcodes of the wave's threads from the table, then the wave takes its share of the queued barcodes -
            // groups are handed out from the LAST thread down, so the two kinds of work run on different wavefronts.
            bool scored = false, scored_a = false;
            long long acc_fx0a = 0, acc_fxpa = 0;                      // the same sums for the barcodes of the major other allele
            int acc_mta = 0, acc_sta = 0;
            constexpr int GB = 2;
            for (int k0 = tid; k0 < ncb; k0 += GB * BLOCK) {
                uint32_t info[GB];
                double pred0[GB], predpad[GB];
#pragma unroll
                for (int j = 0; j < GB; ++j) { const int k = k0 + j * BLOCK; info[j] = k < ncb ? (uint32_t)bcinfo[k] : 0xFFFFu; }
#pragma unroll
                for (int j = 0; j < GB; ++j) {
                    const uint32_t nf = info[j] == 0xFFFFu ? 0u : (info[j] & 0x7FFFu);
                    pred0[j] = g_simple[2 * nf]; predpad[j] = g_simple[2 * nf + 1];
                }
#pragma unroll
                for (int j = 0; j < GB; ++j) {
                    if (info[j] == 0xFFFFu) continue;
                    const bool isa = ALT_OK && (info[j] & 0x8000u) != 0u;         // a barcode of the major other allele
                    const long long f0 = to_fx(pred0[j], fxscale), fp = to_fx(predpad[j], fxscale);
                    const int mt = (pred0[j] > predpad[j] || (info[j] & 0x7FFFu) == 1u) ? 1 : 0;   // unique maximum (:514-519) or :521-523
                    const int st = (pred0[j] > predpad[j] && pred0[j] > P.smt) ? 1 : 0;
                    if (!isa) { acc_fx0 += f0; acc_fxp += fp; acc_mt += mt; acc_st += st; scored = true; }
                    else { acc_fx0a += f0; acc_fxpa += fp; acc_mta += mt; acc_sta += st; scored_a = true; }
                }
            }
            if (tid - lane < ncb) {                                    // (wave-uniform: the wave owns barcodes)
                {
                    const unsigned long long padmask = refa < 4 ? (0xFull & ~(1ull << refa)) : 0x7ull;
                    const long long s0 = wave_add64(acc_fx0), sp = wave_add64(acc_fxp);
                    // (the small counts travel two to a word: none can exceed the barcodes of a chunk, < 2^15)
                    const uint32_t mmst = (uint32_t)wave_add((int)((uint32_t)acc_mt | (uint32_t)acc_st << 16));
                    const int mm = (int)(mmst & 0xFFFFu), st = (int)(mmst >> 16);
                    if (BAL(scored)) {
                        const unsigned long long uq = (1ull << refa) | padmask;
                        touch_lo |= (uint32_t)uq; touch_hi |= (uint32_t)(uq >> 32);
                    }
                    if (lane == 0 && refa < 64) {
                        atomicAdd(&pifx[refa], (unsigned long long)s0);
                        for (int a = 0; a < 4; ++a)
                            if ((padmask >> a) & 1ull) atomicAdd(&pifx[a], (unsigned long long)sp);
                        atomicAdd(&mtc[refa], (uint32_t)mm);
                        atomicAdd(&strong[refa], (uint32_t)st);
                    }
                }
                if (has_alt) {                                         // (block-uniform) the same for the major other allele
                    const unsigned long long padmask = alta < 4 ? (0xFull & ~(1ull << alta)) : 0x7ull;
                    const long long s0 = wave_add64(acc_fx0a), sp = wave_add64(acc_fxpa);
                    const uint32_t mmst = (uint32_t)wave_add((int)((uint32_t)acc_mta | (uint32_t)acc_sta << 16));
                    const int mm = (int)(mmst & 0xFFFFu), st = (int)(mmst >> 16);
                    if (BAL(scored_a)) {
                        const unsigned long long uq = (1ull << alta) | padmask;
                        touch_lo |= (uint32_t)uq; touch_hi |= (uint32_t)(uq >> 32);
                        if (lane == 0) {
                            atomicAdd(&pifx[alta], (unsigned long long)s0);
                            for (int a = 0; a < 4; ++a)
                                if ((padmask >> a) & 1ull) atomicAdd(&pifx[a], (unsigned long long)sp);
                            atomicAdd(&mtc[alta], (uint32_t)mm);
                            atomicAdd(&strong[alta], (uint32_t)st);
                        }
                    }
                }
                {
                    const uint32_t c35 = (uint32_t)wave_add((int)((uint32_t)c3 | (uint32_t)c5 << 16));
                    const uint32_t c710 = (uint32_t)wave_add((int)((uint32_t)c7 | (uint32_t)c10 << 16));
                    c3 = (int)(c35 & 0xFFFFu); c5 = (int)(c35 >> 16); c7 = (int)(c710 & 0xFFFFu); c10 = (int)(c710 >> 16);
                    ufrag = wave_add(ufrag);                           // (one barcode can have more than 2^16 fragments)
                    nb1 = two_pass ? 0u : (uint32_t)wave_add((int)nb1);
                }
                touch_lo = wave_or(touch_lo); touch_hi = wave_or(touch_hi);
                if (lane == 0) {
                    if (!two_pass && nb1) atomicAdd(&H->misc[M_NBC], nb1);
                    atomicAdd(&H->misc[M_MT3], (uint32_t)c3); atomicAdd(&H->misc[M_MT5], (uint32_t)c5);
                    atomicAdd(&H->misc[M_MT7], (uint32_t)c7); atomicAdd(&H->misc[M_MT10], (uint32_t)c10);
                    atomicAdd(&H->misc[M_USEDFRAG], (uint32_t)ufrag);
                    atomicOr(&H->misc[M_TOUCH_LO], touch_lo); atomicOr(&H->misc[M_TOUCH_HI], touch_hi);
                }
            }

            if (SMC_ABLATE == 3) return;
            // ---- the queued barcodes (more than one allele, or not the reference), general path, 8 lanes per barcode
            // (8 lanes per queued barcode; 4 - sixteen groups in a one-wavefront workgroup, one pass nearly always - measured
            // slower on C3: 0.50 vs 0.45 ms per 40 k loci, the walk doubles)
            constexpr int Gc = SMC_GC;
            const int jc = tid % Gc;
            // The fragments of a barcode (verdicts at positions (r0, r1]), lane jc of the group taking every Gc-th flag dword.
            // Most are unpaired fragments of the reference allele - error probability 0.1 whatever their quality (:65-68) -
            // and are only COUNTED (`bulk`); the others (merged pairs: their quality; other alleles; replayed runs) are
            // handed one by one to `each` as state words.
            auto for_fragments = [&](uint32_t r0, uint32_t r1, auto lite_c /* std::true_type: reference fragments only counted */, auto&& bulk, auto&& each) {
                constexpr bool lite = decltype(lite_c)::value;
                const int dA = (int)(r0 >> 2) - qlo, dB = (int)(r1 >> 2) - qlo;
                const uint32_t gtA = 0xFFFFFF00u << (8 * (r0 & 3u)), gtB = 0xFFFFFF00u << (8 * (r1 & 3u));
                for (int d = dA + jc; d <= dB; d += Gc) {
                    const uint32_t w = fb.word_at(d);
                    uint32_t Lv = w & 0x80808080u;
                    if (d == dA) Lv &= gtA;
                    if (d == dB) Lv &= ~gtB;
                    const uint32_t R = (w << 1) & Lv, special = ((w << 5) | (w << 4)) & Lv;    // reference allele / merged pair or replayed run
                    const uint32_t plain = R & ~special;
                    bulk(__popc(Lv), __popc(R), __popc(plain));
                    for (uint32_t todo = Lv & ~(lite ? R : plain); todo; todo &= todo - 1u) {
                        const uint32_t k = (uint32_t)(__ffs((int)todo) - 1) >> 3;
                        each(frag_state(4u * (uint32_t)(d + qlo) + k));
                    }
                }
            };
            auto pow_int = [](double b, int k) -> double {            // b^k by squaring (k: fragments of a lane, small)
                double r = 1.0;
                for (; k; k >>= 1) { if (k & 1) r *= b; b *= b; }
                return r;
            };
            const int n_complex = __builtin_amdgcn_readfirstlane((int)H->misc[M_NCOMPLEX]);
            const int grp1 = (BLOCK - 1 - tid) / Gc, ngrp1 = BLOCK / Gc;   // groups from the last thread down
            for (int w = grp1; w < n_complex; w += ngrp1) {
                const int uk = (int)(worklist[w] & 0x7FFFu);
                // `lite`: the likelihoods of calProb all carry the factor rightP (:62-91), so the posteriors depend on the
                // fragments' odds e / (1 - e) only: T(k) = pcr_no_error * prod(odds of the fragments NOT showing k) + pcrP term,
                // the pcrP term being >= 1e-6.  With P.lite_from or more reference fragments that product is < 1e-30 for every
                // other allele k (host_abi.inc, lite_from_for): it cannot change T(k), and the reference fragments - the merged
                // pairs among them, whose qualities would have to be fetched - are only counted.  What remains is
                // T(ref) = pcr_no_error * prod(odds of the OTHER fragments) + pcrP term; rightP = 1, P(reads | k != ref) = 0.
                const bool lite = (worklist[w] >> 15) != 0;
                const uint32_t r0 = ur[uk] & ~SMC_USTART_DROPPED, r1 = ur[uk + 1] & ~SMC_USTART_DROPPED;
                // pass A: fragment count, allele set, P(no sequencing error); speculatively also the count and product for
                // the locus's reference allele and for "the other allele"
                int nf = 0, cnt_ref = 0, n_plain = 0;
                unsigned long long mk = 0;
                double rightP = 1.0, prod_ref = 1.0, prod_x = 1.0;
                if (lite) {
                    for_fragments(r0, r1, std::true_type{},
                        [&](int n_live, int n_ref, int) { nf += n_live; cnt_ref += n_ref; },
                        [&](uint32_t st) {                            // (only fragments of other alleles come here)
                            if (!(st & XS_PRESENT)) return;
                            const double pv = prob_of(st);
                            mk |= 1ull << KEY_ALLELE(st);
                            prod_ref *= fast_div(pv, 1.0 - pv);
                        });
                    prod_x = jc == 0 ? 0.0 : 1.0;                      // (the group product is 0)
                } else {
                    for_fragments(r0, r1, std::false_type{},
                        [&](int n_live, int n_ref, int n_pl) { nf += n_live; cnt_ref += n_ref; n_plain += n_pl; },
                        [&](uint32_t st) {
                            if (!(st & XS_PRESENT)) return;
                            const double pv = prob_of(st), q1 = 1.0 - pv;
                            const int a = (int)KEY_ALLELE(st);
                            const bool same = a == (int)refa;
                            mk |= 1ull << a;
                            rightP *= q1;
                            prod_ref *= same ? q1 : pv;
                            prod_x *= same ? pv : q1;                 // P(reads | the other allele), if there is just one
                        });
                    const double p9 = pow_int(0.9, n_plain);           // the unpaired reference fragments: 1 - 0.1 each
                    rightP *= p9; prod_ref *= p9; prod_x *= pow_int(0.1, n_plain);
                }
                if (cnt_ref && refa < 64u) mk |= 1ull << refa;
                nf = grpN_add<Gc>(nf);
                cnt_ref = grpN_add<Gc>(cnt_ref);
                const uint32_t mlo = grpN_or<Gc>((uint32_t)mk), mhi = grpN_or<Gc>((uint32_t)(mk >> 32));
                rightP = grpN_mul<Gc>(rightP);
                prod_ref = grpN_mul<Gc>(prod_ref);
                prod_x = grpN_mul<Gc>(prod_x);
                const unsigned long long mask = ((unsigned long long)mhi << 32) | mlo;
                if (nf <= P.mt_drop) continue;                         // (cannot be: such barcodes are not queued)
                // thousands of fragments: the products have left the normal double range - the reference's posterior is then made
                // of denormal rounding in ITS multiplication order (py2 dict order of read ids): computed here, flagged as unpinned
                if (__builtin_expect(!lite && rightP < 0x1p-1000, 0)) { if (jc == 0) H->misc[M_UNDERFLOW] = 1u; }
                if (SMC_ABLATE == 5) { if (jc == 0 && rightP + prod_ref + prod_x + (double)(nf + cnt_ref) + (double)mask == 0.5) H->misc[31] = 1u; continue; }   // (diagnostic: the walk only)
                const int n_exist = __popcll(mask);
                int npad = n_exist < 4 ? 4 - n_exist : 0;
                unsigned long long padmask = 0;
                for (int a = 0, k = 0; a < 4 && k < npad; ++a)
                    if (!((mask >> a) & 1ull)) { padmask |= 1ull << a; ++k; }   // :49-54, atgc order
                const int nk = n_exist + npad;
                const double denom = nf + 0.5 * nk;                    // :80

                if (__builtin_expect(n_exist <= 4, 1)) {
                    int ida[4] = {0, 0, 0, 0}, cnta[4] = {0, 0, 0, 0};
                    double proda[4] = {1.0, 1.0, 1.0, 1.0};
                    {
                        unsigned long long mm = mask;
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (k < n_exist) { ida[k] = __ffsll((long long)mm) - 1; mm &= mm - 1; }
                    }
                    if (refa < 64 && mask == (1ull << refa)) {
                        cnta[0] = cnt_ref; proda[0] = prod_ref;        // speculation hit: no second pass
                    } else if (!lite && n_exist == 1) {
                        // every fragment shows the same OTHER allele (the barcodes of a variant): prod_x has taken 1 - p of each
                        // of them, in the order and with the operations pass B would use - no second pass either
                        cnta[0] = nf; proda[0] = prod_x;
                    } else if (refa < 64 && n_exist == 2 && ((mask >> refa) & 1ull)) {
                        const bool ref_first = ida[0] == (int)refa;
                        cnta[0] = ref_first ? cnt_ref : nf - cnt_ref; cnta[1] = ref_first ? nf - cnt_ref : cnt_ref;
                        proda[0] = ref_first ? prod_ref : prod_x; proda[1] = ref_first ? prod_x : prod_ref;
                    } else {
                        // pass B: per existing allele, count and P(reads | allele)  (:62-77)
                        if (lite) {
                            // counts only; P(reads | k) / rightP is pass A's odds product for the reference allele, 0 for the others
                            for_fragments(r0, r1, std::true_type{}, [&](int, int, int) {},
                                [&](uint32_t st) {
                                    if (!(st & XS_PRESENT)) return;
                                    const int a = (int)KEY_ALLELE(st);
#pragma unroll
                                    for (int k = 0; k < 4; ++k) cnta[k] += (k < n_exist && a == ida[k]);
                                });
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                const bool isref = ida[k] == (int)refa;
                                cnta[k] = grpN_add<Gc>(cnta[k]);
                                if (k < n_exist && isref) cnta[k] = cnt_ref;
                                proda[k] = isref ? prod_ref : 0.0;
                            }
                        } else {
                            int n_pl = 0;
                            for_fragments(r0, r1, std::false_type{}, [&](int, int, int n) { n_pl += n; },
                                [&](uint32_t st) {
                                    if (!(st & XS_PRESENT)) return;
                                    const int a = (int)KEY_ALLELE(st);
                                    const double p = prob_of(st);
#pragma unroll
                                    for (int k = 0; k < 4; ++k)
                                        if (k < n_exist) {
                                            const bool same = a == ida[k];
                                            cnta[k] += same;
                                            proda[k] *= same ? 1.0 - p : p;
                                        }
                                });
                            {
                                const double p9 = pow_int(0.9, n_pl), p1 = pow_int(0.1, n_pl);   // the unpaired reference fragments
#pragma unroll
                                for (int k = 0; k < 4; ++k)
                                    if (k < n_exist) {
                                        const bool same = ida[k] == (int)refa;
                                        cnta[k] += same ? n_pl : 0;
                                        proda[k] *= same ? p9 : p1;
                                    }
                            }
#pragma unroll
                            for (int k = 0; k < 4; ++k) {
                                cnta[k] = grpN_add<Gc>(cnta[k]);
                                proda[k] = grpN_mul<Gc>(proda[k]);
                            }
                        }
                    }
                    // PCR-error terms (:79-81); min over the other keys == value at their max count
                    int max1 = -1, max2 = -1, arg1 = -1, arg2 = -1;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < n_exist) {
                            if (cnta[k] > max1) { max2 = max1; arg2 = arg1; max1 = cnta[k]; arg1 = k; }
                            else if (cnta[k] > max2) { max2 = cnta[k]; arg2 = k; }
                        }
                    // The transcendental chains run lane-parallel: lane k (< n_exist) of the barcode's first quad owns
                    // existing allele k, lane n_exist owns the zero-count PCR term and then the padded keys; values
                    // are exchanged by quad broadcasts (DPP).  Every value is produced by the same instruction
                    // sequence whichever lane computes it, so results do not depend on the lane assignment.
                    const int myc = jc == 0 ? cnta[0] : jc == 1 ? cnta[1] : jc == 2 ? cnta[2] : jc == 3 ? cnta[3] : 0;
                    // (lanes >= n_exist: count 0; the table holds exactly what pcr_of computes)
                    const double mypcr = nf < SMC_PCR_N ? g_pcr[nf * SMC_PCR_N + myc] : pcr_of(myc, denom);
                    double pcrv[4];
                    pcrv[0] = dpp_f64<0x00>(mypcr); pcrv[1] = dpp_f64<0x55>(mypcr);
                    pcrv[2] = dpp_f64<0xAA>(mypcr); pcrv[3] = dpp_f64<0xFF>(mypcr);
                    double prodpcr = 1.0;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < n_exist) prodpcr *= pcrv[k];
                    const double pcr0 = n_exist == 1 ? pcrv[1] : 0.0;
                    const double padOut = rightP * prodpcr;            // :88-91
                    double mytmp = padOut;                             // lane n_exist: the padded keys
                    {
                        const int oi = (jc == arg1) ? arg2 : arg1;
                        double po = pcr0;
#pragma unroll
                        for (int mI = 0; mI < 4; ++mI) po = (mI == oi) ? pcrv[mI] : po;
                        const double myprod = jc == 0 ? proda[0] : jc == 1 ? proda[1] : jc == 2 ? proda[2] : proda[3];
                        if (jc < n_exist) mytmp = pne * myprod + rightP * po;                 // :86
                    }
                    double tmpv[4];
                    tmpv[0] = dpp_f64<0x00>(mytmp); tmpv[1] = dpp_f64<0x55>(mytmp);
                    tmpv[2] = dpp_f64<0xAA>(mytmp); tmpv[3] = dpp_f64<0xFF>(mytmp);
                    double sumP = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < n_exist) sumP += tmpv[k];
                    for (int k = 0; k < npad; ++k) sumP += padOut;
                    // posteriors -> -log10(1-p) (:95-96, :508-510)
                    const double mypost = sumP <= 0 ? 0.0 : fast_div(mytmp, sumP);
                    double mypred;
                    if (jc >= n_exist && mypost < 1e-6) {
                        // padded keys: t is tiny, the series is exact to < 1e-19 below 1e-6
                        mypred = mypost * (1.0 + mypost * (0.5 + mypost * (1.0 / 3.0))) * 0.43429448190325182765;
                    } else {
                        const double x = 1.0 - mypost;
                        mypred = x > 0.0 ? neg_log10_unit(x) : 16.0;
                    }
                    // A barcode of ONE allele (a variant's - the reference's own were scored from the per-count table before they
                    // could get here) takes the table's two values as well (lane 0 the allele, lane 1 the padded keys): equal
                    // barcodes of the reference and of another allele then give bit-equal prediction indices, and an exact tie
                    // between the two at smCounter.py:534 stays one (the route above is ~1e-13 away from the table's).
                    if (n_exist == 1 && nf < P.simple_to && jc < 2) mypred = g_simple[2 * nf + jc];
                    double predv[4], mx = -1.0;
                    predv[0] = dpp_f64<0x00>(mypred); predv[1] = dpp_f64<0x55>(mypred);
                    predv[2] = dpp_f64<0xAA>(mypred); predv[3] = dpp_f64<0xFF>(mypred);
                    double predpad = 0.0;
                    if (npad) predpad = n_exist == 1 ? predv[1] : n_exist == 2 ? predv[2] : predv[3];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        if (k >= n_exist) predv[k] = 0.0;
                        else if (predv[k] > mx) mx = predv[k];
                    }
                    if (npad && predpad > mx) mx = predpad;
                    if (jc <= n_exist && jc < 4) {
                        const long long fx = to_fx(mypred, fxscale);
                        if (jc < n_exist) {
                            const int a = jc == 0 ? ida[0] : jc == 1 ? ida[1] : jc == 2 ? ida[2] : ida[3];
                            atomicAdd(&pifx[a], (unsigned long long)fx);
                        } else if (npad) {
                            for (int b = 0; b < 4; ++b)
                                if ((padmask >> b) & 1ull) atomicAdd(&pifx[b], (unsigned long long)fx);
                        }
                    }
                    if (jc == 0) {
                        int n_max = 0, cons = -1;
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (k < n_exist && predv[k] == mx) { ++n_max; cons = ida[k]; }  // :514
                        if (npad && predpad == mx) {
#pragma unroll
                            for (int a = 0; a < 4; ++a)
                                if ((padmask >> a) & 1ull) { ++n_max; cons = a; }
                        }
                        const unsigned long long uq = mask | padmask;
                        atomicOr(&H->misc[M_TOUCH_LO], (uint32_t)uq); atomicOr(&H->misc[M_TOUCH_HI], (uint32_t)(uq >> 32));
                        if (n_max == 1) {                                                    // :515-519
                            const bool str = mx > P.smt;
                            { atomicAdd(&mtc[cons], 1u); if (str) atomicAdd(&strong[cons], 1u); }
                        } else if (nf == 1) {                                                // :521-523
                            const int a = ida[0];
                            atomicAdd(&mtc[a], 1u);
                        }
                    }
                } else {
                    // > 4 distinct alleles inside one barcode: same arithmetic, recomputed per allele
                    if (lite) {
                        // (rare twice over) this branch keeps the likelihoods as the reference writes them: rightP in full
                        double rp = 1.0;
                        int n_pl = 0;
                        for_fragments(r0, r1, std::false_type{}, [&](int, int, int n) { n_pl += n; },
                            [&](uint32_t st) { if (st & XS_PRESENT) rp *= 1.0 - prob_of(st); });
                        rightP = grpN_mul<Gc>(rp * pow_int(0.9, n_pl));
                    }
                    auto scan_allele = [&](int a, int& cnt, double& prod) {
                        cnt = 0; prod = 1.0;
                        int n_pl = 0;
                        for_fragments(r0, r1, std::false_type{}, [&](int, int, int n) { n_pl += n; },
                            [&](uint32_t st) {
                                if (!(st & XS_PRESENT)) return;
                                const double p = prob_of(st);
                                const bool same = (int)KEY_ALLELE(st) == a;
                                cnt += same;
                                prod *= same ? 1.0 - p : p;
                            });
                        cnt += a == (int)refa ? n_pl : 0;
                        prod *= pow_int(a == (int)refa ? 0.9 : 0.1, n_pl);
                        cnt = grpN_add<Gc>(cnt);
                        prod = grpN_mul<Gc>(prod);
                    };
                    int max1 = -1, max2 = -1, arg1 = -1;
                    for (unsigned long long mm = mask; mm; mm &= mm - 1) {
                        const int a = __ffsll((long long)mm) - 1;
                        int c; double pr;
                        scan_allele(a, c, pr);
                        if (c > max1) { max2 = max1; max1 = c; arg1 = a; }
                        else if (c > max2) max2 = c;
                    }
                    double sumP = 0.0;
                    for (unsigned long long mm = mask; mm; mm &= mm - 1) {
                        const int a = __ffsll((long long)mm) - 1;
                        int c; double pr;
                        scan_allele(a, c, pr);
                        const int other = (a == arg1) ? max2 : max1;
                        sumP += pne * pr + rightP * pcr_of(other, denom);
                    }
                    double mx = -1.0;
                    int n_max = 0, cons = -1;
                    for (unsigned long long mm = mask; mm; mm &= mm - 1) {
                        const int a = __ffsll((long long)mm) - 1;
                        int c; double pr;
                        scan_allele(a, c, pr);
                        const int other = (a == arg1) ? max2 : max1;
                        const double t = pne * pr + rightP * pcr_of(other, denom);
                        const double post = sumP <= 0 ? 0.0 : t / sumP;
                        const double x = 1.0 - post;
                        const double pred = x > 0.0 ? -log10(x) : 16.0;
                        if (pred > mx) { mx = pred; n_max = 1; cons = a; }
                        else if (pred == mx) ++n_max;
                        if (jc == 0) {
                            const long long fx = to_fx(pred, fxscale);
                            atomicAdd(&pifx[a], (unsigned long long)fx);
                        }
                    }
                    if (jc == 0) {
                        atomicOr(&H->misc[M_TOUCH_LO], (uint32_t)mask); atomicOr(&H->misc[M_TOUCH_HI], (uint32_t)(mask >> 32));
                        if (n_max == 1) {
                            const bool str = mx > P.smt;
                            { atomicAdd(&mtc[cons], 1u); if (str) atomicAdd(&strong[cons], 1u); }
                        }
                    }
                }
            }
        }
        __syncthreads();                                               // the chunk's tables are free again
        if (SMC_ABLATE == 4) return;
        cu0 = cu1;
    }
    __syncthreads();

    // =====================================================================================================
    // E: ranking and candidates (:534-555) - by this workgroup (whole locus) or by the last part to arrive
    // =====================================================================================================
    if (!solo) {
        // add this part's header to the locus's global accumulator (integer adds / ors: order-free), then take a ticket;
        // the last part reads the totals back and finishes the row
        uint32_t* acc = g_acc + (size_t)pt.acc * v2_acc_words(a_cap);
        const uint32_t* hw = (const uint32_t*)H->misc;
        const int n_add = 32 + a_cap * SMC_NT;                        // misc[32] then tal[a_cap][SMC_NT], as laid out in LDS
        for (int i = tid; i < n_add; i += BLOCK) {
            const uint32_t v = hw[i + (i >= 32 ? 32 : 0)];           // (scan_tmp sits between misc and tal)
            if (!v) continue;
            if (i == M_TOUCH_LO || i == M_TOUCH_HI || i == M_ERR || i == M_ERR2 || i == M_NINC) atomicOr(&acc[i], v);
            else atomicAdd(&acc[i], v);
        }
        unsigned long long* apifx = (unsigned long long*)(acc + n_add);
        uint32_t* amtc = (uint32_t*)(apifx + a_cap);
        uint32_t* astrong = amtc + a_cap;
        for (int a = tid; a < a_cap; a += BLOCK) {
            if (pifx[a]) atomicAdd(&apifx[a], pifx[a]);
            if (mtc[a]) atomicAdd(&amtc[a], mtc[a]);
            if (strong[a]) atomicAdd(&astrong[a], strong[a]);
        }
        // Everything published above is a device-scope atomic (performed at the L2 / memory side, nothing to write back or
        // to invalidate): each wave waits for its own to be acknowledged, the barrier orders the workgroup, then one
        // thread takes the ticket.  (A __threadfence() here - L2 write-back + invalidate by all 512 threads - cost more
        // than the rest of the part.)
        __builtin_amdgcn_s_waitcnt(0);               // vmcnt(0) lgkmcnt(0) expcnt(0)
        __syncthreads();
        uint32_t* ticket = astrong + a_cap;
        if (tid == 0) H->scan_tmp[2] = atomicAdd(ticket, 1u);
        __syncthreads();
        if ((int)H->scan_tmp[2] != pt.nparts - 1 || SMC_ABLATE == 7) return;
        // totals back into the LDS header (returning atomics: served where the adds were performed)
        uint32_t* hww = (uint32_t*)H->misc;
        for (int i = tid; i < n_add; i += BLOCK) hww[i + (i >= 32 ? 32 : 0)] = atomicAdd(&acc[i], 0u);
        for (int a = tid; a < a_cap; a += BLOCK) {
            pifx[a] = atomicAdd(&apifx[a], 0ull);
            mtc[a] = atomicAdd(&amtc[a], 0u);
            strong[a] = atomicAdd(&astrong[a], 0u);
        }
        __syncthreads();
    }
    if (tid == 0) H->misc[M_ALLMT] = (uint32_t)nU;                     // allMT (:482): every barcode has a read
    __syncthreads();
    if (H->misc[M_ERR] || H->misc[M_ERR2] || H->misc[M_NINC] == 0 || P.ds <= 0) {   // (ds <= 0: usedMT = min(ds, .) = 0)
        special_row((H->misc[M_ERR] || H->misc[M_ERR2]) ? SMC_ST_BAD_INPUT : SMC_ST_ZERO_COVERAGE);
        return;
    }
    for (int i = tid; i < (int)(sizeof(smc_row) / 4); i += BLOCK) ((uint32_t*)rowst)[i] = 0u;
    __syncthreads();
    if (wid == 0) {                                                     // the first wavefront, every lane
        const int n_bc = (int)H->misc[M_NBC];
        finish_row(rowst, L, li, n, nF, n_bc < P.ds ? n_bc : P.ds /* usedMT, :489 */, n_bc > P.ds, fxscale, H->misc, tal,
                   pifx, mtc, strong, flt_list, lane, WAVE);
        if (sampled && (int)H->misc[M_NKEPT] != (n_bc < P.ds ? n_bc : P.ds)) rowst->status = SMC_ST_BAD_INPUT;
    }
    __syncthreads();
    // The eight tallies only filterVariants reads (strand, quality, end-distance counts of the reference allele and the candidate(s)):
    // one more pass over the locus's reads by this workgroup - or, in a batch with loci of the deep class (P.tallies_later), by
    // k_filter_tallies behind this kernel: there the pass was 11 us of ONE workgroup at the tail of a 58,000-read locus, 16 % of the
    // locus kernels' time on the example run's shape, and the whole chip does it in a fifth of that.
    if (SMC_ABLATE != 6 && !P.tallies_later && (rowst->cand[0].flt_applied | rowst->cand[1].flt_applied)) {       // (block-uniform) a candidate goes on to the filters
        const int w0 = refa < (uint32_t)nA ? (int)refa : -1;
        const int w1 = rowst->cand[0].flt_applied ? rowst->cand[0].allele : -1;
        const int w2 = rowst->cand[1].flt_applied ? rowst->cand[1].allele : -1;
        uint32_t* const ftal = tal;                                      // (the locus's own tallies are in the row by now: three sets of SMC_NT words over them)
        __syncthreads();
        if (tid < 3 * SMC_NT) ftal[tid] = 0u;
        __syncthreads();
        if (w2 >= 0) v2_filter_tallies<BLOCK, 3, W16, false>(tid, meta, n, 0, (n + 3) >> 2, w0, w1, w2, cls_lut, ftal);
        else v2_filter_tallies<BLOCK, 2, W16, false>(tid, meta, n, 0, (n + 3) >> 2, w0, w1, -1, cls_lut, ftal);
        __syncthreads();
        if (tid < 24) {
            const int s = tid >> 3, k = 1 + (tid & 7);                   // words 1..8: SMC_T_FWD .. SMC_T_R2PRLE
            if (s == 0) { if (w0 >= 0) rowst->ref_tal[k] = (int32_t)ftal[k]; }
            else if ((s == 1 ? w1 : w2) >= 0) rowst->cand[s - 1].tal[k] = (int32_t)ftal[s * SMC_NT + k];
        }
        __syncthreads();
    }
    const uint32_t* src = (const uint32_t*)rowst;
    uint32_t* dst = (uint32_t*)out;
    for (int i = tid; i < (int)(sizeof(smc_row) / 4); i += BLOCK) dst[i] = src[i];
}

// ------------------------------------------------------------------------------------------
// kernel 1b: the filter-only tallies of the queued loci (smCounter.py:386-389, :408-411, :428-457), by the whole chip
// ------------------------------------------------------------------------------------------
// k_call_v2 queues the loci whose candidate goes on to filterVariants (altPI >= 5, :549); every (queued locus, slice of its reads)
// is a work item here - `split` slices per locus -, a workgroup counts its slice for the reference allele and the candidate(s)
// (nine 5-bit fields per read and allele, widened as v2_filter_tallies does) and adds what it found to the locus's ROW in global
// memory (integer adds: order-free).  k_filter_loci, behind it on the stream, reads the rows as before.
template <bool W16>
__global__ __launch_bounds__(256) void k_filter_tallies(const smc_locus* __restrict__ loci, smc_row* __restrict__ rows, const uint32_t* __restrict__ flt_list,
                                                        const uint32_t* __restrict__ g_words, const double* __restrict__ g_lut, int split) {
    // A WAVEFRONT per work item, no workgroup barrier (a first version gave an item to a workgroup of 256 threads: on 3,000-read loci
    // most of them idled through its barriers and reductions - 0.13 ms for X3's 11,837 loci where this form takes a few microseconds)
    __shared__ uint2 cls_lut[32];
    __shared__ __attribute__((aligned(8))) uint32_t tal_all[4][3 * SMC_NT];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid < 32) cls_lut[tid] = ((const uint2*)(g_lut + (W16 ? 288 : 256)))[tid];
    __syncthreads();
    uint32_t* const tal = tal_all[wid];
    const uint32_t n_items = flt_list[0] * (uint32_t)split, n_waves = gridDim.x * 4u;
    for (uint32_t e = blockIdx.x * 4u + (uint32_t)wid; e < n_items; e += n_waves) {
        const int li = (int)flt_list[1u + e / (uint32_t)split], slice = (int)(e % (uint32_t)split);
        const smc_locus L = loci[li];
        smc_row* R = rows + li;
        const int n = L.n_reads, nA = L.n_alleles, n4 = (n + 3) >> 2;
        const int f0 = R->cand[0].flt_applied, f1 = R->cand[1].flt_applied;
        const int w0 = (int)L.ref_allele < nA ? (int)L.ref_allele : -1, w1 = f0 ? R->cand[0].allele : -1, w2 = f1 ? R->cand[1].allele : -1;
        if (lane < 3 * SMC_NT) tal[lane] = 0u;
        __builtin_amdgcn_wave_barrier();
        const uint32_t* meta = W16 ? (const uint32_t*)((const uint16_t*)g_words + 4ll * L.read_off4) : g_words + 4ll * L.read_off4;
        // (slices of 4,096 reads; the item takes slices `slice`, `slice + split`, ...: a locus of any depth is covered, a shallow one by
        // its first item alone)
        for (int qa = slice * 1024; qa < n4 && (f0 | f1); qa += split * 1024) {   // (wave-uniform)
            const int qb = min(n4, qa + 1024);
            if (w2 >= 0) v2_filter_tallies<64, 3, W16, true>(lane, meta, n, qa, qb, w0, w1, w2, cls_lut, tal);
            else v2_filter_tallies<64, 2, W16, true>(lane, meta, n, qa, qb, w0, w1, -1, cls_lut, tal);
        }
        __builtin_amdgcn_wave_barrier();
        if (lane < 24) {
            const int s = lane >> 3, k = 1 + (lane & 7);                         // words 1..8: SMC_T_FWD .. SMC_T_R2PRLE
            const uint32_t v = tal[s * SMC_NT + k];
            if (v) {
                if (s == 0) { if (w0 >= 0) atomicAdd((uint32_t*)&R->ref_tal[k], v); }
                else if ((s == 1 ? w1 : w2) >= 0) atomicAdd((uint32_t*)&R->cand[s - 1].tal[k], v);
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
}
