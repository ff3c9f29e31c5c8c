// Included by smcounter_hip.hip (after k_build_planes.inc: it uses that file's BpArgs, bp_wave and the extras queue format).
// ------------------------------------------------------------------------------------------
// the walk that writes the planes, transposed (round 4): LANE = ALIGNMENT, a wavefront = 16 consecutive loci
// ------------------------------------------------------------------------------------------
// Round 3's walk gave a wavefront a tile of 64 loci with lane = locus: the words of a locus came out one lane at a time, so
// they went through an LDS transposition (16 words per locus, flushed as 64-byte runs at any alignment: 58 % of the write
// requests were 32-byte partial lines), every alignment's per-row work was serialised over the wavefront (row words through LDS,
// window bytes through LDS: ~ 64 vector + 42 scalar + 8 LDS instructions per alignment of ~ 43 reads) and the kernel sat at
// 0.17 of its roofline as a latency chain.  Here the matrix (sorted alignments x loci) is walked the other way round:
//   * a wavefront takes a GROUP of 16 consecutive loci of a tile and a part of the tile's sorted list, 64 alignments ("rows")
//     at a time, lane = row.  What is per alignment (span, flags, class bases, end-distance constants, window address) is per
//     LANE - a 32-byte row record made once per run by k_bp_rows_write - and needs no LDS;
//   * per locus of the group: the rows that cover it are ONE compare (a ballot: the locus's column as a 64-bit scalar), a read's
//     rank is mbcnt of that mask, and the wavefront's store writes the covering rows' words to CONSECUTIVE slots of the locus
//     (up to 256 contiguous bytes per store instead of 64 lanes x 4 bytes into 64 different loci);
//   * "first read of its barcode / fragment at this locus" for all 16 loci at once: a segmented prefix OR over the lanes of
//     the rows' 16-bit coverage masks (runs of equal barcode / read pair are contiguous: the list is sorted), carried from batch
//     to batch as one 16-bit mask per level;
//   * bases and qualities: each lane loads the 16 bytes of its alignment under the group (two unaligned 16-byte loads) and the
//     per-read arithmetic runs on BYTE LANES, four loci per instruction: letter -> allele id and "is it one of A,C,G,T,N" by
//     v_perm_b32 used as an 8-entry table, bq >= minBQ and the two end-distance tests by carry-free byte adds (v_xad_u32),
//     the read class by a byte-wise select; a word is then one v_perm_b32 away;
//   * alignments with a general CIGAR (insertions, deletions, skips: a few per cent) get a LINEARISED copy of their bases and
//     qualities - one byte per REFERENCE position - and end-distance constants in reference coordinates, made once per run by
//     k_bp_rows_write (resolve_cigar2 semantics as smc_bam.cpp): in the walk they are rows like any other.  The positions that
//     are not a plain base (inside a deletion, an insertion / deletion start) carry a byte that is no letter and take, like an
//     unusual letter of any row, the exact per-lane path (bp2_exact: CIGAR walk, allele key listed for k_bp_xfix).
// Counting (k_bp_count), the per-part prefix (k_bp_scan_tiles) and the extras (k_bp_xgroup / k_bp_xfix) are round 3's.
#define BP2_G 16                 // loci per group: a lane's bases and qualities are loaded 16 at a time
#ifndef BP2_ABL
#define BP2_ABL 0
#endif
#ifndef BP2_STORE_AUX
#define BP2_STORE_AUX 0          // cache policy bits of the word stores (gfx940+: 1 sc0, 2 nt, 16 sc1) - experiments
#endif
#define BP2_LIN_SPAN 4096u       // a general CIGAR spanning more reference positions than this keeps the exact path at every position
#define BP2_SIMPLE 1u            // BpRow.hi: [clip] match [clip] - the window is the alignment's own bases / qualities
#define BP2_MQOK 2u              //   MAPQ >= minMQ and mismatches pass (the alignment's terms of incCond, smCounter.py:378)
#define BP2_R2 4u
#define BP2_FARA 8u              //   the barcode-side end distance runs from the far end (:432-452)
#define BP2_FARP 16u             //   the primer-side one does
#define BP2_SLOW 0x8000u         //   every position of the row takes the exact path
#define BP2_UNFLAG 0x00800000u   //   flagged neither READ1 nor READ2: pairOrder is what the previous pileup read left (smCounter.py:359-362)
// letter codes of the linearised copies (general CIGARs, k_bp_rows_write) for positions that hold no plain base: the walk makes
// their words in its fast path.  As letters they index entries 4-6 of the walk's 8-entry tables (bits 1-3 of the byte)
#define BP2_LIN_LANES 16         // lanes of k_bp_lin that share one general CIGAR
#define BP2_C_NONE 0x01u       // none of the below: the exact path resolves the CIGAR
#define BP2_C_GAP 0x08u        // inside a deletion: allele 'DEL', quality minBQ (smCounter.py:416-418) - the pool's quality byte holds minBQ
#define BP2_C_INS 0x0Au        // the base before an insertion: an allele of its own (listed, numbered by k_bp_xfix2), the base's quality
#define BP2_C_DELS 0x0Cu       // the base before a deletion: likewise
#define BP_ST_NOPAIR 16u         // status: a pileup that begins with such an alignment (the reference has no pairOrder there)
//   bits 5-9 the read class of an excluded regular base, 10-14 of an included one (before its distance bits); bits 16-31 the
//   flag / MAPQ half of the meta word
struct BpRow { int32_t pos; uint32_t len; uint32_t wbase; uint32_t hi; int32_t cA, cP; uint32_t bc, pair; };
static_assert(sizeof(BpRow) == 32, "two 16-byte loads per row");

// is the CIGAR [clip] match [clip]?  -> that << 31 | query offset of the match's first base (the query position of a covered locus
// is then an offset: no CIGAR, no loop)
__device__ __forceinline__ uint32_t bp2_aux(const uint32_t* __restrict__ rec, const uint32_t* __restrict__ cig) {
    const uint32_t nc = rec[4] & 0xFFFFu;
    if (nc < 1u || nc > 3u) return 0u;
    const uint32_t* c = cig + rec[2];
    const uint32_t w0 = c[0], w1 = nc > 1u ? c[1] : 0x5u, w2 = nc > 2u ? c[2] : 0x5u;
    auto is_m = [](uint32_t x) { const uint32_t o = x & 15u; return o == 0u || o == 7u || o == 8u; };
    auto is_c = [](uint32_t x) { const uint32_t o = x & 15u; return o == 4u || o == 5u; };
    if (is_m(w0) && is_c(w1) && is_c(w2) && nc <= 2u) return 0x80000000u;
    if (is_c(w0) && is_m(w1) && is_c(w2)) return 0x80000000u | ((w0 & 15u) == 4u ? min(w0 >> 4, 0xFFFFu) : 0u);
    return 0u;
}
// bytes of the linearised pool a general CIGAR needs (0: it keeps the exact path)
__device__ __forceinline__ uint32_t bp2_lin_need(uint32_t aux, int pos, int end) {
    if (aux >> 31) return 0u;
    const uint32_t span = end > pos ? (uint32_t)(end - pos) : 0u;
    return (span == 0u || span > BP2_LIN_SPAN) ? 0u : ((span + 31u) & ~15u) + 64u;   // (+ 16: the walk loads 16 pairs from any position of the row; + 64: the copy starts where a tile's first position falls on a 128-byte line, as the decoder lays out the pool)
}
// (k_bp_rows_write's cursors, zeroed in stream order by a launch of our own: hipMemsetAsync left the device idle for ~ 100 us
// around its fill kernel - measured with the trace of one step)
__global__ __launch_bounds__(256) void k_bp_zero_words(uint32_t* __restrict__ p, uint32_t n) {
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) p[i] = 0u;
}

// what the pileup engine hands over for reference position p of an alignment (samtools resolve_cigar2 semantics as in
// smc_bam.cpp; smCounter.py:316 column.pileups -> query_position / is_del / indel)
struct BpRes { int qpos, indel; bool isdel; };
template <typename CIGP>
__device__ __forceinline__ BpRes bp2_resolve(CIGP c, int n_cig, int kpos, int p, int l_seq) {
    BpRes r; r.qpos = -1; r.indel = 0; r.isdel = false;
    int x = kpos, y = 0;
    for (int ci = 0; ci < n_cig; ++ci) {
        const uint32_t wv = c[ci];
        const int op = (int)(wv & 15u), len = (int)(wv >> 4);
        const bool ref_op = op == 0 || op == 7 || op == 8, gap_op = op == 2 || op == 3;
        if (ref_op || gap_op) {
            const int d = p - x;
            if ((uint32_t)d < (uint32_t)len) {
                r.qpos = ref_op ? y + d : y;
                r.isdel = gap_op;
                if (d == len - 1 && ci + 1 < n_cig) {                     // the peek at the next operation
                    const uint32_t nw = c[ci + 1];
                    r.indel = (nw & 15u) == 1u ? (int)(nw >> 4) : (nw & 15u) == 2u ? -(int)(nw >> 4) : 0;
                }
            }
            x += len;
            if (ref_op) y += len;
            if (x > p) break;
        } else if (op == 1 || op == 4) y += len;
    }
    if (r.isdel && r.indel != 0 && r.qpos >= l_seq) r.indel = 0;
    return r;
}

// ---- per alignment, once per run: the row record; for a general CIGAR the linearised bases / qualities and the end-distance
// constants in reference coordinates (lane = reference position, the CIGAR wave-uniform)
// ---- per alignment, once per run: the row record.  The alignments with a general CIGAR are listed (glist: by k_bp_rows_need's
// counts, no atomics) for k_bp_lin, which makes their copies in the second pool and their end-distance constants
__global__ __launch_bounds__(256) void k_bp_rows_write(BpArgs A, uint32_t n_aln, uint32_t* __restrict__ cursors /* BP_NCUR cursors of 32 words (a cache line each: one line
                                                       takes ~ 90 atomics per microsecond, and every workgroup asks twice): words 0-1 pairs of the cursor's
                                                       region of the second pool handed out, word 2 general CIGARs in its part of the list; zero before the
                                                       launch */, uint32_t* __restrict__ glist, uint32_t glist_stride,
                                                       BpRow* __restrict__ rows, uint32_t lin_cap, int raw, uint2* __restrict__ k8,
                                                       int32_t* __restrict__ k_end /* the alignment's end position, contiguous like k8: the sort drops
                                                       the rows that end before its tile by it */, uint32_t* __restrict__ zero, uint32_t zero_words, uint32_t* __restrict__ counters) {
    // Round 6: ONE launch where there were three (k_bp_rows_need -> k_bp_scan -> this kernel: each alignment's record and CIGAR read
    // twice, a one-workgroup prefix between them).  Where a general CIGAR's copy lies in the second pool and where it stands in the
    // list of k_bp_lin need not follow the file's order: a workgroup takes the pairs its alignments need and its places in the list
    // with ONE returning atomic each, its threads their shares by a prefix inside the workgroup.  (The pool offsets then differ from
    // launch to launch; nothing that reaches a read word depends on them.)
    __shared__ uint32_t ws[4], wc[4], base_cnt;
    __shared__ unsigned long long base_pool;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    // (the run's cleared scratch and the caller's two counters: nothing before this kernel touches them)
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < zero_words; i += gridDim.x * 256u) zero[i] = 0u;
    if (blockIdx.x == 0 && threadIdx.x < 2) counters[threadIdx.x] = 0u;
    const uint32_t a = blockIdx.x * 256u + (uint32_t)tid;
    const bool valid = a < n_aln;
    uint32_t nd = 0;
    if (valid) {
        const uint32_t* rec0 = (const uint32_t*)(A.aln + a);
        nd = bp2_lin_need(bp2_aux(rec0, A.cig), (int)rec0[0], (int)rec0[1]);
    }
    uint32_t inc = nd;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)inc, o); if (lane >= o) inc += u; }
    const unsigned long long gm = __builtin_amdgcn_ballot_w64(nd != 0u);
    if (lane == 63) { ws[wid] = inc; wc[wid] = (uint32_t)__popcll(gm); }
    __syncthreads();
    if (tid == 0) {
        const uint32_t ts = ws[0] + ws[1] + ws[2] + ws[3], tc = wc[0] + wc[1] + wc[2] + wc[3];
        // (alignments behind the end of the cursor's region keep the exact path: below)
        uint32_t* const cur = cursors + 32u * (blockIdx.x % BP_NCUR);
        base_pool = ts ? atomicAdd((unsigned long long*)cur, (unsigned long long)ts) : 0ull;
        base_cnt = tc ? atomicAdd(&cur[2], tc) : 0u;
    }
    __syncthreads();
    const uint32_t region = lin_cap / BP_NCUR;                                     // pairs of the second pool per cursor
    unsigned long long pre = base_pool;
    uint32_t gpre = (blockIdx.x % BP_NCUR) * glist_stride + base_cnt;
    for (int w = 0; w < wid; ++w) { pre += ws[w]; gpre += wc[w]; }
    if (nd != 0u) glist[gpre + bp_lanes_below(gm)] = a;
    const unsigned long long loc64 = 16ull + pre + inc - nd;                       // within the region (16: the walk may load from just before a row's first position)
    const unsigned long long off64 = (unsigned long long)(blockIdx.x % BP_NCUR) * region + loc64;
    bool lin = false;
    uint32_t off = 0;
    int kpos = 0, kend = 0;
    uint32_t kcig = 0, kseq = 0, k4 = 0, k5 = 0, k6 = 0;
    if (valid) {
        const uint32_t* rec = (const uint32_t*)(A.aln + a);
        kpos = (int)rec[0]; kend = (int)rec[1]; kcig = rec[2]; kseq = rec[3]; k4 = rec[4]; k5 = rec[5]; k6 = rec[6];
        const uint32_t aux = bp2_aux(rec, A.cig);
        const bool simple = aux >> 31;
        const bool unfl = !(((k4 >> 16) & 0xFFu) & (SMC_DA_R1 | SMC_DA_R2));
        lin = !simple && nd != 0u && !raw && !unfl && loc64 + nd <= (unsigned long long)region && (k4 & 0xFFFFu) <= 64u;   // (longer CIGARs: the exact path)
        off = (uint32_t)off64;
        off += ((uint32_t)(kpos - A.start0) - off) & 63u;                         // (position start0 + 64 t of the copy: pair 64 m of the pool)
        const uint32_t oflag = (k4 >> 16) & 0xFFu, mapq = k4 >> 24;
        const bool r2 = (oflag & SMC_DA_R2) != 0, rev = (oflag & SMC_DA_REV) != 0, mmok = (oflag & SMC_DA_MMOK) != 0;
        const bool mq_ok = (int)mapq >= A.min_mq && mmok;
        const bool farA = r2 != rev, farP = r2 && rev;
        // class of a regular base of this alignment, not included and its quality fine / included, before the end-distance terms:
        // smc_read_class's numbers, or smc_class16's for a run built with 16-bit read words
        const uint32_t cb0 = A.w16 ? 3u + (rev ? 2u : 0u) : 6u + (rev ? 8u : 0u), cinc = A.w16 ? 16u + (r2 ? 5u : 3u) + (rev ? 6u : 0u) : cb0 + (r2 ? 4u : 2u);
        BpRow R;
        R.pos = kpos; R.len = kend > kpos ? (uint32_t)(kend - kpos) : 0u;
        R.hi = ((r2 ? 1u : 0u) | (rev ? 2u : 0u) | (mmok ? 4u : 0u)) << 16 | mapq << 24 | (simple ? BP2_SIMPLE : 0u) | (mq_ok ? BP2_MQOK : 0u) |
               (r2 ? BP2_R2 : 0u) | (farA ? BP2_FARA : 0u) | (farP ? BP2_FARP : 0u) | cb0 << 5 | cinc << 10 | (((!simple && !lin) || unfl) ? BP2_SLOW : 0u) |
               (unfl ? BP2_UNFLAG : 0u);
        // end distance of locus p on a [clip] match [clip] row = (p ^ -far) + c (smCounter.py:432-452)
        const int base = (int)(aux & 0xFFFFu) - (int)(k5 & 0xFFFFu) - kpos, fbase = (int)(k5 >> 16) + 1 - base;
        R.cA = farA ? fbase : base;
        R.cP = r2 ? (farP ? fbase : base) : (1 << 29);                             // (read 1: never within primerDist of anything)
        R.wbase = simple ? kseq + (aux & 0xFFFFu) - (uint32_t)kpos : off - (uint32_t)kpos;
        R.bc = rec[7]; R.pair = rec[8];
        k8[a] = make_uint2(R.bc, R.pair);                                         // (what the sort reads: its keys, contiguous)
        k_end[a] = kend;
        uint4* o = (uint4*)(rows + a);
        o[0] = make_uint4((uint32_t)R.pos, R.len, R.wbase, R.hi);
        o[1] = make_uint4((uint32_t)R.cA, (uint32_t)R.cP, R.bc, R.pair);
    }
}

// ---- the general CIGARs, one wavefront per alignment (a grid-stride loop over the list): the copy of its bases and qualities by
// REFERENCE position in the second pool - operation by operation, lane = position within the operation; samtools resolve_cigar2
// semantics as bp2_resolve has them position by position - and the row's end-distance constants in reference coordinates.
//   a base of a match                          (letter, quality)
//   the last base of a match before an insertion / a deletion of length > 0:   BP2_C_INS / BP2_C_DELS with the base's quality
//   a position inside a deletion or a reference skip:   BP2_C_GAP with minBQ - unless it is the block's last position and an
//                                                        insertion / deletion follows while query bases remain (the exact path)
//   anything else                               BP2_C_NONE
// (before round 4's second half every wavefront of k_bp_rows_write walked its general CIGARs position by position, each position
// from the CIGAR's first operation: 0.15 of that kernel's 0.21 ms)
__global__ __launch_bounds__(256) void k_bp_lin(BpArgs A, const uint32_t* __restrict__ glist, uint32_t glist_stride, const uint32_t* __restrict__ cursors,
                                                BpRow* __restrict__ rows, uint8_t* __restrict__ lin_bq) {
    // (BP2_LIN_LANES lanes per alignment: an alignment is a chain of dependent fetches - list entry, records, CIGAR words, bases - and
    // a wavefront that took ONE at a time spent 5.8 us on each; four chains per wavefront, four times as many in flight)
    const int lane = threadIdx.x & (BP2_LIN_LANES - 1);
    // (the list has BP_NCUR parts, k_bp_rows_write's cursors say how long each is: WORKGROUP g takes part g % BP_NCUR - its sixteen
    // teams consecutive entries of it: neighbours in the file, whose records and bases share cache lines -, every
    // (workgroups / BP_NCUR)-th group of sixteen)
    constexpr uint32_t TPW = 256u / BP2_LIN_LANES;                                   // teams per workgroup
    const uint32_t part = blockIdx.x % BP_NCUR, wg_per = max(1u, gridDim.x / BP_NCUR), ng = cursors[32u * part + 2u];
    const bool gap_ok = A.min_bq >= 0 && A.min_bq <= 126;
    if (blockIdx.x / BP_NCUR >= wg_per) return;                                     // (workgroups beyond a whole number per part)
    for (uint32_t w = (blockIdx.x / BP_NCUR) * TPW + threadIdx.x / BP2_LIN_LANES; w < ng; w += wg_per * TPW) {
        const uint32_t a = glist[part * glist_stride + w];
        const BpRow R = rows[a];
        if ((R.hi & BP2_SLOW) || (R.hi & BP2_SIMPLE)) continue;                   // (no copy: unflagged, no room in the pool)
        const uint32_t* rec = (const uint32_t*)(A.aln + a);
        const int kpos = (int)rec[0], kend = (int)rec[1];
        const uint32_t kcig = rec[2], kseq = rec[3], k4 = rec[4], k5 = rec[5];
        const int n_cig = (int)(k4 & 0xFFFFu), l_seq = (int)(rec[6] & 0xFFFFu), left_sp = (int)(k5 & 0xFFFFu), qalen = (int)(k5 >> 16);
        const uint32_t off = R.wbase + (uint32_t)kpos;                              // the copy's first pair
        const int span = kend - kpos;
        const bool r2 = (R.hi & BP2_R2) != 0, farA = (R.hi & BP2_FARA) != 0, farP = (R.hi & BP2_FARP) != 0;
        const uint32_t* const cg = A.cig + kcig;
        uint8_t* const out = lin_bq + 2ull * off;
        const uint8_t* const src = A.bq + 2ull * kseq;
        int a_max = kpos - 1, a_min = kend, p_max = kpos - 1, p_min = kend;
        int x = 0, y = 0;                                                           // reference offset from kpos, query position
        for (int ci = 0; ci < n_cig; ++ci) {
            const uint32_t wv = cg[ci], nx = ci + 1 < n_cig ? cg[ci + 1] : 0u;     // (the same word for the alignment's lanes: one fetch)
            const int op = (int)(wv & 15u), len = (int)(wv >> 4);
            const bool indel_next = ((nx & 15u) == 1u || (nx & 15u) == 2u) && (nx >> 4) != 0u;
            if (op == 0 || op == 7 || op == 8) {
                const int nd = min(len, span - x);
                for (int d0 = lane; d0 < nd; d0 += 4 * BP2_LIN_LANES) {             // (four fetches in flight per lane before the first store)
                    uint32_t sq[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) { const int d = d0 + u * BP2_LIN_LANES; sq[u] = (d < nd && y + d < l_seq) ? *(const uint16_t*)(src + 2 * (y + d)) : 0u; }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int d = d0 + u * BP2_LIN_LANES;
                        if (d >= nd) break;
                        uint32_t site = sq[u] & 0xFFu, bq = sq[u] >> 8;
                        if (d == len - 1 && indel_next) { site = y + d < l_seq ? ((nx & 15u) == 1u ? BP2_C_INS : BP2_C_DELS) : BP2_C_NONE; bq = min(bq, 127u); }
                        else if (y + d >= l_seq) { site = BP2_C_NONE; bq = 0u; }
                        *(uint16_t*)(out + 2 * (x + d)) = (uint16_t)(site | bq << 8);
                    }
                }
                {   // the end-distance constants (smCounter.py:432-452): the positions within 20 of the barcode end (primerDist of the
                    // primer end) form a prefix - measured from the far end a suffix - of the row's plain bases
                    const int lastd = len - 1 - (indel_next ? 1 : 0), px = kpos + x;
                    auto upto = [&](int lim) { return min(lastd, lim + left_sp - y); };              // largest d with rd <= lim (rd = y + d - left_sp)
                    auto from = [&](int lim) { return max(0, qalen - lim + left_sp - y); };        // smallest d with qalen - rd <= lim
                    if (!farA) { const int d = upto(20); if (d >= 0) a_max = max(a_max, px + d); }
                    else { const int d = from(20); if (d <= lastd) a_min = min(a_min, px + d); }
                    if (r2) {
                        if (!farP) { const int d = upto(A.primer_dist); if (d >= 0) p_max = max(p_max, px + d); }
                        else { const int d = from(A.primer_dist); if (d <= lastd) p_min = min(p_min, px + d); }
                    }
                }
                x += len; y += len;
            } else if (op == 2 || op == 3) {
                for (int d = lane; d < len && x + d < span; d += BP2_LIN_LANES) {
                    const bool odd = d == len - 1 && indel_next && y < l_seq;       // (an indel straight after the block, query bases left: the exact path)
                    const uint32_t site = (odd || !gap_ok) ? BP2_C_NONE : BP2_C_GAP;
                    *(uint16_t*)(out + 2 * (x + d)) = (uint16_t)(site | (site == BP2_C_GAP ? (uint32_t)A.min_bq << 8 : 0u));
                }
                x += len;
            } else if (op == 1 || op == 4) y += len;
        }
        for (int d = max(x, 0) + lane; d < span; d += BP2_LIN_LANES) *(uint16_t*)(out + 2 * d) = (uint16_t)BP2_C_NONE;   // (a CIGAR shorter than the record's span)
        if (lane == 0) {
            int32_t* o = (int32_t*)(rows + a);
            o[4] = farA ? a_min + 21 : 20 - a_max;
            o[5] = !r2 ? (1 << 29) : farP ? p_min + A.primer_dist + 1 : A.primer_dist - p_max;
        }
    }
}

// ---- a segmented inclusive prefix OR over the lanes: S bit r = row r starts a run (bits of invalid lanes clear); carry = what
// the run that is open at lane 0 has covered before the batch.  Returns the inclusive scan, `pre` the exclusive one
__device__ __forceinline__ uint32_t bp2_seg_scan(uint32_t M, unsigned long long S, uint32_t carry, uint32_t& pre) {
    uint32_t x = M;
    const unsigned long long A1 = S, A2 = A1 | (A1 << 1), A4 = A2 | (A2 << 2), A8 = A4 | (A4 << 4);
    auto take = [&](unsigned long long keep, uint32_t t) { x |= __builtin_amdgcn_inverse_ballot_w64(keep) ? t : 0u; };
    take(~A1, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xF, 0xF, true));      // row_shr:1
    take(~A2, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xF, 0xF, true));
    take(~A4, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xF, 0xF, true));
    take(~A8, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xF, 0xF, true));
    // starts between the first lane of the lane's row of 16 and the lane
    unsigned long long P = S;
    P |= (P << 1) & ~0x0001000100010001ull; P |= (P << 2) & ~0x0003000300030003ull;
    P |= (P << 4) & ~0x000F000F000F000Full; P |= (P << 8) & ~0x00FF00FF00FF00FFull;
    take(~P & 0xFFFF0000FFFF0000ull, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false));   // row_bcast:15 into rows 1 and 3
    const unsigned long long Q = P | (((P >> 47) & 1ull) ? 0xFFFF000000000000ull : 0ull);                          // starts between lane 32 and the lane
    take(~Q & 0xFFFFFFFF00000000ull, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false));   // row_bcast:31 into rows 2 and 3
    const unsigned long long first = S ? ((S & (0ull - S)) - 1ull) : ~0ull;           // the lanes of the run that was open before the batch
    const uint32_t cin = __builtin_amdgcn_inverse_ballot_w64(first) ? carry : 0u;
    const uint32_t prev = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x138, 0xF, 0xF, true);                 // wave_shr:1
    pre = (__builtin_amdgcn_inverse_ballot_w64(~S) ? prev : 0u) | cin;
    return x | cin;
}
// lane `k` (a compile-time constant: the instruction takes one scalar register) of v := the wave-uniform value s
__device__ __forceinline__ void bp2_writelane(uint32_t& v, uint32_t s, int k) {
    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(v) : "s"(s), "n"(k));
}
__device__ __forceinline__ uint32_t bp2_wave_or(uint32_t v) {
    for (int o = 32; o; o >>= 1) v |= (uint32_t)__shfl_xor((int)v, o);
    return v;
}
__device__ __forceinline__ uint32_t bp2_cover(int d0, uint32_t len, int ng) {        // bit k: the row covers locus k of the group
    const int lo = min(max(-d0, 0), BP2_G), hi = min(max((int)len - d0, 0), ng);
    return hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
}

// The pipeline's loads, by hand.  The compiler's wait insertion treats a wavefront's loads and stores as returning out of order
// once both kinds are in flight (one counter, "mixed events"): every wait for a load it issues then becomes vmcnt(0) - a wait
// for every store of the walk.  The hardware returns them in issue order; so the hot loop's loads are issued here, the
// compiler does not know of them, and the loop waits for them itself with the count of operations it has issued since
// (bp2_landed: vmcnt(n) - at most n operations still in flight, the loads being older than the last n).
typedef uint32_t bp2_u4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void bp2_gload4(bp2_u4& d, const void* p) { asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(d) : "v"(p) : "memory"); }
__device__ __forceinline__ void bp2_gload1(uint32_t& d, const void* p) { asm volatile("global_load_dword %0, %1, off" : "=v"(d) : "v"(p) : "memory"); }
__device__ __forceinline__ unsigned long long bp2_cover64(int d0, uint32_t len, int nt) {   // bit k: the row covers locus k of the tile
    const int lo = min(max(-d0, 0), 64), hi = min(max((int)len - d0, 0), nt);
    if (hi <= lo) return 0ull;
    return (hi >= 64 ? ~0ull : ((1ull << hi) - 1ull)) & ~((1ull << lo) - 1ull);
}
// bp2_seg_scan on 64-bit masks (the scalar keep masks are made once)
__device__ __forceinline__ unsigned long long bp2_seg_scan64(unsigned long long M, unsigned long long S, unsigned long long carry, unsigned long long& pre) {
    uint32_t x0 = (uint32_t)M, x1 = (uint32_t)(M >> 32);
    const unsigned long long A1 = S, A2 = A1 | (A1 << 1), A4 = A2 | (A2 << 2), A8 = A4 | (A4 << 4);
    unsigned long long P = S;
    P |= (P << 1) & ~0x0001000100010001ull; P |= (P << 2) & ~0x0003000300030003ull;
    P |= (P << 4) & ~0x000F000F000F000Full; P |= (P << 8) & ~0x00FF00FF00FF00FFull;
    const unsigned long long Q = P | (((P >> 47) & 1ull) ? 0xFFFF000000000000ull : 0ull);
#define BP2_TAKE(keep, ctrl, rm, bc)                                                                             \
    {                                                                                                            \
        const bool kp = __builtin_amdgcn_inverse_ballot_w64(keep);                                               \
        const uint32_t t0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x0, ctrl, rm, 0xF, bc);               \
        const uint32_t t1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x1, ctrl, rm, 0xF, bc);               \
        x0 |= kp ? t0 : 0u; x1 |= kp ? t1 : 0u;                                                                  \
    }
    BP2_TAKE(~A1, 0x111, 0xF, true) BP2_TAKE(~A2, 0x112, 0xF, true) BP2_TAKE(~A4, 0x114, 0xF, true) BP2_TAKE(~A8, 0x118, 0xF, true)
    BP2_TAKE(~P & 0xFFFF0000FFFF0000ull, 0x142, 0xA, false) BP2_TAKE(~Q & 0xFFFFFFFF00000000ull, 0x143, 0xC, false)
#undef BP2_TAKE
    const unsigned long long first = S ? ((S & (0ull - S)) - 1ull) : ~0ull;
    const bool fl = __builtin_amdgcn_inverse_ballot_w64(first), ns = __builtin_amdgcn_inverse_ballot_w64(~S);
    const uint32_t c0 = fl ? (uint32_t)carry : 0u, c1 = fl ? (uint32_t)(carry >> 32) : 0u;
    const uint32_t p0 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x0, 0x138, 0xF, 0xF, true), p1 = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x1, 0x138, 0xF, 0xF, true);
    pre = (unsigned long long)((ns ? p0 : 0u) | c0) | (unsigned long long)((ns ? p1 : 0u) | c1) << 32;
    return (unsigned long long)(x0 | c0) | (unsigned long long)(x1 | c1) << 32;
}
__device__ __forceinline__ unsigned long long bp2_rl64(unsigned long long v, int l) {
    return (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l) |
           (unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l) << 32;
}

// ---- the walk: ONE wavefront per (tile of 64 loci, part of the tile's sorted list); 64 rows at a time, lane = row.  A row's
// record, its coverage of the tile (a 64-bit mask) and the run structure are per batch; bases and qualities are taken 16 loci
// (a GROUP) at a time - two 16-byte loads per lane and group, requested one group ahead -, and the per-locus state (where
// the locus's next word goes, its column of the batch) lives in VGPR lanes with lane = locus.
// (The first transposed version gave each group of 16 loci a wavefront of its own, four per workgroup: the four loaded the
// same row records and neighbouring window bytes at the same time - the counters showed the vector L1 stalled on lines already
// pending for 66 % of the kernel's cycles and every row record fetched four times.)
template <bool RAW /* the raw-field planes as well (checks only) */, bool W16 /* the read words in 16 bits (smc_read_word16): not with RAW */>
// (NO register cap on this kernel: its pipeline loads are inline assembly whose results are in flight until bp2's own waits - a
// spill of such a register, which a cap forces, stores it before it has arrived.  tests/test_host_logic.py checks that the
// built kernel uses no scratch.)
__global__ __launch_bounds__(64) void k_bp_emit2(BpArgs A, const BpRow* __restrict__ rows, const uint8_t* __restrict__ lin_bq) {
    __shared__ uint32_t xq[BP_XQ * BP_XW];
    __shared__ uint32_t stage[(BP2_ABL & 0x8000) ? 33 * 68 : 1];
    const int lane = threadIdx.x;
    constexpr int WSH = W16 ? 1 : 2;                                              // log2 of a read word's bytes
    static_assert(!(RAW && W16), "the raw-field planes go with 32-bit words");
    // (tile, part) wavefronts that follow each other in the list - the same tile, then the next: they read the same alignments -
    // go to ONE XCD (workgroups are dealt round-robin over the eight), so that its L2 serves the second reader
    uint32_t vb = blockIdx.x;
    if (!(BP2_ABL & 16)) {
        const uint32_t G = A.xcd_rot >> 8;                      // (experiments, SMC_BP_XCD_GROUP) 0: every XCD takes a contiguous eighth of the wavefronts
        if (G == 0u) { const uint32_t per = gridDim.x >> 3; if (vb < per * 8u) vb = (((vb & 7u) + (A.xcd_rot & 7u)) & 7u) * per + (vb >> 3); }
        else {                                                  // groups of G consecutive wavefronts (~ a tile's parts) dealt round-robin to the XCDs
            const uint32_t full = gridDim.x / (8u * G) * (8u * G);
            if (vb < full) { const uint32_t x = vb & 7u, idx = vb >> 3; vb = ((idx / G) * 8u + x) * G + idx % G; }
        }
    }
    const BpWave W = bp_wave<false>(A, lane, vb);
    const int tile = W.tile, l0 = tile * BP_TILE, p0 = W.p_first;
    const int nt = W.p_last - W.p_first + 1;                                      // loci of the tile
    if (*(volatile uint32_t*)A.status & BP_ST_DEPTH) return;                       // (a depth the host did not count: k_bp_scan_tiles; the caller falls back)
    const uint32_t a_lo = W.a_lo, a_hi = W.a_hi, j0 = W.j0, j1 = W.j1;
    if (j0 >= j1) return;
    // ---- per locus of the tile (lane k = locus k): where its next word / umi_start entry goes - BYTE offsets from the tile's
    // first slot / entry, so that a store is scalar base + 32-bit lane offset -, what it has seen so far
    uint32_t v_wb = 0, v_rel = 0, v_ub = 0, v_cf = 0, v_cu = 0;
    unsigned long long wdsm;
    uint32_t slot0, ustart0;
    {
        bool v_wds = false;
        uint32_t so = 0xFFFFFFFFu, uo = 0xFFFFFFFFu, c_r = 0, c_u = 0;
        if (lane < nt) {
            const smc_dev_locus LC = A.loc[l0 + lane];
            // (k_bp_scan_tiles' prefix up to the count walk's part + that part's earlier stretches of 64 rows, a byte per count)
            const uint32_t* cw = A.cnt + (size_t)W.cpart * 192u + (uint32_t)lane;
            c_r = cw[0]; v_cf = cw[64]; c_u = cw[128];
            for (uint32_t i = 0; i < W.csub; ++i) {
                const uint32_t pk = A.cntp[(size_t)(vb - W.csub + i) * 64u + (uint32_t)lane];
                c_r += pk & 0xFFu; v_cf += (pk >> 8) & 0xFFu; c_u += pk >> 16;
            }
            so = A.slot_base + LC.slot_off; uo = A.umi_base + LC.slot_off + (uint32_t)(l0 + lane);
            v_rel = c_r; v_cu = c_u;
            v_wds = A.ds > 0 && A.loci[l0 + lane].n_umi > A.ds;                     // (written by k_bp_scan_tiles)
        }
        wdsm = __builtin_amdgcn_ballot_w64(v_wds);
        uint32_t m0 = so, m1 = uo;
        for (int o = 32; o; o >>= 1) { m0 = min(m0, (uint32_t)__shfl_xor((int)m0, o)); m1 = min(m1, (uint32_t)__shfl_xor((int)m1, o)); }
        slot0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)m0); ustart0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)m1);
        const bool far = lane < nt && (so - slot0 + c_r >= (1u << 29) || uo - ustart0 + c_u >= (1u << 29));
        if (__builtin_amdgcn_ballot_w64(far)) {                                   // (a tile whose loci lie gigabytes apart: not a run the decoder makes)
            if (lane == 0) atomicOr(A.status, BP_ST_DEPTH);
            return;
        }
        if (lane < nt) { v_wb = (so - slot0 + c_r) << WSH; v_ub = (uo - ustart0 + c_u) << 2; }
    }
    uint32_t* const outp[4] = {A.meta, A.frag, A.umi, A.dist};
    const uint32_t* const sorted = A.sorted;
    const uint8_t* const bqp = A.bq;
    uint32_t xq_n = 0;
    auto xflush = [&]() {                                                         // the listed extra-allele reads -> the global list, one atomic
        if (xq_n == 0u) return;
        __builtin_amdgcn_wave_barrier();
        uint32_t xb = 0;
        if (lane == 0) { xb = atomicAdd(A.xraw_n, xq_n); atomicAdd(&A.tcnt[tile], xq_n); }
        xb = (uint32_t)__builtin_amdgcn_readfirstlane((int)xb);
        for (uint32_t i = (uint32_t)lane; i < xq_n; i += 64u) {
            if (xb + i < A.xraw_cap) {
                uint32_t* e = xq + BP_XW * i;
                if (e[3] == 0xFFFFFFFFu) {                                        // listed by the fast path: query position and length from the CIGAR
                    const uint32_t* rec = (const uint32_t*)(A.aln + e[2]);
                    const BpRes r = bp2_resolve(A.cig + rec[2], (int)(rec[4] & 0xFFFFu), (int)rec[0], p0 + (int)e[0] - l0, (int)(rec[6] & 0xFFFFu));
                    e[3] = (uint32_t)r.qpos; e[4] = (uint32_t)r.indel;
                }
                {   // the allele key's hash, here where thousands of wavefronts hide its fetches (k_bp_xfix2 has one wavefront per tile)
                    const unsigned long long h = bp_key_hash(A.aln[e[2]], A.bq, (int)e[3], (int)e[4]);
                    e[6] = (uint32_t)h; e[7] = (uint32_t)(h >> 32);
                }
                uint32_t* o = A.xraw + (size_t)BP_XW * (xb + i);
#pragma unroll
                for (int k = 0; k < BP_XW; ++k) o[k] = e[k];
                atomicAdd(&A.xcnt[e[0]], 1u);
            } else atomicOr(A.status, BP_ST_XLIST);
        }
        __builtin_amdgcn_wave_barrier();
        xq_n = 0;
    };
    // ---- the open runs before the part: what they have covered (the stretch [jb, j0) holds one barcode: bp_wave)
    // (k_bp_count has left them: which loci the barcode / the read pair of this wavefront's first row has covered before it)
    uint32_t carry_bc = 0xFFFFFFFFu, carry_pair = 0xFFFFFFFFu;
    unsigned long long CB, CP;
    {
        const uint32_t* stw = A.pstate + (size_t)vb * 4u;
        CB = (unsigned long long)stw[0] | (unsigned long long)stw[1] << 32;
        CP = (unsigned long long)stw[2] | (unsigned long long)stw[3] << 32;
    }
    const int min_bq_c = min(max(A.min_bq, 0), 127);
    const uint32_t KOK = (uint32_t)(128 - min_bq_c) * 0x01010101u;   // byte + KOK: bit 7 = quality >= minBQ (qualities < 128)
    const int primer_dist = A.primer_dist;
    // ---- the pipeline.  No branch around any load or store of the hot loop, and the loads issued by hand: loads and stores of a
    // wavefront share one in-order counter, and the compiler's wait insertion (a) counts over every path into a block - one path
    // without the stores makes the wait a wait for all of them - and (b) treats loads and stores in flight together as out of
    // order: vmcnt(0).  So every load has a valid address (indices clamped, rows without a window read byte 0 of the pool), a
    // store reaches memory or not by its OFFSET (buffer stores: an offset beyond the descriptor's range is dropped), and the
    // requests run ahead - sorted-list indices two batches, row records one, the row's bases and qualities from the head of its batch.
    const uint32_t jl = j1 - 1u;
    auto idx_ptr = [&](uint32_t c0) -> const uint32_t* { return sorted + min(c0 + (uint32_t)lane, jl); };
    // where a row's 64 bases / qualities under the tile lie; ok: it has such a window (else every covered position is exact).
    // ALL of them are requested at the head of the row's batch, in one go: the first version of this kernel fetched them 16 at
    // a time, a group ahead - and 58 % of those 16-byte loads found their 128-byte line gone from L1 AND from L2 again (13 us
    // between two groups of a batch: 8.4 GB of DRAM reads per launch for 1.2 GB of bases and qualities)
    auto win_ptr = [&](const bp2_u4& r0, unsigned long long M, bool& ok, const uint8_t*& wp) {
        const uint32_t hi = r0.w;
        const long long off = (long long)(uint32_t)(r0.z + r0.x) + (long long)(p0 - (int)r0.x);
        ok = M != 0ull && !(hi & BP2_SLOW) && off >= 0;                            // (off < 0: the run's very first bases - nothing readable before them)
        const bool own = (hi & BP2_SIMPLE) != 0 || !ok;
        wp = (own ? bqp : lin_bq) + (ok ? 2ll * off : 0ll);                        // (letter, quality) pairs: 128 bytes under the tile
        if (BP2_ABL & 2) wp = bqp;
        if (BP2_ABL & 0x700) wp = (const uint8_t*)((unsigned long long)wp & ~(unsigned long long)((BP2_ABL & 0x100) ? 3 : (BP2_ABL & 0x200) ? 15 : 31));   // (timing only: aligned windows)
    };
    auto cover_of = [&](uint32_t c0, uint32_t a, const bp2_u4& r0) -> unsigned long long {
        const bool in = c0 < j1 && c0 + (uint32_t)lane < j1;
        return (in && a >= a_lo && a < a_hi) ? bp2_cover64(p0 - (int)r0.x, r0.y, nt) : 0ull;
    };
    // BP2_ABL: timing-only builds (1: no word reaches memory, 2: every window is the pool's first bytes, 4: every batch reads the
    // same 64 row records, 8: no umi_start entry reaches memory)
    const __amdgpu_buffer_rsrc_t rs_words = __builtin_amdgcn_make_buffer_rsrc((char*)A.words + ((size_t)slot0 << WSH), 0, (BP2_ABL & 1) ? 0 : 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_umi = __builtin_amdgcn_make_buffer_rsrc((char*)(A.umi_start + ustart0), 0, (BP2_ABL & 8) ? 0 : 0x7FFFFFFF, 0x00020000);
    // state at the head of batch i: its rows (arrived), the indices of batch i + 1 (arrived)
    uint32_t a_cur = *idx_ptr(j0), a_p1 = *idx_ptr(j0 + 64u);
    bp2_u4 r0c, r1c;
    {
        const bp2_u4* rp = (const bp2_u4*)(rows + a_cur);
        r0c = rp[0]; r1c = rp[1];
    }
    // (a first row whose barcode / pair HAS covered something before continues that run; else it starts one, as before)
    if (CB) carry_bc = (uint32_t)__builtin_amdgcn_readfirstlane((int)r1c.z);
    if (CP) carry_pair = (uint32_t)__builtin_amdgcn_readfirstlane((int)r1c.w);
    // (these - the compiler's own loads - have to have ARRIVED when the loop is entered: see above)
    asm volatile("" ::"v"(r0c), "v"(r1c), "v"(a_p1));
    for (uint32_t c0 = j0; c0 < j1; c0 += 64u) {
        const uint32_t nv = min(64u, j1 - c0), last = nv - 1u;                    // rows of the batch
        const uint32_t a = a_cur;
        const bool in = (uint32_t)lane < nv;
        const int pos = (int)r0c.x;
        const uint32_t hi = r0c.w, bcv = r1c.z, prv = r1c.w;
        const int cAv = (int)r1c.x, cPv = (int)r1c.y;
        const unsigned long long Mc = cover_of(c0, a, r0c);
        // ---- the row's bases and qualities under the tile: eight loads into registers, used 16 loci at a time
        bp2_u4 S[4], Q[4];                                                       // of group g: S its loci 0-7, Q its loci 8-15
        bool wokc;
        {
            const uint8_t* wp;
            win_ptr(r0c, Mc, wokc, wp);
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int go = (BP2_ABL & 32) ? 0 : (BP2_ABL & 64) ? 4096 * g : 2 * BP2_G * g;   // (timing only: 32 one chunk four times, 64 four different lines)
                bp2_gload4(S[g], wp + go); bp2_gload4(Q[g], wp + go + 16);
            }
        }
        // ---- the batches after: row records of i + 1, indices of i + 2
        uint32_t a_new;
        bp2_u4 r0_new, r1_new;
        {
            const bp2_u4* rp = (const bp2_u4*)(rows + a_p1);
            bp2_gload4(r0_new, rp); bp2_gload4(r1_new, rp + 1);
            bp2_gload1(a_new, idx_ptr(c0 + 128u));
        }
        // ---- runs of equal barcode / read pair among the rows
        const uint32_t bcp = (uint32_t)__builtin_amdgcn_update_dpp((int)carry_bc, (int)bcv, 0x138, 0xF, 0xF, false);     // the row before (lane 0: before the batch)
        const uint32_t prp = (uint32_t)__builtin_amdgcn_update_dpp((int)carry_pair, (int)prv, 0x138, 0xF, 0xF, false);
        const unsigned long long SB = __builtin_amdgcn_ballot_w64(in && bcv != bcp), SP = __builtin_amdgcn_ballot_w64(in && prv != prp);
        carry_bc = (uint32_t)__builtin_amdgcn_readlane((int)bcv, (int)last); carry_pair = (uint32_t)__builtin_amdgcn_readlane((int)prv, (int)last);
        // ---- which rows start a barcode / a fragment at which loci (64-bit masks per lane)
        unsigned long long preB, preP, xP;
        const unsigned long long xB = bp2_seg_scan64(Mc, SB, CB, preB);
        {
            const unsigned long long vm = nv >= 64u ? ~0ull : ((1ull << nv) - 1ull), cont = ~SP & vm;
            if (cont & (cont >> 1)) xP = bp2_seg_scan64(Mc, SP, CP, preP);       // a read pair with three or more alignments in the batch
            else {                                                              // runs of one or two rows: the row before is all there is
                const bool ns = __builtin_amdgcn_inverse_ballot_w64(~SP);
                const uint32_t q0 = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)CP, (int)(uint32_t)Mc, 0x138, 0xF, 0xF, false);
                const uint32_t q1 = (uint32_t)__builtin_amdgcn_update_dpp((int)(uint32_t)(CP >> 32), (int)(uint32_t)(Mc >> 32), 0x138, 0xF, 0xF, false);
                preP = (unsigned long long)(ns ? q0 : 0u) | (unsigned long long)(ns ? q1 : 0u) << 32;
                xP = Mc | preP;
            }
        }
        const unsigned long long HB = Mc & ~preB, NF = Mc & ~preP;
        CB = bp2_rl64(xB, (int)last); CP = bp2_rl64(xP, (int)last);
        // ---- what is the same for the row's 64 loci
        const bool mq = (hi & BP2_MQOK) != 0, farA = (hi & BP2_FARA) != 0, farP = (hi & BP2_FARP) != 0;
        // (class of a regular base of this row when it is not included and its quality is fine / when it is included, before the
        // end-distance terms - smc_read_class's numbering from the row record, smc_class16's from the row's strand and read number)
        // (k_bp_rows_write numbers them for the words the run is built with)
        const uint32_t rev1 = (hi >> 17) & 1u;
        const uint32_t cb0 = (hi >> 5) & 31u, cinc = (hi >> 10) & 31u;
        const uint32_t CEX1 = (cb0 + 1u) * 0x01010101u, CIN = (mq ? cinc : cb0) * 0x01010101u, MQ2 = mq ? 0x02020202u : 0u;
        const uint32_t XA = farA ? 0u : 0x0F0F0F0Fu, XP = farP ? 0u : 0x0F0F0F0Fu;
        // locus k of a group starting at position pg is within 20 of the barcode end iff k >= t (far end) or k <= t:
        // as "byte + c has bit 7" on k or on 15 - k; t moves by 16 from group to group
        const int tA0 = farA ? cAv - 21 - p0 : 15 - (20 - cAv - p0), tP0 = farP ? cPv - primer_dist - 1 - p0 : 15 - (primer_dist - cPv - p0);
        unsigned long long spm = RAW ? Mc : 0ull;                                 // the lane's positions for the exact path
        uint32_t xs = 0xFFu;                                                      // the locus of the row's insertion / deletion start the fast path met: to be listed
        uint32_t v_Clo = 0, v_Chi = 0;                                            // lane k: the column of locus k - which rows cover it
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const uint32_t Mg = (uint32_t)(Mc >> (BP2_G * g)) & 0xFFFFu, NFg = (uint32_t)(NF >> (BP2_G * g)) & 0xFFFFu;
            // (the windows were requested at the head of the batch, before its scans; the 11 loads are the batch's first memory
            // operations, so everything but the stores of the groups before has to have come back)
            // (the next batch's row records and the index after them ride on the same wait: as operands of it no use or copy of
            // them can be scheduled ahead of it, whatever the block layout - ADVICE r4)
            if (g == 0) asm volatile("s_waitcnt vmcnt(0)" : "+v"(S[0]), "+v"(Q[0]), "+v"(S[1]), "+v"(Q[1]), "+v"(S[2]), "+v"(Q[2]), "+v"(S[3]), "+v"(Q[3]),
                                                           "+v"(r0_new), "+v"(r1_new), "+v"(a_new)::"memory");
            const int dg = farA ? -BP2_G * g : BP2_G * g, dgp = farP ? -BP2_G * g : BP2_G * g;
            const int uA = !mq ? BP2_G : min(max(tA0 + dg, 0), BP2_G), uP = !mq ? BP2_G : min(max(tP0 + dgp, 0), BP2_G);
            const uint32_t cA4 = (uint32_t)(128 - uA) * 0x01010101u, cP4 = (uint32_t)(128 - uP) * 0x01010101u;
            uint32_t qacc = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                // four loci's (letter, quality) pairs -> their four letters and their four qualities
                const uint32_t w_lo = q == 0 ? S[g].x : q == 1 ? S[g].z : q == 2 ? Q[g].x : Q[g].z, w_hi = q == 0 ? S[g].y : q == 1 ? S[g].w : q == 2 ? Q[g].y : Q[g].w;
                const uint32_t s = __builtin_amdgcn_perm(w_hi, w_lo, 0x06040200u), qq = __builtin_amdgcn_perm(w_hi, w_lo, 0x07050301u);
                // four loci as byte lanes: letter -> allele id / canonical letter through v_perm_b32 as an 8-entry table indexed by
                // bits 1-3 of the letter (A 0, C 1, T 2, G 3, N 7)
                const uint32_t sel = (s >> 1) & 0x07070707u;
                const uint32_t a4 = __builtin_amdgcn_perm(0x04060605u, 0x02010300u, sel);   // (4-6: the codes of k_bp_rows_write - 'DEL', two alleles to be numbered)
                const uint32_t l4 = __builtin_amdgcn_perm(0x4E0C0A08u, 0x47544341u, sel);
                const uint32_t x4 = l4 ^ s;                                      // a byte that is not zero: not one of A, C, G, T, N
                {   // qualities under the loci the row covers (the other bytes may be anything)
                    const uint32_t cb = ((((Mg >> (4 * q)) & 15u) * 0x00204081u) & 0x01010101u) << 7, cm = (cb - (cb >> 7)) | cb, qc = qq & cm;
                    // (32-bit words: a quality beyond 126 - bit 7 of the byte or of the byte + 1; 16-bit words: beyond 63 - bit 6 or 7 of
                    // the byte ITSELF: with the + 1 a quality of exactly 63 read as 64, and a file that has one was built a second time
                    // with 32-bit words for nothing (ADVICE r5); a run that breaks either is rebuilt with 32-bit words, whose walk looks again)
                    qacc |= W16 ? qc : (qc | ((qc & 0x7F7F7F7Fu) + 0x01010101u));
                }
                // (the add is carry-free only for bytes < 0x80: a quality byte under a locus the row does NOT cover may be anything - the
                // pairs around a general CIGAR's copy in the second pool are never written - and 0x8D or more there carried into the
                // byte above it: a read with bq = minBQ - 1 at its row's first position became an included one.  Found by
                // scripts/fa_soak.py in round 5, there since round 4; tests/test_gpu_from_alignments.py poisons the scratch.)
                const uint32_t okb = ((qq & 0x7F7F7F7Fu) + KOK) & 0x80808080u, okm = okb - (okb >> 7);   // 0x7F where bq >= minBQ (every byte it selects from is < 0x80)
                const uint32_t K4 = 0x03020100u + 0x04040404u * (uint32_t)q;
                const uint32_t dA = (K4 ^ XA) + cA4, dP = (K4 ^ XP) + cP4;
                const uint32_t X = CIN + ((dA >> 7) & 0x01010101u) + ((dP >> 6) & 0x02020202u);
                uint32_t c4 = ((X & okm) | (CEX1 & ~okm)) << 3;                  // (smc_read_class of a regular base) << 3
                const uint32_t nf4 = (((NFg >> (4 * q)) & 15u) * 0x00204081u) & 0x01010101u;   // the four loci's fragment-start bits, one per byte
                const uint32_t f4 = (okm & MQ2) | 0x04040404u | nf4;             // (SMC_RW_NF | SMC_RW_INC | SMC_RW_OK) >> 16
                // (rare) bytes that are codes of k_bp_rows_write: the class byte comes from the row's table CSP instead - four loci at a
                // time, as everything here; an insertion / deletion start is noted for the list
                const uint32_t isp = (s >> 3) & (~s >> 6) & 0x01010101u;           // bit 3 without bit 6: 0x08, 0x0A, 0x0C (and nothing a letter is)
                if (__builtin_amdgcn_ballot_w64(isp != 0u && wokc)) {
                    const uint32_t cov4 = (Mg >> (4 * q)) & 15u;
                    const uint32_t ib = (isp | isp >> 7 | isp >> 14 | isp >> 21) & cov4;        // one bit per covered locus with a code
                    if (!wokc || !isp) {}
                    else if (hi & BP2_SIMPLE) spm |= (unsigned long long)ib << (BP2_G * g + 4 * q);   // (not a row of the linearised pool: whatever these bytes are)
                    else {
                        // (class << 3 of a read inside a deletion: 0 + incCond with incCond = MAPQ and mismatches fine; at an insertion /
                        // deletion start with bq >= minBQ, and with bq below: 2 + 2 * reverse + incCond, incCond as for a base - smc_read_class)
                        const uint32_t CSP = W16 ? ((mq ? 128u : 0u) | ((mq ? 128u : 0u) + 8u + 8u * rev1) << 8 | (8u + 8u * rev1) << 16)   // (smc_class16 << 3: INC << 7 | (1 + reverse) << 3)
                                                 : ((mq ? 8u : 0u) | (16u + ((hi >> 13) & 16u) + (mq ? 8u : 0u)) << 8 | (16u + ((hi >> 13) & 16u)) << 16);
                        const uint32_t m = (isp << 8) - isp, t = (((s >> 1) | (s >> 2)) & isp);   // t: 1 = a start (0x0A, 0x0C), 0 = inside a deletion
                        const uint32_t ti = t + (t & ~okm);                                       // the entry of CSP: 0 in-deletion, 1 start with bq >= minBQ, 2 below
                        c4 = __builtin_amdgcn_perm(CSP, c4, (0x03020100u & ~m) | ((0x04040404u + ti) & m));
                        uint32_t sb = (t | t >> 7 | t >> 14 | t >> 21) & cov4;                    // covered starts
                        if (sb && xs == 0xFFu) { xs = (uint32_t)(BP2_G * g + 4 * q) + (uint32_t)__builtin_ctz(sb); sb &= sb - 1u; }
                        spm |= (unsigned long long)sb << (BP2_G * g + 4 * q);                     // (a second start of the row in the tile: the exact path)
                    }
                }
                // 32-bit words: (allele, quality) and (flags, class << 3) halves of two loci each.  16-bit words (smc_read_word16): low
                // byte allele | NF << 4 | INC << 5 | class index bits 0-1 << 6, high byte quality | class index bits 2-3 << 6 - the class
                // byte is smc_class16 << 3, its bit 7 the INC bit
                const uint32_t lo4 = a4 | nf4 << 4 | ((c4 >> 2) & 0x20202020u) | ((c4 << 3) & 0xC0C0C0C0u), hi4 = (qq & 0x3F3F3F3Fu) | ((c4 << 1) & 0xC0C0C0C0u);
                const uint32_t aq[2] = {__builtin_amdgcn_perm(qq, a4, 0x05010400u), __builtin_amdgcn_perm(qq, a4, 0x07030602u)};
                const uint32_t fc[2] = {__builtin_amdgcn_perm(c4, f4, 0x05010400u), __builtin_amdgcn_perm(c4, f4, 0x07030602u)};
                if (__builtin_amdgcn_ballot_w64(x4 != 0u && wokc)) {             // (rare: an unusual letter - which of the four, and is it under a covered locus)
#pragma unroll
                    for (int jq = 0; jq < 4; ++jq)
                        if (wokc && ((x4 >> (8 * jq)) & 0xFFu)) spm |= (unsigned long long)(Mg & (1u << (4 * q + jq))) << (BP2_G * g);
                }
#pragma unroll
                for (int jq = 0; jq < 4; ++jq) {
                    const int k = 4 * q + jq;
                    const unsigned long long C = __builtin_amdgcn_ballot_w64((Mg >> k) & 1u);
                    const uint32_t wbk = (uint32_t)__builtin_amdgcn_readlane((int)v_wb, BP2_G * g + k);
                    const uint32_t word = W16 ? __builtin_amdgcn_perm(hi4, lo4, 0x0C0C0400u + 0x0101u * (uint32_t)jq)     // (low byte, high byte) of locus jq
                                              : __builtin_amdgcn_perm(fc[jq >> 1], aq[jq >> 1], (jq & 1) ? 0x07060302u : 0x05040100u);
                    if (BP2_ABL & 0xE000) {       // (timing only: the words leave after the groups, as 16-byte pieces: below)
                        if (BP2_ABL & 0x8000) {   // ... through LDS: the write half of the transposition
                            const uint32_t la = __builtin_amdgcn_inverse_ballot_w64(C) ? ((uint32_t)(k & 31) * 68u + bp_lanes_below(C)) : (32u * 68u + (uint32_t)lane);
                            stage[la] = word;
                        }
                    } else
                    if (BP2_ABL & 0x800)          // (timing only: two bytes per read instead of four - the same store instructions, half the bytes)
                        __builtin_amdgcn_raw_buffer_store_b16((short)word, rs_words, __builtin_amdgcn_inverse_ballot_w64(C) ? (bp_lanes_below(C) << 1) + (wbk >> 1) : 0xFFFFFFFFu, 0, 0);
                    else if (BP2_ABL & 0x1000) {  // (timing only: the same bytes in half the store instructions - even loci store two dwords per lane)
                        typedef uint32_t u2 __attribute__((ext_vector_type(2)));
                        if (!(k & 1)) __builtin_amdgcn_raw_buffer_store_b64(u2{word, word}, rs_words, __builtin_amdgcn_inverse_ballot_w64(C) ? (bp_lanes_below(C) << 3) + wbk : 0xFFFFFFFFu, 0, 0);
                    } else if (W16)
                    __builtin_amdgcn_raw_buffer_store_b16((short)word, rs_words, __builtin_amdgcn_inverse_ballot_w64(C) ? (bp_lanes_below(C) << 1) + wbk : 0xFFFFFFFFu, 0, BP2_STORE_AUX);
                    else
                    __builtin_amdgcn_raw_buffer_store_b32(word, rs_words, __builtin_amdgcn_inverse_ballot_w64(C) ? (bp_lanes_below(C) << 2) + wbk : 0xFFFFFFFFu, 0, BP2_STORE_AUX);
                    if (BP2_ABL & 0xF800) {       // (the ablation builds' register allocation puts the ballot into a VGPR: the asm wants an SGPR)
                        bp2_writelane(v_Clo, (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)C), BP2_G * g + k);
                        bp2_writelane(v_Chi, (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(C >> 32)), BP2_G * g + k);
                    } else {
                    bp2_writelane(v_Clo, (uint32_t)C, BP2_G * g + k); bp2_writelane(v_Chi, (uint32_t)(C >> 32), BP2_G * g + k);
                    }
                }
            }
            // (16-bit words: bit 6 of a quality byte itself says "beyond 63" - no room in the word)
            if (__builtin_amdgcn_ballot_w64((qacc & (W16 ? 0xC0C0C0C0u : 0x80808080u)) != 0u)) {   // a quality beyond 126 somewhere near: under a covered locus?
                if (wokc && (qacc & (W16 ? 0xC0C0C0C0u : 0x80808080u))) atomicOr(A.status, ((qacc & 0x80808080u) ? BP_ST_BQ : 0u) | (W16 ? BP_ST_NARROW : 0u));
            }
        }
        const uint32_t v_nC = (uint32_t)__popc(v_Clo) + (uint32_t)__popc(v_Chi);   // lane k: reads of the batch at locus k
        if (BP2_ABL & 0xE000) {
            // timing only: what a transposed flush would issue - sixteen stores of 16 bytes per lane, four loci each (a locus's run
            // of the batch as up to sixteen pieces), instead of 64 of one dword per covering row.  0x2000: at the run's own (4-byte)
            // alignment; 0x4000: pieces on 16-byte boundaries; 0x8000: + the LDS traffic of the transposition
            typedef uint32_t u4s __attribute__((ext_vector_type(4)));
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int loc = 4 * j + (lane >> 4), piece = lane & 15;
                const uint32_t n = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * loc, (int)v_nC), wb = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * loc, (int)v_wb);
                u4s dat = {n, wb, (uint32_t)j, (uint32_t)lane};
                if (BP2_ABL & 0x8000) dat = *(const u4s*)&stage[(uint32_t)(loc & 31) * 68u + 4u * (uint32_t)piece];
                const uint32_t off = ((BP2_ABL & 0x4000) ? (wb & ~15u) : wb) + 16u * (uint32_t)piece;
                __builtin_amdgcn_raw_buffer_store_b128(dat, rs_words, 4u * (uint32_t)piece < n ? off : 0xFFFFFFFFu, 0, 0);
            }
        }
        // ---- umi_start: the rows that start a barcode somewhere are few (one or two per barcode); each is taken with LANE = LOCUS -
        // its rank at locus k is a popcount of the locus's column below the row
        uint32_t v_nB = 0;                                                        // lane k: barcode heads of the batch at locus k so far
        for (unsigned long long hl = __builtin_amdgcn_ballot_w64(HB != 0ull); hl; hl &= hl - 1ull) {
            const int r = __builtin_ctzll(hl);
            const bool act = __builtin_amdgcn_inverse_ballot_w64(bp2_rl64(HB, r));
            const unsigned long long lt = (1ull << r) - 1ull;
            const uint32_t rank = (uint32_t)__popc(v_Clo & (uint32_t)lt) + (uint32_t)__popc(v_Chi & (uint32_t)(lt >> 32));
            __builtin_amdgcn_raw_buffer_store_b32(v_rel + rank, rs_umi, act ? v_ub + (v_nB << 2) : 0xFFFFFFFFu, 0, 0);
            v_nB += act ? 1u : 0u;
        }
        // ---- the insertion / deletion starts the fast path met are listed (their allele ids come later, k_bp_xgroup ...): per such
        // (row, locus) the slot its word went to - the locus's column and offset come from the locus's lane
        {
            const bool has = !RAW && xs != 0xFFu && !((wdsm >> xs) & 1ull);          // (with RAW, and at loci over the barcode cap, the exact path lists them)
            const unsigned long long xm = __builtin_amdgcn_ballot_w64(has);
            if (xm) {
                const int k = has ? (int)xs : 0;
                const uint32_t clo = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * k, (int)v_Clo), chi = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * k, (int)v_Chi);
                const uint32_t wbk = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * k, (int)v_wb);
                const unsigned long long lt = (1ull << lane) - 1ull;
                const uint32_t slot = slot0 + (wbk >> WSH) + (uint32_t)__popc(clo & (uint32_t)lt) + (uint32_t)__popc(chi & (uint32_t)(lt >> 32));
                const uint32_t nx = (uint32_t)__popcll(xm);
                if (xq_n + nx > (uint32_t)BP_XQ) xflush();
                if (has) {
                    uint32_t* e = xq + BP_XW * (xq_n + bp_lanes_below(xm));
                    e[0] = (uint32_t)(l0 + k); e[1] = slot; e[2] = a; e[3] = 0xFFFFFFFFu; e[4] = 0u; e[5] = 0u;
                }
                xq_n += nx;
            }
        }
        // ---- the exact path: positions that are no plain base or hold an unusual letter, rows without a window; with RAW every
        // covered position (the raw-field planes are written here); every read of a locus over the barcode cap (its barcode ids
        // and first included reads go to the host).  One copy of the code, a loop over the tile's loci
        if (!wokc) spm |= Mc;                                                     // (a row without a window: every position it covers)
        if (__builtin_amdgcn_ballot_w64(spm != 0ull) || (wdsm && __builtin_amdgcn_ballot_w64((Mc & wdsm) != 0ull))) {
            const bool r2row = (hi & BP2_R2) != 0, rev = (hi & (2u << 16)) != 0;
#pragma unroll 1
            for (int k = 0; k < nt; ++k) {
                const bool wdk = (wdsm >> k) & 1ull;
                const bool cov = (Mc >> k) & 1ull, nf = (NF >> k) & 1ull, hb = (HB >> k) & 1ull;
                const bool sp = ((spm >> k) & 1ull) || (wdk && cov);
                if (!__builtin_amdgcn_ballot_w64(sp)) continue;
                const int p = p0 + k;
                const unsigned long long C = __builtin_amdgcn_ballot_w64(cov), HBm = __builtin_amdgcn_ballot_w64(hb), NFm = __builtin_amdgcn_ballot_w64(nf);
                const uint32_t slot = slot0 + ((uint32_t)__builtin_amdgcn_readlane((int)v_wb, k) >> WSH) + bp_lanes_below(C);
                const uint32_t hrank = bp_lanes_below(HBm) + (hb ? 1u : 0u), frank = bp_lanes_below(NFm) + (nf ? 1u : 0u);   // heads up to and including the row
                bool inc = false, isx = false;
                int x_qpos = 0, x_indel = 0;
                if (sp) {
                    const uint32_t* rec = (const uint32_t*)(A.aln + a);
                    const uint32_t kcig = rec[2], kseq = rec[3], k4 = rec[4], k5 = rec[5];
                    const int n_cig = (int)(k4 & 0xFFFFu), l_seq = (int)(rec[6] & 0xFFFFu), left_sp = (int)(k5 & 0xFFFFu), qalen = (int)(k5 >> 16);
                    bool r2 = r2row;
                    if (hi & BP2_UNFLAG) {
                        // neither READ1 nor READ2: the reference's pairOrder keeps the value of the previous pileup read of the locus
                        // (smCounter.py:359-362) - the nearest alignment before this one in the file that covers the position and has
                        // a flag.  None: the reference itself fails there (its variable is unbound) - the run goes back to the host
                        // (once some pileup of the run has begun with such a read the run is the host's anyway: no more searches - a
                        // file of single-end reads would otherwise walk back over the whole window for every read of every locus)
                        bool found = false;
                        if (!(*(volatile uint32_t*)A.status & BP_ST_NOPAIR))
                        for (uint32_t b = a; b-- > a_lo;) {
                            const uint32_t* rb = (const uint32_t*)(A.aln + b);
                            const uint32_t fl = (rb[4] >> 16) & 0xFFu;
                            if ((int)rb[0] <= p && p < (int)rb[1] && (fl & (SMC_DA_R1 | SMC_DA_R2))) { r2 = (fl & SMC_DA_R2) != 0; found = true; break; }
                        }
                        if (!found) atomicOr(A.status, BP_ST_NOPAIR);
                    }
                    // (bl_read of k_build_listed.inc restates the lines from here to the word for a flagged alignment - gap / site /
                    // quality, kind, the end distances, incCond, the class, the word: an edit here is an edit there, and
                    // tests/test_gpu_build_listed.py holds the two to the same bytes)
                    const BpRes r = bp2_resolve(A.cig + kcig, n_cig, pos, p, l_seq);
                    const bool gap = (r.isdel && r.indel == 0) || r.qpos < 0;
                    uint32_t site = 0, bq = 0;
                    if (!gap) { const uint32_t sq = *(const uint16_t*)(bqp + 2ull * (kseq + (uint32_t)r.qpos)); site = sq & 0xFFu; bq = sq >> 8; }
                    if (bq > 126u) atomicOr(A.status, BP_ST_BQ);
                    bq = min(bq, 126u);
                    const int f = bp_fixed_allele(site);
                    const uint32_t fa = gap ? 5u : (r.indel == 0 && f >= 0 ? (uint32_t)f : 0xFFu);
                    const uint32_t kind = r.indel > 0 ? 2u : r.indel < 0 ? 3u : r.isdel ? 1u : 0u;
                    uint32_t dist = 0;
                    if (kind == 0u) {                                          // end distances, regular bases only (:432-452)
                        const int rd = r.qpos - left_sp, far = qalen - rd;
                        const int dbc = (r2 != rev) ? far : rd, dpr = r2 ? (rev ? far : rd) : 0;
                        dist = (uint32_t)min(max(dbc, 0), 65535) | (uint32_t)min(max(dpr, 0), 65535) << 16;
                    }
                    const bool bq_ok = (int)bq >= A.min_bq;
                    inc = (bq_ok || kind == 1u) && mq;                                                      // incCond, :378
                    const uint32_t cls = smc_read_class((int)kind, rev, r2, inc, bq_ok, (dist & 0xFFFFu) <= 20u, (int)(dist >> 16) <= primer_dist);
                    isx = fa == 0xFFu;
                    x_qpos = r.qpos; x_indel = r.indel;
                    const uint32_t mword = (isx ? 6u : fa) | (kind == 1u ? (uint32_t)A.min_bq : bq) << 8;    // in-deletion: minBQ, :418
                    // (with RAW the words of plain bases stay the fast path's: the raw-field planes written here check them)
                    if (W16) {
                        if (bq > 63u && kind != 1u) atomicOr(A.status, BP_ST_NARROW);                      // (the caller builds the run with 32-bit words)
                        ((uint16_t*)A.words)[slot] = (uint16_t)smc_read_word16(mword | (nf ? SMC_RW_NF : 0u) | cls << SMC_RW_CLASS_SHIFT);
                    } else if (!RAW || !wokc || isx || kind != 0u || gap)
                        A.words[slot] = mword | (nf ? SMC_RW_NF : 0u) | (inc ? SMC_RW_INC : 0u) | SMC_RW_OK | cls << SMC_RW_CLASS_SHIFT;
                    if (RAW) {
                        const uint32_t val[4] = {mword | (hi & 0xFF7E0000u) | (r2 ? 1u << 16 : 0u) | kind << 19,
                                                 ((uint32_t)__builtin_amdgcn_readlane((int)v_cf, k) + frank - 1u) | cls << SMC_FRAG_CLASS_SHIFT,
                                                 (uint32_t)__builtin_amdgcn_readlane((int)v_cu, k) + hrank - 1u, dist};
#pragma unroll
                        for (int pl = 0; pl < 4; ++pl) if (outp[pl]) outp[pl][slot] = val[pl];
                    }
                }
                const unsigned long long xm = __builtin_amdgcn_ballot_w64(isx);
                if (xm) {                                                          // listed (first in LDS), numbered later (k_bp_xfix)
                    const uint32_t nx = (uint32_t)__popcll(xm);
                    if (xq_n + nx > (uint32_t)BP_XQ) xflush();
                    if (isx) {
                        uint32_t* e = xq + BP_XW * (xq_n + bp_lanes_below(xm));
                        e[0] = (uint32_t)(l0 + k); e[1] = slot; e[2] = a; e[3] = (uint32_t)x_qpos; e[4] = (uint32_t)x_indel; e[5] = 0u;
                    }
                    xq_n += nx;
                }
                if (wdk) {                                                         // barcode ids, first included read (:496-498 on the host)
                    const uint32_t u = ustart0 + ((uint32_t)__builtin_amdgcn_readlane((int)v_ub, k) >> 2) + hrank - 1u;
                    if (hb) A.u_gid[u] = bcv;
                    if (cov && inc) atomicMin(&A.u_finc[u], a);
                }
                if (RAW && lane == k) v_cf += (uint32_t)__popcll(NFm);
            }
        }
        v_wb += v_nC << WSH; v_rel += v_nC; v_ub += v_nB << 2;
        if (RAW) v_cu += v_nB;
        // ---- the rows and indices requested at the head came back with the windows
        a_cur = a_p1; r0c = r0_new; r1c = r1_new;
        a_p1 = a_new;
    }
    xflush();
}

// ---- the walk's WRITE PATTERN without the walk (smc_mem_write_probe): wavefront (tile, part) appends, batch after batch, a run of
// `run` words to each of the tile's 64 rows of `row_words` words - what k_bp_emit2 does to the read words of a 3000x panel.  How long
// that takes depends on which physical pages back the block (DESIGN.md section 5: up to 10 % between allocations of one process,
// the same from launch to launch); smc_mem_alloc_best times it into several allocations and keeps the fastest.
__global__ __launch_bounds__(64) void k_mem_write_probe(uint32_t* __restrict__ base, uint32_t n_tiles, uint32_t parts, uint32_t batches,
                                                        uint32_t row_words, uint32_t run, uint32_t spin) {
    const uint32_t lane = threadIdx.x;
    uint32_t vb = blockIdx.x;
    { const uint32_t per = gridDim.x >> 3; if (vb < per * 8u) vb = (vb & 7u) * per + (vb >> 3); }      // (the walk's dealing to the XCDs)
    const uint32_t tile = vb / parts, q = vb - tile * parts;
    if (tile >= n_tiles) return;
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc((char*)(base + (size_t)tile * 64u * row_words), 0, 0x7FFFFFFF, 0x00020000);
    uint32_t v = lane * 2654435761u + vb;
    for (uint32_t b = 0; b < batches; ++b) {
        const uint32_t r0 = (q * batches + b) * run;
#pragma unroll 4
        for (uint32_t k = 0; k < 64u; ++k) {
            for (uint32_t i = 0; i < spin; ++i) v = v * 1664525u + 1013904223u;                       // (the walk's arithmetic between two stores)
            __builtin_amdgcn_raw_buffer_store_b32(v, rs, lane < run ? (k * row_words + r0 + lane) << 2 : 0xFFFFFFFFu, 0, 0);
        }
    }
}
