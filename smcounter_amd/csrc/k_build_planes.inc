// Included by smcounter_hip.hip.
// ------------------------------------------------------------------------------------------
// kernel group 0: build the planes on the device from a run's alignments (round 3: no per-locus sort, no global tables)
// ------------------------------------------------------------------------------------------
// What the reference does per pileup read inside vc() before any counting (smCounter.py:316-366 feature extraction,
// :371-452 allele / quality / inclusion / end distances, :462-471 barcode and fragment bookkeeping).  A locus's reads must
// come out barcode-major (barcode, fragment, pileup order within the fragment: include/smcounter_hip.h).  Round 2 sorted
// every locus's reads on its own (a bitonic sort per locus, two device-scope atomics per read); but locus l + 1 is covered
// by 99 % of the alignments that cover locus l, so the ORDER is a property of the run's alignments, not of a locus:
//   1. sort ONCE: the alignments of a segment of 64 - 512 consecutive loci (those that can cover one of them: a window
//      of the file) are sorted by (barcode id, fragment id, file index) - a stable LSD radix sort of (key, index) pairs,
//      8 bits a pass, segments side by side in the same launches (k_bp_hist / k_bp_scan / k_bp_scatter).  That is 1 / 125
//      of the pileup reads (an alignment covers ~ 125 loci), once per run;
//   2. the pileup of a locus in barcode-major order is then the subsequence of that sorted list that covers it: an
//      ordered compaction.  A wavefront takes a TILE of 64 consecutive loci (lane = locus) and a PART of the segment's
//      sorted list; it takes the part's alignments in batches ("rows"): the rows mark where they start and end in the tile,
//      a prefix XOR over the lanes gives every locus its COLUMN (which rows cover it), and "first read of its barcode /
//      fragment at this locus" is the first set bit of the column within a run of rows with the same barcode / read pair
//      (bp_columns).  Rank, fragment start and barcode number of a read are then popcounts of the column below its row -
//      no step depends on the step before it.  k_bp_count counts (reads, fragment heads, barcode heads per locus and part),
//      k_bp_scan_tiles turns the counts into each part's first rank / slot / barcode number per locus and writes the
//      descriptors, k_bp_emit2 (k_bp_emit2.inc: the transposed walk, lane = alignment) walks again and writes the planes
//      (CIGAR walk with samtools resolve_cigar2 semantics as in smc_bam.cpp, allele, quality, flags, end distances, read class);
//   3. alleles beyond the six fixed ones (insertion / deletion starts, unusual letters: a few per thousand reads) are listed
//      by the walk and numbered per locus by first appearance afterwards (k_bp_xgroup / k_bp_xfix), as the reference's dict
//      meets them (:371-396).
// Barcodes and fragments are numbered in the order of their run-wide ids (first appearance in the RUN, not at the locus:
// the contract of smcounter_hip.h asks for a dense barcode-major numbering, not for a particular one - nothing vc() computes
// depends on it, and the reference's down-sampling, which does depend on the order in which bcDict met its keys, gets that
// order from u_finc below).
// The host keeps what is per ALIGNMENT (inflate, record parsing, read-name split, barcode / read-name interning) and what
// needs strings (allele key texts, the py2 down-sampling on barcode texts).
// Limits (the caller falls back to smc_bam_planes otherwise): < 2^24 reads per locus, at most 64 alleles per locus; a read
// flagged neither READ1 nor READ2 needs a flagged read before it in the locus's pileup (the reference fails without one).
#define BP_TILE 64             // loci per tile = lanes of the wavefront that builds them
// Tiles per sort segment, chosen per run (BpArgs.seg_tiles): 1 where a tile's window of the file fits the one-workgroup sort -
// the segment's sorted list then IS the tile's list and its parts are equal shares of the tile's work (with more tiles per
// segment the list, which follows the file order of the barcodes' first reads, puts a tile's alignments into a few of its
// parts: measured 2 x on the 3000x shape) -; BP_SEG_TILES_DEEP for deeper data, where every tile has hundreds of parts and
// sorting each alignment once per tile it touches would cost more than the imbalance.
#define BP_SEG_TILES_DEEP 8
#define BP_RS_TILE 1024        // elements a radix-sort wavefront takes per step (16 per lane)
#define BP_RS_MAXBLK 4096      // sort workgroups per pass over all segments (bounds the histogram matrix: 4 MB; 1024: + 3.5 % on the example-depth step)
#ifndef BP_SORT_WAVES
#define BP_SORT_WAVES 16
#endif
// BP_SORT_WAVES: wavefronts of the one-workgroup segment sort
#define BP_SORT_LDS_MAX 6144   // entries of a segment the one-workgroup sort keeps in registers + LDS (8 B each): the small instantiation
#ifndef BP_SORT_WAVES_SMALL
#define BP_SORT_WAVES_SMALL 8  // wavefronts of the small instantiation (round 5: two workgroups of 16 never shared a CU - 15 wavefronts resident by the
                               // counters; 16 / 12 / 8 / 6 wavefronts: 240 / 178 / 168 / 245 us on the 3000x shape)
#endif
#define BP_SORT_REG (BP_SORT_LDS_MAX / (64 * BP_SORT_WAVES_SMALL))   // entries per thread (5 with 16 wavefronts; 8 wavefronts: + 4 % on the whole builder, 4: + 70 %)
// (round 5) the same path with 16 entries per thread: every segment the one-workgroup sort takes (BP_LSORT_MAX = 16384 entries,
// 128 KB of LDS: one workgroup per CU).  Tiles of 8000x data (13,700 entries) went through global memory between the passes:
// 1.23 ms per 100,000 loci of C5's shape, a quarter of that step
#define BP_SORT_REG_BIG (BP_LSORT_MAX / (64 * BP_SORT_WAVES))
#define BP_LSORT_MAX 16384     // a segment of up to this many alignments is sorted by ONE workgroup (16 wavefronts x 1024)
#define BP_XQ 64               // extra-allele reads a wavefront collects in LDS before it appends them to the global list
#define BP_XREP 256            // reports (distinct extra alleles) a tile collects in LDS before its one append to the caller's list
#define BP_NCUR 64              // cursors k_bp_rows_write hands out pool space and list places from (each its own region / part)
#define BP_XW 8                // words per listed extra-allele read: locus, plane slot, alignment, query position, indel, key slot, the allele key's hash (2)
#define BP_ST_DEPTH 1u         // a locus's depth disagrees with the host's count
#define BP_ST_XLIST 2u         // the extras list (reads or distinct alleles) is full
#define BP_ST_BQ 4u            // base quality > 126
#define BP_ST_ALLELES 8u       // more than 64 alleles at a locus
#define BP_ST_NARROW 32u       // 16-bit read words asked for, and an allele id beyond 15 or a base quality beyond 63 met: no room (16u: BP_ST_NOPAIR)

struct BpSeg {                 // one per segment of seg_tiles x 64 loci
    uint32_t w0, w1;           // its alignments: file indices [w0, w1)
    uint32_t off;              // first entry of the segment in the sorted list
    uint32_t part_base, ppt;   // first (tile, part) wavefront of the segment; parts per tile - parts of BP_SUB rows: k_bp_scan_tiles, k_bp_emit2
    uint32_t blk_base, n_blk;  // its radix-sort workgroups
    uint32_t n_tiles;
    uint32_t cpart_base, cppt; // the same for k_bp_count, whose wavefronts take BpArgs.part rows (a multiple of BP_SUB) each
};
#define BP_SUB 64              // rows of the sorted list per wavefront of the walk that writes: ONE batch (round 5, see k_bp_count)

struct BpArgs {
    const smc_dev_aln* aln; const uint32_t* cig; const uint8_t* bq;   // bq: (letter, quality) pairs, two bytes per base
    const smc_dev_locus* loc; const uint8_t* refseq;      // refseq[l]: upper-cased reference letter of locus l
    int32_t start0, n_loci, n_seg, part;                  // part: sorted-list entries per part
    int32_t seg_tiles;                                    // tiles per segment
    int32_t min_bq, min_mq, primer_dist, ds;
    uint32_t fp;                                          // smc_param_fingerprint << SMC_LF_FP_SHIFT
    uint32_t xcd_rot;                                     // (experiments, SMC_BP_XCD_ROT) the walk's eighth of the tiles that XCD x takes: (x + rot) & 7
    uint32_t slot_base, umi_base;                         // where this run starts in the batch's planes / umi_start
    uint32_t *words;                                      // one word per read (smc_read_word): what the locus kernels read
    uint32_t w16;                                         // 1: `words` is an array of 16-bit read words (smc_read_word16)
    uint32_t *meta, *umi, *frag, *dist, *umi_start, *u_gid, *u_finc;   // meta, umi, frag, dist: the raw-field planes (optional: checks)
    smc_locus* loci;
    const BpSeg* seg;
    const uint32_t* n_live;                               // [segment of `seg`]: entries of its sorted list - w1 - w0, or fewer where the sort has dropped
                                                          // the rows that end before the tile (k_bp_sort_seg); the walks stop there (bp_wave)
    const uint32_t* sorted;                               // alignment indices, segment by segment, each in (barcode, fragment, file) order
    uint32_t* cnt;                                        // [wavefront of k_bp_count][3][64]: reads / fragment heads / barcode heads per locus in its A.part rows
    uint32_t* cntp;                                       // [wavefront of BP_SUB rows][64]: the same three counts of that stretch alone, a byte each
    uint32_t* pstate;                                     // [wavefront of BP_SUB rows][4]: which loci the barcode (words 0-1) / read pair (2-3) of the
                                                          // wavefront's first row has covered before it (k_bp_count -> k_bp_emit2: no replay there)
    uint32_t *xraw, xraw_cap, *xraw_n;                    // listed extra-allele reads, BP_XW words each
    uint32_t *xcnt, *tcnt, *tcur, *gidx;                  // per locus / per tile counts, grouping cursor, entries grouped by tile
    uint32_t *gidx2;                                      // the entries of a heavy tile grouped by LOCUS (k_bp_xfix)
    uint32_t *xlist, xcap, *xcount, *status;              // distinct extras for the host: 5 words each (locus, allele id, alignment, qpos, indel)
};

// the allele id of an extra allele into the read's word: byte 0 of a 32-bit word (a byte store), the low nibble of a 16-bit one
// (the walk left the code 6 there; a slot is patched by one thread, its neighbours are other bytes)
__device__ __forceinline__ void bp_patch_allele(const BpArgs& A, uint32_t sp, uint32_t id) {
    if (!A.words) return;
    if (A.w16) {
        if (id > 15u) { atomicOr(A.status, BP_ST_NARROW); return; }
        uint8_t* b = (uint8_t*)A.words + 2ull * sp;
        *b = (uint8_t)((*b & 0xF0u) | id);
    } else ((uint8_t*)A.words)[4ull * sp] = (uint8_t)id;
}
#include "bp_masks.h"   // bp_heads: the rows that start a run at a locus; bp_row_dead / bp_part_rows: the live rows of a tile's list (plain C++:
                        // also compiled and tested on the host)
__device__ __forceinline__ uint32_t bp_lanes_below(unsigned long long m) {
    return (uint32_t)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// ---- a radix pass's ranking step: among the wavefront's VALID lanes, those that hold this lane's digit - how many of them are
// below this lane (rank) and how many there are (np).  One ballot per digit bit; the lane's own copy of the match mask is kept as
// two 32-bit halves and narrowed by (mask XNOR the lane's bit, spread to 0 / -1 by a signed bit-field extract): 5 vector
// instructions a bit where `peers &= one ? m : ~m` on a 64-bit value compiled to 11 (round 5: the sort of a panel's tiles was
// bound by exactly these - 1,900 vector instructions per wavefront, three quarters of them here).  An invalid lane's digit must be 0.
__device__ __forceinline__ void bp_match(uint32_t dgt, bool valid, int nbits, uint32_t& rank, uint32_t& np) {
    const unsigned long long v = __builtin_amdgcn_ballot_w64(valid);
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int bit = 0; bit < 8; ++bit) {
        if (bit < nbits) {                                                      // (wave-uniform)
            const uint32_t x = (uint32_t)(((int)(dgt << (31 - bit))) >> 31);    // 0 or -1: the lane's bit
            const unsigned long long m = __builtin_amdgcn_ballot_w64(x != 0u);
            lo &= ~((uint32_t)m ^ x); hi &= ~((uint32_t)(m >> 32) ^ x);
        }
    }
    rank = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
    np = (uint32_t)__popc(lo) + (uint32_t)__popc(hi);
}
// largest s with base(s) <= x (empty segments share their base with the next one: the last of equals is the one that owns x)
template <int BY /* 0: sort block, 1: (tile, part) of BP_SUB rows, 2: k_bp_count's (tile, part) */>
__device__ __forceinline__ int bp_seg_of(const BpSeg* __restrict__ seg, int n_seg, uint32_t x) {
    int lo = 0, hi = n_seg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        const uint32_t b = BY == 1 ? seg[mid].part_base : BY == 2 ? seg[mid].cpart_base : seg[mid].blk_base;
        if (b <= x) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// key of an allele beyond A,T,G,C,N,'DEL' as a 64-bit hash (FNV-1a): an insertion start ('I', site, inserted bases as
// the host's substr clamps them), a deletion start ('D', site, length) or an unusual letter ('L', letter)
__device__ __forceinline__ unsigned long long bp_key_hash(const smc_dev_aln& a, const uint8_t* __restrict__ bq, int qpos, int indel) {
    unsigned long long h = 1469598103934665603ull;
    auto mix = [&](uint32_t b) { h ^= (unsigned long long)(b & 0xffu); h *= 1099511628211ull; };
    const uint8_t* s = bq + 2ull * a.seq_off;                                    // (the letter of base k: byte 2k)
    mix(indel > 0 ? 'I' : indel < 0 ? 'D' : 'L');
    mix(s[2 * qpos]);
    if (indel > 0) { for (int k = qpos + 1; k < (int)a.l_seq && k < qpos + 1 + indel; ++k) mix(s[2 * k]); }
    else if (indel < 0) { const uint32_t l = (uint32_t)(-indel); mix(l); mix(l >> 8); mix(l >> 16); mix(l >> 24); }
    return h;
}
__device__ __forceinline__ int bp_fixed_allele(uint32_t site) {       // allele ids 0-4 = A,T,G,C,N (pileup.py BASE_ALLELES)
    return site == 'A' ? 0 : site == 'T' ? 1 : site == 'G' ? 2 : site == 'C' ? 3 : site == 'N' ? 4 : -1;
}

// ---- the segment table, on the device from the per-locus windows (the host computes the same totals from its copy of `loc`
// to size the scratch and the grids: smc_build_planes)
__host__ __device__ static inline uint32_t bp_seg_blocks(uint32_t cnt, uint32_t max_blk) {
    if (cnt <= BP_LSORT_MAX) return 0u;                    // (sorted by one workgroup, all passes in one launch: k_bp_sort_seg)
    const uint32_t t = (cnt + BP_RS_TILE - 1) / BP_RS_TILE;
    return t < max_blk ? t : max_blk;
}
__global__ __launch_bounds__(1024) void k_bp_segtab(const smc_dev_locus* __restrict__ loc, int n_loci, int n_seg, int seg_loci, uint32_t part, uint32_t max_blk,
                                                    BpSeg* __restrict__ seg, uint32_t* __restrict__ n_live) {
    __shared__ uint32_t ws[4][16];
    __shared__ uint32_t carry[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid < 4) carry[tid] = 0u;
    __syncthreads();
    for (int base = 0; base < n_seg; base += 1024) {
        const int s = base + tid;
        BpSeg S{};
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (s < n_seg) {
            const int l0 = s * seg_loci, l1 = min(n_loci, l0 + seg_loci) - 1;
            S.w0 = loc[l0].w0;
            const uint32_t e = loc[l1].w1;
            S.w1 = e > S.w0 ? e : S.w0;
            const uint32_t cnt = S.w1 - S.w0;
            S.n_tiles = (uint32_t)((l1 - l0) / BP_TILE + 1);
            S.ppt = (cnt + BP_SUB - 1) / BP_SUB;
            S.cppt = (cnt + part - 1) / part;
            S.n_blk = bp_seg_blocks(cnt, max_blk);
            v[0] = cnt; v[1] = S.ppt * S.n_tiles; v[2] = S.n_blk; v[3] = S.cppt * S.n_tiles;
        }
        uint32_t ex[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint32_t inc = v[c];
            for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)inc, o); if (lane >= o) inc += u; }
            if (lane == 63) ws[c][wid] = inc;
            ex[c] = inc - v[c];
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            uint32_t pre = carry[c];
            for (int w = 0; w < wid; ++w) pre += ws[c][w];
            ex[c] += pre;
        }
        if (s < n_seg) { S.off = ex[0]; S.part_base = ex[1]; S.blk_base = ex[2]; S.cpart_base = ex[3]; seg[s] = S; n_live[s] = v[0]; }   // (every row, until the sort says otherwise)
        __syncthreads();
        if (tid < 4) { uint32_t t = 0; for (int w = 0; w < 16; ++w) t += ws[tid][w]; carry[tid] += t; }
        __syncthreads();
    }
}

// ---- exclusive scan of a u32 array in place (one workgroup: the arrays are small - histogram matrices, per-tile counts)
__global__ __launch_bounds__(1024) void k_bp_scan(uint32_t* __restrict__ d, uint32_t n, const uint32_t* __restrict__ n_dev) {
    __shared__ uint32_t ws[16];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (n_dev) n = min(*n_dev, n) + 1u;                    // (a length only the device knows: that many entries and a closing one)
    uint32_t carry = 0;
    // (16 entries per thread and round: the histogram matrix of a deep run's sort pass is 262,144 entries - with four per thread
    // the 64 rounds of this one workgroup took 148 us a pass, five passes a run: a third of the step on the example run's shape)
    constexpr int PER = 16;
    for (uint32_t base = 0; base < n; base += 1024u * PER) {
        const uint32_t i = base + (uint32_t)PER * (uint32_t)tid;
        uint32_t v[PER];
        if (i + PER <= n && (((uintptr_t)(d + i)) & 15u) == 0u) {
#pragma unroll
            for (int k = 0; k < PER; k += 4) { const uint4 q = *(const uint4*)(d + i + k); v[k] = q.x; v[k + 1] = q.y; v[k + 2] = q.z; v[k + 3] = q.w; }
        } else {
#pragma unroll
            for (int k = 0; k < PER; ++k) v[k] = i + k < n ? d[i + k] : 0u;
        }
        uint32_t t = 0;
#pragma unroll
        for (int k = 0; k < PER; ++k) t += v[k];
        uint32_t inc = t;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)inc, o); if (lane >= o) inc += u; }
        if (lane == 63) ws[wid] = inc;
        __syncthreads();
        uint32_t pre = carry, tot = 0;
        for (int w = 0; w < 16; ++w) { const uint32_t x = ws[w]; if (w < wid) pre += x; tot += x; }
        uint32_t run = pre + inc - t;
#pragma unroll
        for (int k = 0; k < PER; ++k) { if (i + k < n) d[i + k] = run; run += v[k]; }
        carry += tot;
        __syncthreads();
    }
}

// ---- stable LSD radix sort of (key, alignment index), 8 bits a pass, all segments in the same launches.  A workgroup is one
// wavefront (no barriers); it owns a contiguous range of BP_RS_TILE-element steps of ONE segment.  hist[(blk_base(s) * 256) +
// digit * n_blk(s) + local block]: scanned as one array that is the destination of every (segment, digit, block) bucket.
struct BpBlk { uint32_t e0, e1, hidx, hstride, w0, off, h0; int seg; };
__device__ __forceinline__ BpBlk bp_blk(const BpSeg* __restrict__ seg, int n_seg, uint32_t b) {
    const int s = bp_seg_of<0>(seg, n_seg, b);
    const BpSeg S = seg[s];
    const uint32_t bl = b - S.blk_base, cnt = S.w1 - S.w0, steps = (cnt + BP_RS_TILE - 1) / BP_RS_TILE;
    const uint32_t t0 = (uint32_t)((unsigned long long)bl * steps / S.n_blk), t1 = (uint32_t)((unsigned long long)(bl + 1) * steps / S.n_blk);
    BpBlk B;
    B.e0 = S.off + t0 * BP_RS_TILE;
    const uint32_t e1 = S.off + t1 * BP_RS_TILE, end = S.off + cnt;
    B.e1 = e1 < end ? e1 : end;
    B.hidx = S.blk_base * 256u + bl; B.hstride = S.n_blk;
    B.w0 = S.w0; B.off = S.off; B.h0 = S.blk_base * 256u; B.seg = s;
    return B;
}
template <bool FIRST /* the keys do not exist yet: make them from the alignments */>
__global__ __launch_bounds__(64) void k_bp_hist(const BpSeg* __restrict__ seg, int n_seg, const uint2* __restrict__ k8, int pair_bits,
                                                unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals, int shift,
                                                uint32_t* __restrict__ hist) {
    __shared__ uint32_t lh[256];
    const int lane = threadIdx.x;
    const BpBlk B = bp_blk(seg, n_seg, blockIdx.x);
#pragma unroll
    for (int k = 0; k < 4; ++k) lh[lane + 64 * k] = 0u;
    __builtin_amdgcn_wave_barrier();
    for (uint32_t e = B.e0 + (uint32_t)lane; e < B.e1; e += 64u) {
        unsigned long long key;
        if (FIRST) {
            const uint32_t a = B.w0 + (e - B.off);
            const uint2 kv = k8[a];                                              // (barcode, pair): k_bp_rows_write's compact copy
            key = ((unsigned long long)kv.x << pair_bits) | (unsigned long long)kv.y;
            keys[e] = key; vals[e] = a;
        } else key = keys[e];
        atomicAdd(&lh[(uint32_t)(key >> shift) & 255u], 1u);
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 4; ++k) { const uint32_t dgt = (uint32_t)lane + 64u * k; hist[B.hidx + dgt * B.hstride] = lh[dgt]; }
}
// ---- between the two: every (segment, digit) ROW of the histogram matrix - the counts of that digit in the segment's blocks,
// contiguous - becomes its exclusive prefix, by one wavefront; the row's total goes to dtot[segment][digit].  (Round 5: until then
// ONE workgroup scanned the whole matrix - 262,144 entries on the example run's depth, 137-148 us a pass, five passes a run: a
// third of that shape's step.  The prefix over a segment's 256 digit totals is left to the scatter's wavefronts: 4 per lane.)
__global__ __launch_bounds__(64) void k_bp_rowscan(const BpSeg* __restrict__ seg, uint32_t* __restrict__ hist, uint32_t* __restrict__ dtot) {
    const int lane = threadIdx.x;
    const uint32_t s = blockIdx.x >> 8, dgt = blockIdx.x & 255u;
    const BpSeg S = seg[s];
    if (!S.n_blk) { if (lane == 0) dtot[blockIdx.x] = 0u; return; }
    uint32_t* row = hist + (size_t)S.blk_base * 256u + (size_t)dgt * S.n_blk;
    uint32_t carry = 0;
    for (uint32_t b0 = 0; b0 < S.n_blk; b0 += 256u) {
        const uint32_t i = b0 + 4u * (uint32_t)lane;
        uint32_t v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = i + k < S.n_blk ? row[i + k] : 0u;
        const uint32_t t = v[0] + v[1] + v[2] + v[3];
        uint32_t inc = t;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)inc, o); if (lane >= o) inc += u; }
        uint32_t run = carry + inc - t;
#pragma unroll
        for (int k = 0; k < 4; ++k) { if (i + k < S.n_blk) row[i + k] = run; run += v[k]; }
        carry += (uint32_t)__builtin_amdgcn_readlane((int)inc, 63);
    }
    if (lane == 0) dtot[blockIdx.x] = carry;
}
__global__ __launch_bounds__(64) void k_bp_scatter(const BpSeg* __restrict__ seg, int n_seg, const unsigned long long* __restrict__ kin,
                                                   const uint32_t* __restrict__ vin, unsigned long long* __restrict__ kout,
                                                   uint32_t* __restrict__ vout, int shift, const uint32_t* __restrict__ hist,
                                                   const uint32_t* __restrict__ dtot) {
    __shared__ uint32_t offs[256];
    const int lane = threadIdx.x;
    const BpBlk B = bp_blk(seg, n_seg, blockIdx.x);
    // a bucket's destination: the segment's region of the list (`off`: behind EVERY earlier segment, also those k_bp_sort_seg sorts
    // in one workgroup) + the entries of the segment's smaller digits (a prefix over its 256 digit totals, made here) + the entries
    // of this digit in the segment's earlier blocks (k_bp_rowscan)
    {
        uint32_t v[4], t = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { v[k] = dtot[(uint32_t)B.seg * 256u + 4u * (uint32_t)lane + (uint32_t)k]; t += v[k]; }
        uint32_t inc = t;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)inc, o); if (lane >= o) inc += u; }
        uint32_t run = B.off + inc - t;
#pragma unroll
        for (int k = 0; k < 4; ++k) { offs[4 * lane + k] = run; run += v[k]; }
    }
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 4; ++k) { const uint32_t dgt = (uint32_t)lane + 64u * k; offs[dgt] += hist[B.hidx + dgt * B.hstride]; }
    __builtin_amdgcn_wave_barrier();
    for (uint32_t e0 = B.e0; e0 < B.e1; e0 += 64u) {
        const uint32_t e = e0 + (uint32_t)lane;
        const bool valid = e < B.e1;
        unsigned long long key = 0; uint32_t val = 0;
        if (valid) { key = kin[e]; val = vin[e]; }
        const uint32_t dgt = (uint32_t)(key >> shift) & 255u;
        uint32_t rank, n;                                                       // among the lanes with this lane's digit
        bp_match(dgt, valid, 8, rank, n);
        const uint32_t base = valid ? offs[dgt] : 0u;
        __builtin_amdgcn_wave_barrier();                                        // (every lane has read its bucket's cursor)
        if (valid && rank == 0u) offs[dgt] = base + n;
        __builtin_amdgcn_wave_barrier();
        if (valid) { kout[base + rank] = key; vout[base + rank] = val; }
    }
}

// ---- the same sort for a segment of up to BP_LSORT_MAX alignments (every segment of a panel at up to ~ 3000x): ONE workgroup
// of 16 wavefronts runs every pass - per-wavefront digit counts in LDS, the data ping-pongs between the two global buffers
// (L2-resident; a workgroup's wavefronts share their CU's L1, so a barrier orders their loads behind each other's stores).
// The first pass reads its keys from the compact (barcode, pair) copy k_bp_rows_write has left (round 5: 8 contiguous bytes per
// entry instead of 8 of a 36-byte record, and every alignment is in 3.4 tiles' lists).  One launch instead of three per pass.
// The keys are narrowed first: barcode and pair ids are numbered by first appearance in the file, so the ids a segment's window
// holds lie in a small range of the run's - (id - the segment's smallest) needs 20-odd bits where the run-wide key has 39: three
// passes instead of five (kept at the parity of `passes`: the result has to land in the buffer the walks read).
// up to 16 registers as four groups of four: ONE array of 16 is a 16-wide vector value to the compiler - every element update
// copies the whole tuple, and the 16-entry instantiation of the sort below spilled 2,880 bytes; the index is a constant after unrolling
struct BpReg16 {
    uint32_t a[4], b[4], c[4], d[4];
    __device__ __forceinline__ uint32_t& at(int i) { return i < 4 ? a[i] : i < 8 ? b[i - 4] : i < 12 ? c[i - 8] : d[i - 12]; }
};
template <int REG /* entries per thread of the register + LDS path: BP_SORT_REG or BP_SORT_REG_BIG */, int WAVES /* wavefronts of the workgroup */, bool BIG>
__global__ __launch_bounds__(64 * WAVES) void k_bp_sort_seg(const BpSeg* __restrict__ seg, const uint2* __restrict__ k8 /* (barcode, pair) per alignment */, int pair_bits, int passes,
                                                      unsigned long long* k0, unsigned long long* k1, uint32_t* v0, uint32_t* v1, uint32_t only_above, uint32_t only_upto,
                                                      const int32_t* __restrict__ kend /* end position per alignment, beside k8 */, int start0,
                                                      uint32_t* __restrict__ n_live /* nullptr: every window row stays (segments of several tiles, or the switch) */) {
    // The live rows (a segment that is ONE tile: n_live given).  An entry whose alignment ends at or before the tile's first position
    // (bp_row_dead) is handled like the positions behind e1 of a partial last iteration from the start: not in the key range, no digit
    // count, no rank, not written.  The first pass therefore leaves the nl live entries at [0, nl) in their old relative order - the
    // sort stays stable -, the later passes run on those alone, and n_live[segment] = nl is where the walks end the list.  A segment
    // this kernel returns early on keeps the full count the segment table came with.
    constexpr int LDS_MAX = 64 * WAVES * REG;
    if (!BIG && (seg[blockIdx.x].w1 - seg[blockIdx.x].w0) > only_upto) return;
    __shared__ uint32_t whist[WAVES][256];
    __shared__ uint32_t dtot[256], dbase[256];
    const BpSeg S = seg[blockIdx.x];
    const uint32_t n = S.w1 - S.w0;
    // (a run with segments either side of BP_SORT_LDS_MAX launches both instantiations: each takes its own sizes)
    if (n == 0u || n > BP_LSORT_MAX || (BIG ? n <= only_above : false)) return;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const uint32_t chunk = ((n + (uint32_t)WAVES - 1u) / (uint32_t)WAVES + 63u) & ~63u;
    uint32_t e0 = min(n, (uint32_t)wid * chunk), e1 = min(n, e0 + chunk);       // the wavefront's entries: of the window in the first pass, of the live rows after it
    unsigned long long* kb[2] = {k0 + S.off, k1 + S.off};
    uint32_t* vb[2] = {v0 + S.off, v1 + S.off};
    const bool filter = n_live != nullptr;                                      // (wave-uniform: a kernel argument)
    const int p_first = start0 + (int)blockIdx.x * BP_TILE;                     // (filter: the segment is tile blockIdx.x)
    auto live = [&](uint32_t e) -> bool { return !filter || !bp_row_dead(kend[S.w0 + e], p_first); };   // e: an entry of the window
    __shared__ uint32_t rng[5];                                                 // smallest / largest barcode id, smallest / largest pair id, live rows
    if (tid == 0) { rng[0] = 0xFFFFFFFFu; rng[1] = 0u; rng[2] = 0xFFFFFFFFu; rng[3] = 0u; rng[4] = 0u; }
    __syncthreads();
    // (the register + LDS path below takes a wavefront's whole share in REG entries per lane: its keys and end positions are then
    // fetched ONCE, here, every load asked for before the first is waited for - the index of a lane behind e1 is clamped, so no load
    // stands behind a branch - and stay in the registers the path sorts them in)
    const bool in_regs = n <= (uint32_t)LDS_MAX && chunk <= 64u * REG;           // (wave-uniform)
    BpReg16 key, val;       // (REG <= 16 registers each; until the ranges are known: barcode and pair id as fetched)
    uint32_t vm = 0u;       // bit it: the thread's entry `it` takes part in the pass (first pass: in the window and live; then: below f1)
#pragma unroll
    for (int it = 0; it < 16; ++it) { key.at(it) = 0u; val.at(it) = 0u; }
    {
        uint32_t b_lo = 0xFFFFFFFFu, b_hi = 0u, p_lo = 0xFFFFFFFFu, p_hi = 0u, nlv = 0u;
        if (in_regs) {
            if (e0 < e1) {
                int ke[REG];
#pragma unroll
                for (int it = 0; it < REG; ++it) {
                    const uint32_t a = S.w0 + min(e0 + 64u * (uint32_t)it + (uint32_t)lane, e1 - 1u);
                    const uint2 kv = k8[a];
                    key.at(it) = kv.x; val.at(it) = kv.y;
                    ke[it] = filter ? kend[a] : 0x7FFFFFFF;
                }
#pragma unroll
                for (int it = 0; it < REG; ++it) {
                    const bool ok = e0 + 64u * (uint32_t)it + (uint32_t)lane < e1 && !bp_row_dead(ke[it], p_first);
                    vm |= ok ? 1u << it : 0u;
                    b_lo = min(b_lo, ok ? key.at(it) : 0xFFFFFFFFu); b_hi = max(b_hi, ok ? key.at(it) : 0u);
                    p_lo = min(p_lo, ok ? val.at(it) : 0xFFFFFFFFu); p_hi = max(p_hi, ok ? val.at(it) : 0u);
                }
                nlv = (uint32_t)__popc(vm);
            }
        } else for (uint32_t e = e0 + (uint32_t)lane; e < e1; e += 64u) {
            const uint2 kv = k8[S.w0 + e];
            if (!live(e)) continue;
            const uint32_t b = kv.x, q = kv.y;
            b_lo = min(b_lo, b); b_hi = max(b_hi, b); p_lo = min(p_lo, q); p_hi = max(p_hi, q);
            ++nlv;
        }
        for (int o = 32; o; o >>= 1) {
            b_lo = min(b_lo, (uint32_t)__shfl_xor((int)b_lo, o)); b_hi = max(b_hi, (uint32_t)__shfl_xor((int)b_hi, o));
            p_lo = min(p_lo, (uint32_t)__shfl_xor((int)p_lo, o)); p_hi = max(p_hi, (uint32_t)__shfl_xor((int)p_hi, o));
            nlv += (uint32_t)__shfl_xor((int)nlv, o);
        }
        if (lane == 0 && nlv) { atomicMin(&rng[0], b_lo); atomicMax(&rng[1], b_hi); atomicMin(&rng[2], p_lo); atomicMax(&rng[3], p_hi); atomicAdd(&rng[4], nlv); }
    }
    __syncthreads();
    const uint32_t nl = rng[4];                                                 // (= n without the filter)
    if (filter && tid == 0) n_live[blockIdx.x] = nl;
    if (nl == 0u) return;                                                       // (every row of the window ends before the tile)
    // the wavefronts' shares of the live rows, once the first pass has put them at [0, nl)
    const uint32_t chunk2 = ((nl + (uint32_t)WAVES - 1u) / (uint32_t)WAVES + 63u) & ~63u;
    const uint32_t f0 = min(nl, (uint32_t)wid * chunk2), f1 = min(nl, f0 + chunk2);
    const uint32_t bc_min = rng[0], pair_min = rng[2];
    const int pb = 32 - __builtin_clz((rng[3] - pair_min) | 1u), bb = 32 - __builtin_clz((rng[1] - bc_min) | 1u);
    int my_passes = (pb + bb + 7) / 8;
    if (pb + bb > 8 * passes) my_passes = passes;                               // (cannot be: the host sized `passes` for the run-wide ids)
    (void)pair_bits;
    // ---- a segment of up to BP_SORT_LDS_MAX entries with keys of up to 32 bits (a tile of a panel at 3000x: 4,500 entries, 21 bits):
    // every thread keeps its (up to five) entries in registers from pass to pass and the workgroup exchanges them through LDS -
    // no trip through global memory between passes, only the last pass's alignment indices leave
    if (in_regs && pb + bb <= 32) {
        // (an entry's value on its way through LDS is its index in the segment's window, 16 bits: with 32-bit values the 6-entry
        // instantiation claimed 68 KB and ONE workgroup ran per CU - 15 wavefronts resident on average by the counters)
        __shared__ uint32_t lk[LDS_MAX];
        __shared__ uint16_t lv[LDS_MAX];
        static_assert(LDS_MAX <= 65536, "lv holds window indices in 16 bits");
#pragma unroll
        for (int it = 0; it < REG; ++it) {                                      // (barcode, pair) as fetched -> the narrowed key; the value: the entry's index in the window
            const bool ok = (vm >> it) & 1u;
            key.at(it) = ok ? (key.at(it) - bc_min) << pb | (val.at(it) - pair_min) : 0u;
            val.at(it) = ok ? e0 + 64u * (uint32_t)it + (uint32_t)lane : 0u;
        }
        // (where the walks read the sorted list.  Typed as global: picked from an array of two pointers it is a generic one to the
        // compiler, its stores flat_ ones - and a flat store also counts as an LDS operation in flight, so every wait for the
        // digit cursors below would wait for the store before it to come back from memory)
        typedef __attribute__((address_space(1))) uint32_t glb_u32;
        glb_u32* const out = (glb_u32*)vb[passes & 1];
        // (the passes share the key's bits evenly: 21 bits are three digits of 7, and a ranking step costs one ballot per digit bit)
        const int dbits = __builtin_amdgcn_readfirstlane(max(1, (pb + bb + my_passes - 1) / max(1, my_passes)));   // (in a scalar register: the ranking step branches on it)
        const uint32_t dmask = (1u << dbits) - 1u;
        for (int ps = 0; ps < my_passes; ++ps) {
            const int shift = dbits * ps;
            const bool last = ps == my_passes - 1;
#pragma unroll
            for (int k = 0; k < 4; ++k) whist[wid][lane + 64 * k] = 0u;
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int it = 0; it < REG; ++it)
                if ((vm >> it) & 1u) atomicAdd(&whist[wid][(key.at(it) >> shift) & dmask], 1u);
            __syncthreads();
            if (tid < 256) {
                uint32_t run = 0;
#pragma unroll
                for (int w = 0; w < WAVES; ++w) { const uint32_t v = whist[w][tid]; whist[w][tid] = run; run += v; }
                dtot[tid] = run;
            }
            __syncthreads();
            if (wid == 0) {
                uint32_t v[4], t = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) { v[k] = dtot[4 * lane + k]; t += v[k]; }
                uint32_t inc = t;
                for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)inc, o); if (lane >= o) inc += u; }
                uint32_t run = inc - t;
#pragma unroll
                for (int k = 0; k < 4; ++k) { dbase[4 * lane + k] = run; run += v[k]; }
            }
            __syncthreads();
#pragma unroll
            for (int it = 0; it < REG; ++it) {                          // (in entry order: the sort is stable)
                if (e0 + 64u * (uint32_t)it >= e1) break;                       // (wave-uniform)
                const bool valid = (vm >> it) & 1u;
                const uint32_t dgt = valid ? (key.at(it) >> shift) & dmask : 0u;
                uint32_t rank, np;
                bp_match(dgt, valid, dbits, rank, np);
                const uint32_t wo = valid ? whist[wid][dgt] : 0u;
                __builtin_amdgcn_wave_barrier();
                if (valid && rank == 0u) whist[wid][dgt] = wo + np;
                __builtin_amdgcn_wave_barrier();
                if (valid) {
                    const uint32_t d = dbase[dgt] + wo + rank;
                    if (last) out[d] = S.w0 + val.at(it);
                    else { lk[d] = key.at(it); lv[d] = (uint16_t)val.at(it); }
                }
            }
            if (last) break;
            __syncthreads();
            e0 = f0; e1 = f1; vm = 0u;                                          // (the live rows, dealt to the wavefronts again)
#pragma unroll
            for (int it = 0; it < REG; ++it) {
                const uint32_t e = e0 + 64u * (uint32_t)it + (uint32_t)lane;
                if (e < e1) { vm |= 1u << it; key.at(it) = lk[e]; val.at(it) = lv[e]; }
            }
            __syncthreads();
        }
        return;
    }
    my_passes += (passes - my_passes) & 1;
    for (int ps = 0; ps < my_passes; ++ps) {
        const int shift = 8 * ps;
        const unsigned long long* kin = kb[ps & 1];
        const uint32_t* vin = vb[ps & 1];
        unsigned long long* kout = kb[(ps & 1) ^ 1];
        uint32_t* vout = vb[(ps & 1) ^ 1];
        auto fetch = [&](uint32_t e, unsigned long long& key, uint32_t& val) -> bool {   // -> the entry takes part (first pass: it is live)
            if (ps == 0) {
                if (!live(e)) return false;
                val = S.w0 + e;
                const uint2 kv = k8[val];
                key = ((unsigned long long)(kv.x - bc_min) << pb) | (unsigned long long)(kv.y - pair_min);
            } else { key = kin[e]; val = vin[e]; }
            return true;
        };
#pragma unroll
        for (int k = 0; k < 4; ++k) whist[wid][lane + 64 * k] = 0u;
        __builtin_amdgcn_wave_barrier();
        for (uint32_t e = e0 + (uint32_t)lane; e < e1; e += 64u) {
            unsigned long long key = 0; uint32_t val = 0;
            if (fetch(e, key, val)) atomicAdd(&whist[wid][(uint32_t)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 256) {
            uint32_t run = 0;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) { const uint32_t v = whist[w][tid]; whist[w][tid] = run; run += v; }
            dtot[tid] = run;
        }
        __syncthreads();
        if (wid == 0) {
            uint32_t v[4], t = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) { v[k] = dtot[4 * lane + k]; t += v[k]; }
            uint32_t inc = t;
            for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)inc, o); if (lane >= o) inc += u; }
            uint32_t run = inc - t;
#pragma unroll
            for (int k = 0; k < 4; ++k) { dbase[4 * lane + k] = run; run += v[k]; }
        }
        __syncthreads();
        for (uint32_t eb = e0; eb < e1; eb += 64u) {
            const uint32_t e = eb + (uint32_t)lane;
            bool valid = e < e1;
            unsigned long long key = 0; uint32_t val = 0;
            if (valid) valid = fetch(e, key, val);
            const uint32_t dgt = valid ? (uint32_t)(key >> shift) & 255u : 0u;
            uint32_t rank, np;
            bp_match(dgt, valid, 8, rank, np);
            const uint32_t wo = valid ? whist[wid][dgt] : 0u;
            __builtin_amdgcn_wave_barrier();
            if (valid && rank == 0u) whist[wid][dgt] = wo + np;
            __builtin_amdgcn_wave_barrier();
            if (valid) { const uint32_t d = dbase[dgt] + wo + rank; kout[d] = key; vout[d] = val; }
        }
        __syncthreads();                                                        // (stores drained: the next pass reads them)
        e0 = f0; e1 = f1;                                                       // (the live rows, dealt to the wavefronts again)
    }
}

// ---- which (tile, part) a wavefront of the two walks below is, and what is the same in both
struct BpWave {
    int tile, l, p, p_first, p_last;
    bool active;
    uint32_t a_lo, a_hi, seg_off, j0, j1, jb, sub0, cpart, csub;
};
template <bool COUNT /* k_bp_count's geometry: parts of A.part rows, and where the part's first barcode began */>
__device__ __forceinline__ BpWave bp_wave(const BpArgs& A, int lane, uint32_t w) {   // w: which (tile, part) wavefront
    BpWave W;
    const int s = bp_seg_of<COUNT ? 2 : 1>(A.seg, A.n_seg, w);
    const BpSeg SG = A.seg[s];
    const uint32_t rr = w - (COUNT ? SG.cpart_base : SG.part_base), ppt = COUNT ? SG.cppt : SG.ppt, part = COUNT ? (uint32_t)A.part : (uint32_t)BP_SUB;
    const uint32_t tis = rr / ppt, q = rr - tis * ppt;
    W.tile = s * A.seg_tiles + (int)tis;
    const int l_first = W.tile * BP_TILE;
    const int l_last = min(A.n_loci, l_first + BP_TILE) - 1;
    W.l = l_first + lane;
    W.active = W.l <= l_last;
    W.p = A.start0 + W.l; W.p_first = A.start0 + l_first; W.p_last = A.start0 + l_last;
    W.a_lo = A.loc[l_first].w0; W.a_hi = A.loc[l_last].w1;                        // the tile's window of the file
    W.seg_off = SG.off;
    // (the list's end is its LIVE end - grids, ppt and cppt are the host's upper bounds from w1 - w0: a wavefront behind it has j0 >= j1)
    bp_part_rows(SG.off, A.n_live[s], q, part, W.j0, W.j1);
    W.sub0 = SG.part_base + tis * SG.ppt + q * (part / (uint32_t)BP_SUB);        // the first BP_SUB-row wavefront of this one's rows
    {   // (the walk that writes) which of k_bp_count's wavefronts counted this stretch, and how many stretches of that one lie before it
        const uint32_t per = (uint32_t)A.part / (uint32_t)BP_SUB;
        W.cpart = SG.cpart_base + tis * SG.cppt + q / per; W.csub = q % per;
    }
    // The barcode / fragment of the part's first alignment may have begun in the previous part: walk back to the first entry
    // of that barcode; the stretch [jb, j0) is replayed (state only) - "has this barcode / fragment covered the lane's locus
    // before" is then right from the part's first alignment on.
    W.jb = W.j0;
    if (COUNT && W.j0 > SG.off && W.j0 < W.j1) {
        const uint32_t bc0 = A.aln[A.sorted[W.j0]].bc_gid;
        while (W.jb > SG.off) {
            const uint32_t base = W.jb - SG.off >= 64u ? W.jb - 64u : SG.off;
            const uint32_t j = base + (uint32_t)lane;
            const bool in = j < W.jb;
            const uint32_t b = in ? A.aln[A.sorted[j]].bc_gid : bc0;
            const unsigned long long other = __builtin_amdgcn_ballot_w64(in && b != bc0);
            if (other) { W.jb = base + (uint32_t)(63 - __builtin_clzll(other)) + 1u; break; }
            W.jb = base;
        }
    }
    return W;
}
// ---- the walks take the sorted list up to 32 alignments at a time, without a step per alignment: the alignments of a batch ("rows") mark where they
// start and end in the tile (two LDS atomics each); a prefix XOR over the lanes turns the marks into each locus's COLUMN - bit r:
// row r covers the locus; a row that starts a barcode (a fragment) at the locus is the first set bit of its barcode's (read
// pair's) rows - rows are sorted, so those are runs: a segmented prefix OR, five doubling steps on masks the wavefront shares.
// Reads, fragment heads and barcode heads of the batch are then three popcounts.
__device__ __forceinline__ uint32_t bp_scan_xor(uint32_t v) {                    // inclusive, over the wavefront's lanes
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, true);      // row_shr:1 (zeros shifted in)
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, true);
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, true);
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, true);
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);     // row_bcast:15 into rows 1 and 3
    v ^= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);     // row_bcast:31 into rows 2 and 3
    return v;
}
#define BP_MASK_LDS (66 + 32 + 32)   // words: the start / end marks per tile position (+ the one behind the tile), barcode and pair of each row
struct BpCols { uint32_t C, NF, NB; };
// the batch's rows (lanes with in_b: row rr, tile-relative span [lo, hi), barcode, pair) -> the lane's columns; advances last_bc / last_pair
__device__ __forceinline__ BpCols bp_columns(uint32_t* lds, int lane, bool in_b, uint32_t rr, uint32_t nrows, int lo, int hi, uint32_t bc,
                                             uint32_t pair, uint32_t& last_bc, uint32_t& last_pair) {
    uint32_t* const ev = lds;
    uint32_t* const rbc = lds + 66;
    uint32_t* const rpair = rbc + 32;
    ev[lane] = 0u;
    if (lane < 2) ev[64 + lane] = 0u;
    __builtin_amdgcn_wave_barrier();
    if (in_b) { atomicOr(&ev[lo], 1u << rr); atomicOr(&ev[hi], 1u << rr); rbc[rr] = bc; rpair[rr] = pair; }
    __builtin_amdgcn_wave_barrier();
    BpCols R;
    R.C = bp_scan_xor(ev[lane]);
    const uint32_t x = rbc[lane & 31], xp = rbc[(lane - 1) & 31], y = rpair[lane & 31], yp = rpair[(lane - 1) & 31];
    const bool row = lane >= 1 && (uint32_t)lane < nrows;
    const uint32_t SB = (uint32_t)__builtin_amdgcn_ballot_w64(row && x == xp), SP = (uint32_t)__builtin_amdgcn_ballot_w64(row && y == yp);
    R.NB = bp_heads(R.C, SB, last_bc == rbc[0]);
    R.NF = bp_heads(R.C, SP, last_pair == rpair[0]);
    if (R.C) { const int top = 31 - __builtin_clz(R.C); last_bc = rbc[top]; last_pair = rpair[top]; }
    __builtin_amdgcn_wave_barrier();
    return R;
}
// one batch of up to 64 rows of the sorted list, its records already asked for: what the rows add to the loci's columns
struct BpRec { int pos, end; uint32_t bc, pair; bool inwin; };
__device__ __forceinline__ uint32_t bp_batch_index(const BpArgs& A, uint32_t c0, uint32_t c_to, int lane) {
    const uint32_t j = c0 + (uint32_t)lane;
    return j < c_to ? A.sorted[j] : 0xFFFFFFFFu;                               // (no alignment has that index)
}
__device__ __forceinline__ BpRec bp_batch_rec(const BpArgs& A, const BpWave& W, uint32_t a) {
    BpRec R; R.pos = 0x7FFFFFFF; R.end = 0; R.bc = 0; R.pair = 0;
    R.inwin = a != 0xFFFFFFFFu && a >= W.a_lo && a < W.a_hi;
    if (R.inwin) { const uint32_t* rec = (const uint32_t*)(A.aln + a); R.pos = (int)rec[0]; R.end = (int)rec[1]; R.bc = rec[7]; R.pair = rec[8]; }
    return R;
}
template <bool COUNT>
__device__ __forceinline__ void bp_walk_batch(const BpWave& W, int lane, const BpRec& R, uint32_t& last_bc, uint32_t& last_pair, uint32_t& c_r,
                                              uint32_t& c_f, uint32_t& c_u, uint32_t* lds) {
    const bool ov = R.inwin && R.end > W.p_first && R.pos <= W.p_last;
    const unsigned long long todo = __builtin_amdgcn_ballot_w64(ov);
    if (!todo) return;
    const uint32_t r = bp_lanes_below(todo), n = (uint32_t)__popcll(todo);
    const int lo = max(R.pos - W.p_first, 0), hi = min(R.end - W.p_first, 64);
    for (uint32_t b0 = 0; b0 < n; b0 += 32u) {
        const BpCols K = bp_columns(lds, lane, ov && r >= b0 && r < b0 + 32u, r - b0, min(32u, n - b0), lo, hi, R.bc, R.pair, last_bc, last_pair);
        if (COUNT) { c_r += (uint32_t)__popc(K.C); c_f += (uint32_t)__popc(K.NF); c_u += (uint32_t)__popc(K.NB); }
    }
}

// ---- the first walk: reads, fragment heads and barcode heads per locus of the tile in this part of the sorted list
// Round 5: the counts are left per stretch of BP_SUB (64) rows - the wavefronts of k_bp_emit2 take ONE batch each, so that the 70
// runs a locus of the 3000x shape gets are written side by side at about the same time instead of four at a time by eighteen
// wavefronts 25 us apart - and with them what such a wavefront would otherwise have to replay: which loci the barcode / the read
// pair of its first row has covered before it.  Here that is a comparison: the lane's (= the locus's) last covering row is of that
// barcode / pair or it is not.  This walk itself keeps parts of A.part rows: one replay per 256 rows, not per 64.
// The batches - first those of the replay [jb, j0), then the part's stretches - are a chain of two dependent gathers each (index
// of the sorted list -> alignment record) in front of a little LDS work: the records of batch k + 1 and the indices of batch
// k + 2 are asked for before batch k is worked on (round 5; until then a wavefront waited for both, batch after batch - the
// counters had it parked in s_waitcnt 72 % of its time, 30 % of its L2 requests hits).
__global__ __launch_bounds__(64) void k_bp_count(BpArgs A) {
    __shared__ uint32_t lds[BP_MASK_LDS];
    const int lane = threadIdx.x;
    const BpWave W = bp_wave<true>(A, lane, blockIdx.x);
    uint32_t last_bc = 0xFFFFFFFFu, last_pair = 0xFFFFFFFFu, c_r = 0, c_f = 0, c_u = 0;
    // (barcode and read pair of every stretch's first row, lane i the i-th stretch: asked for before the replay, used after it)
    uint32_t s_bc = 0, s_pair = 0;
    {
        const uint32_t c0 = W.j0 + (uint32_t)BP_SUB * (uint32_t)lane;
        if (c0 < W.j1) { const smc_dev_aln* r0 = A.aln + A.sorted[c0]; s_bc = r0->bc_gid; s_pair = r0->pair_gid; }
    }
    const uint32_t n_rep = W.j0 > W.jb ? (W.j0 - W.jb + 63u) / 64u : 0u, n_main = W.j1 > W.j0 ? (W.j1 - W.j0 + (uint32_t)BP_SUB - 1u) / (uint32_t)BP_SUB : 0u;
    const uint32_t n_bat = n_rep + n_main;
    auto bounds = [&](uint32_t k, uint32_t& b0, uint32_t& b1) {                    // rows [b0, b1) of batch k
        if (k < n_rep) { b0 = W.jb + 64u * k; b1 = min(W.j0, b0 + 64u); }
        else { b0 = W.j0 + (uint32_t)BP_SUB * (k - n_rep); b1 = min(W.j1, b0 + (uint32_t)BP_SUB); }
    };
    auto index_of = [&](uint32_t k) -> uint32_t {
        if (k >= n_bat) return 0xFFFFFFFFu;
        uint32_t b0, b1; bounds(k, b0, b1);
        return bp_batch_index(A, b0, b1, lane);
    };
    uint32_t a_next = index_of(0);
    BpRec R = bp_batch_rec(A, W, a_next);
    a_next = index_of(1);
    uint32_t sub = W.sub0, t_r = 0, t_f = 0, t_u = 0;
    for (uint32_t k = 0; k < n_bat; ++k) {
        const BpRec Rn = bp_batch_rec(A, W, a_next);                           // batch k + 1's records
        a_next = index_of(k + 2u);                                             // batch k + 2's indices
        if (k < n_rep) { bp_walk_batch<false>(W, lane, R, last_bc, last_pair, c_r, c_f, c_u, lds); R = Rn; continue; }
        const uint32_t i = k - n_rep;
        {   // the state k_bp_emit2's wavefront `sub` starts from
            const uint32_t bc0 = (uint32_t)__builtin_amdgcn_readlane((int)s_bc, (int)(i & 63u)), pair0 = (uint32_t)__builtin_amdgcn_readlane((int)s_pair, (int)(i & 63u));
            const unsigned long long cb = __builtin_amdgcn_ballot_w64(last_bc == bc0), cp = __builtin_amdgcn_ballot_w64(last_pair == pair0);
            if (lane < 4) A.pstate[(size_t)sub * 4u + (uint32_t)lane] = lane == 0 ? (uint32_t)cb : lane == 1 ? (uint32_t)(cb >> 32) : lane == 2 ? (uint32_t)cp : (uint32_t)(cp >> 32);
        }
        c_r = c_f = c_u = 0;
        bp_walk_batch<true>(W, lane, R, last_bc, last_pair, c_r, c_f, c_u, lds);
        A.cntp[(size_t)sub * 64u + (uint32_t)lane] = c_r | c_f << 8 | c_u << 16;     // (each at most BP_SUB = 64: a byte)
        t_r += c_r; t_f += c_f; t_u += c_u;
        ++sub;
        R = Rn;
    }
    uint32_t* const cw = A.cnt + (size_t)blockIdx.x * 192u;
    cw[lane] = t_r; cw[64 + lane] = t_f; cw[128 + lane] = t_u;
}

// ---- deep runs (segments of BP_SEG_TILES_DEEP tiles, sorted together by the multi-launch passes): the segment's sorted list
// filtered into ONE LIST PER TILE - the alignments of the tile's own window of the file, in the segment's order - so that the
// walks behind it run on a tile's own rows as they do on a panel.  (Until the end of round 5 every tile's wavefronts walked the
// whole segment's list and dropped the rows outside their window: at the example run's depth 70 % of the rows a wavefront loaded -
// the walk that writes the read words took 4.7 ns per pileup read there against 1.7 on the 3000x shape.)  The list of tile t has
// exactly w1(t) - w0(t) entries (the segment's window holds the tile's), so the host sizes everything; two launches: matches per
// (tile, chunk of BP_TL_CH entries of the segment's list), then the stable scatter behind the chunks before it.
#define BP_TL_CH 4096
__global__ __launch_bounds__(256) void k_bp_tile_count(const BpSeg* __restrict__ sseg, int seg_tiles, const BpSeg* __restrict__ wseg, int n_tiles, int nch,
                                                       const uint32_t* __restrict__ sorted, uint32_t* __restrict__ tc) {
    __shared__ uint32_t ws[4];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int tile = blockIdx.x / nch, c = blockIdx.x % nch;
    const BpSeg S = sseg[tile / seg_tiles], W = wseg[tile];
    const uint32_t cnt = S.w1 - S.w0, e0 = (uint32_t)c * BP_TL_CH, e1 = min(cnt, e0 + BP_TL_CH);
    uint32_t m = 0;
    for (uint32_t e = e0 + (uint32_t)tid; e < e1; e += 256u) { const uint32_t a = sorted[S.off + e]; m += (a >= W.w0 && a < W.w1) ? 1u : 0u; }
    for (int o = 32; o; o >>= 1) m += (uint32_t)__shfl_xor((int)m, o);
    if (lane == 0) ws[wid] = m;
    __syncthreads();
    if (tid == 0) tc[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}
__global__ __launch_bounds__(256) void k_bp_tile_scatter(const BpSeg* __restrict__ sseg, int seg_tiles, const BpSeg* __restrict__ wseg, int n_tiles, int nch,
                                                         const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ tc, uint32_t* __restrict__ sorted2) {
    __shared__ uint32_t ws[4], wbase;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int tile = blockIdx.x / nch, c = blockIdx.x % nch;
    const BpSeg S = sseg[tile / seg_tiles], W = wseg[tile];
    const uint32_t cnt = S.w1 - S.w0, e0 = (uint32_t)c * BP_TL_CH, e1 = min(cnt, e0 + BP_TL_CH);
    if (e0 >= e1) return;
    uint32_t before = 0;                                                      // the tile's matches in the chunks before this one
    for (int k = tid; k < c; k += 256) before += tc[(size_t)tile * nch + k];
    for (int o = 32; o; o >>= 1) before += (uint32_t)__shfl_xor((int)before, o);
    if (lane == 0) ws[wid] = before;
    __syncthreads();
    uint32_t base = W.off + ws[0] + ws[1] + ws[2] + ws[3];
    __syncthreads();
    for (uint32_t r0 = e0; r0 < e1; r0 += 256u) {                             // in order: the filter is stable
        const uint32_t e = r0 + (uint32_t)tid;
        const uint32_t a = e < e1 ? sorted[S.off + e] : 0xFFFFFFFFu;
        const bool hit = e < e1 && a >= W.w0 && a < W.w1;
        const unsigned long long hm = __builtin_amdgcn_ballot_w64(hit);
        if (lane == 0) ws[wid] = (uint32_t)__popcll(hm);
        __syncthreads();
        uint32_t pre = base;
        for (int w = 0; w < wid; ++w) pre += ws[w];
        if (hit) sorted2[pre + bp_lanes_below(hm)] = a;
        base += ws[0] + ws[1] + ws[2] + ws[3];
        __syncthreads();
    }
}

// ---- per tile: the parts' counts become each part's starting rank / slot / barcode number (exclusive prefix over the parts,
// in place); the totals are the locus's depth, fragments and barcodes: descriptor, closing umi_start entry, padding slots
__global__ __launch_bounds__(256) void k_bp_scan_tiles(BpArgs A) {
    __shared__ uint32_t ws[4][3][64];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int tile = blockIdx.x, s = tile / A.seg_tiles;
    const BpSeg SG = A.seg[s];
    const uint32_t P = SG.cppt;
    uint32_t* const base = A.cnt + ((size_t)SG.cpart_base + (size_t)(tile - s * A.seg_tiles) * P) * 192u;
    const uint32_t q0 = P * (uint32_t)wid / 4u, q1 = P * (uint32_t)(wid + 1) / 4u;
    uint32_t sum[3] = {0u, 0u, 0u};
#pragma unroll 4
    for (uint32_t q = q0; q < q1; ++q) {
        const uint32_t* c = base + (size_t)q * 192u;
        sum[0] += c[lane]; sum[1] += c[64 + lane]; sum[2] += c[128 + lane];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) ws[wid][c][lane] = sum[c];
    __syncthreads();
    uint32_t run[3], tot[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        run[c] = 0u; tot[c] = 0u;
        for (int w = 0; w < 4; ++w) { const uint32_t x = ws[w][c][lane]; if (w < wid) run[c] += x; tot[c] += x; }
    }
#pragma unroll 4
    for (uint32_t q = q0; q < q1; ++q) {
        uint32_t* c = base + (size_t)q * 192u;
        const uint32_t v0 = c[lane], v1 = c[64 + lane], v2 = c[128 + lane];
        c[lane] = run[0]; c[64 + lane] = run[1]; c[128 + lane] = run[2];
        run[0] += v0; run[1] += v1; run[2] += v2;
    }
    const int l = tile * BP_TILE + lane;
    if (wid == 0 && l < A.n_loci) {
        const smc_dev_locus LC = A.loc[l];
        uint32_t n = tot[0];
        const uint32_t nF = tot[1], nU = tot[2];
        if (n != LC.n || n >= (1u << 24)) { atomicOr(A.status, BP_ST_DEPTH); n = n < LC.n ? n : LC.n; }
        const uint32_t so = A.slot_base + LC.slot_off, uo = A.umi_base + LC.slot_off + (uint32_t)l;
        A.umi_start[uo + nU] = n;
        for (uint32_t j = n; j < ((n + 3u) & ~3u); ++j) {
            if (A.words) { if (A.w16) ((uint16_t*)A.words)[so + j] = 0; else A.words[so + j] = 0u; }
            if (A.meta) A.meta[so + j] = 0u;
            if (A.umi) A.umi[so + j] = 0u;
            if (A.frag) A.frag[so + j] = 0u;
            if (A.dist) A.dist[so + j] = 0u;
        }
        if (A.ds > 0 && (int)nU > A.ds)
            for (uint32_t u = 0; u < nU; ++u) A.u_finc[uo + u] = 0xFFFFFFFFu;    // "no included read" until the walk finds one
        smc_locus L;
        L.read_off4 = so >> 2; L.umi_off = uo;
        L.n_reads = (int32_t)n; L.n_umi = (int32_t)nU; L.n_frag = (int32_t)nF;
        const int ra = bp_fixed_allele(A.refseq[l]);
        L.ref_allele = (uint8_t)(ra < 0 ? 255 : ra); L.n_alleles = 6;            // (k_bp_xfix: the loci that met more alleles)
        L.flags = (uint16_t)A.fp; L.snp_mask = 0x1f;
        A.loci[l] = L;
    }
}

// ---- extras: group the listed reads by tile (tcnt has been scanned into offsets), then number each locus's distinct alleles
// by first appearance in the pileup (= lowest alignment index: the reference's dict meets them in that order, :371-396),
// patch the allele byte of their reads, report one (locus, id, alignment, qpos, indel) per distinct allele to the host
__global__ __launch_bounds__(256) void k_bp_xgroup(BpArgs A) {
    if (*A.xraw_n > A.xraw_cap) return;                                        // (overflow: flagged by the walk, the caller falls back)
    const uint32_t n = *A.xraw_n;
    // (neighbours in the list mostly come from one flush of one wavefront - one tile: one returning atomic per run of equal tiles)
    for (uint32_t i0 = blockIdx.x * 256u + (threadIdx.x & ~63u); i0 < n; i0 += gridDim.x * 256u) {
        const uint32_t i = i0 + (threadIdx.x & 63u);
        const bool in = i < n;
        const uint32_t t = in ? A.xraw[(size_t)BP_XW * i] / BP_TILE : 0xFFFFFFFFu;
        const uint32_t tp = (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFEu, (int)t, 0x138, 0xF, 0xF, false);   // the lane before (lane 0: none)
        const unsigned long long heads = __builtin_amdgcn_ballot_w64(in && t != tp);
        const unsigned long long mine = heads & ((2ull << (threadIdx.x & 63u)) - 1ull);          // run heads up to this lane
        const int h = 63 - __builtin_clzll(mine | 1ull);                                           // the lane's run starts at lane h
        const unsigned long long after = heads & ~((2ull << h) - 1ull);
        const int e = after ? __builtin_ctzll(after) : (int)min(64u, n - i0);                     // ... and ends before lane e
        uint32_t base = 0;
        if (in && (int)(threadIdx.x & 63u) == h) base = A.tcnt[t] + atomicAdd(&A.tcur[t], (uint32_t)(e - h));
        base = (uint32_t)__builtin_amdgcn_ds_bpermute(4 * h, (int)base);
        if (in) A.gidx[base + (threadIdx.x & 63u) - (uint32_t)h] = i;
    }
}
#define BP_XF2_MAX 256         // extra-allele reads of a tile up to which k_bp_xfix2 takes it (its LDS table: 512 keys)
#define BP_XF_WAVES 16          // wavefronts of k_bp_xfix: each takes every 16th locus of the tile (a locus is a chain of dependent
                               // accesses - entry, alignment, bases: four wavefronts with 16 loci each took 0.19 ms on the 3000x shape)
__global__ __launch_bounds__(64 * BP_XF_WAVES) void k_bp_xfix(BpArgs A) {
    __shared__ unsigned long long khash[BP_XF_WAVES][64], kfirst[BP_XF_WAVES][64];
    __shared__ uint32_t kid[BP_XF_WAVES][64];
    // the tile's reports - one per distinct extra allele of a locus - wait here for ONE append to the caller's list at the end
    // (a counter every locus bumps on its own takes ~ 90 atomics per microsecond; the few reports beyond the buffer go one by one)
    __shared__ uint32_t rep[BP_XREP][5], rep_n, rep_base;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int tile = blockIdx.x;
    const uint32_t nt = A.tcur[tile];
    if (nt <= (uint32_t)BP_XF2_MAX || *A.xraw_n > A.xraw_cap) return;            // (the tiles k_bp_xfix2 has taken)
    if (tid == 0) rep_n = 0u;
    __syncthreads();
    const uint32_t* g = A.gidx + A.tcnt[tile];
    // The tile's entries once more, grouped by locus (end of round 5): every wavefront used to look through ALL of the tile's entries
    // for each of its four loci - on the example run's shape (tens of thousands of listed reads per tile, 32 tiles) 177 us of a
    // 1.4 ms step, by 32 workgroups.  One pass of the workgroup scatters the entries' indices behind per-locus offsets (the loci's
    // own counts, xcnt); a locus then reads its own entries only.
    __shared__ uint32_t loff[BP_TILE + 1], lcur[BP_TILE];
    if (tid < BP_TILE) {
        const int l = tile * BP_TILE + tid;
        const uint32_t c = l < A.n_loci ? A.xcnt[l] : 0u;
        uint32_t inc = c;
        for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)inc, o); if (lane >= o) inc += u; }
        loff[tid] = inc - c; lcur[tid] = 0u;
        if (tid == BP_TILE - 1) loff[BP_TILE] = inc;
    }
    __syncthreads();
    uint32_t* const g2 = A.gidx2 + A.tcnt[tile];
    for (uint32_t i = (uint32_t)tid; i < nt; i += 64u * BP_XF_WAVES) {
        const uint32_t gi = g[i], ll = A.xraw[(size_t)BP_XW * gi] - (uint32_t)(tile * BP_TILE);
        if (ll < (uint32_t)BP_TILE) g2[loff[ll] + atomicAdd(&lcur[ll], 1u)] = gi;
    }
    __threadfence_block();
    __syncthreads();
    for (int ll = wid; ll < BP_TILE; ll += BP_XF_WAVES) {
        const int l = tile * BP_TILE + ll;
        if (l >= A.n_loci || A.xcnt[l] == 0u) continue;                          // (wave-uniform)
        const uint32_t* const gl = g2 + loff[ll];
        const uint32_t nl = min(loff[ll + 1] - loff[ll], lcur[ll]);              // the locus's entries
        uint32_t nk = 0;
        for (uint32_t c = 0; c < nl; c += 64u) {
            const uint32_t i = c + (uint32_t)lane;
            uint32_t* e = nullptr;
            const bool mine = i < nl;
            uint32_t gi = 0;
            if (mine) { gi = gl[i]; e = A.xraw + (size_t)BP_XW * gi; }
            unsigned long long h = 0;
            uint32_t ai = 0;
            if (mine) { ai = e[2]; h = (unsigned long long)e[6] | (unsigned long long)e[7] << 32; }
            int slot = -1;
            for (uint32_t k = 0; k < nk; ++k) if (mine && khash[wid][k] == h) slot = (int)k;
            unsigned long long open = __builtin_amdgcn_ballot_w64(mine && slot < 0);
            while (open) {
                const int kx = __builtin_ctzll(open);
                const unsigned long long hx = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(h >> 32), kx) << 32) |
                                              (uint32_t)__builtin_amdgcn_readlane((int)h, kx);
                uint32_t ns = nk;
                if (nk >= 58u) { if (lane == 0) atomicOr(A.status, BP_ST_ALLELES); ns = 57u; }
                else { if (lane == 0) { khash[wid][nk] = hx; kfirst[wid][nk] = ~0ull; } ++nk; }
                __builtin_amdgcn_wave_barrier();
                if (mine && slot < 0 && h == hx) slot = (int)ns;
                open = __builtin_amdgcn_ballot_w64(mine && slot < 0);
            }
            if (mine) { atomicMin(&kfirst[wid][slot], ((unsigned long long)ai << 32) | gi); e[5] = (uint32_t)slot; }
        }
        __builtin_amdgcn_wave_barrier();
        // ids by first appearance; one report per distinct allele
        bool single = false;
        uint32_t letter = 0, id = 0;
        if ((uint32_t)lane < nk) {
            const unsigned long long f = kfirst[wid][lane];
            uint32_t rank = 0;
            for (uint32_t k = 0; k < nk; ++k) rank += kfirst[wid][k] < f ? 1u : 0u;
            id = 6u + rank;
            kid[wid][lane] = id;
            const uint32_t* e = A.xraw + (size_t)BP_XW * (uint32_t)f;
            const uint32_t ai = (uint32_t)(f >> 32), qpos = e[3], indel = e[4];
            single = indel == 0u;
            if (single) letter = A.bq[2ull * (A.aln[ai].seq_off + qpos)];
            uint32_t slot = atomicAdd(&rep_n, 1u);
            uint32_t* o = nullptr;
            if (slot < (uint32_t)BP_XREP) o = rep[slot];
            else {                                                        // (a tile with hundreds of distinct extra alleles)
                slot = atomicAdd(A.xcount, 1u);
                if (slot < A.xcap) o = A.xlist + 5 * (size_t)slot; else atomicOr(A.status, BP_ST_XLIST);
            }
            if (o) { o[0] = (uint32_t)l; o[1] = id; o[2] = ai; o[3] = qpos; o[4] = indel; }
        }
        __builtin_amdgcn_wave_barrier();
        for (uint32_t c = 0; c < nl; c += 64u) {
            const uint32_t i = c + (uint32_t)lane;
            if (i < nl) {
                const uint32_t* e = A.xraw + (size_t)BP_XW * gl[i];
                const uint32_t sp = e[1];
                bp_patch_allele(A, sp, kid[wid][e[5]]);
                if (A.meta) ((uint8_t*)A.meta)[4ull * sp] = (uint8_t)kid[wid][e[5]];
            }
        }
        // descriptor: allele count, which extras are single letters, the reference letter when it is one of them
        const uint32_t rc = A.refseq[l];
        const unsigned long long sm = __builtin_amdgcn_ballot_w64(single);
        const unsigned long long rm = __builtin_amdgcn_ballot_w64(single && letter == rc);
        unsigned long long mask = 0x1f;
        int ra = bp_fixed_allele(rc);
        for (unsigned long long m = sm; m; m &= m - 1ull) mask |= 1ull << (uint32_t)__builtin_amdgcn_readlane((int)id, __builtin_ctzll(m));
        if (ra < 0) ra = rm ? (int)(uint32_t)__builtin_amdgcn_readlane((int)id, __builtin_ctzll(rm)) : 255;
        if (lane == 0) { A.loci[l].ref_allele = (uint8_t)ra; A.loci[l].n_alleles = (uint8_t)(6u + nk); A.loci[l].snp_mask = mask; }
        __builtin_amdgcn_wave_barrier();
    }
    __syncthreads();
    const uint32_t nrep = min(rep_n, (uint32_t)BP_XREP);
    if (tid == 0 && nrep) rep_base = atomicAdd(A.xcount, nrep);
    __syncthreads();
    for (uint32_t i = (uint32_t)tid; i < 5u * nrep; i += 64u * BP_XF_WAVES) {
        const uint32_t slot = rep_base + i / 5u;
        if (slot < A.xcap) A.xlist[5 * (size_t)slot + i % 5u] = rep[i / 5u][i % 5u];
        else if (i % 5u == 0u) atomicOr(A.status, BP_ST_XLIST);
    }
}


// ---- the same for the tiles with up to BP_XF2_MAX listed reads - all of a panel's - with LANE = LISTED READ: one wavefront per
// tile, the distinct (locus, allele) keys in an LDS hash table (64-bit compare-and-swap), numbered per locus by first appearance.
// (k_bp_xfix gives a locus to a wavefront, whose lanes scan the tile's entries for the one or two of that locus: a chain of
// dependent accesses per locus, 150 k loci: 0.19 ms on the 3000x shape whatever the number of wavefronts.)
__global__ __launch_bounds__(64) void k_bp_xfix2(BpArgs A) {
    __shared__ unsigned long long tkey[2 * BP_XF2_MAX], tfirst[2 * BP_XF2_MAX];     // key: allele hash (bit 63 set) with the locus in bits 0-5
    __shared__ uint32_t ck[BP_XF2_MAX], cid[2 * BP_XF2_MAX], nkl[64], refid[64], n_keys, rep_base;
    __shared__ unsigned long long smask[64];
    const int lane = threadIdx.x, tile = blockIdx.x;
    const uint32_t nt = A.tcur[tile];
    if (!nt || nt > (uint32_t)BP_XF2_MAX || *A.xraw_n > A.xraw_cap) return;
    const uint32_t* g = A.gidx + A.tcnt[tile];
    for (int i = lane; i < 2 * BP_XF2_MAX; i += 64) { tkey[i] = 0ull; tfirst[i] = ~0ull; }
    nkl[lane] = 0u; refid[lane] = 0u; smask[lane] = 0ull;
    if (lane == 0) n_keys = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // ---- every listed read: its key's slot, the key's first appearance (lowest alignment index, then lowest list position)
    for (uint32_t c = 0; c < nt; c += 64u) {
        const uint32_t i = c + (uint32_t)lane;
        if (i < nt) {
            uint32_t* e = A.xraw + (size_t)BP_XW * g[i];
            const uint32_t ll = e[0] - (uint32_t)(tile * BP_TILE), ai = e[2];
            const unsigned long long h = (unsigned long long)e[6] | (unsigned long long)e[7] << 32;      // (bp_key_hash, made by the walk when it listed the read)
            const unsigned long long key = ((h | 0x8000000000000000ull) & ~63ull) | (unsigned long long)ll;
            uint32_t slot = (uint32_t)((h >> 17) ^ (h >> 41) ^ (ll * 0x9E3779B1u)) & (2u * BP_XF2_MAX - 1u);
            for (;;) {
                const unsigned long long prev = atomicCAS(&tkey[slot], 0ull, key);
                if (prev == 0ull || prev == key) break;
                slot = (slot + 1u) & (2u * BP_XF2_MAX - 1u);
            }
            atomicMin(&tfirst[slot], ((unsigned long long)ai << 32) | g[i]);
            e[5] = slot;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // ---- the distinct keys, compacted
    for (int s = lane; s < 2 * BP_XF2_MAX; s += 64)
        if (tkey[s] != 0ull) ck[atomicAdd(&n_keys, 1u)] = (uint32_t)s;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const uint32_t K = n_keys;
    if (lane == 0) rep_base = atomicAdd(A.xcount, K);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // ---- ids by first appearance within the locus; one report per key
    for (uint32_t j = (uint32_t)lane; j < K; j += 64u) {
        const uint32_t s = ck[j];
        const unsigned long long key = tkey[s], f = tfirst[s];
        const uint32_t ll = (uint32_t)(key & 63ull);
        uint32_t rank = 0;
        for (uint32_t t = 0; t < K; ++t) { const uint32_t s2 = ck[t]; rank += ((tkey[s2] & 63ull) == (unsigned long long)ll && tfirst[s2] < f) ? 1u : 0u; }
        uint32_t id = 6u + rank;
        if (rank >= 58u) { atomicOr(A.status, BP_ST_ALLELES); id = 63u; }
        cid[s] = id;
        atomicAdd(&nkl[ll], 1u);
        const uint32_t* e = A.xraw + (size_t)BP_XW * (uint32_t)f;
        const uint32_t ai = (uint32_t)(f >> 32), qpos = e[3], indel = e[4];
        const int l = tile * BP_TILE + (int)ll;
        if (indel == 0u) {                                                      // an unusual letter: TYPE 'SNP', and maybe the reference's own
            atomicOr(&smask[ll], 1ull << id);
            if ((uint32_t)A.bq[2ull * (A.aln[ai].seq_off + qpos)] == (uint32_t)A.refseq[l]) refid[ll] = id;
        }
        const uint32_t slot = rep_base + j;
        if (slot < A.xcap) { uint32_t* o = A.xlist + 5 * (size_t)slot; o[0] = (uint32_t)l; o[1] = id; o[2] = ai; o[3] = qpos; o[4] = indel; }
        else atomicOr(A.status, BP_ST_XLIST);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    // ---- the reads' allele bytes; the descriptors
    for (uint32_t c = 0; c < nt; c += 64u) {
        const uint32_t i = c + (uint32_t)lane;
        if (i < nt) {
            const uint32_t* e = A.xraw + (size_t)BP_XW * g[i];
            const uint32_t sp = e[1], id = cid[e[5]];
            // (the allele id is byte 0 of the word: a byte store, no read of the word before it)
            bp_patch_allele(A, sp, id);
            if (A.meta) ((uint8_t*)A.meta)[4ull * sp] = (uint8_t)id;
        }
    }
    const int l = tile * BP_TILE + lane;
    if (l < A.n_loci && nkl[lane] != 0u) {
        int ra = bp_fixed_allele(A.refseq[l]);
        if (ra < 0) ra = refid[lane] ? (int)refid[lane] : 255;
        A.loci[l].ref_allele = (uint8_t)ra; A.loci[l].n_alleles = (uint8_t)min(6u + nkl[lane], 64u); A.loci[l].snp_mask = 0x1full | smask[lane];
    }
}
