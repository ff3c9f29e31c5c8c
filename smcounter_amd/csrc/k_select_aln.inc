// Included by smcounter_hip.hip (after k_philox_marks.inc: it uses smc_philox4x32_10).
// ------------------------------------------------------------------------------------------
// in-run molecule down-sampling: the alignments of the kept barcodes of a run, and the decoder's windows / depths over them
// (smc_select_alignments)
// ------------------------------------------------------------------------------------------
// ds.mt.py:23-72 keeps every molecular barcode (with all its reads) with probability f and writes a BAM; smCounter then runs on
// that BAM.  Here the run's alignments are already in HBM: the drop is done on them, and the descriptors are recomputed exactly as
// smc_bam_alignments (csrc/smc_bam.cpp) would compute them for the down-sampled BAM - so the plane builder and everything after it
// run unchanged on the result.  A barcode is all in or all out, so the kept alignments keep the file order, the ids keep their
// order (with gaps: the builder only compares them), and the decoder's rules carry over.
// (ABI 10) The key of the rule can also be the read: ds.reads.withinMT.py keeps whole read names (all alignments of a name or none),
// by read-name id (pair_gid) - the host makes sure no id of the run covers two names.  A read name is all in or all out, so the
// windows and depths below carry over.  The ids do not: a barcode whose first read was dropped can come out of first-appearance
// order, and the builder's rows are not independent of the ids' numeric order (tests/test_gpu_ds_rpb.py puts a run's ids through a
// random bijection: the rows of two fixtures change).  So the read-level rule renumbers the kept ids by first kept appearance, as
// the decoder numbers the down-sampled BAM's (k_sel_first / k_sel_rcount / k_sel_offsets / k_sel_rank / k_sel_regid below):
//   w0'  = first kept alignment with end > p       (= first index whose running maximum of end passes p: a monotone predicate)
//   w1'  = max(w0', first kept alignment with pos > p)
//   n'   = kept alignments with pos <= p < end     (a difference array over the run's positions, then a scan)
//   slot_off' = exclusive scan of n' rounded up to 4
// Five launches on one stream:
//   k_sel_count    per block of SEL_ITEMS alignments: how many are kept
//   k_sel_offsets  one workgroup: exclusive scan of the block counts (the kept total into the summary); clears the difference array
//   k_sel_scatter  the kept alignments and their input index compacted in file order (ballot ranks, the same rounds as k_sel_count);
//                  +1 / -1 of every kept alignment into the difference array through an LDS window; the block's largest kept end
//   k_sel_loci     one workgroup: running maximum of the block ends, the depths by a scan of the difference array, slot_off', the
//                  deepest locus and the slots into the summary
//   k_sel_windows  a wavefront per locus: w0' by a 64-way search over the blocks' running end maximum, then a scan of that block's
//                  kept ends; w1' by a 64-way search over the kept positions
#define SEL_BLOCK 256
#define SEL_ROUNDS 4
#define SEL_ITEMS (SEL_BLOCK * SEL_ROUNDS)   // alignments per block (a round: SEL_BLOCK consecutive ones, one per thread)
#define SEL_SCAN 1024                        // threads of the one-workgroup scans
#define SEL_WIN 4096                         // LDS window of the difference array per block (positions beyond it: global atomics)
#define SEL_DOMAIN 0x64734D54u               // counter word 2 of the down-sampling draw ("dsMT"); smc_philox_marks uses 0 there

struct SelRule {
    const uint32_t* mask;              // non-null: bit g of the mask keeps barcode g (the host's set: the reference's semantics)
    const unsigned long long* ident;   // else: one 64-bit identity per barcode, kept iff Philox word 0 < thr
    unsigned long long seed, thr;      // thr = floor(f * 2^32); >= 2^32: everything
    uint32_t n_ids;                    // ids at or beyond this are not kept (never met: the decoder numbers below n_bc / n_pair)
    uint32_t by_read;                  // 0: the key is the barcode id (bc_gid); 1: the read-name id (pair_gid)
};

__device__ __forceinline__ uint32_t sel_key(const SelRule& R, const smc_dev_aln& a) { return R.by_read ? a.pair_gid : a.bc_gid; }

// the barcode draw of the philox rule: word 0 of Philox4x32-10(identity lo, hi, SEL_DOMAIN, 0; seed).  (Shared with --dsGrid's passes
// over the file-wide table, k_read_groups.inc: the two cannot drift.)
__device__ __forceinline__ uint32_t sel_draw(unsigned long long id, unsigned long long seed) {
    uint32_t x[4];
    smc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), SEL_DOMAIN, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
    return x[0];
}

__device__ __forceinline__ bool sel_keep(const SelRule& R, uint32_t gid) {
    if (gid >= R.n_ids) return false;
    if (R.mask) return ((R.mask[gid >> 5] >> (gid & 31u)) & 1u) != 0u;
    if (R.thr >= (1ull << 32)) return true;
    return (unsigned long long)sel_draw(R.ident[gid], R.seed) < R.thr;
}

__global__ __launch_bounds__(SEL_BLOCK) void k_sel_count(const smc_dev_aln* __restrict__ aln, uint32_t n_aln, SelRule R,
                                                         uint32_t* __restrict__ blk_cnt) {
    __shared__ uint32_t wsum[SEL_BLOCK / WAVE];
    const uint32_t base = blockIdx.x * (uint32_t)SEL_ITEMS;
    uint32_t mine = 0;
#pragma unroll
    for (int r = 0; r < SEL_ROUNDS; ++r) {
        const uint32_t i = base + (uint32_t)r * SEL_BLOCK + threadIdx.x;
        if (i < n_aln && sel_keep(R, R.by_read ? aln[i].pair_gid : aln[i].bc_gid)) ++mine;
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((threadIdx.x & (WAVE - 1)) == 0) wsum[threadIdx.x / WAVE] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < SEL_BLOCK / WAVE; ++w) s += wsum[w];
        blk_cnt[blockIdx.x] = s;
    }
}

// one workgroup's exclusive scan (op: sum or max) of the values v[t] of its SEL_SCAN threads; -> (exclusive, total)
template <bool MAX>
__device__ __forceinline__ void sel_wg_scan(int64_t v, int64_t* buf, int64_t id, int64_t& excl, int64_t& total) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int o = 1; o < SEL_SCAN; o <<= 1) {
        const int64_t a = t >= o ? buf[t - o] : id;
        __syncthreads();
        buf[t] = MAX ? (a > buf[t] ? a : buf[t]) : buf[t] + a;
        __syncthreads();
    }
    excl = t ? buf[t - 1] : id;
    total = buf[SEL_SCAN - 1];
    __syncthreads();
}

// (the stage's work for one selection: k_sel_offsets, and k_selc_offsets per selection of a batch)
__device__ __forceinline__ void sel_offsets_body(uint32_t* __restrict__ blk_cnt, uint32_t n_blk, int32_t* __restrict__ diff, uint32_t n_diff,
                                                 uint32_t* __restrict__ summary) {
    __shared__ int64_t buf[SEL_SCAN];
    const uint32_t t = threadIdx.x, per = (n_blk + SEL_SCAN - 1) / SEL_SCAN, b0 = min(n_blk, t * per), b1 = min(n_blk, b0 + per);
    int64_t s = 0;
    for (uint32_t b = b0; b < b1; ++b) s += blk_cnt[b];
    int64_t excl, total;
    sel_wg_scan<false>(s, buf, 0, excl, total);
    for (uint32_t b = b0; b < b1; ++b) { const uint32_t c = blk_cnt[b]; blk_cnt[b] = (uint32_t)excl; excl += c; }
    if (t == 0) { blk_cnt[n_blk] = (uint32_t)total; summary[0] = (uint32_t)total; }
    for (uint32_t i = t; i < n_diff; i += SEL_SCAN) diff[i] = 0;
}

__global__ __launch_bounds__(SEL_SCAN) void k_sel_offsets(uint32_t* __restrict__ blk_cnt, uint32_t n_blk, int32_t* __restrict__ diff,
                                                          uint32_t n_diff, uint32_t* __restrict__ summary) {
    sel_offsets_body(blk_cnt, n_blk, diff, n_diff, summary);
}

__global__ __launch_bounds__(SEL_BLOCK) void k_sel_scatter(const smc_dev_aln* __restrict__ aln, uint32_t n_aln, SelRule R,
                                                           const uint32_t* __restrict__ blk_off, int32_t start0, uint32_t n_loci,
                                                           smc_dev_aln* __restrict__ out, uint32_t* __restrict__ orig_index,
                                                           int32_t* __restrict__ diff, int32_t* __restrict__ blk_maxend) {
    __shared__ int32_t win[SEL_WIN];
    __shared__ uint32_t wcnt[SEL_BLOCK / WAVE];
    __shared__ int32_t wmax[SEL_BLOCK / WAVE];
    const uint32_t t = threadIdx.x, wv = t / WAVE, base = blockIdx.x * (uint32_t)SEL_ITEMS;
    for (uint32_t k = t; k < SEL_WIN; k += SEL_BLOCK) win[k] = 0;
    // (the block's alignments are sorted by position: the window starts at the first one's)
    const int32_t wbase = max(aln[base].pos, start0) - start0;
    __syncthreads();
    uint32_t dst = blk_off[blockIdx.x];
    int32_t me = INT_MIN;
    auto add = [&](int32_t x, int32_t d) {
        const uint32_t k = (uint32_t)(x - wbase);
        if (k < (uint32_t)SEL_WIN) atomicAdd(&win[k], d); else atomicAdd(&diff[x], d);
    };
#pragma unroll 1
    for (int r = 0; r < SEL_ROUNDS; ++r) {
        const uint32_t i = base + (uint32_t)r * SEL_BLOCK + t;
        smc_dev_aln a;
        bool keep = false;
        if (i < n_aln) { a = aln[i]; keep = sel_keep(R, sel_key(R, a)); }
        const unsigned long long m = __ballot(keep);
        const uint32_t lane = t & (WAVE - 1), rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wcnt[wv] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (uint32_t w = 0; w < SEL_BLOCK / WAVE; ++w) { before += w < wv ? wcnt[w] : 0u; all += wcnt[w]; }
        if (keep) {
            out[dst + before + rank] = a;
            orig_index[dst + before + rank] = i;
            const int32_t lo = max(a.pos, start0) - start0, hi = (int32_t)min<int64_t>((int64_t)a.end, (int64_t)start0 + n_loci) - start0;
            if (lo < hi) { add(lo, 1); add(hi, -1); }
            me = max(me, a.end);
        }
        dst += all;
        __syncthreads();                                   // (wcnt is rewritten by the next round)
    }
    for (int o = WAVE / 2; o > 0; o >>= 1) me = max(me, __shfl_xor(me, o));
    if ((t & (WAVE - 1)) == 0) wmax[wv] = me;
    __syncthreads();
    if (t == 0) {
        int32_t m = INT_MIN;
        for (int w = 0; w < SEL_BLOCK / WAVE; ++w) m = max(m, wmax[w]);
        blk_maxend[blockIdx.x] = m;
    }
    for (uint32_t k = t; k < SEL_WIN; k += SEL_BLOCK) {
        const int32_t v = win[k];
        if (v && wbase + (int32_t)k <= (int32_t)n_loci) atomicAdd(&diff[wbase + (int32_t)k], v);
    }
}

__device__ __forceinline__ void sel_loci_body(int32_t* __restrict__ blk_maxend, uint32_t n_blk, const int32_t* __restrict__ diff,
                                              uint32_t n_loci, smc_dev_locus* __restrict__ loc_out, uint32_t* __restrict__ summary) {
    __shared__ int64_t buf[SEL_SCAN];
    __shared__ uint32_t deepest;
    const uint32_t t = threadIdx.x;
    if (t == 0) deepest = 0u;
    // the running maximum of the blocks' largest kept end (inclusive): what k_sel_windows searches for w0'
    {
        const uint32_t per = (n_blk + SEL_SCAN - 1) / SEL_SCAN, b0 = min(n_blk, t * per), b1 = min(n_blk, b0 + per);
        int64_t m = INT_MIN;
        for (uint32_t b = b0; b < b1; ++b) m = max(m, (int64_t)blk_maxend[b]);
        int64_t excl, total;
        sel_wg_scan<true>(m, buf, INT_MIN, excl, total);
        for (uint32_t b = b0; b < b1; ++b) { excl = max(excl, (int64_t)blk_maxend[b]); blk_maxend[b] = (int32_t)excl; }
    }
    // depths: a scan of the difference array (each thread a stretch of loci); then the 4-aligned slots
    const uint32_t per = (n_loci + SEL_SCAN - 1) / SEL_SCAN, l0 = min(n_loci, t * per), l1 = min(n_loci, l0 + per);
    int64_t s = 0;
    for (uint32_t l = l0; l < l1; ++l) s += diff[l];
    int64_t d_before, d_total;
    sel_wg_scan<false>(s, buf, 0, d_before, d_total);
    int64_t depth = d_before, slots = 0;
    uint32_t dmax = 0;
    for (uint32_t l = l0; l < l1; ++l) { depth += diff[l]; slots += (depth + 3) / 4 * 4; dmax = max(dmax, (uint32_t)depth); }
    int64_t so, s_total;
    sel_wg_scan<false>(slots, buf, 0, so, s_total);
    depth = d_before;
    for (uint32_t l = l0; l < l1; ++l) {
        depth += diff[l];
        loc_out[l].slot_off = (uint32_t)so;
        loc_out[l].n = (uint32_t)depth;
        so += (depth + 3) / 4 * 4;
    }
    atomicMax(&deepest, dmax);
    __syncthreads();
    if (t == 0) { summary[1] = deepest; summary[2] = (uint32_t)s_total; }
}

__global__ __launch_bounds__(SEL_SCAN) void k_sel_loci(int32_t* __restrict__ blk_maxend, uint32_t n_blk, const int32_t* __restrict__ diff,
                                                       uint32_t n_loci, smc_dev_locus* __restrict__ loc_out, uint32_t* __restrict__ summary) {
    sel_loci_body(blk_maxend, n_blk, diff, n_loci, loc_out, summary);
}

// first index j in [lo, hi) with pred(j), pred monotone (false ... false true ... true); hi when there is none.  64 probes a step.
template <typename P>
__device__ __forceinline__ uint32_t sel_search(uint32_t lo, uint32_t hi, P pred) {
    const uint32_t lane = threadIdx.x & (WAVE - 1);
    while (hi - lo > WAVE) {
        // probes s_k = lo + k * step (a probe at or beyond hi counts as true); the answer lies behind the last false probe and at or
        // before the first true one
        const uint32_t step = (hi - lo + WAVE - 1) / WAVE, s = lo + lane * step;
        const unsigned long long m = __ballot(s >= hi || pred(s));
        if (m == 0ull) { lo += (WAVE - 1) * step + 1; continue; }
        const uint32_t f = (uint32_t)__ffsll((long long)m) - 1u;
        if (f == 0) return lo;
        const uint32_t sf = lo + f * step;
        lo += (f - 1) * step + 1;
        hi = min(hi, sf);
    }
    const uint32_t s = lo + lane;
    const unsigned long long m = __ballot(s < hi && pred(s));
    return m ? lo + (uint32_t)__ffsll((long long)m) - 1u : hi;
}

// a wavefront per locus: w0' = first kept alignment whose end passes p (the block by the running maximum of the blocks' ends - a
// monotone predicate - then the first such end within that block's kept range); w1' = max(w0', first kept alignment with pos > p)
__device__ __forceinline__ void sel_windows_body(const smc_dev_aln* __restrict__ out, const uint32_t* __restrict__ blk_off,
                                                 const int32_t* __restrict__ blk_runmax, uint32_t n_blk, int32_t start0, uint32_t n_loci,
                                                 smc_dev_locus* __restrict__ loc_out) {
    const uint32_t l = blockIdx.x * (SEL_BLOCK / WAVE) + threadIdx.x / WAVE;
    if (l >= n_loci) return;
    const int32_t p = start0 + (int32_t)l;
    const uint32_t kept = blk_off[n_blk];
    const uint32_t b = sel_search(0u, n_blk, [&](uint32_t j) { return blk_runmax[j] > p; });
    uint32_t w0 = kept;
    if (b < n_blk) {
        // (ends are not sorted: the block's kept range is scanned in order, 64 at a time; its first end beyond p is the answer - every
        // kept alignment of the blocks before it ends at or before p)
        const uint32_t lane = threadIdx.x & (WAVE - 1), j1 = blk_off[b + 1];
        for (uint32_t j0 = blk_off[b]; j0 < j1; j0 += WAVE) {
            const unsigned long long m = __ballot(j0 + lane < j1 && out[j0 + lane].end > p);
            if (m) { w0 = j0 + (uint32_t)__ffsll((long long)m) - 1u; break; }
        }
    }
    const uint32_t w1 = sel_search(w0, kept, [&](uint32_t j) { return out[j].pos > p; });
    if ((threadIdx.x & (WAVE - 1)) == 0) { loc_out[l].w0 = w0; loc_out[l].w1 = w1; }
}

__global__ __launch_bounds__(SEL_BLOCK) void k_sel_windows(const smc_dev_aln* __restrict__ out, const uint32_t* __restrict__ blk_off,
                                                           const int32_t* __restrict__ blk_runmax, uint32_t n_blk, int32_t start0,
                                                           uint32_t n_loci, smc_dev_locus* __restrict__ loc_out) {
    sel_windows_body(out, blk_off, blk_runmax, n_blk, start0, n_loci, loc_out);
}

// ---- (read level) the kept ids renumbered by first kept appearance: both bc_gid and pair_gid of d_aln_out, dense from 0 in the order
// the kept alignments first meet them - the decoder's numbering of the down-sampled BAM.  Grids cover the n_aln input alignments
// (an upper bound of the kept ones: their count is on the device); first[] / map[] hold one word per input id (n_bc + n_pair).
struct SelIds {
    uint32_t* first;          // [n_bc + n_pair]: the first kept index of every id (0xFFFFFFFF: not kept); pair ids behind the barcodes'
    uint32_t* map;            // [n_bc + n_pair]: the new id of every kept id
    uint32_t n_bc, n_pair;
};

__device__ __forceinline__ uint32_t sel_slot(const SelIds& I, const smc_dev_aln& a, int which) {   // -> index into first / map, or ~0
    return which == 0 ? (a.bc_gid < I.n_bc ? a.bc_gid : 0xFFFFFFFFu) : (a.pair_gid < I.n_pair ? I.n_bc + a.pair_gid : 0xFFFFFFFFu);
}

__device__ __forceinline__ void sel_first_body(const smc_dev_aln* __restrict__ out, const uint32_t* __restrict__ summary, const SelIds& I) {
    const uint32_t kept = summary[0], base = blockIdx.x * (uint32_t)SEL_ITEMS;
    for (int r = 0; r < SEL_ROUNDS; ++r) {
        const uint32_t k = base + (uint32_t)r * SEL_BLOCK + threadIdx.x;
        if (k >= kept) break;
        const smc_dev_aln a = out[k];
        for (int w = 0; w < 2; ++w) {
            const uint32_t s = sel_slot(I, a, w);
            if (s != 0xFFFFFFFFu) atomicMin(&I.first[s], k);
        }
    }
}

__global__ __launch_bounds__(SEL_BLOCK) void k_sel_first(const smc_dev_aln* __restrict__ out, const uint32_t* __restrict__ summary, SelIds I) {
    sel_first_body(out, summary, I);
}

// per block: the kept alignments that are the first of their barcode (cnt[b]) / of their read name (cnt[n_blk + 1 + b])
__device__ __forceinline__ void sel_rcount_body(const smc_dev_aln* __restrict__ out, const uint32_t* __restrict__ summary, const SelIds& I,
                                                uint32_t n_blk, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t wsum[2][SEL_BLOCK / WAVE];
    const uint32_t kept = summary[0], base = blockIdx.x * (uint32_t)SEL_ITEMS;
    uint32_t mine[2] = {0u, 0u};
    for (int r = 0; r < SEL_ROUNDS; ++r) {
        const uint32_t k = base + (uint32_t)r * SEL_BLOCK + threadIdx.x;
        if (k >= kept) break;
        const smc_dev_aln a = out[k];
        for (int w = 0; w < 2; ++w) {
            const uint32_t s = sel_slot(I, a, w);
            if (s != 0xFFFFFFFFu && I.first[s] == k) ++mine[w];
        }
    }
    for (int w = 0; w < 2; ++w) {
        for (int o = WAVE / 2; o > 0; o >>= 1) mine[w] += __shfl_xor(mine[w], o);
        if ((threadIdx.x & (WAVE - 1)) == 0) wsum[w][threadIdx.x / WAVE] = mine[w];
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        uint32_t t = 0;
        for (int v = 0; v < SEL_BLOCK / WAVE; ++v) t += wsum[threadIdx.x][v];
        cnt[threadIdx.x * (n_blk + 1) + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(SEL_BLOCK) void k_sel_rcount(const smc_dev_aln* __restrict__ out, const uint32_t* __restrict__ summary, SelIds I,
                                                          uint32_t n_blk, uint32_t* __restrict__ cnt) {
    sel_rcount_body(out, summary, I, n_blk, cnt);
}

// per block (block offsets: the exclusive scans of k_sel_rcount's counts): the first kept alignment of every id gives it its new id
// (ballot ranks within a round, the rounds in order - as k_sel_scatter ranks the kept alignments)
__device__ __forceinline__ void sel_rank_body(const smc_dev_aln* __restrict__ out, const uint32_t* __restrict__ summary, const SelIds& I,
                                              uint32_t n_blk, const uint32_t* __restrict__ off) {
    __shared__ uint32_t wcnt[2][SEL_BLOCK / WAVE];
    const uint32_t t = threadIdx.x, wv = t / WAVE, lane = t & (WAVE - 1), kept = summary[0], base = blockIdx.x * (uint32_t)SEL_ITEMS;
    uint32_t dst[2] = {off[blockIdx.x], off[n_blk + 1 + blockIdx.x]};
#pragma unroll 1
    for (int r = 0; r < SEL_ROUNDS; ++r) {
        const uint32_t k = base + (uint32_t)r * SEL_BLOCK + t;
        uint32_t s[2] = {0xFFFFFFFFu, 0xFFFFFFFFu};
        bool head[2] = {false, false};
        if (k < kept) {
            const smc_dev_aln a = out[k];
            for (int w = 0; w < 2; ++w) { s[w] = sel_slot(I, a, w); head[w] = s[w] != 0xFFFFFFFFu && I.first[s[w]] == k; }
        }
        uint32_t rank[2];
        for (int w = 0; w < 2; ++w) {
            const unsigned long long m = __ballot(head[w]);
            rank[w] = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[w][wv] = (uint32_t)__popcll(m);
        }
        __syncthreads();
        for (int w = 0; w < 2; ++w) {
            uint32_t before = 0, all = 0;
            for (uint32_t v = 0; v < SEL_BLOCK / WAVE; ++v) { before += v < wv ? wcnt[w][v] : 0u; all += wcnt[w][v]; }
            if (head[w]) I.map[s[w]] = dst[w] + before + rank[w];
            dst[w] += all;
        }
        __syncthreads();                                   // (wcnt is rewritten by the next round)
    }
}

__global__ __launch_bounds__(SEL_BLOCK) void k_sel_rank(const smc_dev_aln* __restrict__ out, const uint32_t* __restrict__ summary, SelIds I,
                                                        uint32_t n_blk, const uint32_t* __restrict__ off) {
    sel_rank_body(out, summary, I, n_blk, off);
}

__device__ __forceinline__ void sel_regid_body(smc_dev_aln* __restrict__ out, const uint32_t* __restrict__ summary, const SelIds& I) {
    const uint32_t kept = summary[0], base = blockIdx.x * (uint32_t)SEL_ITEMS;
    for (int r = 0; r < SEL_ROUNDS; ++r) {
        const uint32_t k = base + (uint32_t)r * SEL_BLOCK + threadIdx.x;
        if (k >= kept) break;
        const smc_dev_aln a = out[k];
        const uint32_t sb = sel_slot(I, a, 0), sp = sel_slot(I, a, 1);
        if (sb != 0xFFFFFFFFu) out[k].bc_gid = I.map[sb];
        if (sp != 0xFFFFFFFFu) out[k].pair_gid = I.map[sp];
    }
}

__global__ __launch_bounds__(SEL_BLOCK) void k_sel_regid(smc_dev_aln* __restrict__ out, const uint32_t* __restrict__ summary, SelIds I) {
    sel_regid_body(out, summary, I);
}

// ------------------------------------------------------------------------------------------
// the philox selections of several copies of a run at several fractions in one call (smc_select_alignments_copies)
// ------------------------------------------------------------------------------------------
// --spikeScanDepth and its kin select every spiked copy of a run at every listed fraction: n_copies x n_fracs single calls, each five
// launches and a download.  The draw of a barcode depends on (identity, seed) alone, so one draw per (alignment, copy) serves every
// fraction.  The same five stages, the selection s = fraction x n_copies + copy a grid dimension, every array of the single call
// (block counts / offsets, block end maxima, difference array, outputs, summary) once per selection:
//   k_selc_count    grid (blocks, copies): one draw per alignment, a ballot per fraction, the kept counts of the block per fraction
//   k_selc_offsets  a workgroup per selection: k_sel_offsets' work
//   k_selc_scatter  grid (blocks, copies): the draws kept in registers; per fraction k_sel_scatter's rounds, the one LDS window of
//                   the difference array zeroed and flushed per fraction
//   k_selc_loci     a workgroup per selection: k_sel_loci's work
//   k_selc_windows  grid (loci / 4, selections): k_sel_windows' work
// Seeds and thresholds travel in the launch's arguments, SEL_CP_COPIES x SEL_CP_FRACS of them: a larger batch takes several launches
// of the two record stages (a draw is then made once per group of SEL_CP_FRACS fractions).
#define SEL_CP_COPIES 32
#define SEL_CP_FRACS 32

struct SelCopies {
    unsigned long long seed[SEL_CP_COPIES];   // of copies c0 .. c0 + gridDim.y - 1
    unsigned long long thr[SEL_CP_FRACS];     // of fractions f0 .. f0 + n_f - 1: floor(f * 2^32), 2^32: everything
    uint32_t c0, f0, n_f;
    uint32_t n_copies;                        // of the whole call: selection s = f * n_copies + c
};

// the copy's record i of a block round, whether it can be kept at all (a barcode id the table holds) and its barcode's draw
__device__ __forceinline__ bool selc_draw(const smc_dev_aln* __restrict__ aln, uint32_t i, uint32_t n_aln,
                                          const unsigned long long* __restrict__ ident, uint32_t n_ids, unsigned long long seed, uint32_t& draw) {
    draw = 0u;
    if (i >= n_aln) return false;
    const uint32_t g = aln[i].bc_gid;
    if (g >= n_ids) return false;
    draw = sel_draw(ident[g], seed);
    return true;
}

// The keep rule of a batch's two record stages: per (alignment, copy) one word made once (`load`: false when the record cannot be
// kept at all), tested per selection j of the launch (`keep`).  SelcPhilox: the barcode's draw against the nested thresholds;
// SelcBits (smc_select_alignments_reads_copies, below): bit j of the word = the read name's bit in mask m0 + j of the copy.
struct SelcPhilox {
    const unsigned long long* __restrict__ ident;
    uint32_t n_ids;
    unsigned long long seed;
    const SelCopies& K;
    __device__ __forceinline__ bool load(const smc_dev_aln* __restrict__ aln, uint32_t i, uint32_t n_aln, uint32_t& v) const {
        return selc_draw(aln, i, n_aln, ident, n_ids, seed, v);
    }
    __device__ __forceinline__ bool keep(bool ok, uint32_t v, uint32_t j) const { return ok && (unsigned long long)v < K.thr[j]; }
};

// (n_j selections j0 .. j0 + n_j - 1 of copy c, of a call of n_copies copies: selection s = j x n_copies + c)
template <typename P>
__device__ __forceinline__ void selc_count_body(const smc_dev_aln* __restrict__ aln, uint32_t n_aln, const P& rule, uint32_t c, uint32_t j0,
                                                uint32_t n_j, uint32_t n_copies, uint32_t n_blk, uint32_t* __restrict__ blk_cnt_all) {
    __shared__ uint32_t cnt[SEL_CP_FRACS];
    const uint32_t t = threadIdx.x, base = blockIdx.x * (uint32_t)SEL_ITEMS;
    if (t < SEL_CP_FRACS) cnt[t] = 0u;
    __syncthreads();
#pragma unroll 1
    for (int r = 0; r < SEL_ROUNDS; ++r) {
        uint32_t v;
        const bool ok = rule.load(aln, base + (uint32_t)r * SEL_BLOCK + t, n_aln, v);
        for (uint32_t j = 0; j < n_j; ++j) {
            const unsigned long long m = __ballot(rule.keep(ok, v, j));
            if ((t & (WAVE - 1)) == 0 && m) atomicAdd(&cnt[j], (uint32_t)__popcll(m));
        }
    }
    __syncthreads();
    if (t < n_j) blk_cnt_all[((size_t)(j0 + t) * n_copies + c) * (n_blk + 1u) + blockIdx.x] = cnt[t];
}

__global__ __launch_bounds__(SEL_BLOCK) void k_selc_count(const char* __restrict__ aln_base, unsigned long long aln_stride, uint32_t n_aln,
                                                          const unsigned long long* __restrict__ ident, uint32_t n_ids, SelCopies K,
                                                          uint32_t n_blk, uint32_t* __restrict__ blk_cnt_all) {
    const uint32_t c = K.c0 + blockIdx.y;
    const SelcPhilox rule{ident, n_ids, K.seed[blockIdx.y], K};
    selc_count_body((const smc_dev_aln*)(aln_base + (size_t)c * aln_stride), n_aln, rule, c, K.f0, K.n_f, K.n_copies, n_blk, blk_cnt_all);
}

__global__ __launch_bounds__(SEL_SCAN) void k_selc_offsets(uint32_t* __restrict__ blk_cnt_all, uint32_t n_blk, int32_t* __restrict__ diff_all,
                                                           uint32_t n_diff, uint32_t* __restrict__ summary) {
    const size_t s = blockIdx.x;
    sel_offsets_body(blk_cnt_all + s * (n_blk + 1u), n_blk, diff_all + s * n_diff, n_diff, summary + 4 * s);
}

template <typename P>
__device__ __forceinline__ void selc_scatter_body(const smc_dev_aln* __restrict__ aln, uint32_t n_aln, const P& rule, uint32_t c, uint32_t j0,
                                                  uint32_t n_j, uint32_t n_copies, uint32_t n_blk, const uint32_t* __restrict__ blk_off_all,
                                                  int32_t start0, uint32_t n_loci, smc_dev_aln* __restrict__ out_all,
                                                  uint32_t* __restrict__ orig_all, int32_t* __restrict__ diff_all,
                                                  int32_t* __restrict__ blk_maxend_all) {
    __shared__ int32_t win[SEL_WIN];
    __shared__ uint32_t wcnt[SEL_BLOCK / WAVE];
    __shared__ int32_t wmax[SEL_BLOCK / WAVE];
    const uint32_t t = threadIdx.x, wv = t / WAVE, lane = t & (WAVE - 1), base = blockIdx.x * (uint32_t)SEL_ITEMS;
    uint32_t v[SEL_ROUNDS];
    bool ok[SEL_ROUNDS];
#pragma unroll
    for (int r = 0; r < SEL_ROUNDS; ++r) ok[r] = rule.load(aln, base + (uint32_t)r * SEL_BLOCK + t, n_aln, v[r]);
    // (the block's alignments are sorted by position: the window starts at the first one's)
    const int32_t wbase = max(aln[base].pos, start0) - start0;
#pragma unroll 1
    for (uint32_t j = 0; j < n_j; ++j) {
        const size_t s = (size_t)(j0 + j) * n_copies + c;
        smc_dev_aln* out = out_all + s * n_aln;
        uint32_t* orig_index = orig_all + s * n_aln;
        int32_t* diff = diff_all + s * ((size_t)n_loci + 1u);
        for (uint32_t k = t; k < SEL_WIN; k += SEL_BLOCK) win[k] = 0;
        __syncthreads();
        uint32_t dst = blk_off_all[s * (n_blk + 1u) + blockIdx.x];
        int32_t me = INT_MIN;
        auto add = [&](int32_t x, int32_t d) {
            const uint32_t k = (uint32_t)(x - wbase);
            if (k < (uint32_t)SEL_WIN) atomicAdd(&win[k], d); else atomicAdd(&diff[x], d);
        };
#pragma unroll
        for (int r = 0; r < SEL_ROUNDS; ++r) {
            const uint32_t i = base + (uint32_t)r * SEL_BLOCK + t;
            const bool keep = rule.keep(ok[r], v[r], j);
            const unsigned long long m = __ballot(keep);
            const uint32_t rank = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (lane == 0) wcnt[wv] = (uint32_t)__popcll(m);
            __syncthreads();
            uint32_t before = 0, all = 0;
            for (uint32_t w = 0; w < SEL_BLOCK / WAVE; ++w) { before += w < wv ? wcnt[w] : 0u; all += wcnt[w]; }
            if (keep) {
                const smc_dev_aln a = aln[i];
                out[dst + before + rank] = a;
                orig_index[dst + before + rank] = i;
                const int32_t lo = max(a.pos, start0) - start0, hi = (int32_t)min<int64_t>((int64_t)a.end, (int64_t)start0 + n_loci) - start0;
                if (lo < hi) { add(lo, 1); add(hi, -1); }
                me = max(me, a.end);
            }
            dst += all;
            __syncthreads();                               // (wcnt is rewritten by the next round)
        }
        for (int o = WAVE / 2; o > 0; o >>= 1) me = max(me, __shfl_xor(me, o));
        if (lane == 0) wmax[wv] = me;
        __syncthreads();
        if (t == 0) {
            int32_t m = INT_MIN;
            for (int w = 0; w < SEL_BLOCK / WAVE; ++w) m = max(m, wmax[w]);
            blk_maxend_all[s * (n_blk + 1u) + blockIdx.x] = m;
        }
        for (uint32_t k = t; k < SEL_WIN; k += SEL_BLOCK) {
            const int32_t x = win[k];
            if (x && wbase + (int32_t)k <= (int32_t)n_loci) atomicAdd(&diff[wbase + (int32_t)k], x);
        }
        __syncthreads();                                   // (win and wmax are rewritten by the next selection)
    }
}

__global__ __launch_bounds__(SEL_BLOCK) void k_selc_scatter(const char* __restrict__ aln_base, unsigned long long aln_stride, uint32_t n_aln,
                                                            const unsigned long long* __restrict__ ident, uint32_t n_ids, SelCopies K,
                                                            uint32_t n_blk, const uint32_t* __restrict__ blk_off_all, int32_t start0,
                                                            uint32_t n_loci, smc_dev_aln* __restrict__ out_all, uint32_t* __restrict__ orig_all,
                                                            int32_t* __restrict__ diff_all, int32_t* __restrict__ blk_maxend_all) {
    const uint32_t c = K.c0 + blockIdx.y;
    const SelcPhilox rule{ident, n_ids, K.seed[blockIdx.y], K};
    selc_scatter_body((const smc_dev_aln*)(aln_base + (size_t)c * aln_stride), n_aln, rule, c, K.f0, K.n_f, K.n_copies, n_blk, blk_off_all,
                      start0, n_loci, out_all, orig_all, diff_all, blk_maxend_all);
}

__global__ __launch_bounds__(SEL_SCAN) void k_selc_loci(int32_t* __restrict__ blk_maxend_all, uint32_t n_blk, const int32_t* __restrict__ diff_all,
                                                        uint32_t n_loci, smc_dev_locus* __restrict__ loc_out, uint32_t* __restrict__ summary) {
    const size_t s = blockIdx.x;
    sel_loci_body(blk_maxend_all + s * (n_blk + 1u), n_blk, diff_all + s * ((size_t)n_loci + 1u), n_loci, loc_out + s * n_loci, summary + 4 * s);
}

__global__ __launch_bounds__(SEL_BLOCK) void k_selc_windows(const smc_dev_aln* __restrict__ out_all, uint32_t n_aln,
                                                            const uint32_t* __restrict__ blk_off_all, const int32_t* __restrict__ blk_runmax_all,
                                                            uint32_t n_blk, int32_t start0, uint32_t n_loci, smc_dev_locus* __restrict__ loc_out) {
    const size_t s = blockIdx.y;
    sel_windows_body(out_all + s * n_aln, blk_off_all + s * (n_blk + 1u), blk_runmax_all + s * (n_blk + 1u), n_blk, start0, n_loci,
                     loc_out + s * n_loci);
}

// ------------------------------------------------------------------------------------------
// the read-level selections of several copies of a run under several keep masks in one call (smc_select_alignments_reads_copies)
// ------------------------------------------------------------------------------------------
// --spikeScanRpb selects every spiked copy of a run at every reads-per-barcode target: the read-level rule of
// smc_select_alignments_keyed (SMC_SEL_KEY_READ) with a keep mask per (copy, target) - ReadGroups.masks writes them; the sets of a
// copy are NOT nested - and the renumbering of the kept ids per selection.  Selection s = mask x n_copies + copy.  The five selection
// stages are k_selc_*'s: the record stages with the SelcBits rule (a record's pair_gid tested against the launch's masks of its copy
// once, the bits kept in a register), k_selc_offsets / k_selc_loci / k_selc_windows as they are.  The five renumbering stages are
// k_sel_first / k_sel_rcount / k_sel_offsets / k_sel_rank / k_sel_regid's bodies with the selection on blockIdx.y: each reads its own
// summary[4 s]; first / map hold n_bc + n_pair words per selection, the counts 2 x (n_blk + 1) per selection.
struct SelReadCopies {
    const uint32_t* masks;                    // mask (copy c, mask m) at masks + c * copy_stride + m * mask_words (words)
    unsigned long long mask_words, copy_stride;
    uint32_t n_ids;                           // read-name ids at or beyond this are not kept
    uint32_t m0, n_m;                         // the launch's masks m0 .. m0 + n_m - 1 (n_m <= SEL_CP_FRACS: a bit each)
    uint32_t n_copies;                        // of the whole call
};

struct SelcBits {
    const uint32_t* __restrict__ masks;       // the copy's mask m0
    unsigned long long mask_words;
    uint32_t n_m, n_ids;
    __device__ __forceinline__ bool load(const smc_dev_aln* __restrict__ aln, uint32_t i, uint32_t n_aln, uint32_t& v) const {
        v = 0u;
        if (i >= n_aln) return false;
        const uint32_t g = aln[i].pair_gid;
        if (g >= n_ids) return false;
        for (uint32_t j = 0; j < n_m; ++j) v |= ((masks[(size_t)j * mask_words + (g >> 5)] >> (g & 31u)) & 1u) << j;
        return v != 0u;
    }
    __device__ __forceinline__ bool keep(bool, uint32_t v, uint32_t j) const { return ((v >> j) & 1u) != 0u; }
};

__device__ __forceinline__ SelcBits selr_rule(const SelReadCopies& K, uint32_t c) {
    return SelcBits{K.masks + (size_t)c * K.copy_stride + (size_t)K.m0 * K.mask_words, K.mask_words, K.n_m, K.n_ids};
}

__global__ __launch_bounds__(SEL_BLOCK) void k_selr_count(const char* __restrict__ aln_base, unsigned long long aln_stride, uint32_t n_aln,
                                                          SelReadCopies K, uint32_t n_blk, uint32_t* __restrict__ blk_cnt_all) {
    const uint32_t c = blockIdx.y;
    selc_count_body((const smc_dev_aln*)(aln_base + (size_t)c * aln_stride), n_aln, selr_rule(K, c), c, K.m0, K.n_m, K.n_copies, n_blk, blk_cnt_all);
}

__global__ __launch_bounds__(SEL_BLOCK) void k_selr_scatter(const char* __restrict__ aln_base, unsigned long long aln_stride, uint32_t n_aln,
                                                            SelReadCopies K, uint32_t n_blk, const uint32_t* __restrict__ blk_off_all,
                                                            int32_t start0, uint32_t n_loci, smc_dev_aln* __restrict__ out_all,
                                                            uint32_t* __restrict__ orig_all, int32_t* __restrict__ diff_all,
                                                            int32_t* __restrict__ blk_maxend_all) {
    const uint32_t c = blockIdx.y;
    selc_scatter_body((const smc_dev_aln*)(aln_base + (size_t)c * aln_stride), n_aln, selr_rule(K, c), c, K.m0, K.n_m, K.n_copies, n_blk,
                      blk_off_all, start0, n_loci, out_all, orig_all, diff_all, blk_maxend_all);
}

// the renumbering's arrays of selection s = blockIdx.y
__device__ __forceinline__ SelIds selr_ids(const SelIds& I) {
    const size_t o = (size_t)blockIdx.y * ((size_t)I.n_bc + I.n_pair);
    return SelIds{I.first + o, I.map + o, I.n_bc, I.n_pair};
}

__global__ __launch_bounds__(SEL_BLOCK) void k_selr_first(const smc_dev_aln* __restrict__ out_all, uint32_t n_aln,
                                                          const uint32_t* __restrict__ summary, SelIds I) {
    const size_t s = blockIdx.y;
    sel_first_body(out_all + s * n_aln, summary + 4 * s, selr_ids(I));
}

__global__ __launch_bounds__(SEL_BLOCK) void k_selr_rcount(const smc_dev_aln* __restrict__ out_all, uint32_t n_aln,
                                                           const uint32_t* __restrict__ summary, SelIds I, uint32_t n_blk,
                                                           uint32_t* __restrict__ cnt_all) {
    const size_t s = blockIdx.y;
    sel_rcount_body(out_all + s * n_aln, summary + 4 * s, selr_ids(I), n_blk, cnt_all + s * 2u * (n_blk + 1u));
}

// a workgroup per (selection, barcodes / read names): the exclusive scan of its n_blk + 1 counts; the totals into rsum (not read)
__global__ __launch_bounds__(SEL_SCAN) void k_selr_offsets(uint32_t* __restrict__ cnt_all, uint32_t n_blk, uint32_t* __restrict__ rsum) {
    const size_t j = blockIdx.x;
    sel_offsets_body(cnt_all + j * (n_blk + 1u), n_blk, (int32_t*)nullptr, 0u, rsum + j);
}

__global__ __launch_bounds__(SEL_BLOCK) void k_selr_rank(const smc_dev_aln* __restrict__ out_all, uint32_t n_aln,
                                                         const uint32_t* __restrict__ summary, SelIds I, uint32_t n_blk,
                                                         const uint32_t* __restrict__ off_all) {
    const size_t s = blockIdx.y;
    sel_rank_body(out_all + s * n_aln, summary + 4 * s, selr_ids(I), n_blk, off_all + s * 2u * (n_blk + 1u));
}

__global__ __launch_bounds__(SEL_BLOCK) void k_selr_regid(smc_dev_aln* __restrict__ out_all, uint32_t n_aln,
                                                          const uint32_t* __restrict__ summary, SelIds I) {
    const size_t s = blockIdx.y;
    sel_regid_body(out_all + s * n_aln, summary + 4 * s, selr_ids(I));
}
