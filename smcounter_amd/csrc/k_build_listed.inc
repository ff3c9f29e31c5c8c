// Included by smcounter_hip.hip (after k_bp_emit2.inc: it calls bp2_resolve, bp_fixed_allele, bp_key_hash and bp_match as they are).
// ------------------------------------------------------------------------------------------
// smc_build_listed (--spikeScanBuild listed): the planes of G LISTED loci of B copies of a run, one call
// ------------------------------------------------------------------------------------------
// A scan pass lists one or two loci of a run and calls them in dozens of spiked copies; smc_build_planes builds every locus of every
// copy, a dozen launches and two downloads per copy.  This builder makes, for B copies and G listed loci (run offsets a_g,
// ascending), what the whole build writes for those loci - read words, umi_start / u_gid / u_finc, descriptors, extras entries,
// status bits: byte for byte - as a dense batch of B x G loci (copy-major: batch locus c * G + g), in five launches for all of them:
//   k_bl_check   (copy)                 is there an alignment flagged neither READ1 nor READ2?  Such a copy is DECLINED (status
//                                       BL_ST_UNFLAGGED, nothing else written for it: the look-back rule of smCounter.py:359-362 is
//                                       the whole builder's); clears the copy's status words
//   k_bl_sort    (listed locus, copy)   the locus's window loc[a_g].w0 .. w1 compacted to the alignments that cover it (file order),
//                                       sorted by (bc_gid, pair_gid, file index) - a stable LSD radix sort of (key, index) pairs by ONE
//                                       workgroup in global scratch, 8 bits a pass -, then per sorted entry "first of its barcode",
//                                       "first of its read pair" and the barcode's number.  With `shared` set - the copies of one run
//                                       that smc_spike_*_reps make: spiking changes bases, CIGARs and NM, no span and no id - the
//                                       order is made once from copy 0 and serves all B (a declined copy 0 declines them all)
//   k_bl_words   (read block, locus, copy)   LANE = (copy, read): the per-read semantics of k_bp_emit2's exact path (bp2_resolve, gap /
//                                       site / quality, bp_fixed_allele, kind, the end distances, incCond, smc_read_class, the word in
//                                       16 or 32 bits) on the copy's own record; the barcode heads' umi_start / u_gid entries
//   k_bl_finish  (locus, copy)          closing umi_start entry, u_finc of a locus over the barcode cap (a walk over each barcode's run
//                                       of words: no atomic), the alleles beyond the six fixed ones numbered by first appearance in
//                                       pileup order and patched into their reads' words, the descriptor, the locus's extras entries
//   k_bl_gather  (copy)                 the loci's extras entries into the copy's list in locus order, its counters
// No atomic touches an output: ranks come from prefix counts, the extras list is gathered in a fixed order, and two calls leave
// the same bytes.  (The status words and the allele table of k_bl_finish are scratch / LDS.)
// The unit of the design is the locus's workgroup: a locus of any depth below 2^24 is sorted by the 16 wavefronts of one
// workgroup, each taking a sixteenth of the list per pass (one wavefront step is 64 entries, one compaction round 1024).
#define BL_MAX_LOCI 64          // listed loci per call (their offsets and capacities travel in the kernels' argument block)
#define BL_MAX_COPIES 1024
#define BL_SORT_WAVES 16
#define BL_XMAX 58              // distinct extra alleles of a locus (ids 6 .. 63)
#define BL_XTAB 128             // slots of k_bl_finish's allele table
#define BL_ST_UNFLAGGED 64u     // status: the copy has an alignment flagged neither READ1 nor READ2 - declined, nothing written

struct BlArgs {
    const smc_listed_copy* copies;
    const uint8_t* refseq;
    int32_t n_copies, n_listed, shared, dense, start0;  // dense: an extras entry's locus field holds g, not the run offset
    int32_t min_bq, min_mq, primer_dist, ds;
    uint32_t fp, w16, slot_base, umi_base;
    uint32_t stride;                                      // slots of one copy: the sum of its loci's capacities
    uint32_t off[BL_MAX_LOCI];                            // run offset a_g of listed locus g
    uint32_t capoff[BL_MAX_LOCI + 1];                     // first slot of listed locus g within a copy (capacities: multiples of 4)
    void* words; uint32_t *umi_start, *u_gid, *u_finc; smc_locus* loci; uint32_t *xlist, xcap, *counters;
    // scratch
    unsigned long long* key[2]; uint32_t* val[2];         // the sort's ping and pong, [order copy][stride]
    uint32_t *order, *hinfo;                              // sorted alignment indices; bit 31 barcode head, bit 30 pair head, bits 0-23 barcode number
    uint32_t *meta;                                       // [order copy][G][4]: covering reads, barcodes, read pairs, 1 = more reads than the capacity
    uint32_t *cstat, *st, *nx, *xtmp;                     // [copy]; [copy][G] status, extras entries; [copy][G][BL_XMAX][5]
};

__global__ __launch_bounds__(256) void k_bl_check(BlArgs A) {
    __shared__ uint32_t any;
    const uint32_t c = blockIdx.x, G = (uint32_t)A.n_listed;
    const smc_listed_copy D = A.copies[c];
    if (threadIdx.x == 0) any = 0u;
    __syncthreads();
    bool unfl = false;
    for (uint32_t a = threadIdx.x; a < (uint32_t)max(D.n_aln, 0); a += 256u) unfl |= !(D.aln[a].oflag & (SMC_DA_R1 | SMC_DA_R2));
    if (unfl) any = 1u;
    __syncthreads();
    if (threadIdx.x == 0) A.cstat[c] = any ? BL_ST_UNFLAGGED : 0u;
    for (uint32_t g = threadIdx.x; g < G; g += 256u) { A.st[c * G + g] = 0u; A.nx[c * G + g] = 0u; }
}

__device__ __forceinline__ int bl_bits(int32_t n) {
    int b = 1;
    while (b < 32 && (1ll << b) < (long long)max(1, n)) ++b;
    return b;
}

__global__ __launch_bounds__(64 * BL_SORT_WAVES) void k_bl_sort(BlArgs A) {
    __shared__ uint32_t hist[256 * BL_SORT_WAVES];        // [digit][wavefront]: counts, then each wavefront's next destination
    __shared__ uint32_t wsum[BL_SORT_WAVES], wsum2[BL_SORT_WAVES];
    constexpr uint32_t NT = 64u * BL_SORT_WAVES;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wid = tid >> 6;
    const uint32_t g = blockIdx.x, c = blockIdx.y, G = (uint32_t)A.n_listed;
    if (A.cstat[c]) return;                               // (declined: with `shared` c is copy 0, whose order would have served all)
    const smc_listed_copy D = A.copies[c];
    const uint32_t cap = A.capoff[g + 1] - A.capoff[g];
    const size_t base = (size_t)c * A.stride + A.capoff[g];
    const smc_dev_locus LC = D.loc[A.off[g]];
    const int p = A.start0 + (int)A.off[g];
    const uint32_t w0 = LC.w0, w1 = min(LC.w1, (uint32_t)max(D.n_aln, 0));
    const int pb = bl_bits(D.n_pair), bb = bl_bits(D.n_bc);
    // ---- the covering alignments of the window, in file order
    uint32_t run = 0;
    {
        unsigned long long* const k0 = A.key[0] + base;
        uint32_t* const v0 = A.val[0] + base;
        for (uint32_t b0 = w0; b0 < w1; b0 += NT) {
            const uint32_t a = b0 + tid;
            bool cov = false;
            unsigned long long key = 0;
            if (a < w1) {
                const uint32_t* rec = (const uint32_t*)(D.aln + a);
                cov = (int)rec[0] <= p && p < (int)rec[1];
                key = ((unsigned long long)rec[7] << pb) | (unsigned long long)rec[8];
            }
            const unsigned long long m = __builtin_amdgcn_ballot_w64(cov);
            if (lane == 0) wsum[wid] = (uint32_t)__popcll(m);
            __syncthreads();
            uint32_t pre = run, tot = 0;
            for (uint32_t w = 0; w < BL_SORT_WAVES; ++w) { const uint32_t x = wsum[w]; if (w < wid) pre += x; tot += x; }
            const uint32_t dst = pre + bp_lanes_below(m);
            if (cov && dst < cap) { k0[dst] = key; v0[dst] = a; }
            run += tot;
            __syncthreads();
        }
    }
    const uint32_t n = min(run, cap);
    // ---- the sort: every wavefront owns a sixteenth of the list; per pass its digit counts, a prefix over (digit, wavefront), and
    // its entries placed 64 at a time (bp_match: a lane's rank among the lanes of its digit)
    const int passes = (pb + bb + 7) / 8;
    int cur = 0;
    const uint32_t e0 = (uint32_t)((unsigned long long)n * wid / BL_SORT_WAVES), e1 = (uint32_t)((unsigned long long)n * (wid + 1u) / BL_SORT_WAVES);
    for (int ps = 0; ps < passes; ++ps) {
        const int shift = 8 * ps;
        const unsigned long long* const kin = A.key[cur] + base;
        const uint32_t* const vin = A.val[cur] + base;
        unsigned long long* const kout = A.key[cur ^ 1] + base;
        uint32_t* const vout = A.val[cur ^ 1] + base;
        for (uint32_t i = tid; i < 256u * BL_SORT_WAVES; i += NT) hist[i] = 0u;
        __syncthreads();
        for (uint32_t e = e0 + lane; e < e1; e += 64u) atomicAdd(&hist[((uint32_t)(kin[e] >> shift) & 255u) * BL_SORT_WAVES + wid], 1u);
        __syncthreads();
        {
            constexpr uint32_t PER = 256u * BL_SORT_WAVES / NT;                  // 4
            uint32_t v[PER], t = 0;
#pragma unroll
            for (uint32_t k = 0; k < PER; ++k) { v[k] = hist[PER * tid + k]; t += v[k]; }
            uint32_t inc = t;
            for (int o = 1; o < 64; o <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)inc, o); if ((int)lane >= o) inc += u; }
            if (lane == 63u) wsum[wid] = inc;
            __syncthreads();
            uint32_t r = inc - t;
            for (uint32_t w = 0; w < wid; ++w) r += wsum[w];
#pragma unroll
            for (uint32_t k = 0; k < PER; ++k) { hist[PER * tid + k] = r; r += v[k]; }
            __syncthreads();
        }
        for (uint32_t e = e0; e < e1; e += 64u) {
            const uint32_t i = e + lane;
            const bool valid = i < e1;
            const unsigned long long key = valid ? kin[i] : 0ull;
            const uint32_t v = valid ? vin[i] : 0u;
            const uint32_t dg = valid ? (uint32_t)(key >> shift) & 255u : 0u;
            uint32_t rank, np;
            bp_match(dg, valid, 8, rank, np);
            uint32_t b = 0;
            if (valid) b = hist[dg * BL_SORT_WAVES + wid];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
            if (valid) {
                kout[b + rank] = key; vout[b + rank] = v;
                if (rank == np - 1u) hist[dg * BL_SORT_WAVES + wid] = b + np;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
            __builtin_amdgcn_wave_barrier();
        }
        __syncthreads();
        cur ^= 1;
    }
    // ---- heads: an entry starts a barcode / a read pair where the one before it has another id; the barcode's number
    const unsigned long long* const ks = A.key[cur] + base;
    const uint32_t* const vs = A.val[cur] + base;
    uint32_t* const ord = A.order + base;
    uint32_t* const hinf = A.hinfo + base;
    const unsigned long long pmask = (1ull << pb) - 1ull;
    uint32_t nU = 0, nF = 0;
    for (uint32_t b0 = 0; b0 < n; b0 += NT) {
        const uint32_t i = b0 + tid;
        const bool valid = i < n;
        const unsigned long long k = valid ? ks[i] : 0ull, kp = (valid && i > 0u) ? ks[i - 1u] : 0ull;
        const bool head = valid && (i == 0u || (k >> pb) != (kp >> pb)), nf = valid && (i == 0u || (k & pmask) != (kp & pmask));
        const unsigned long long mh = __builtin_amdgcn_ballot_w64(head), mf = __builtin_amdgcn_ballot_w64(nf);
        if (lane == 0) { wsum[wid] = (uint32_t)__popcll(mh); wsum2[wid] = (uint32_t)__popcll(mf); }
        __syncthreads();
        uint32_t pre = nU, toth = 0, totf = 0;
        for (uint32_t w = 0; w < BL_SORT_WAVES; ++w) { const uint32_t x = wsum[w]; if (w < wid) pre += x; toth += x; totf += wsum2[w]; }
        if (valid) {
            const uint32_t u = pre + bp_lanes_below(mh) + (head ? 1u : 0u) - 1u;
            ord[i] = vs[i];
            hinf[i] = (u & 0x00FFFFFFu) | (head ? 0x80000000u : 0u) | (nf ? 0x40000000u : 0u);
        }
        nU += toth; nF += totf;
        __syncthreads();
    }
    if (tid == 0) {
        uint32_t* M = A.meta + 4u * (c * G + g);
        M[0] = n; M[1] = nU; M[2] = nF; M[3] = run > cap ? 1u : 0u;
    }
}

// what the pileup engine and the reference's per-read rules give for alignment `a` of the copy at position p: k_bp_emit2's exact
// path for a flagged alignment, called from here lane by lane
struct BlRead { uint32_t mword, cls; bool inc, isx; int qpos, indel; uint32_t st; };
__device__ __forceinline__ BlRead bl_read(const BlArgs& A, const smc_listed_copy& D, uint32_t a, int p) {
    BlRead o;
    const uint32_t* rec = (const uint32_t*)(D.aln + a);
    const int pos = (int)rec[0];
    const uint32_t kcig = rec[2], kseq = rec[3], k4 = rec[4], k5 = rec[5];
    const int n_cig = (int)(k4 & 0xFFFFu), l_seq = (int)(rec[6] & 0xFFFFu), left_sp = (int)(k5 & 0xFFFFu), qalen = (int)(k5 >> 16);
    const uint32_t oflag = (k4 >> 16) & 0xFFu, mapq = k4 >> 24;
    const bool r2 = (oflag & SMC_DA_R2) != 0, rev = (oflag & SMC_DA_REV) != 0;
    const bool mq = (int)mapq >= A.min_mq && (oflag & SMC_DA_MMOK) != 0;
    o.st = 0u;
    const BpRes r = bp2_resolve(D.cig + kcig, n_cig, pos, p, l_seq);
    const bool gap = (r.isdel && r.indel == 0) || r.qpos < 0;
    uint32_t site = 0, bq = 0;
    if (!gap) { const uint32_t sq = *(const uint16_t*)(D.bq + 2ull * (kseq + (uint32_t)r.qpos)); site = sq & 0xFFu; bq = sq >> 8; }
    if (bq > 126u) o.st |= BP_ST_BQ;
    bq = min(bq, 126u);
    const int f = bp_fixed_allele(site);
    const uint32_t fa = gap ? 5u : (r.indel == 0 && f >= 0 ? (uint32_t)f : 0xFFu);
    const uint32_t kind = r.indel > 0 ? 2u : r.indel < 0 ? 3u : r.isdel ? 1u : 0u;
    uint32_t dist = 0;
    if (kind == 0u) {                                          // end distances, regular bases only (smCounter.py:432-452)
        const int rd = r.qpos - left_sp, far = qalen - rd;
        const int dbc = (r2 != rev) ? far : rd, dpr = r2 ? (rev ? far : rd) : 0;
        dist = (uint32_t)min(max(dbc, 0), 65535) | (uint32_t)min(max(dpr, 0), 65535) << 16;
    }
    const bool bq_ok = (int)bq >= A.min_bq;
    o.inc = (bq_ok || kind == 1u) && mq;                       // incCond, :378
    o.cls = smc_read_class((int)kind, rev, r2, o.inc, bq_ok, (dist & 0xFFFFu) <= 20u, (int)(dist >> 16) <= A.primer_dist);
    o.isx = fa == 0xFFu;
    o.qpos = r.qpos; o.indel = r.indel;
    o.mword = (o.isx ? 6u : fa) | (kind == 1u ? (uint32_t)A.min_bq : bq) << 8;   // in-deletion: minBQ, :418
    if (A.w16 && bq > 63u && kind != 1u) o.st |= BP_ST_NARROW;
    return o;
}

__global__ __launch_bounds__(256) void k_bl_words(BlArgs A) {
    const uint32_t g = blockIdx.y, c = blockIdx.z, G = (uint32_t)A.n_listed, cs = A.shared ? 0u : c;
    if (A.cstat[c] | A.cstat[cs]) return;                 // (no order where the copy it comes from is declined)
    const uint32_t* M = A.meta + 4u * (cs * G + g);
    const uint32_t n = M[0], nU = M[1];
    const uint32_t cap = A.capoff[g + 1] - A.capoff[g];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= cap) return;
    const uint32_t so = A.slot_base + c * A.stride + A.capoff[g], uo = A.umi_base + c * (A.stride + G) + A.capoff[g] + g;
    if (i >= n) {                                              // the padding slots up to the next 4-read boundary
        if (i < ((n + 3u) & ~3u)) { if (A.w16) ((uint16_t*)A.words)[so + i] = 0; else ((uint32_t*)A.words)[so + i] = 0u; }
        return;
    }
    const smc_listed_copy D = A.copies[c];
    const size_t sb = (size_t)cs * A.stride + A.capoff[g];
    const uint32_t a = A.order[sb + i], hf = A.hinfo[sb + i];
    const int p = A.start0 + (int)A.off[g];
    const uint32_t* rec = (const uint32_t*)(D.aln + a);
    // (an order made from copy 0 names an alignment this copy has, and one that covers the locus: spiking moves no span)
    if (a >= (uint32_t)max(D.n_aln, 0) || !((int)rec[0] <= p && p < (int)rec[1])) { atomicOr(&A.st[c * G + g], BP_ST_DEPTH); return; }
    const BlRead R = bl_read(A, D, a, p);
    if (R.st) atomicOr(&A.st[c * G + g], R.st);
    const bool nf = (hf & 0x40000000u) != 0;
    const uint32_t w = R.mword | (nf ? SMC_RW_NF : 0u) | R.cls << SMC_RW_CLASS_SHIFT;
    if (A.w16) ((uint16_t*)A.words)[so + i] = (uint16_t)smc_read_word16(w);
    else ((uint32_t*)A.words)[so + i] = w | (R.inc ? SMC_RW_INC : 0u) | SMC_RW_OK;
    if (hf & 0x80000000u) {
        const uint32_t u = hf & 0x00FFFFFFu;
        A.umi_start[uo + u] = i;
        if (A.ds > 0 && (int)nU > A.ds) A.u_gid[uo + u] = rec[7];
    }
}

__global__ __launch_bounds__(256) void k_bl_finish(BlArgs A) {
    __shared__ unsigned long long tkey[BL_XTAB], tfirst[BL_XTAB], smask;
    __shared__ uint32_t tidv[BL_XTAB], nk, refid, s_st;
    const uint32_t tid = threadIdx.x;
    const uint32_t g = blockIdx.x, c = blockIdx.y, G = (uint32_t)A.n_listed, cs = A.shared ? 0u : c;
    if (A.cstat[c] | A.cstat[cs]) return;                 // (no order where the copy it comes from is declined)
    const uint32_t* M = A.meta + 4u * (cs * G + g);
    const uint32_t n = M[0], nU = M[1], nF = M[2];
    const smc_listed_copy D = A.copies[c];
    const uint32_t l = A.off[g];
    const smc_dev_locus LC = D.loc[l];
    const int p = A.start0 + (int)l;
    const uint32_t so = A.slot_base + c * A.stride + A.capoff[g], uo = A.umi_base + c * (A.stride + G) + A.capoff[g] + g;
    const uint32_t* const ord = A.order + (size_t)cs * A.stride + A.capoff[g];
    const uint32_t n_aln = (uint32_t)max(D.n_aln, 0);
    for (uint32_t s = tid; s < BL_XTAB; s += 256u) { tkey[s] = 0ull; tfirst[s] = ~0ull; tidv[s] = 0u; }
    if (tid == 0) { nk = 0u; refid = 0u; s_st = 0u; smask = 0ull; }
    __syncthreads();
    if (tid == 0) {
        if (M[3] || n != LC.n || n >= (1u << 24)) s_st = BP_ST_DEPTH;
        A.umi_start[uo + nU] = n;
    }
    auto allele_of = [&](uint32_t i) -> uint32_t { return A.w16 ? (uint32_t)((const uint16_t*)A.words)[so + i] & 15u : ((const uint32_t*)A.words)[so + i] & 0xFFu; };
    // ---- a locus over the barcode cap: per barcode its first INCLUDED pileup read (the lowest alignment index among its included reads)
    if (A.ds > 0 && (int)nU > A.ds)
        for (uint32_t u = tid; u < nU; u += 256u) {
            const uint32_t s = A.umi_start[uo + u], e = u + 1u < nU ? A.umi_start[uo + u + 1u] : n;
            uint32_t first = 0xFFFFFFFFu;
            for (uint32_t i = s; i < e && i < n; ++i) {
                const bool inc = A.w16 ? (((const uint16_t*)A.words)[so + i] & 32u) != 0 : (((const uint32_t*)A.words)[so + i] & SMC_RW_INC) != 0;
                if (inc) first = min(first, ord[i]);
            }
            A.u_finc[uo + u] = first;
        }
    // ---- the alleles beyond the six fixed ones: the walk left the code 6 in their reads' words.  Distinct keys (bp_key_hash) into an
    // LDS table, each with its first appearance - the lowest alignment index: the order in which the reference's dict meets them
    auto key_of = [&](uint32_t a, int& qpos, int& indel) -> unsigned long long {
        const uint32_t* rec = (const uint32_t*)(D.aln + a);
        const BpRes r = bp2_resolve(D.cig + rec[2], (int)(rec[4] & 0xFFFFu), (int)rec[0], p, (int)(rec[6] & 0xFFFFu));
        qpos = r.qpos; indel = r.indel;
        return bp_key_hash(D.aln[a], D.bq, r.qpos, r.indel) | 0x8000000000000000ull;
    };
    auto slot_of = [&](unsigned long long key, bool insert) -> int {
        uint32_t s = (uint32_t)((key >> 17) ^ (key >> 41)) & (BL_XTAB - 1u);
        for (int t = 0; t < BL_XTAB; ++t) {
            const unsigned long long prev = insert ? atomicCAS(&tkey[s], 0ull, key) : tkey[s];
            if (prev == key || (insert && prev == 0ull)) return (int)s;
            if (!insert && prev == 0ull) return -1;
            s = (s + 1u) & (BL_XTAB - 1u);
        }
        return -1;
    };
    for (uint32_t i = tid; i < n; i += 256u) {
        if (allele_of(i) != 6u) continue;
        const uint32_t a = ord[i];
        if (a >= n_aln) continue;
        int qpos, indel;
        const unsigned long long key = key_of(a, qpos, indel);
        const int s = slot_of(key, true);
        if (s < 0) { atomicOr(&s_st, BP_ST_ALLELES); continue; }
        atomicMin(&tfirst[s], ((unsigned long long)a << 32) | i);
    }
    __syncthreads();
    // ---- ids by first appearance; one report per distinct allele, in the order of the ids
    if (tid < BL_XTAB && tkey[tid] != 0ull) {
        const unsigned long long f = tfirst[tid];
        uint32_t rank = 0;
        for (uint32_t s = 0; s < BL_XTAB; ++s) rank += (tkey[s] != 0ull && tfirst[s] < f) ? 1u : 0u;
        atomicAdd(&nk, 1u);
        uint32_t id = 6u + rank;
        if (rank >= (uint32_t)BL_XMAX) { atomicOr(&s_st, BP_ST_ALLELES); id = 63u; }
        tidv[tid] = id;
        if (rank < (uint32_t)BL_XMAX) {
            const uint32_t ai = (uint32_t)(f >> 32);
            int qpos, indel;
            (void)key_of(ai, qpos, indel);
            if (indel == 0) {                                                   // an unusual letter: TYPE 'SNP', and maybe the reference's own
                atomicOr(&smask, 1ull << id);
                if ((uint32_t)D.bq[2ull * (D.aln[ai].seq_off + (uint32_t)qpos)] == (uint32_t)A.refseq[l]) refid = id;
            }
            uint32_t* o = A.xtmp + 5u * ((size_t)(c * G + g) * BL_XMAX + rank);
            o[0] = A.dense ? g : l; o[1] = id; o[2] = ai; o[3] = (uint32_t)qpos; o[4] = (uint32_t)indel;
        }
    }
    __syncthreads();
    // ---- the reads' allele ids: the low byte of a 32-bit word, the low nibble of a 16-bit one
    if (nk)
        for (uint32_t i = tid; i < n; i += 256u) {
            if (allele_of(i) != 6u) continue;
            const uint32_t a = ord[i];
            if (a >= n_aln) continue;
            int qpos, indel;
            const int s = slot_of(key_of(a, qpos, indel), false);
            if (s < 0) continue;
            const uint32_t id = tidv[s];
            if (A.w16) {
                uint16_t* hw = (uint16_t*)A.words + so + i;
                if (id > 15u) atomicOr(&s_st, BP_ST_NARROW); else *hw = (uint16_t)((*hw & 0xFFF0u) | id);
            } else {
                uint32_t* ww = (uint32_t*)A.words + so + i;
                *ww = (*ww & 0xFFFFFF00u) | id;
            }
        }
    __syncthreads();
    if (tid == 0) {
        smc_locus L;
        L.read_off4 = so >> 2; L.umi_off = uo;
        L.n_reads = (int32_t)n; L.n_umi = (int32_t)nU; L.n_frag = (int32_t)nF;
        int ra = bp_fixed_allele(A.refseq[l]);
        if (ra < 0) ra = refid ? (int)refid : 255;
        L.ref_allele = (uint8_t)ra; L.n_alleles = (uint8_t)min(6u + nk, 64u);
        L.flags = (uint16_t)A.fp; L.snp_mask = 0x1full | smask;
        A.loci[c * G + g] = L;
        A.nx[c * G + g] = min(nk, (uint32_t)BL_XMAX);
        if (s_st) A.st[c * G + g] |= s_st;
    }
}

__global__ __launch_bounds__(64) void k_bl_gather(BlArgs A) {
    const uint32_t c = blockIdx.x, G = (uint32_t)A.n_listed, lane = threadIdx.x;
    uint32_t status = A.cstat[c] | A.cstat[A.shared ? 0u : c], total = 0;
    if (!status)
        for (uint32_t g = 0; g < G; ++g) {
            status |= A.st[c * G + g];
            const uint32_t nxg = min(A.nx[c * G + g], (uint32_t)BL_XMAX);
            const uint32_t* src = A.xtmp + 5u * (size_t)(c * G + g) * BL_XMAX;
            for (uint32_t j = lane; j < 5u * nxg; j += 64u) {
                const uint32_t slot = total + j / 5u;
                if (slot < A.xcap) A.xlist[5u * ((size_t)c * A.xcap + slot) + j % 5u] = src[j];
            }
            total += nxg;
        }
    if (total > A.xcap) status |= BP_ST_XLIST;
    if (lane == 0) { A.counters[2u * c] = total; A.counters[2u * c + 1u] = status; }
}
