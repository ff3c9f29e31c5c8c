// Included by smcounter_hip.hip (after k_spike_cells.inc: SPC_COUNTERS, spd_hits, the spike draw's domain and, for k_spg_counts at the
// end of this file, what k_spike_cells itself takes from k_af_depth.inc and k_select_aln.inc: afd_keep_depth, sel_draw; after k_read_groups.inc:
// rg_draw, the read draw k_rg_masks makes; after k_allele_carriers.inc: af_shows; after k_spike_indel.inc: spi_walk, spi_first).
// ------------------------------------------------------------------------------------------
// --spikeRpb: what every cell (spike target t, reads-per-barcode target r) of R replicate spike-ins achieves per listed SNV, counted
// PER READ (smc_spike_read_bits, smc_spike_rpb_counts)
// ------------------------------------------------------------------------------------------
// A cell is the --spikeAF spike-in at t, then the --dsRpb philox thinning at r, both drawn with the key s_j, each a stream of its own:
//   the spike rule at t   hit  = u(b) = k_spike_rewrite's draw (domain "spAF", counter word 3 the variant's 1-based position) < thr[t],
//                         one draw per barcode;
//   the read rule at r    kept = the record's name is the first of its barcode, file-wide, or rg_draw(name) - k_rg_masks' draw,
//                         domain "dsRP" - < rthr[r] = floor(probKeep_r * 2^32): one draw per read name.
// k_spike_cells decides whole barcodes from three counters the run fixes.  Thinning reads moves those counters per r and per seed: it
// can flip a barcode's majority and can take a barcode out of the locus altogether.  So the counters are made here, per replicate,
// from one FLAG BYTE per covering record:
//   k_spr_bits    (smc_spike_read_bits) a lane per alignment, a row of workgroups per listed SNV: bit 0 the record covers the
//                 position, bit 1 it shows ALT as it is (af_shows), bit 2 its allele key there is a single letter - the records
//                 k_spike_rewrite touches.  A plain byte store per alignment, 0 outside the locus's window: no atomics.
//   k_spr_counts  (smc_spike_rpb_counts, smc_spike_indel_rpb_counts, smc_spike_phase_rpb_counts) ONE body, <MAXR, FOUR, SETS>: a lane
//                 per barcode of a row (blockIdx.y = row, blockIdx.z strides over the replicates), one spike draw per (barcode, row,
//                 replicate).  The lane walks a CSR segment of records (name identity and flag byte, bit 0 = first name, bits 1 / 2 =
//                 alt / single from k_spr_bits): ONE philox per record and replicate, its compares against the Rr read thresholds one
//                 bit set; per r the lane keeps (reads_r, alt_r, single_r) over the kept records.  Then per barcode and r:
//                 N' = reads_r > 0,  car0 = 2 alt_r > reads_r,  car1 = 2 single_r > reads_r,  and per cell (t, r)
//                   V0' = N' && car0    S' = N' && hit    READS' = single_r over N' && hit    V1' = N' && (hit ? car1 : car0)
//                 reduced as k_spike_cells reduces: ballots + popcounts and a DPP sum for READS', the workgroup's wavefronts added in
//                 LDS, one integer atomic add per workgroup, replicate, cell and counter that is not 0 - two calls give the same words.
// The per-r counters are indexed by unrolled loops only (they stay in registers: 3 x MAXR of them, so the kernel is compiled for MAXR =
// 8 - what a run asks for - and for MAXR = 32, the most the cells' limit admits; n_rr <= MAXR).  Once per run / once per file: not on
// the per-locus hot path.
// --spikeIndelRpb (smc_spike_indel_read_bits, smc_spike_indel_rpb_counts): for an insertion or a deletion `single` is two numbers, as
// in k_spike_cells - alt1, the records that show the key when the barcode is hit, and touch, the records the rewrite changes then.
//   k_spr_indel_bits  k_spr_bits over smc_spike_indel_variant records: bits 0 / 1 as there (af_shows with the INS / DEL key), bit 2 =
//                 alt1, bit 3 = touch.  An SNV's bits 2 and 3 are both k_spr_bits' bit 2 (spr_snv_bits, shared); an indel's touch is
//                 spi_walk<false, SPI_TOUCH_ONE> - the rewrite's own eligibility lines, the 16-bit limits included -, its alt1 a
//                 touched record whose anchor letter is REF's first, or an untouched one that shows the key already.
//   FOUR          a fourth per-r counter: car1 from alt1_r (flag bit 2), READS' from touch_r (flag bit 3).  Without it touch IS alt1
//                 and no fourth array exists.
// --spikePhaseRpb (smc_spike_phase_rpb_counts): the JOINT numbers of phase sets under read thinning.  A set's barcode counts when it
// keeps a read at EVERY member and carries it when it does so at EVERY member; thinning can take it out of one member's pileup, or flip
// its majority at one member only, so the joint numbers cannot be had from the members' own cells: they are made per record as well.
//   SETS          a row is a phase set, a lane one of its JOINT barcodes, the spike draw made with the leader's position.  The lane
//                 walks its M_g members one after the other (segment seg_base[g] + (e - off[g]) * M_g + m), folds each member's
//                 3 x MAXR counters into three bit sets over r - there, car0, car1 - and ANDs them into the running all-members
//                 sets: registers do not grow with M_g.  Four counters per cell, (N_ALL', V0_ALL', S_ALL', V1_ALL'): a set has no
//                 READS', so flag bit 3 is not read and there is no <MAXR, true, true>.  A record that spans several members is a
//                 record of each of their segments, and its read draw is made once per member.  Without SETS a row is a listed
//                 variant - a set of one member whose segments are its covering barcodes - and its bit sets are never formed.
// --spikeScanMnvRpb (smc_scan_phase_rpb_counts): the same joint numbers for a SCAN, where every locus of the panel is a set and a
// per-variant record CSR made on the host would be loci x members x depth records sorted and gathered pass after pass.
//   k_spr_run_counts  the SETS body of k_spr_counts (spr_counts, one body for both kernels) over a second record source, SprRun: the
//                 run in barcode-major order, made once per decoded run, and k_spr_bits' bytes left in HBM.  A lane walks ALL records
//                 of its joint barcode once per member and keeps those whose byte at the member has bit 0; names and first flags
//                 come pre-gathered in walk order, so the walk streams and its one scattered load is the byte.
#define SPB_BLOCK 256
#define SPB_COVERS 1u
#define SPB_ALT 2u
#define SPB_SINGLE 4u
#define SPB_ALT1 4u                          // (k_spr_indel_bits: the same bit as SPB_SINGLE - an SNV's alt1 is its single-letter bit)
#define SPB_TOUCH 8u
#define SPB_FIRST 1u                         // (a record's flag byte for k_spr_counts) first name of its barcode, file-wide

// bits 1 and 2 of a record that covers the SNV V at p: shows ALT as it is, the allele key a single letter
// (a record that points beyond a pool covers, and shows nothing: k_spike_rewrite leaves it alone as well)
__device__ __forceinline__ uint32_t spr_snv_bits(const smc_af_variant& V, const smc_dev_aln& a, const uint32_t* __restrict__ cig,
                                                 unsigned long long n_cig_words, const uint8_t* __restrict__ bq, unsigned long long n_pairs, int p) {
    if ((unsigned long long)a.cig_off + a.n_cig > n_cig_words) return 0u;
    const BpRes r = bp2_resolve(cig + a.cig_off, (int)a.n_cig, a.pos, p, (int)a.l_seq);
    if (r.isdel || r.indel != 0 || r.qpos < 0 || r.qpos >= (int)a.l_seq || (unsigned long long)a.seq_off + (unsigned long long)r.qpos >= n_pairs)
        return 0u;
    return SPB_SINGLE | (af_shows(V, a, cig, bq, nullptr, p) ? SPB_ALT : 0u);
}

// out[v * n_aln + i]: the three bits of alignment i at variant v (an SNV: var[v].letter its ALT); every byte of the row is written.
// Against k_af_count on MALFORMED records: a record is counted here whatever its bc_gid (the host groups the bytes by barcode, and
// takes the covering barcodes from smc_allele_carriers' bits), and one whose CIGAR or bases lie beyond the pools covers but shows
// nothing, as k_spike_rewrite treats it - k_af_count skips the first and reads the second.  The two then disagree, and the host,
// which compares the bytes' sums per barcode with the pre-pass's counters for every run, ends the run: no wrong number is printed.
__global__ __launch_bounds__(SPB_BLOCK) void k_spr_bits(const smc_dev_aln* __restrict__ aln, uint32_t n_aln, const uint32_t* __restrict__ cig,
                                                        unsigned long long n_cig_words, const uint8_t* __restrict__ bq,
                                                        unsigned long long n_pairs, const smc_dev_locus* __restrict__ loc, int32_t start0,
                                                        const smc_af_variant* __restrict__ var, uint8_t* __restrict__ out) {
    const smc_af_variant V = var[blockIdx.y];
    const smc_dev_locus L = loc[V.locus];
    const uint32_t w1 = min(L.w1, n_aln);
    const int p = start0 + (int)V.locus;
    uint8_t* const o = out + (size_t)n_aln * blockIdx.y;
    for (uint32_t i = blockIdx.x * SPB_BLOCK + threadIdx.x; i < n_aln; i += gridDim.x * SPB_BLOCK) {
        uint32_t b = 0u;
        if (i >= L.w0 && i < w1) {
            const smc_dev_aln a = aln[i];
            if (a.pos <= p && p < a.end) b = SPB_COVERS | spr_snv_bits(V, a, cig, n_cig_words, bq, n_pairs, p);
        }
        o[i] = (uint8_t)b;
    }
}

// out[v * n_aln + i]: the four bits of alignment i at variant v of `var` (SNVs, insertions, deletions, ascending by position: what
// smc_spike_indel_touch takes); every byte of the row is written, 0 outside the window of v's locus (var[v].pos0 - start0; the host
// checked that it is one of the run's).  Malformed records as in k_spr_bits: whatever its bc_gid a record counts, and one whose CIGAR
// words or whose l_seq pairs lie beyond the pools covers and shows nothing (spi_in_run's bounds: k_spi_count leaves it where it is).
__global__ __launch_bounds__(SPB_BLOCK) void k_spr_indel_bits(const smc_dev_aln* __restrict__ aln, uint32_t n_aln, const uint32_t* __restrict__ cig,
                                                              unsigned long long n_cig_words, const uint8_t* __restrict__ bq,
                                                              unsigned long long n_pairs, const smc_dev_locus* __restrict__ loc, int32_t start0,
                                                              const smc_spike_indel_variant* __restrict__ var, int n_var,
                                                              const uint8_t* __restrict__ ins, uint8_t* __restrict__ out) {
    const smc_spike_indel_variant S = var[blockIdx.y];
    const int p = S.pos0;
    smc_af_variant V;                                            // (af_shows' record: the key's letter is the ALT of an SNV, the anchor's else)
    V.locus = (uint32_t)(p - start0); V.kind = S.kind; V.letter = S.kind == SMC_AF_SNV ? S.alt : S.ref; V.len = S.len; V.ins_off = S.ins_off;
    const smc_dev_locus L = loc[V.locus];
    const uint32_t w1 = min(L.w1, n_aln);
    uint8_t* const o = out + (size_t)n_aln * blockIdx.y;
    for (uint32_t i = blockIdx.x * SPB_BLOCK + threadIdx.x; i < n_aln; i += gridDim.x * SPB_BLOCK) {
        uint32_t b = 0u;
        if (i >= L.w0 && i < w1) {
            const smc_dev_aln a = aln[i];
            if (a.pos <= p && p < a.end) {
                b = SPB_COVERS;
                if (S.kind == SMC_AF_SNV) {
                    b |= spr_snv_bits(V, a, cig, n_cig_words, bq, n_pairs, p);
                    if (b & SPB_SINGLE) b |= SPB_TOUCH;              // (an SNV: the rewrite changes the single-letter records, which then show ALT)
                } else if ((unsigned long long)a.cig_off + a.n_cig <= n_cig_words && (unsigned long long)a.seq_off + a.l_seq <= n_pairs) {
                    const bool shows = af_shows(V, a, cig, bq, ins, p);
                    SpiRes R;
                    R.want = (int)blockIdx.y;
                    spi_walk<false, SPI_TOUCH_ONE>(a, cig + a.cig_off, nullptr, var, spi_first(var, n_var, a.pos), n_var, nullptr, 0ull, 0ull, 0ull, 0,
                                                   nullptr, nullptr, nullptr, 0, R);
                    bool alt1 = shows;
                    if (R.took) {
                        // (eligible: the anchor is a base of an M / = / X operation inside l_seq - bp2_resolve's qpos is its query position)
                        const BpRes r = bp2_resolve(cig + a.cig_off, (int)a.n_cig, a.pos, p, (int)a.l_seq);
                        alt1 = r.qpos >= 0 && r.qpos < (int)a.l_seq && bq[2ull * ((unsigned long long)a.seq_off + (unsigned long long)r.qpos)] == S.ref;
                    }
                    b |= (shows ? SPB_ALT : 0u) | (alt1 ? SPB_ALT1 : 0u) | (R.took ? SPB_TOUCH : 0u);
                }
            }
        }
        o[i] = (uint8_t)b;
    }
}

// records [r0, r1) of segment s, clamped to the n_rec there are
__device__ __forceinline__ void spr_segment(const uint32_t* __restrict__ rec_off, uint32_t s, uint32_t n_rec, uint32_t& r0, uint32_t& r1) {
    r0 = min(rec_off[s], n_rec);
    r1 = min(rec_off[s + 1], n_rec);
}

#define SPP_COUNTERS 4
// WHERE THE RECORDS OF A (BARCODE, MEMBER) COME FROM - the one thing in which the entries of spr_counts differ.  A source answers,
// per lane: row(g) -> the row's members; barcode(e) -> the identity of entry e of the row's barcodes; segment(e, m, r0, r1) -> the
// records the lane walks for member m (PER_MEMBER: they differ by member, else they are fetched once per barcode); member(m) before
// the walk of member m; flag(i, fl) -> whether record i is one of the member's, and its flag byte (bit 0 first name, bits 1 .. 3);
// name(i) -> its read-name identity, asked for only where the draw is made.
//   SprCsr<SETS>  a record CSR the host made (smc_spike_rpb_counts, smc_spike_indel_rpb_counts, smc_spike_phase_rpb_counts): row g's
//                 barcodes are [off[g], off[g + 1]) of `ident`; segment s: records [rec_off[s], rec_off[s + 1]) of rec_name / rec_flag,
//                 clamped to n_rec.  A listed variant is a set of ONE member whose segments are its covering barcodes (segment e for
//                 barcode e: set_m and seg_base are not read); with SETS row g has set_m[g] members (1 .. SMC_SPIKE_PHASE_MAX_MEMBERS:
//                 the host checked) and its segments start at seg_base[g].  Every record of a segment is the member's.
//   SprRun        (smc_scan_phase_rpb_counts) no CSR: the run in barcode-major order and smc_spike_read_bits' bytes, both in HBM.
//                 Entry e is the run-wide barcode id joint_gid[e]; the lane walks ALL records of that barcode, [bc_start[b],
//                 bc_start[b + 1]) of bm_aln / bm_name / bm_first (streamed, clamped to n_aln), once per member, and record k is member
//                 m's when bit 0 (covers) of bits[row_var[m] * n_aln + bm_aln[k]] is set - the one scattered load of the walk, a byte;
//                 bits 1 and 2 of that byte are the flag's.  A record of another amplicon has a byte of 0 and is passed over.  An id
//                 that is not below n_bc, or an alignment index that is not below n_aln, reads nothing.
template <bool SETS>
struct SprCsr {
    static constexpr bool PER_MEMBER = SETS;
    const unsigned long long* __restrict__ ident;
    const uint32_t* __restrict__ off;
    const uint32_t* __restrict__ set_m;
    const uint32_t* __restrict__ seg_base;
    const uint32_t* __restrict__ rec_off;
    const unsigned long long* __restrict__ rec_name;
    const uint8_t* __restrict__ rec_flag;
    uint32_t n_rec;
    uint32_t e0, n_mem, s_base;
    __device__ __forceinline__ uint32_t row(uint32_t g) {
        e0 = off[g]; n_mem = SETS ? set_m[g] : 1u; s_base = SETS ? seg_base[g] : 0u;
        return n_mem;
    }
    __device__ __forceinline__ unsigned long long barcode(uint32_t e) { return ident[e]; }
    __device__ __forceinline__ void segment(uint32_t e, uint32_t m, uint32_t& r0, uint32_t& r1) const {
        spr_segment(rec_off, SETS ? s_base + (e - e0) * n_mem + m : e, n_rec, r0, r1);
    }
    __device__ __forceinline__ void member(uint32_t) {}
    __device__ __forceinline__ bool flag(uint32_t i, uint32_t& fl) const { fl = rec_flag[i]; return true; }
    __device__ __forceinline__ unsigned long long name(uint32_t i) const { return rec_name[i]; }
};

struct SprRun {
    static constexpr bool PER_MEMBER = false;
    const uint32_t* __restrict__ bm_aln;
    const unsigned long long* __restrict__ bm_name;
    const uint8_t* __restrict__ bm_first;
    const uint32_t* __restrict__ bc_start;
    const unsigned long long* __restrict__ idents;
    const uint8_t* __restrict__ bits;
    const uint32_t* __restrict__ row_off;
    const uint32_t* __restrict__ row_var;
    const uint32_t* __restrict__ joint_gid;
    uint32_t n_aln, n_bc;
    uint32_t v0, b;
    const uint8_t* __restrict__ mine;
    __device__ __forceinline__ uint32_t row(uint32_t g) { v0 = row_off[g]; return row_off[g + 1] - v0; }
    __device__ __forceinline__ unsigned long long barcode(uint32_t e) {
        b = joint_gid[e];
        return b < n_bc ? idents[b] : 0ull;
    }
    __device__ __forceinline__ void segment(uint32_t, uint32_t, uint32_t& r0, uint32_t& r1) const {
        r0 = r1 = 0u;
        if (b < n_bc) { r0 = min(bc_start[b], n_aln); r1 = min(bc_start[b + 1], n_aln); }
    }
    __device__ __forceinline__ void member(uint32_t m) { mine = bits + (size_t)row_var[v0 + m] * n_aln; }      // (uniform: the host checked row_var)
    __device__ __forceinline__ bool flag(uint32_t i, uint32_t& fl) const {
        const uint32_t a = bm_aln[i];
        if (a >= n_aln) return false;
        const uint32_t byte = mine[a];
        fl = (byte & (SPB_ALT | SPB_SINGLE)) | (bm_first[i] ? SPB_FIRST : 0u);
        return (byte & SPB_COVERS) != 0u;
    }
    __device__ __forceinline__ unsigned long long name(uint32_t i) const { return bm_name[i]; }
};

// Without SETS  out[(((g * n_reps + j) * n_tgt + t) * n_rr + r) * 5 + k] += counter k of (N', V0', S', READS', V1'),
// with SETS     out[(((g * n_reps + j) * n_tgt + t) * n_rr + r) * 4 + k] += counter k of (N_ALL', V0_ALL', S_ALL', V1_ALL')
// (zeroed before the launch); n_tgt * n_rr <= SMC_AF_DEPTH_MAX_CELLS, n_rr <= MAXR (the host picks the instance).  Row g: entries
// [off[g], off[g + 1]) of the source's barcodes; its records: the source's (above).
// FOUR (smc_spike_indel_rpb_counts): flag bit 2 is alt1 and bit 3 touch, a per-r counter each; without it bit 2 is both (`single`) and
// bit 3 is not read - a set has no READS', so it never reads it.
template <int MAXR, bool FOUR, bool SETS, class SRC>
__device__ __forceinline__ void spr_counts(SRC src, const uint32_t* __restrict__ off, const uint32_t* __restrict__ pos1, SpkThr T, int n_tgt,
                                           RgThr Q, int n_rr, const unsigned long long* __restrict__ seeds, int n_reps,
                                           uint32_t* __restrict__ out) {
    static_assert(!(FOUR && SETS), "spr_counts: a set never reads flag bit 3");
    constexpr int NC = SETS ? SPP_COUNTERS : SPC_COUNTERS;
    constexpr int TAIL = SETS ? 1 : MAXR;                  // (the cells' tail unrolled over the per-r arrays; a set's reads bit r of three words: a loop)
    __shared__ uint32_t part[SPB_BLOCK / WAVE][SMC_AF_DEPTH_MAX_CELLS][NC];
    const uint32_t g = blockIdx.y;
    const uint32_t e0 = off[g], e1 = off[g + 1], pos = pos1[g];
    const uint32_t n_mem = src.row(g);
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int n_cells = n_tgt * n_rr;
    const uint32_t every = n_rr >= 32 ? 0xFFFFFFFFu : (1u << n_rr) - 1u;
    const uint32_t stride = gridDim.x * SPB_BLOCK;
    for (uint32_t base = e0 + blockIdx.x * SPB_BLOCK; base < e1; base += stride) {     // (whole workgroups: the barriers below)
        const uint32_t e = base + threadIdx.x;
        const bool in_row = e < e1;
        const unsigned long long id = in_row ? src.barcode(e) : 0ull;
        uint32_t r0 = 0, r1 = 0;                                                       // (a lane beyond the row: no records, N' = 0 everywhere)
        if (!SRC::PER_MEMBER && in_row) src.segment(e, 0u, r0, r1);                    // (one segment for every member and replicate)
        for (int j = blockIdx.z; j < n_reps; j += gridDim.z) {
            const unsigned long long seed = seeds[j];
            uint32_t x[4];
            smc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), SPK_DOMAIN, pos, (uint32_t)seed, (uint32_t)(seed >> 32), x);
            const uint32_t k_hit = spd_hits(T, x[0], n_tgt);
            uint32_t reads[MAXR], alt[MAXR], sgl[MAXR], tch[FOUR ? MAXR : 1];
            uint32_t all_there = in_row ? every : 0u, all_c0 = every, all_c1 = every;  // (SETS; a lane beyond the row: N_ALL' = 0 everywhere)
            for (uint32_t m = 0; m < n_mem; ++m) {                                     // (uniform bound; once without SETS)
                if (SRC::PER_MEMBER && in_row) src.segment(e, m, r0, r1);
                src.member(m);
#pragma unroll
                for (int r = 0; r < MAXR; ++r) { reads[r] = alt[r] = sgl[r] = 0u; if (FOUR) tch[r] = 0u; }
                for (uint32_t i = r0; i < r1; ++i) {
                    uint32_t fl;
                    if (!src.flag(i, fl)) continue;
                    uint32_t kept = every;
                    if (!(fl & SPB_FIRST)) {
                        const uint32_t u = rg_draw(src.name(i), seed);
                        kept = 0u;
                        for (int r = 0; r < n_rr; ++r) kept |= (uint32_t)((unsigned long long)u < Q.t[r]) << r;
                    }
                    const uint32_t is_alt = (fl >> 1) & 1u, is_sgl = (fl >> 2) & 1u, is_tch = (fl >> 3) & 1u;
#pragma unroll
                    for (int r = 0; r < MAXR; ++r) {
                        const uint32_t k = (kept >> r) & 1u;
                        reads[r] += k; alt[r] += k & is_alt; sgl[r] += k & is_sgl;
                        if (FOUR) tch[r] += k & is_tch;
                    }
                }
                if (SETS) {                                                            // (the member's counters fold into three bit sets over r)
                    uint32_t there = 0u, c0 = 0u, c1 = 0u;
#pragma unroll
                    for (int r = 0; r < MAXR; ++r) {
                        there |= (uint32_t)(reads[r] > 0u) << r;
                        c0 |= (uint32_t)(2ull * alt[r] > (unsigned long long)reads[r]) << r;
                        c1 |= (uint32_t)(2ull * sgl[r] > (unsigned long long)reads[r]) << r;
                    }
                    all_there &= there; all_c0 &= c0; all_c1 &= c1;
                }
            }
#pragma unroll TAIL
            for (int r = 0; r < (SETS ? n_rr : MAXR); ++r) {
                if (r < n_rr) {                                                        // (uniform)
                    const bool there = SETS ? ((all_there >> r) & 1u) != 0u : reads[r] > 0u;
                    const bool car0 = SETS ? ((all_c0 >> r) & 1u) != 0u : 2ull * alt[r] > (unsigned long long)reads[r];
                    const bool car1 = SETS ? ((all_c1 >> r) & 1u) != 0u : 2ull * sgl[r] > (unsigned long long)reads[r];
                    const unsigned long long m_n = __ballot(there), m_v0 = __ballot(there && car0);
                    for (int t = 0; t < n_tgt; ++t) {
                        const bool hit = ((k_hit >> t) & 1u) != 0u;
                        const unsigned long long m_s = __ballot(there && hit), m_v1 = __ballot(there && (hit ? car1 : car0));
                        int rd = 0;                                                    // (a run holds fewer than 2^32 - 256 alignments: no wrap that matters)
                        if (!SETS) rd = wave_add((int)((there && hit) ? (FOUR ? tch[r] : sgl[r]) : 0u));
                        if (lane == 0) {
                            uint32_t* const p = part[wave][t * n_rr + r];
                            p[0] = (uint32_t)__popcll(m_n); p[1] = (uint32_t)__popcll(m_v0); p[2] = (uint32_t)__popcll(m_s);
                            if (!SETS) p[3] = (uint32_t)rd;
                            p[NC - 1] = (uint32_t)__popcll(m_v1);
                        }
                    }
                }
            }
            __syncthreads();
            if ((int)threadIdx.x < NC * n_cells) {                                     // (5 * 32 = 160 < SPB_BLOCK)
                const int c = threadIdx.x / NC, q = threadIdx.x % NC;
                uint32_t sum = 0;
                for (int w = 0; w < SPB_BLOCK / WAVE; ++w) sum += part[w][c][q];
                if (sum) atomicAdd(&out[(((size_t)g * n_reps + j) * n_cells + c) * NC + q], sum);
            }
            __syncthreads();
        }
    }
}

// spr_counts over a record CSR of the host's
template <int MAXR, bool FOUR, bool SETS>
__global__ __launch_bounds__(SPB_BLOCK) void k_spr_counts(const unsigned long long* __restrict__ ident, const uint32_t* __restrict__ off,
                                                          const uint32_t* __restrict__ set_m, const uint32_t* __restrict__ seg_base,
                                                          const uint32_t* __restrict__ rec_off, const unsigned long long* __restrict__ rec_name,
                                                          const uint8_t* __restrict__ rec_flag, uint32_t n_rec,
                                                          const uint32_t* __restrict__ pos1, SpkThr T, int n_tgt, RgThr Q, int n_rr,
                                                          const unsigned long long* __restrict__ seeds, int n_reps, uint32_t* __restrict__ out) {
    SprCsr<SETS> src;
    src.ident = ident; src.off = off; src.set_m = set_m; src.seg_base = seg_base; src.rec_off = rec_off; src.rec_name = rec_name;
    src.rec_flag = rec_flag; src.n_rec = n_rec;
    spr_counts<MAXR, FOUR, SETS>(src, off, pos1, T, n_tgt, Q, n_rr, seeds, n_reps, out);
}

// spr_counts over the run in barcode-major order and the read bits in HBM (smc_scan_phase_rpb_counts): always the sets' four counters,
// a row of one member a listed variant
template <int MAXR>
__global__ __launch_bounds__(SPB_BLOCK) void k_spr_run_counts(SprRun src, const uint32_t* __restrict__ joint_off, const uint32_t* __restrict__ pos1,
                                                              SpkThr T, int n_tgt, RgThr Q, int n_rr,
                                                              const unsigned long long* __restrict__ seeds, int n_reps,
                                                              uint32_t* __restrict__ out) {
    spr_counts<MAXR, false, true>(src, joint_off, pos1, T, n_tgt, Q, n_rr, seeds, n_reps, out);
}
static_assert(SMC_RG_MAX_TARGETS == SMC_AF_DEPTH_MAX_CELLS && SPP_COUNTERS <= SPC_COUNTERS && SPC_COUNTERS * SMC_AF_DEPTH_MAX_CELLS <= SPB_BLOCK,
              "spr_counts: a bit per read threshold, a lane per cell and counter");

// ------------------------------------------------------------------------------------------
// --spikeGrid (smc_spike_grid_counts): the cells (spike target t, barcode fraction f, reads-per-barcode target r)
// ------------------------------------------------------------------------------------------
// Cell (t, f, r) of replicate j is the spike-in at t, then --dsGrid's philox rule at (f, r), all three streams keyed by s_j: a record
// stays when its barcode's sel_draw is below bc_thr[f] AND it is a first name or its rg_draw is below the cell's read threshold.
// Under a grid the read threshold is no constant of the file: probKeep of (f, r) is made from the barcodes kept at f, which move with
// the seed - so the thresholds come per replicate, rd_thr[(j * n_frac + f) * n_rr + r] in device memory, and k_spr_counts, whose
// thresholds are one by-value set for every replicate, cannot serve.  A PAIR q = f * n_rr + r takes the place of k_spr_counts' r: one
// rg_draw per record and replicate, its compares against the replicate's n_frac * n_rr thresholds one bit set, (reads_q, alt_q,
// single_q) per pair in registers (unrolled loops only; MAXQ = 8 and 32 as there).  The barcode rule drops whole barcodes, so it is
// ONE sel_draw per (barcode, replicate), a bit set over f, applied behind the record walk:
//   there = kept_f && reads_q > 0      N' = there      V0' = there && 2 alt_q > reads_q      S' = there && hit_t
//   READS' = single_q over there && hit_t             V1' = there && (hit_t ? 2 single_q > reads_q : 2 alt_q > reads_q)
// reduced exactly as k_spr_counts reduces.  With one fraction of 2^32 and every replicate's thresholds equal the words are
// k_spr_counts<., false, false>'s; with one read threshold of 2^32 they are k_spike_cells' on the per-barcode sums of the flag bits.
// out[((((g * n_reps + j) * n_tgt + t) * n_frac + f) * n_rr + r) * 5 + k] (zeroed before the launch); n_tgt * n_frac * n_rr <=
// SMC_AF_DEPTH_MAX_CELLS, n_frac * n_rr <= MAXQ (the host picks the instance).
template <int MAXQ>
__global__ __launch_bounds__(SPB_BLOCK) void k_spg_counts(const unsigned long long* __restrict__ ident, const uint32_t* __restrict__ off,
                                                          const uint32_t* __restrict__ rec_off, const unsigned long long* __restrict__ rec_name,
                                                          const uint8_t* __restrict__ rec_flag, uint32_t n_rec,
                                                          const uint32_t* __restrict__ pos1, SpkThr T, int n_tgt, AfdThr D, int n_frac, int n_rr,
                                                          const unsigned long long* __restrict__ rd_thr,
                                                          const unsigned long long* __restrict__ seeds, int n_reps, uint32_t* __restrict__ out) {
    __shared__ uint32_t part[SPB_BLOCK / WAVE][SMC_AF_DEPTH_MAX_CELLS][SPC_COUNTERS];
    __shared__ unsigned long long Q[SMC_AF_DEPTH_MAX_CELLS];                            // the replicate's thresholds, one per pair
    const uint32_t g = blockIdx.y;
    const uint32_t e0 = off[g], e1 = off[g + 1], pos = pos1[g];
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const int n_q = n_frac * n_rr, n_cells = n_tgt * n_q;
    const uint32_t every = n_q >= 32 ? 0xFFFFFFFFu : (1u << n_q) - 1u;
    const uint32_t stride = gridDim.x * SPB_BLOCK;
    for (uint32_t base = e0 + blockIdx.x * SPB_BLOCK; base < e1; base += stride) {     // (whole workgroups: the barriers below)
        const uint32_t e = base + threadIdx.x;
        const bool in_row = e < e1;
        const unsigned long long id = in_row ? ident[e] : 0ull;
        uint32_t r0 = 0, r1 = 0;                                                       // (a lane beyond the row: no records, N' = 0 everywhere)
        if (in_row) spr_segment(rec_off, e, n_rec, r0, r1);
        for (int j = blockIdx.z; j < n_reps; j += gridDim.z) {
            const unsigned long long seed = seeds[j];
            // (the replicate's own thresholds, fetched ONCE into LDS - not per record; the barrier behind the last reduction, or the one
            // below, stands between a lane's reads of the previous replicate's and these stores)
            if ((int)threadIdx.x < n_q) Q[threadIdx.x] = rd_thr[(size_t)j * n_q + threadIdx.x];
            __syncthreads();
            uint32_t x[4];
            smc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), SPK_DOMAIN, pos, (uint32_t)seed, (uint32_t)(seed >> 32), x);
            const uint32_t k_hit = spd_hits(T, x[0], n_tgt);
            const uint32_t k_d = in_row ? afd_keep_depth(D, sel_draw(id, seed), n_frac) : 0u;
            uint32_t reads[MAXQ], alt[MAXQ], sgl[MAXQ];
#pragma unroll
            for (int q = 0; q < MAXQ; ++q) reads[q] = alt[q] = sgl[q] = 0u;
            for (uint32_t i = r0; i < r1; ++i) {
                const uint32_t fl = rec_flag[i];
                uint32_t kept = every;
                if (!(fl & SPB_FIRST)) {
                    const uint32_t u = rg_draw(rec_name[i], seed);
                    kept = 0u;
                    for (int q = 0; q < n_q; ++q) kept |= (uint32_t)((unsigned long long)u < Q[q]) << q;
                }
                const uint32_t is_alt = (fl >> 1) & 1u, is_sgl = (fl >> 2) & 1u;
#pragma unroll
                for (int q = 0; q < MAXQ; ++q) {
                    const uint32_t k = (kept >> q) & 1u;
                    reads[q] += k; alt[q] += k & is_alt; sgl[q] += k & is_sgl;
                }
            }
            int f = 0, r = 0;                                                          // (pair q = f * n_rr + r, stepped: no division)
#pragma unroll
            for (int q = 0; q < MAXQ; ++q) {
                if (q < n_q) {                                                         // (uniform)
                    const bool there = ((k_d >> f) & 1u) != 0u && reads[q] > 0u;
                    const bool car0 = 2ull * alt[q] > (unsigned long long)reads[q];
                    const bool car1 = 2ull * sgl[q] > (unsigned long long)reads[q];
                    const unsigned long long m_n = __ballot(there), m_v0 = __ballot(there && car0);
                    for (int t = 0; t < n_tgt; ++t) {
                        const bool hit = ((k_hit >> t) & 1u) != 0u;
                        const unsigned long long m_s = __ballot(there && hit), m_v1 = __ballot(there && (hit ? car1 : car0));
                        const int rd = wave_add((int)((there && hit) ? sgl[q] : 0u));    // (fewer than 2^32 - 256 records: no wrap that matters)
                        if (lane == 0) {
                            uint32_t* const p = part[wave][t * n_q + q];
                            p[0] = (uint32_t)__popcll(m_n); p[1] = (uint32_t)__popcll(m_v0); p[2] = (uint32_t)__popcll(m_s);
                            p[3] = (uint32_t)rd; p[4] = (uint32_t)__popcll(m_v1);
                        }
                    }
                    if (++r == n_rr) { r = 0; ++f; }
                }
            }
            __syncthreads();
            if ((int)threadIdx.x < SPC_COUNTERS * n_cells) {                           // (5 * 32 = 160 < SPB_BLOCK)
                const int c = threadIdx.x / SPC_COUNTERS, k = threadIdx.x % SPC_COUNTERS;
                uint32_t sum = 0;
                for (int w = 0; w < SPB_BLOCK / WAVE; ++w) sum += part[w][c][k];
                if (sum) atomicAdd(&out[(((size_t)g * n_reps + j) * n_cells + c) * SPC_COUNTERS + k], sum);
            }
            __syncthreads();
        }
    }
}
