// Included by smcounter_hip.hip (after k_spike.inc: SPK_DOMAIN, the SNV rule it restates; after k_bp_emit2.inc: bp2_resolve).
// ------------------------------------------------------------------------------------------
// --spikeIndels: listed insertions and deletions (and SNVs beside them) planted in a copy of a run (smc_spike_indels);
// --spikeIndelReps: several such copies from one call (smc_spike_indels_reps), and the records each listed indel can touch
// (smc_spike_indel_touch)
// ------------------------------------------------------------------------------------------
// An indel changes a record's length, CIGAR and query layout: the records that take one are RELOCATED - their pairs and CIGAR words
// written anew behind the run's own, in alignment order, densely - and every other record goes through k_spike_rewrite's rule in
// place.  Three launches, none of which waits for the host or for another workgroup:
//   k_spi_count     a lane per alignment: the listed variants in [pos, end) by the binary search of k_spike_rewrite, the draw of every
//                   insertion / deletion among them, its footprint resolved against the CIGAR (spi_walk<false>).  A record with at
//                   least one indel hit reports its new l_seq and n_cig, every other 0; the workgroup's sums of both go to bsum[].
//   k_spi_scan      ONE workgroup: the exclusive scan of the workgroups' sums, chunk by chunk with a carry; totals[].
//   k_spi_scatter   a lane per alignment: its place = the workgroup's scanned sum + the exclusive scan of the lanes before it in the
//                   workgroup.  A relocated record walks its CIGAR and its variants once more (spi_walk<true>) and stores operations
//                   and pairs; the others take the SNV rule in place.  Every record, nm_out, n_indel_out; stats by atomics.
// The scan is a sum of integers in a fixed tree: the offsets are the same in every call.
// SEVERAL COPIES (smc_spike_indels_reps): blockIdx.y = copy c in all three kernels - its seed and threshold come by value (SpkCopies,
// every variant at the copy's threshold unless `own_thr`), its cnt[] / bsum[] / totals[] / statistics stand one copy behind the
// other, its outputs at byte strides.  The run's two pools reach every copy by k_spike_pool (read once, stored n_copies times in
// 16-byte chunks) before the scatter appends to them.  One copy with own_thr is smc_spike_indels.
//   k_spi_touch     a lane per alignment: spi_walk<false, SPI_TOUCH_SUM> - no draw, every listed insertion / deletion taken as hit - adds 1 to
//                   out[v][bc_gid] for every one the record is eligible for: the records the rewrite changes at v when the barcode is
//                   spiked.  The eligibility is spi_walk's own lines, not a restatement.
// Eligible (the specification is tools/spike_variants.py): the variant's footprint - the anchor and the position behind it (an
// insertion), the anchor, the d deleted positions and the one behind them (a deletion) - inside ONE M / = / X operation of the
// ORIGINAL CIGAR, its query positions inside l_seq; the record's l_seq and n_cig, as the variants before it left them, still in 16
// bits.  Variants are taken in ascending position; their footprints are disjoint (the host checked), so a split operation's rest
// holds the next one whole or not at all.  For the same reason whether a record takes variant v depends on no other variant's draw,
// but for the two 16-bit limits, which count what the variants before it added: the host of --spikeIndelReps refuses a run in which
// they could bind (devplanes.spike_indel_limits), and then k_spi_touch's numbers hold for every draw.
// --spikeIndelPhase: a member of a phase set (V.lead != 0) draws with the position of its set's leader, var[k - V.lead], in both draw
// sites (spi_walk, the in-place SNV loop of k_spi_scatter) - k_spike_rewrite's rule: one load more, for such records only; the leader
// may stand in front of the record's first variant `lo`, the host checked lead <= k.  Every member of a set then makes the same draw
// and is applied under its own rule; what a record is eligible for does not depend on it.  k_spi_touch draws nothing.
#define SPI_BLOCK 256
#define SPI_MAX16 65535u
static_assert(sizeof(smc_spike_indel_variant) == 24, "abi.SPIKE_INDEL_VARIANT_DTYPE");

// a workgroup's exclusive scan of one value per thread -> the thread's prefix; `total` the workgroup's sum.  lds: SPI_BLOCK / 64 words
template <typename T>
__device__ __forceinline__ T spi_block_excl(T v, T* lds, T& total) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    T inc = v;
    for (int o = 1; o < 64; o <<= 1) { const T u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    __syncthreads();                                             // (lds may still be read from the call before)
    if (lane == 63) lds[wid] = inc;
    __syncthreads();
    T pre = 0, tot = 0;
    for (int w = 0; w < SPI_BLOCK / 64; ++w) { if (w < wid) pre += lds[w]; tot += lds[w]; }
    total = tot;
    return pre + inc - v;
}

struct SpiRes { uint32_t l_seq, n_cig; int nm_inc, indel_inc; int want; bool took; };
// what spi_walk does beside (or in place of) drawing: count the eligible records per barcode, or answer for ONE variant of one record
#define SPI_TOUCH_SUM 1
#define SPI_TOUCH_ONE 2

// One record against its variants var[lo ..] (those with pos0 < a.end).  EMIT false: only the indel kinds are drawn, nothing is stored
// -> whether any hit is eligible, R.l_seq / R.n_cig the record's new sizes.  EMIT true: the SNVs are drawn too, the operations go to
// oc[], the pairs to op[] (the caller made sure that R.n_cig words and R.l_seq pairs fit), stats[] counts.  A variant's threshold is
// its own with `own_thr`, else `thr_c`.  TOUCH (with EMIT false): nothing is drawn - every insertion / deletion counts as hit - and
// SPI_TOUCH_SUM: stats[k * touch_stride] counts every one the record is eligible for; SPI_TOUCH_ONE (--spikeIndelRpb, per record):
// nothing is stored, R.took says whether the record is eligible for variant R.want (an index into var[], set by the caller).
template <bool EMIT, int TOUCH = 0>
__device__ __forceinline__ bool spi_walk(const smc_dev_aln& a, const uint32_t* __restrict__ cg, const uint8_t* __restrict__ src,
                                         const smc_spike_indel_variant* __restrict__ var, int lo, int n_var, const uint8_t* __restrict__ ins,
                                         unsigned long long id, unsigned long long seed, unsigned long long thr_c, int own_thr,
                                         uint32_t* __restrict__ oc, uint8_t* __restrict__ op, uint32_t* __restrict__ stats, size_t touch_stride,
                                         SpiRes& R) {
    static_assert(!(EMIT && TOUCH), "spi_walk: TOUCH counts, it stores no record");
    const int n_cig = (int)a.n_cig, l_seq = (int)a.l_seq;
    int ci = 0, x = a.pos, y = 0, used = 0;                      // operation ci starts at reference x, query y; `used` of it are out already
    int yq = 0;                                                  // pairs [0, yq) of the record are dealt with
    uint32_t oci = 0, oq = 0, cur_l = (uint32_t)l_seq, cur_c = (uint32_t)n_cig;
    bool any = false;
    R.nm_inc = 0; R.indel_inc = 0; R.took = false;
    auto copy_to = [&](int q_end) {                              // pairs [yq, q_end) as they are
        q_end = min(q_end, l_seq);
        if (EMIT) for (int q = yq; q < q_end; ++q) *(uint16_t*)(op + 2ull * (oq + (uint32_t)(q - yq))) = *(const uint16_t*)(src + 2ull * q);
        if (q_end > yq) { oq += (uint32_t)(q_end - yq); yq = q_end; }
    };
    auto leave_op = [&]() {                                      // the rest of operation ci, then on to the next
        const uint32_t w = cg[ci];
        const int o = (int)(w & 15u), len = (int)(w >> 4);
        if (EMIT) oc[oci] = used ? ((uint32_t)(len - used) << 4 | (uint32_t)o) : w;
        ++oci;
        if (o == 0 || o == 7 || o == 8) { x += len; y += len; }
        else if (o == 2 || o == 3) x += len;
        else if (o == 1 || o == 4) y += len;
        used = 0; ++ci;
    };
    for (int k = lo; k < n_var; ++k) {
        const smc_spike_indel_variant V = var[k];
        if (V.pos0 >= a.end) break;
        if (!EMIT && V.kind == SMC_AF_SNV) continue;
        if (!TOUCH) {
            uint32_t u[4];
            smc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), SPK_DOMAIN, (uint32_t)(V.lead ? var[k - (int)V.lead].pos0 : V.pos0) + 1u,
                              (uint32_t)seed, (uint32_t)(seed >> 32), u);
            if (!((unsigned long long)u[0] < (own_thr ? V.thr : thr_c))) continue;
        }
        if (V.kind == SMC_AF_SNV) {                              // k_spike_rewrite's rule, on the original CIGAR
            const BpRes r = bp2_resolve(cg, n_cig, a.pos, V.pos0, l_seq);
            if (r.isdel || r.indel != 0 || r.qpos < yq || r.qpos >= l_seq) continue;
            copy_to(r.qpos);
            const uint16_t pr = *(const uint16_t*)(src + 2ull * r.qpos);
            if (EMIT) {
                *(uint16_t*)(op + 2ull * oq) = (uint16_t)((pr & 0xFF00u) | V.alt);
                atomicAdd(&stats[2 * k], 1u);
                if ((uint8_t)(pr & 0xFFu) == V.ref) atomicAdd(&stats[2 * k + 1], 1u);
            }
            if ((uint8_t)(pr & 0xFFu) == V.ref) ++R.nm_inc;
            ++oq; yq = r.qpos + 1;
            continue;
        }
        const int p = V.pos0, n = (int)V.len, fp = V.kind == SMC_AF_INS ? 1 : n + 1;
        while (ci < n_cig) {                                     // the operation that holds p
            const uint32_t w = cg[ci];
            const int o = (int)(w & 15u), len = (int)(w >> 4);
            if ((o == 0 || o == 7 || o == 8 || o == 2 || o == 3) && (long long)p < (long long)x + len) break;
            leave_op();
        }
        if (ci >= n_cig) break;                                  // (a CIGAR shorter than the record's span: nothing behind it either)
        const uint32_t w = cg[ci];
        const int o = (int)(w & 15u), len = (int)(w >> 4);
        if (!(o == 0 || o == 7 || o == 8)) continue;
        const int d0 = p - x, qa = y + d0;                       // the anchor within the operation, its query position
        if (d0 < used || (long long)d0 + fp >= (long long)len || qa + fp >= l_seq || qa < yq) continue;
        if (cur_c + 2u > SPI_MAX16 || (V.kind == SMC_AF_INS && cur_l + (uint32_t)n > SPI_MAX16)) continue;
        any = true;
        if (TOUCH == SPI_TOUCH_SUM) atomicAdd(&stats[(size_t)k * touch_stride], 1u);
        if (TOUCH == SPI_TOUCH_ONE && k == R.want) R.took = true;
        cur_c += 2u;
        const int head = d0 - used + 1;
        if (EMIT) { oc[oci] = (uint32_t)head << 4 | (uint32_t)o; oc[oci + 1] = (uint32_t)n << 4 | (V.kind == SMC_AF_INS ? 1u : 2u); }
        oci += 2u;
        copy_to(qa + 1);
        if (V.kind == SMC_AF_INS) {
            if (EMIT) {
                const uint32_t q = (uint32_t)src[2ull * qa + 1] << 8;
                for (int j = 0; j < n; ++j) *(uint16_t*)(op + 2ull * (oq + (uint32_t)j)) = (uint16_t)(q | ins[V.ins_off + (uint32_t)j]);
            }
            oq += (uint32_t)n; cur_l += (uint32_t)n;
            used = d0 + 1;
        } else {
            yq = qa + 1 + n; cur_l -= (uint32_t)n;
            used = d0 + 1 + n;
        }
        R.nm_inc += n; R.indel_inc += n;
        if (EMIT) { atomicAdd(&stats[2 * k], 1u); atomicAdd(&stats[2 * k + 1], 1u); }
    }
    while (ci < n_cig) leave_op();
    copy_to(l_seq);
    R.l_seq = oq; R.n_cig = oci;
    return any;
}

__device__ __forceinline__ int spi_first(const smc_spike_indel_variant* __restrict__ var, int n_var, int pos) {
    int lo = 0, hi = n_var;                                      // first variant with pos0 >= pos
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (var[mid].pos0 < pos) lo = mid + 1; else hi = mid; }
    return lo;
}

// (a record that points beyond the pools, or whose barcode id is none of the run's, is left where it is and counts nowhere)
__device__ __forceinline__ bool spi_in_run(const smc_dev_aln& a, int lo, const smc_spike_indel_variant* __restrict__ var, int n_var, uint32_t n_bc,
                                           unsigned long long n_pairs, unsigned long long n_cig_words) {
    return a.bc_gid < n_bc && lo < n_var && var[lo].pos0 < a.end && (unsigned long long)a.seq_off + a.l_seq <= n_pairs &&
           (unsigned long long)a.cig_off + a.n_cig <= n_cig_words;
}

// copy c = blockIdx.y.  cnt_c[i] / cnt_c[n_aln + i]: the new l_seq / n_cig of a record that is relocated, else 0; bsum_c[2 b],
// bsum_c[2 b + 1]: workgroup b's sums; cnt_c = cnt + 2 c n_aln, bsum_c = bsum + 2 c gridDim.x
__global__ __launch_bounds__(SPI_BLOCK) void k_spi_count(const smc_dev_aln* __restrict__ aln, uint32_t n_aln, const uint32_t* __restrict__ cig,
                                                         unsigned long long n_pairs, unsigned long long n_cig_words,
                                                         const smc_spike_indel_variant* __restrict__ var, int n_var,
                                                         const unsigned long long* __restrict__ ident, uint32_t n_bc, SpkCopies C, int own_thr,
                                                         uint32_t* __restrict__ cnt, unsigned long long* __restrict__ bsum) {
    __shared__ uint32_t lds[SPI_BLOCK / 64];
    const uint32_t i = blockIdx.x * SPI_BLOCK + threadIdx.x, c = blockIdx.y;
    cnt += 2ull * c * n_aln; bsum += 2ull * c * gridDim.x;
    uint32_t np = 0, nc = 0;
    if (i < n_aln) {
        const smc_dev_aln a = aln[i];
        const int lo = spi_first(var, n_var, a.pos);
        if (spi_in_run(a, lo, var, n_var, n_bc, n_pairs, n_cig_words)) {
            SpiRes R;
            if (spi_walk<false>(a, cig + a.cig_off, nullptr, var, lo, n_var, nullptr, ident[a.bc_gid], C.seed[c], C.thr[c], own_thr, nullptr, nullptr,
                                nullptr, 0, R)) {
                np = R.l_seq; nc = R.n_cig;
            }
        }
        cnt[i] = np; cnt[(size_t)n_aln + i] = nc;
    }
    uint32_t tp, tc;
    spi_block_excl(np, lds, tp);
    spi_block_excl(nc, lds, tc);
    if (threadIdx.x == 0) { bsum[2ull * blockIdx.x] = tp; bsum[2ull * blockIdx.x + 1] = tc; }
}

// one workgroup per copy (blockIdx.x = c): bsum_c[] -> its exclusive scan, in place; totals[3 c + 0] / [1] = pairs / CIGAR words the
// copy needs, the run's own included, totals[3 c + 2] bit 1 = more than the capacities
__global__ __launch_bounds__(SPI_BLOCK) void k_spi_scan(unsigned long long* __restrict__ bsum, uint32_t n_blocks, unsigned long long n_pairs,
                                                        unsigned long long n_cig_words, unsigned long long cap_pairs, unsigned long long cap_cig,
                                                        unsigned long long* __restrict__ totals) {
    __shared__ unsigned long long lds[SPI_BLOCK / 64];
    bsum += 2ull * blockIdx.x * n_blocks; totals += 3ull * blockIdx.x;
    unsigned long long carry_p = 0, carry_c = 0;
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += SPI_BLOCK) {
        const uint32_t b = b0 + threadIdx.x;
        const unsigned long long vp = b < n_blocks ? bsum[2ull * b] : 0ull, vc = b < n_blocks ? bsum[2ull * b + 1] : 0ull;
        unsigned long long tp, tc;
        const unsigned long long ep = spi_block_excl(vp, lds, tp), ec = spi_block_excl(vc, lds, tc);
        if (b < n_blocks) { bsum[2ull * b] = carry_p + ep; bsum[2ull * b + 1] = carry_c + ec; }
        carry_p += tp; carry_c += tc;
    }
    if (threadIdx.x == 0) {
        totals[0] = n_pairs + carry_p; totals[1] = n_cig_words + carry_c;
        totals[2] = (n_pairs + carry_p > cap_pairs || n_cig_words + carry_c > cap_cig) ? 1ull : 0ull;
    }
}

__global__ __launch_bounds__(SPI_BLOCK) void k_spi_scatter(const smc_dev_aln* __restrict__ aln, uint32_t n_aln, const uint32_t* __restrict__ cig,
                                                           const uint8_t* __restrict__ bq, unsigned long long n_pairs, unsigned long long n_cig_words,
                                                           const smc_spike_indel_variant* __restrict__ var, int n_var, const uint8_t* __restrict__ ins,
                                                           const unsigned long long* __restrict__ ident, uint32_t n_bc, SpkCopies C, int own_thr,
                                                           double mismatch_thr, const int32_t* __restrict__ nm, const int32_t* __restrict__ n_indel,
                                                           const uint32_t* __restrict__ cnt, const unsigned long long* __restrict__ bsum,
                                                           unsigned long long cap_pairs, unsigned long long cap_cig, uint8_t* __restrict__ aln_out_b,
                                                           unsigned long long aln_stride, uint8_t* __restrict__ bq_out, unsigned long long bq_stride,
                                                           uint8_t* __restrict__ cig_out_b, unsigned long long cig_stride, int32_t* __restrict__ nm_out,
                                                           int32_t* __restrict__ n_indel_out, uint32_t* __restrict__ stats) {
    __shared__ uint32_t lds[SPI_BLOCK / 64];
    const uint32_t i = blockIdx.x * SPI_BLOCK + threadIdx.x, c = blockIdx.y;
    // copy c: its scratch, its outputs (the pools at byte strides, NM' / n_indel' / statistics one copy behind the other)
    const unsigned long long seed = C.seed[c], thr_c = C.thr[c];
    cnt += 2ull * c * n_aln; bsum += 2ull * c * gridDim.x;
    smc_dev_aln* const aln_out = reinterpret_cast<smc_dev_aln*>(aln_out_b + c * aln_stride);
    uint32_t* const cig_out = reinterpret_cast<uint32_t*>(cig_out_b + c * cig_stride);
    bq_out += c * bq_stride; nm_out += (size_t)c * n_aln; n_indel_out += (size_t)c * n_aln; stats += 2ull * c * (unsigned long long)n_var;
    const bool valid = i < n_aln;
    const uint32_t np = valid ? cnt[i] : 0u, nc = valid ? cnt[(size_t)n_aln + i] : 0u;
    uint32_t tp, tc;
    const unsigned long long off_p = n_pairs + bsum[2ull * blockIdx.x] + spi_block_excl(np, lds, tp);
    const unsigned long long off_c = n_cig_words + bsum[2ull * blockIdx.x + 1] + spi_block_excl(nc, lds, tc);
    if (!valid) return;
    smc_dev_aln a = aln[i];
    const int lo = spi_first(var, n_var, a.pos);
    long long new_nm = (long long)nm[i], new_indel = (long long)n_indel[i];
    if (nc != 0u) {
        // (nothing beyond the capacities is written: such a record stays as the run has it, and totals[2] says so)
        if (off_p + np <= cap_pairs && off_c + nc <= cap_cig && off_p + np <= 0xFFFFFFFFull && off_c + nc <= 0xFFFFFFFFull) {
            SpiRes R;
            spi_walk<true>(a, cig + a.cig_off, bq + 2ull * a.seq_off, var, lo, n_var, ins, ident[a.bc_gid], seed, thr_c, own_thr, cig_out + off_c,
                           bq_out + 2ull * off_p, stats, 0, R);
            new_nm += R.nm_inc; new_indel += R.indel_inc;
            a.qalen = (uint16_t)((int)a.qalen + (int)R.l_seq - (int)a.l_seq);
            a.l_seq = (uint16_t)R.l_seq; a.n_cig = (uint16_t)R.n_cig;
            a.seq_off = (uint32_t)off_p; a.cig_off = (uint32_t)off_c;
        }
    } else if (a.bc_gid < n_bc) {                                // k_spike_rewrite's loop over the SNVs, in place
        const unsigned long long id = ident[a.bc_gid];
        for (int k = lo; k < n_var; ++k) {
            const smc_spike_indel_variant V = var[k];
            if (V.pos0 >= a.end) break;
            if (V.kind != SMC_AF_SNV) continue;
            uint32_t u[4];
            smc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), SPK_DOMAIN, (uint32_t)(V.lead ? var[k - (int)V.lead].pos0 : V.pos0) + 1u,
                              (uint32_t)seed, (uint32_t)(seed >> 32), u);
            if (!((unsigned long long)u[0] < (own_thr ? V.thr : thr_c))) continue;
            const BpRes r = bp2_resolve(cig + a.cig_off, (int)a.n_cig, a.pos, V.pos0, (int)a.l_seq);
            if (r.isdel || r.indel != 0 || r.qpos < 0 || r.qpos >= (int)a.l_seq) continue;
            const unsigned long long at = (unsigned long long)a.seq_off + (unsigned long long)r.qpos;
            if (at >= n_pairs) continue;
            uint8_t* const s = bq_out + 2ull * at;
            const uint8_t old = s[0];
            s[0] = V.alt;
            atomicAdd(&stats[2 * k], 1u);
            if (old == V.ref) { ++new_nm; atomicAdd(&stats[2 * k + 1], 1u); }
        }
    }
    const long long mm = max(0ll, new_nm - new_indel);
    const double mm100 = a.l_seq > 0 ? 100.0 * (double)mm / (double)a.l_seq : 0.0;     // smCounter.py:352-356
    a.oflag = (uint8_t)((a.oflag & ~SMC_DA_MMOK) | (mm100 <= mismatch_thr ? SMC_DA_MMOK : 0u));
    aln_out[i] = a;
    nm_out[i] = (int32_t)new_nm; n_indel_out[i] = (int32_t)new_indel;
}

// out[v * n_bc + b] += the records of barcode b that take the listed insertion / deletion v when b is spiked (zeroed before the launch;
// an SNV's row stays 0).  Bounds as in k_spi_count.
__global__ __launch_bounds__(SPI_BLOCK) void k_spi_touch(const smc_dev_aln* __restrict__ aln, uint32_t n_aln, const uint32_t* __restrict__ cig,
                                                         unsigned long long n_pairs, unsigned long long n_cig_words,
                                                         const smc_spike_indel_variant* __restrict__ var, int n_var, uint32_t n_bc,
                                                         uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * SPI_BLOCK + threadIdx.x;
    if (i >= n_aln) return;
    const smc_dev_aln a = aln[i];
    const int lo = spi_first(var, n_var, a.pos);
    if (!spi_in_run(a, lo, var, n_var, n_bc, n_pairs, n_cig_words)) return;
    SpiRes R;
    spi_walk<false, SPI_TOUCH_SUM>(a, cig + a.cig_off, nullptr, var, lo, n_var, nullptr, 0ull, 0ull, 0ull, 0, nullptr, nullptr, out + a.bc_gid, (size_t)n_bc, R);
}
