// Included by smcounter_hip.hip (after k_spike_rpb.inc; reads smc_row as k_call_v2 / k_filter_loci leave it).
// ------------------------------------------------------------------------------------------
// --spikeScan: was the planted SNV called?  One verdict per (copy, listed locus) of a called batch, the rows staying in HBM
// (smc_scan_detect)
// ------------------------------------------------------------------------------------------
// A pass of the scan calls B spiked copies of a run with one plan: rows[c * n_loci + l] is locus l of copy c.  Of those n_loci rows
// only the G listed ones - where the pass planted its SNVs - say anything, and of their 432 bytes only five fields: status, biallelic,
// used_mt and cand[0]'s allele, vmt and pi.  The .cut file's rule for "the planted ALT was called" (writers.cut_row behind
// rows.format_row) on such a row is
//     status == 0, the row not bi-allelic, cand[0].allele == ALT's fixed id (A, T, G, C = 0 .. 3), and int(float(py2 round(PI, 2))) >= thr
// and round(PI, 2) >= thr for an integer thr is PI >= thr - 0.005 up to how py2 rounds a double that close to the half.  So
//   k_scan_detect  a lane per (copy = blockIdx.y, listed locus): with lo = thr - 0.005 - 1e-6 and hi = thr - 0.005 + 1e-6 (made once on
//                  the host, passed by value)
//                    CALLED  status 0, not bi-allelic, cand[0].allele == alt, cand[0].pi > hi
//                    NOT     status 0, not bi-allelic, and cand[0].allele != alt or cand[0].pi < lo
//                    HOST    everything else: a bi-allelic row (rows._head_and_filter chooses the candidate with the genome in hand),
//                            a status that is not 0, a PI inside [lo, hi] or NaN - py2's round decides there.
//                  The lane writes one 16-byte record (PI, VMT, and the used MT below the verdict's two bits) with one vector
//                  store, and a HOST lane appends its record's index (copy * G + listed locus) to a list through one atomic cursor:
//                  the host downloads those rows only.  The list's ORDER is that of the atomics - not fixed from call to call; its
//                  CONTENT is.  Nothing else is written.
// Once per called batch, G x B lanes: not on the per-locus hot path.  The gathers are scattered (five dwords of a 432-byte row per
// lane), which at a few thousand lanes is nothing beside the batch's build.
#define SCD_BLOCK 256

// The member rule, shared by k_scan_detect and k_scan_detect_sets: the record of (copy c, listed locus L) and its verdict.
__device__ __forceinline__ uint32_t scd_member(const smc_row* __restrict__ rows, uint32_t n_loci, uint32_t c, const smc_scan_locus L,
                                               double lo, double hi, smc_scan_verdict& rec) {
    const smc_row* const r = rows + ((size_t)c * n_loci + L.offset);          // (the host checked offset < n_loci on its copy)
    const int32_t status = r->status, bi = r->biallelic, used = r->used_mt;
    const int32_t allele = r->cand[0].allele, vmt = r->cand[0].vmt;
    const double pi = r->cand[0].pi;
    uint32_t v = SMC_SCAN_HOST;
    if (status == 0 && bi == 0) {
        if (allele != (int32_t)L.alt || pi < lo) v = SMC_SCAN_NOT;
        else if (pi > hi) v = SMC_SCAN_CALLED;
    }
    rec.pi = pi;
    rec.vmt = vmt;
    rec.mt_verdict = (v << 30) | (uint32_t)min(max(used, 0), (int32_t)SMC_SCAN_MT_MASK);
    return v;
}

__global__ __launch_bounds__(SCD_BLOCK) void k_scan_detect(const smc_row* __restrict__ rows, uint32_t n_loci,
                                                           const smc_scan_locus* __restrict__ listed, uint32_t n_listed, double lo, double hi,
                                                           smc_scan_verdict* __restrict__ out, uint32_t* __restrict__ host_list,
                                                           uint32_t* __restrict__ n_host) {
    const uint32_t c = blockIdx.y;
    for (uint32_t g = blockIdx.x * SCD_BLOCK + threadIdx.x; g < n_listed; g += gridDim.x * SCD_BLOCK) {
        const uint32_t idx = c * n_listed + g;
        smc_scan_verdict rec;
        const uint32_t v = scd_member(rows, n_loci, c, listed[g], lo, hi, rec);
        out[idx] = rec;
        if (v == SMC_SCAN_HOST) host_list[atomicAdd(n_host, 1u)] = idx;       // (at most n_copies * n_listed appends: the list's size)
    }
}

// ------------------------------------------------------------------------------------------
// --spikeScanMnv: the verdicts of phase SETS - an MNV is called when every member SNV is (smc_scan_detect_sets)
// ------------------------------------------------------------------------------------------
// The listed records are tiled by sets: set s holds the records set_off[s] .. set_off[s + 1] - 1, one to SMC_SPIKE_PHASE_MAX_MEMBERS
// (= 8) of them - the host checked both on its copy.
//   k_scan_detect_sets  a group of eight neighbouring lanes per (copy = blockIdx.y, set): lane m of the group takes member m with
//                  scd_member - so the up to eight scattered row gathers of a set are in flight together, not behind one another in
//                  one lane - and writes its 16-byte record exactly as k_scan_detect does.  Each lane makes a word with its bit m in
//                  byte 0 (CALLED), 1 (HOST) or 2 (NOT); three xor-shuffles OR the eight words (a group never straddles a wavefront:
//                  eight divides 64, and every lane of the wavefront runs every round - the loop's bound is the workgroup's).  The
//                  joint verdict - NOT when any member is NOT, else HOST when any is HOST, else CALLED - goes into bits 31..30 above
//                  the three bytes, written by lane 0 of the group with one vector store.  The HOST members append their record's
//                  index to the list ONLY when the joint verdict is HOST: beside a NOT member a HOST member decides nothing.
// Nothing else is written.  The list's ORDER is that of the atomics; its CONTENT is fixed.
#define SCD_SET_LANES 8

__global__ __launch_bounds__(SCD_BLOCK) void k_scan_detect_sets(const smc_row* __restrict__ rows, uint32_t n_loci,
                                                                const smc_scan_locus* __restrict__ listed, uint32_t n_listed,
                                                                const uint32_t* __restrict__ set_off, uint32_t n_sets, double lo, double hi,
                                                                smc_scan_verdict* __restrict__ out, uint32_t* __restrict__ joint,
                                                                uint32_t* __restrict__ host_list, uint32_t* __restrict__ n_host) {
    const uint32_t c = blockIdx.y, m = threadIdx.x & (SCD_SET_LANES - 1);
    const uint32_t per_block = SCD_BLOCK / SCD_SET_LANES;
    for (uint32_t s0 = blockIdx.x * per_block; s0 < n_sets; s0 += gridDim.x * per_block) {       // (uniform over the workgroup)
        const uint32_t s = s0 + threadIdx.x / SCD_SET_LANES;
        uint32_t w = 0, v = SMC_SCAN_NOT, idx = 0;
        bool mine = false;
        if (s < n_sets) {
            const uint32_t first = set_off[s], size = set_off[s + 1] - first;
            mine = m < size;
            if (mine) {
                const uint32_t g = first + m;                                  // (below n_listed: the offsets tile the records)
                idx = c * n_listed + g;
                smc_scan_verdict rec;
                v = scd_member(rows, n_loci, c, listed[g], lo, hi, rec);
                out[idx] = rec;
                w = 1u << (m + (v == SMC_SCAN_CALLED ? 0u : v == SMC_SCAN_HOST ? 8u : 16u));
            }
        }
        w |= __shfl_xor(w, 1);
        w |= __shfl_xor(w, 2);
        w |= __shfl_xor(w, 4);
        const uint32_t jv = (w & 0xFF0000u) ? SMC_SCAN_NOT : (w & 0xFF00u) ? SMC_SCAN_HOST : SMC_SCAN_CALLED;
        if (s < n_sets && m == 0) joint[c * n_sets + s] = (jv << 30) | w;
        if (mine && v == SMC_SCAN_HOST && jv == SMC_SCAN_HOST)
            host_list[atomicAdd(n_host, 1u)] = idx;                            // (at most n_copies * n_listed appends: the list's size)
    }
}

// ------------------------------------------------------------------------------------------
// --spikeScanIndel: the same verdict when the planted variant is an allele KEY (smc_scan_detect_keys)
// ------------------------------------------------------------------------------------------
// An insertion's or a deletion's allele id is not fixed: the builder numbers the keys a locus meets 6 and up, per build, in the order
// it meets them, and leaves one extras entry (locus, allele id, alignment, query position, indel) per such key - the alignment is the
// one whose text the host would print as the key (smc_bam_allele_key).  A pass's copies are built one behind the other, each leaving
// its extras list in a region of its own; per called batch
//   k_sdk_init     a lane per (copy = blockIdx.y, listed variant): an SNV's id is its letter's fixed id, a key's SMC_SCAN_ID_NONE;
//   k_sdk_resolve  a lane per extras entry of copy blockIdx.y (the count clipped to xcap): the listed variants of the entry's locus by
//                  a lower-bound search over the ascending `locus` fields, then af_shows' rule on the COPY's record and pairs - the
//                  anchor letter the variant's; a deletion: indel == -len; an insertion: the inserted letters, clamped at the read's
//                  end as the host's slice clamps them, the pool's.  (The entry holds the query position and the indel the walk
//                  resolved: the CIGAR is not walked again.)  A match puts the entry's id into the slot by compare-and-swap; a slot
//                  that was taken already - two entries show the key: must not happen -, or an entry whose record cannot be read
//                  (an alignment beyond n_aln, a query position beyond l_seq, pairs beyond cap_pairs), gets SMC_SCAN_ID_HOST, which
//                  nothing replaces: the slot's end state does not depend on the order of the lanes;
//   k_sdk_detect   k_scan_detect with cand[0].allele == the slot's id: SMC_SCAN_ID_NONE - nobody shows the key in that copy - is NOT
//                  on a row that is otherwise decidable, SMC_SCAN_ID_HOST is HOST.
// Three launches behind one another on the stream, once per called batch; the extras of a copy are a few entries per locus next to an
// indel and none elsewhere, so the resolve pass is a few thousand lanes.  A lane per entry (not a lane per (copy, listed variant) that
// walks the copy's list): the lists are unsorted, and a walk per listed variant would read every list G times.
struct SdkCopies {
    const uint8_t* aln; unsigned long long aln_stride;          // copy c's records at aln + c * aln_stride (bytes)
    const uint8_t* bq; unsigned long long bq_stride;            // ... its (letter, quality) pairs
    uint32_t n_aln; unsigned long long cap_pairs;
    const uint32_t* x; unsigned long long x_stride;             // ... its extras entries at x + c * x_stride (words)
    const uint32_t* xcount; unsigned long long xcount_stride;   // ... their number at xcount[c * xcount_stride]
    uint32_t xcap;
};

__device__ __forceinline__ uint32_t sdk_letter_id(uint32_t letter) {                 // (pileup.BASE_ALLELES: A, T, G, C = 0 .. 3)
    return letter == 'A' ? 0u : letter == 'T' ? 1u : letter == 'G' ? 2u : 3u;
}

__global__ __launch_bounds__(SCD_BLOCK) void k_sdk_init(const smc_af_variant* __restrict__ var, uint32_t n_listed, uint32_t* __restrict__ alt_id) {
    const uint32_t c = blockIdx.y;
    for (uint32_t g = blockIdx.x * SCD_BLOCK + threadIdx.x; g < n_listed; g += gridDim.x * SCD_BLOCK) {
        const smc_af_variant V = var[g];
        alt_id[(size_t)c * n_listed + g] = V.kind == SMC_AF_SNV ? sdk_letter_id(V.letter) : SMC_SCAN_ID_NONE;
    }
}

__global__ __launch_bounds__(SCD_BLOCK) void k_sdk_resolve(SdkCopies C, const smc_af_variant* __restrict__ var, uint32_t n_listed,
                                                           const uint8_t* __restrict__ ins, uint32_t* __restrict__ alt_id) {
    const uint32_t c = blockIdx.y;
    const uint32_t n = min(C.xcount[(size_t)c * C.xcount_stride], C.xcap);
    const uint32_t* const x = C.x + (size_t)c * C.x_stride;
    const smc_dev_aln* const aln = (const smc_dev_aln*)(C.aln + (size_t)c * C.aln_stride);
    const uint8_t* const bq = C.bq + (size_t)c * C.bq_stride;
    for (uint32_t e = blockIdx.x * SCD_BLOCK + threadIdx.x; e < n; e += gridDim.x * SCD_BLOCK) {
        const uint32_t l = x[5ull * e], aid = x[5ull * e + 1], ai = x[5ull * e + 2], qpos = x[5ull * e + 3];
        const int32_t indel = (int32_t)x[5ull * e + 4];
        uint32_t g = 0, hi = n_listed;
        while (g < hi) {
            const uint32_t mid = g + (hi - g) / 2;
            if (var[mid].locus < l) g = mid + 1; else hi = mid;
        }
        for (; g < n_listed; ++g) {
            const smc_af_variant V = var[g];
            if (V.locus != l) break;
            if (V.kind != SMC_AF_INS && V.kind != SMC_AF_DEL) continue;
            uint32_t* const slot = alt_id + (size_t)c * n_listed + g;
            bool bad = ai >= C.n_aln, shows = false;
            if (!bad) {
                const smc_dev_aln a = aln[ai];
                bad = qpos >= (uint32_t)a.l_seq || (unsigned long long)a.seq_off + a.l_seq > C.cap_pairs;
                if (!bad) {
                    const uint8_t* const s = bq + 2ull * a.seq_off;                   // (the letter of base k: byte 2k)
                    if ((uint32_t)s[2ull * qpos] == V.letter) {
                        if (V.kind == SMC_AF_DEL) {
                            shows = indel < 0 && (0u - (uint32_t)indel) == V.len;
                        } else if (indel > 0) {
                            // the inserted letters as the host's slice clamps them: query [qpos + 1, min(l_seq, qpos + 1 + indel))
                            const uint32_t k_max = min((uint32_t)a.l_seq - (qpos + 1u), (uint32_t)indel);
                            shows = k_max == V.len;
                            for (uint32_t k = 0; shows && k < k_max; ++k) shows = s[2ull * (qpos + 1u + k)] == ins[V.ins_off + k];
                        }
                    }
                }
            }
            if (bad) atomicExch(slot, SMC_SCAN_ID_HOST);
            else if (shows && atomicCAS(slot, SMC_SCAN_ID_NONE, aid) != SMC_SCAN_ID_NONE) atomicExch(slot, SMC_SCAN_ID_HOST);
        }
    }
}

__global__ __launch_bounds__(SCD_BLOCK) void k_sdk_detect(const smc_row* __restrict__ rows, uint32_t n_loci,
                                                          const smc_af_variant* __restrict__ var, uint32_t n_listed,
                                                          const uint32_t* __restrict__ alt_id, double lo, double hi,
                                                          smc_scan_verdict* __restrict__ out, uint32_t* __restrict__ host_list,
                                                          uint32_t* __restrict__ n_host) {
    const uint32_t c = blockIdx.y;
    for (uint32_t g = blockIdx.x * SCD_BLOCK + threadIdx.x; g < n_listed; g += gridDim.x * SCD_BLOCK) {
        const uint32_t idx = c * n_listed + g;
        const uint32_t id = alt_id[idx];
        const smc_row* const r = rows + ((size_t)c * n_loci + var[g].locus);  // (the host checked locus < n_loci on its copy)
        const int32_t status = r->status, bi = r->biallelic, used = r->used_mt;
        const int32_t allele = r->cand[0].allele, vmt = r->cand[0].vmt;
        const double pi = r->cand[0].pi;
        uint32_t v = SMC_SCAN_HOST;
        if (id != SMC_SCAN_ID_HOST && status == 0 && bi == 0) {
            if (id == SMC_SCAN_ID_NONE || (uint32_t)allele != id || pi < lo) v = SMC_SCAN_NOT;
            else if (pi > hi) v = SMC_SCAN_CALLED;
        }
        smc_scan_verdict rec;
        rec.pi = pi;
        rec.vmt = vmt;
        rec.mt_verdict = (v << 30) | (uint32_t)min(max(used, 0), (int32_t)SMC_SCAN_MT_MASK);
        out[idx] = rec;
        if (v == SMC_SCAN_HOST) host_list[atomicAdd(n_host, 1u)] = idx;       // (at most n_copies * n_listed appends: the list's size)
    }
}

// ------------------------------------------------------------------------------------------
// --spikeScanFilter: the FILTER column of a listed locus's row as a word of bits (smc_scan_filter)
// ------------------------------------------------------------------------------------------
// What the user of a run acts on is a .cut row whose FILTER is PASS.  Of the 14 names the column can hold, eight are decided by
// k_filter_loci and stand in cand.flt; HP and LowC need the genome (rows.filter_string), the repeat names the run's BEDs
// (postfilter._apply_one) - but for the variant a pass PLANTED at the locus those depend on chromosome, position, REF, ALT and the
// files alone: constants of the listed variant, made once on the host as two words
//     gate     SMC_F_HP and / or SMC_F_LOWC of hpregion.is_hp_or_lowcomp - they apply where filterVariants ran and cand.vmf_lt_099;
//     always   the repeat names of the position (bits 10 .. 13, and SMC_F_LOWC for RepeatMasker's Low_complexity) - they apply where
//              int(float(py2 round(PI, 2))) >= 5, filterVariants or not: PI > 4.995 outside a band of 1e-6 that py2's round decides.
//   k_scan_filter  a lane per (copy = blockIdx.y, listed locus), from cand[0] alone: the word with one vector store, bit 31
//                  (SMC_SCAN_FLT_HOST) where the host has to print the row - a status that is not 0, a bi-allelic row (the candidate
//                  printed is chosen with the genome in hand), PI NaN or inside the band, flt_applied neither 0 nor 1.
// The host reads a word only where the detect call's verdict is CALLED (cand[0] is the planted variant there).  Nothing but `out`
// is written; the verdict records are neither read nor written.  Once per called batch, G x B lanes.
// The member rule, shared by k_scan_filter and k_scan_filter_sets: the word of (copy c, listed locus g).
__device__ __forceinline__ uint32_t scf_member(const smc_row* __restrict__ rows, uint32_t n_loci, uint32_t c, uint32_t offset, uint32_t gate,
                                               uint32_t always, double lo, double hi) {
    const smc_row* const r = rows + ((size_t)c * n_loci + offset);            // (the host checked the offset < n_loci on its copy)
    const int32_t status = r->status, bi = r->biallelic;
    const int32_t applied = r->cand[0].flt_applied, below = r->cand[0].vmf_lt_099;
    const uint32_t flt = r->cand[0].flt;
    const double pi = r->cand[0].pi;
    uint32_t w = 0;
    if (applied != 0) w = (flt & SMC_SCAN_FLT_DEVICE_MASK) | (below != 0 ? gate : 0u);
    if (pi > hi) w |= always;
    if (status != 0 || bi != 0 || !(pi < lo || pi > hi) || (applied != 0 && applied != 1)) w |= SMC_SCAN_FLT_HOST;
    return w;
}

__global__ __launch_bounds__(SCD_BLOCK) void k_scan_filter(const smc_row* __restrict__ rows, uint32_t n_loci,
                                                           const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ gate,
                                                           const uint32_t* __restrict__ always, uint32_t n_listed, double lo, double hi,
                                                           uint32_t* __restrict__ out) {
    const uint32_t c = blockIdx.y;
    for (uint32_t g = blockIdx.x * SCD_BLOCK + threadIdx.x; g < n_listed; g += gridDim.x * SCD_BLOCK)
        out[(size_t)c * n_listed + g] = scf_member(rows, n_loci, c, offsets[g], gate[g], always[g], lo, hi);
}

// ------------------------------------------------------------------------------------------
// --spikeScanMnvFilter: the FILTER of phase SETS - an MNV is PASS when every member SNV's row is (smc_scan_filter_sets)
// ------------------------------------------------------------------------------------------
// The listed loci are tiled by sets as k_scan_detect_sets takes them (the host checked the offsets on its copy).
//   k_scan_filter_sets  k_scan_detect_sets' geometry: a group of SCD_SET_LANES neighbouring lanes per (copy = blockIdx.y, set), lane m
//                  takes member m with scf_member - the set's scattered row gathers are in flight together - and writes its word
//                  exactly as k_scan_filter does.  Each lane makes a word of its name bits, its bit 31, and bit 16 + m where it has a
//                  name bit (member m is not PASS); three xor-shuffles OR the eight words (the loop's bound is the workgroup's: every
//                  lane of the wavefront runs every round), and lane 0 of the group writes the joint word with one vector store.
// No atomics and no list: the host finds the sets it has to print from the joint words' bit 31 themselves.  Nothing but the two
// outputs is written.  Once per called batch, 8 x sets x B lanes: launch latency, not a hot loop - what it buys is that four bytes per
// (copy, set) come down and not four per member, and that the joint rule has one home.
__global__ __launch_bounds__(SCD_BLOCK) void k_scan_filter_sets(const smc_row* __restrict__ rows, uint32_t n_loci,
                                                                const uint32_t* __restrict__ offsets, const uint32_t* __restrict__ gate,
                                                                const uint32_t* __restrict__ always, uint32_t n_listed,
                                                                const uint32_t* __restrict__ set_off, uint32_t n_sets, double lo, double hi,
                                                                uint32_t* __restrict__ members, uint32_t* __restrict__ joint) {
    const uint32_t c = blockIdx.y, m = threadIdx.x & (SCD_SET_LANES - 1);
    const uint32_t per_block = SCD_BLOCK / SCD_SET_LANES;
    for (uint32_t s0 = blockIdx.x * per_block; s0 < n_sets; s0 += gridDim.x * per_block) {       // (uniform over the workgroup)
        const uint32_t s = s0 + threadIdx.x / SCD_SET_LANES;
        uint32_t w = 0;
        if (s < n_sets) {
            const uint32_t first = set_off[s], size = set_off[s + 1] - first;
            if (m < size) {
                const uint32_t g = first + m;                                  // (below n_listed: the offsets tile the listed loci)
                const uint32_t mw = scf_member(rows, n_loci, c, offsets[g], gate[g], always[g], lo, hi);
                members[(size_t)c * n_listed + g] = mw;
                w = (mw & (SMC_SCAN_FLT_NAMES_MASK | SMC_SCAN_FLT_HOST)) | ((mw & SMC_SCAN_FLT_NAMES_MASK) ? 1u << (SMC_SCAN_FLT_MEMBER_SHIFT + m) : 0u);
            }
        }
        w |= __shfl_xor(w, 1);
        w |= __shfl_xor(w, 2);
        w |= __shfl_xor(w, 4);
        if (s < n_sets && m == 0) joint[(size_t)c * n_sets + s] = w;
    }
}
