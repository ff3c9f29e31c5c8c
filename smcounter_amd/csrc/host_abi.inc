// Included by smcounter_hip.hip.
// ------------------------------------------------------------------------------------------
// host side: C ABI
// ------------------------------------------------------------------------------------------
// Environment switches of this library are EXPERIMENT knobs (measurements, tests, A/B runs: README.md lists them): they are read
// only when SMC_EXPERIMENTAL is set (to anything but 0) - a stray variable in a production environment changes nothing - and the
// first one that is set without it is named on stderr, once.
static const char* exp_env(const char* name) {
    const char* const xv = getenv("SMC_EXPERIMENTAL");
    const bool on = xv && *xv && strcmp(xv, "0") != 0;                             // (looked at every time: tests switch it on and off)
    const char* v = getenv(name);
    if (v && !on) {
        static bool told = false;
        if (!told) { told = true; fprintf(stderr, "smcounter_hip: %s is set but SMC_EXPERIMENTAL is not: experiment switches are ignored\n", name); }
        return nullptr;
    }
    return v;
}
static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x)                                                                                   \
    do {                                                                                            \
        hipError_t e_ = (x);                                                                        \
        if (e_ != hipSuccess)                                                                       \
            return fail(SMC_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_));                 \
    } while (0)

struct smc_ctx {
    int device;
    // scratch of smc_build_planes, grown on demand: the segment table, sort buffers, per-part counts, the extras lists
    void* bp_scratch = nullptr;
    size_t bp_bytes = 0;
    hipEvent_t bp_done_ev = nullptr;          // behind the last kernel of the last smc_build_planes: the next build, on whatever stream, waits for it (one scratch)
    // scratch of smc_select_alignments (block counts / offsets, the blocks' largest ends, the difference array), grown on demand
    void* sel_scratch = nullptr;
    size_t sel_bytes = 0;
    // scratch of smc_lod_table (roots, then iteration counts), grown on demand
    void* lod_scratch = nullptr;
    size_t lod_bytes = 0;
    // scratch of smc_allele_carriers (the counters of a call that does not ask for them), grown on demand
    void* af_scratch = nullptr;
    size_t af_bytes = 0;
    // scratch of smc_spike_indels (per alignment the relocated sizes, per workgroup their sums), grown on demand
    void* spi_scratch = nullptr;
    size_t spi_bytes = 0;
    // scratch of smc_build_listed (the loci's sort buffers, orders and head marks, per-locus status and extras), grown on demand
    void* bl_scratch = nullptr;
    size_t bl_bytes = 0;
    hipEvent_t bl_done_ev = nullptr;          // behind the last kernel of the last smc_build_listed (one scratch: as bp_done_ev)
    // scratch of the checking entries smc_fisher_tables / smc_lfact_values (arguments, then results), grown on demand
    void* chk_scratch = nullptr;
    size_t chk_bytes = 0;
    // the segment table of a build travels from page-locked memory (a copy from pageable memory blocks the host until the stream has
    // drained): a small ring, an entry reused once the copy that read it has run (its event)
    struct SegStage { void* host = nullptr; size_t cap = 0; hipEvent_t ev = nullptr; bool used = false; };
    SegStage seg_stage[4];
    int seg_next = 0;
    std::vector<hipEvent_t> bp_ev0, bp_ev1;   // optional timing of the plane-writing walk (smc_build_set_timing)
    int64_t bp_timed = 0;
    size_t bp_nlive_off = 0;                  // the last build's per-list live row counts in bp_scratch, and how many lists (smc_build_live_rows)
    int32_t bp_nlive_n = 0;
    // device blocks of destroyed plans, kept for the next plan (a plan per batch allocates and frees half a dozen lists: every
    // hipFree synchronises the device - 0.3 ms between two steps of the from_alignments run); size class -> blocks
    std::vector<std::pair<size_t, void*>> plan_pool;
    struct PendingFree { hipEvent_t ev; std::vector<std::pair<size_t, void*>> blocks; };
    std::vector<PendingFree> plan_pending;   // blocks of destroyed plans whose last run may still be in flight (its event)
    void* plan_stats = nullptr;   // smc_plan_create_dev: PlanStats on the device, its page-locked mirror, the deep-locus list
    void* plan_stats_host = nullptr;
    bool plan_stats_clean = false;   // the last k_plan_fill has been launched: it leaves the record zeroed
    hipEvent_t plan_fill_ev = nullptr;   // behind that launch: the next plan's kernels wait for it, whatever stream they are on
    void* plan_deep = nullptr;
    size_t plan_deep_cap = 0;
    // what the next plan made without the host is sized from: the record of the last plan that was made the exact way or has been
    // checked (smc_plan_spec_ok), and how many loci it had; page-locked blocks for the records of such plans
    bool hint_ok = false;
    int64_t hint_loci = 0;
    PlanStats hint_stats;
    uint32_t* d_spec_fail = nullptr;  // device counter: plans made without the host whose batch did not fit (k_plan_fill_spec)
    std::vector<void*> spec_host_free;
    int64_t spec_made = 0, spec_failed = 0, spec_exact = 0;
    // large allocations of smc_mem_alloc: a virtual range backed by physical handles of SMC_VMM_CHUNK_MB each (see smc_mem_alloc)
    struct VmmBlock { void* va; size_t total; std::vector<hipMemGenericAllocationHandle_t> handles; };   // (handles: kept until the unmap)
    std::vector<VmmBlock> vmm;
    std::mutex vmm_mu;
    double* lut;   // 10^(-q/10), q = 0..255
    double* simple; // [SMC_SIMPLE_N][2]: -log10(1 - posterior) of a one-allele barcode by fragment count
    double* pcr;    // [SMC_PCR_N][SMC_PCR_N]: PCR-error term by (fragments of the barcode, count of the allele)
    double* lfact = nullptr;  // [SMC_LFACT_N]: log(n!) for the Fisher tests of k_filter_loci
    int max_lds;   // bytes of LDS a workgroup may use
    int n_cu = 256; // compute units of the device
};

// A scratch buffer of the context, grown on demand: `need` bytes are used now; where it has fewer, `want` (need plus the entry's
// margin) are allocated.  `sync`: the stream to wait for before the old block goes - the entry's earlier kernels on it may still
// use the block; null: the entry waits for its own kernels before it returns (and hipFree synchronises the device).
static int grow_scratch(void*& ptr, size_t& have, size_t need, size_t want, const char* who, const hipStream_t* sync) {
    if (need <= have) return SMC_OK;
    if (sync) { const hipStream_t st = *sync; HIPCHK(hipStreamSynchronize(st)); }
    (void)hipFree(ptr);
    ptr = nullptr; have = 0;
    hipError_t e = hipMalloc(&ptr, want);
    if (e != hipSuccess) return fail(SMC_E_HIP, std::string(who) + ": " + std::to_string(want) + " bytes of scratch: " + hipGetErrorString(e));
    have = want;
    return SMC_OK;
}

// size classes of the pool: powers of two up to 256 MB, multiples of 64 MB beyond (a 12 GB block is not rounded to 16)
static size_t plan_size_class(size_t bytes) {
    if (bytes > ((size_t)256 << 20)) return (bytes + ((size_t)64 << 20) - 1) & ~(((size_t)64 << 20) - 1);
    size_t c = 256;
    while (c < bytes) c <<= 1;
    return c;
}
// a block of at least `bytes` for a plan: from the context's pool when one of the size class waits there
#define SMC_POOL_BLOCKS 64
#define SMC_POOL_BYTES ((size_t)8 << 30)
static void plan_pool_put(smc_ctx* ctx, size_t cls, void* p) {
    if (cls > ((size_t)1 << 30)) { (void)hipFree(p); return; }
    // bounded in blocks and in bytes; when full the OLDEST block goes (a pool filled with size classes nobody asks for again would
    // otherwise turn every later return into a hipFree - the device-wide synchronisation the pool exists to avoid - ADVICE r3)
    size_t held = cls;
    for (auto& b : ctx->plan_pool) held += b.first;
    while (!ctx->plan_pool.empty() && (ctx->plan_pool.size() >= SMC_POOL_BLOCKS || held > SMC_POOL_BYTES)) {
        held -= ctx->plan_pool.front().first;
        (void)hipFree(ctx->plan_pool.front().second);
        ctx->plan_pool.erase(ctx->plan_pool.begin());
    }
    ctx->plan_pool.emplace_back(cls, p);
}
// blocks whose plan's last run has finished move to the pool; `all`: wait for the runs
static void plan_pool_collect(smc_ctx* ctx, bool all) {
    for (size_t i = 0; i < ctx->plan_pending.size();) {
        auto& q = ctx->plan_pending[i];
        if (all || ctx->plan_pending.size() > 16) (void)hipEventSynchronize(q.ev);
        else if (hipEventQuery(q.ev) != hipSuccess) { ++i; continue; }
        for (auto& b : q.blocks) plan_pool_put(ctx, b.first, b.second);
        (void)hipEventDestroy(q.ev);
        ctx->plan_pending.erase(ctx->plan_pending.begin() + (long)i);
    }
}
static hipError_t plan_alloc(smc_ctx* ctx, void** out, size_t bytes) {
    const size_t cls = plan_size_class(bytes);
    plan_pool_collect(ctx, false);
    hipError_t e = hipErrorOutOfMemory;
    for (size_t i = 0; i < ctx->plan_pool.size(); ++i)
        if (ctx->plan_pool[i].first == cls) { *out = ctx->plan_pool[i].second; ctx->plan_pool.erase(ctx->plan_pool.begin() + (long)i); e = hipSuccess; break; }
    if (e != hipSuccess) e = hipMalloc(out, cls);
    // (debugging and tests: SMC_PLAN_POISON=<byte> fills every block a plan takes - the lists, the deep class's scratch - before
    // use: a recycled block is not zero, and nothing may depend on what it held)
    if (e == hipSuccess) if (const char* v = exp_env("SMC_PLAN_POISON")) {
        (void)hipDeviceSynchronize();                                  // (the fill must not race the streams the plan's kernels run on)
        e = hipMemset(*out, atoi(v) & 0xFF, cls);
        if (e == hipSuccess) e = hipDeviceSynchronize();
    }
    return e;
}

static size_t host_hdr_bytes(int a_cap) {
    return sizeof(Hdr) + (size_t)a_cap * SMC_NT * 4 + (size_t)a_cap * 8 + (size_t)a_cap * 4 + (size_t)a_cap * 4 + 128 * 8 + 32 * 8;
}
// LDS a locus needs when one workgroup takes it whole, in one chunk: header + one flag dword per
// quad (+ 2: the quad before the first read's and the one behind the last) + 9 bytes per barcode (first read, queue,
// counts, kept-key flag)
static size_t whole_locus_lds(const smc_locus& L, int a_cap) {
    return host_hdr_bytes(a_cap) + 4 * (((size_t)L.n_reads + 3) / 4 + 2) + 9 * (size_t)L.n_umi + 32;
}
// LDS of a workgroup of a bin whose tables hold fcap flag dwords and ucap barcodes (a whole-locus class's largest locus, or the
// deep class's chunk), in units of 256 bytes
static size_t bin_lds_bytes(int a_cap, size_t fcap, size_t ucap) { return (host_hdr_bytes(a_cap) + 4 * fcap + 9 * ucap + 32 + 255) & ~(size_t)255; }

// Workgroup size by locus size: the smallest block that still keeps the CU's SIMDs busy while the locus's reads stream
// - small blocks pay less for the barriers between phases and for the parts one wavefront runs alone.  Thresholds
// (reads per locus) tunable at build time for experiments.
#ifndef SMC_R0
#define SMC_R0 4096       // <= : 64 threads (one wavefront: no barrier waits, no idle wave)
#endif
#ifndef SMC_R1
#define SMC_R1 8192       // <= : 128 (C5, 7980 reads: 0.48 ms per 20 k loci here, 0.58 with 256 threads)
#endif
#ifndef SMC_R2
#define SMC_R2 12288      // <= : 256
#endif
#ifndef SMC_R3
#define SMC_R3 24576      // <= : 512; above: the deep class
#endif
// Deep loci: several workgroups per locus ("parts": shares of its barcodes), each taking its share in chunks of whole
// barcodes that fit a fixed LDS budget; the parts add their headers into a global accumulator and the last one ranks.
#ifndef SMC_DEEP_BLOCK
#define SMC_DEEP_BLOCK 512
#endif
#ifndef SMC_DEEP_FCAP
#define SMC_DEEP_FCAP 5376       // flag dwords per chunk (21.5 k reads: a part's share plus slack)
#endif
#ifndef SMC_DEEP_UCAP
#define SMC_DEEP_UCAP 2560       // barcodes per chunk
#endif
#ifndef SMC_DEEP_PART_READS
#define SMC_DEEP_PART_READS 20480 // reads a part should get at most (its share of the barcodes; one chunk)
#endif
#define SMC_CLS_DEEP 4

struct Bin {
    int cls;              // 0: 64 threads, 1: 128, 2: 256, 3: 512 (whole locus, one chunk), 4: deep (parts x chunks)
    int a_cap = 8;
    int fcap = 0, ucap = 0;
    size_t lds_bytes = 0;
    std::vector<int> order;            // loci of the bin, heaviest first
    std::vector<V2Part> parts;         // one per workgroup (host-made plans; empty when the list was written on the device)
    size_t n_parts = 0;                // workgroups of the launch
    V2Part* d_parts = nullptr;
    smc_locus* d_desc = nullptr;       // the loci's descriptors once more, in launch order: one per workgroup (no load that depends on a
                                       // load at the head of every workgroup)
    size_t desc_bytes = 0;
    int64_t* d_flags_off = nullptr;    // deep: per workgroup, dword offset of its locus's flag scratch (+ 2 * part)
    uint32_t* d_flags = nullptr;       // deep: 1 byte per read of scratch for a barcode larger than a chunk
    uint32_t* d_acc = nullptr;         // deep: one accumulator per multi-part locus
    size_t acc_bytes = 0, flags_bytes = 0, parts_bytes = 0, foff_bytes = 0;
    int64_t reads = 0;
    const uint32_t* d_launch_n = nullptr;   // a plan made without the host: the workgroups of the launch that have work (n_parts is an upper bound)
};

struct smc_plan {
    smc_ctx* ctx;
    int64_t n_loci;
    smc_locus* d_loci = nullptr;
    bool own_loci = true;             // false: the caller's device array (smc_plan_create_dev)
    uint32_t* d_flt_list = nullptr;   // [0] = count, then locus indices queued for k_filter_loci
    uint16_t fp = 0;                  // smc_param_fingerprint the batch was built with (smc_locus.flags bits 1-15)
    int64_t need_quads = 0;           // quads of read words the batch's loci span (max over loci of read_off4 + quads of the locus)
    hipEvent_t done_ev = nullptr;     // recorded behind the last run's launches: when the plan's device blocks may be reused
    bool flt_clean = false;           // both worklists' counts are known to be zero where the next run needs them (see smc_plan_run_words)
    int flt_parity = 0;               // which of the two worklists the next run uses
    size_t loci_bytes = 0, flt_bytes = 0, words_bytes = 0;
    uint32_t* d_words = nullptr;      // smc_plan_run (raw-field planes in): the read words packed from them, kept for the next run
    std::vector<Bin> bins;
    // optional HIP-event timing of the dominant k_call_v2 launch (the bin with most reads)
    int timing = 0, dom_bin = -1;
    int64_t dom_loci = 0, dom_reads = 0;
    std::vector<hipEvent_t> ev0, ev1;   // ring of event pairs, one per timed run
    int64_t n_timed = 0;
    // a plan made without the host in the loop (smc_plan_create_dev_spec): what its launches were sized for, the record
    // k_plan_classify summed (a copy in page-locked memory, valid once the plan's stream has been synchronised), its device record
    bool spec = false;
    PlanCaps caps;
    void* spec_host = nullptr;        // PlanStats, page-locked (the context's free list)
    PlanSpec* d_spec = nullptr;
    int spec_checked = -1;            // -1: not looked at yet; else the verdict
};

// ---- making a plan: what smc_plan_create (from host descriptors), smc_plan_create_dev (classified on the device, waits for the record)
// and smc_plan_create_dev_spec (sized from the last plan, waits for nothing) share
// The classes' thresholds and the deep class's geometry.  (Experiments and tests: the geometry and its threshold can be overridden
// when the plan is made - the environment is read on every call: tests switch the knobs on and off in one process.)
static PlanCfg plan_cfg_from_env(int& deep_fcap) {
    auto env_int = [](const char* name, int dflt) { const char* v = exp_env(name); return v && *v ? atoi(v) : dflt; };
    PlanCfg C;
    C.cls_reads[0] = SMC_R0; C.cls_reads[1] = SMC_R1; C.cls_reads[2] = SMC_R2; C.cls_reads[3] = SMC_R3;
    C.deep_from = env_int("SMC_DEEP_FROM_READS", SMC_R3);                  // more reads than this: the deep class
    // reads per locus: 2^24 (the limits are the 27-bit slot field and memory; pysam's max_depth in the reference is 10^6)
    C.max_reads = 1 << 24;
    deep_fcap = std::max(8, env_int("SMC_DEEP_FCAP", SMC_DEEP_FCAP));
    C.deep_ucap = std::min(32767, std::max(1, env_int("SMC_DEEP_UCAP", SMC_DEEP_UCAP)));   // (15-bit queue entries)
    C.deep_part_reads = std::max(64, env_int("SMC_DEEP_PART_READS", SMC_DEEP_PART_READS));
    return C;
}

// A plan under construction and the bins being filled, one per class.  Every failure after `new smc_plan()` goes through fail():
// the blocks the bins hold by then are handed to the plan first, so that smc_plan_destroy returns them to the pool with the plan's
// own (ADVICE r3) - no exit leaves the plan or a pooled block behind.
struct PlanBuild {
    smc_plan* p;
    Bin bins[5];
    PlanBuild(smc_ctx* ctx, int64_t n_loci) : p(new smc_plan()) {
        p->ctx = ctx; p->n_loci = n_loci;
        for (int c = 0; c < 5; ++c) bins[c].cls = c;
    }
    int fail(int code, const std::string& msg) {
        for (auto& b : bins) p->bins.push_back(b);
        smc_plan_destroy(p);
        return ::fail(code, msg);
    }
    // the bins that have a launch go to the plan, in class order, with their LDS sizes; a bin handed over is cleared here: fail()
    // must not give it twice
    void hand_over() {
        for (auto& b : bins) {
            if (!b.n_parts) continue;
            b.lds_bytes = bin_lds_bytes(b.a_cap, (size_t)b.fcap, (size_t)b.ucap);
            p->bins.push_back(std::move(b));
            b = Bin();
        }
    }
    smc_plan* commit() { hand_over(); return p; }
};
#define PCHK(x)                                                                                         \
    do {                                                                                                \
        hipError_t e_ = (x);                                                                            \
        if (e_ != hipSuccess) return B.fail(SMC_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
    } while (0)

// a whole-locus bin of n_parts workgroups: its launch list and the loci's descriptors in launch order, sized and allocated
static int bin_blocks(PlanBuild& B, Bin& b, size_t n_parts) {
    smc_ctx* ctx = B.p->ctx;
    b.n_parts = n_parts;
    b.parts_bytes = sizeof(V2Part) * n_parts;
    b.desc_bytes = sizeof(smc_locus) * n_parts;
    PCHK(plan_alloc(ctx, (void**)&b.d_parts, b.parts_bytes));
    PCHK(plan_alloc(ctx, (void**)&b.d_desc, b.desc_bytes));
    return SMC_OK;
}
// the deep bin (its a_cap is set): also an accumulator per locus cut into more than one part, fdw flag dwords of scratch and the
// workgroups' offsets into them
static int deep_bin_blocks(PlanBuild& B, Bin& b, size_t n_parts, size_t n_acc, uint64_t fdw) {
    smc_ctx* ctx = B.p->ctx;
    b.acc_bytes = std::max<size_t>(1, n_acc) * v2_acc_words(b.a_cap) * 4;
    b.flags_bytes = (size_t)fdw * 4;
    b.foff_bytes = sizeof(int64_t) * n_parts;
    PCHK(plan_alloc(ctx, (void**)&b.d_acc, b.acc_bytes));
    PCHK(plan_alloc(ctx, (void**)&b.d_flags, b.flags_bytes));
    PCHK(plan_alloc(ctx, (void**)&b.d_flags_off, b.foff_bytes));
    return bin_blocks(B, b, n_parts);
}

// The device prologue of smc_plan_create_dev and smc_plan_create_dev_spec: the context's record and list of deep loci are there and
// free (one of each per context: a plan made on another stream waits for the plan before it to be through with them), the record is
// zero, and k_plan_classify sums this batch into it.
static int plan_classify(PlanBuild& B, const smc_locus* d_loci, const PlanCfg& C, hipStream_t st) {
    smc_plan* p = B.p;
    smc_ctx* ctx = p->ctx;
    const int64_t n_loci = p->n_loci;
    if (!ctx->plan_stats) {
        PCHK(hipMalloc(&ctx->plan_stats, sizeof(PlanStats)));
        PCHK(hipHostMalloc(&ctx->plan_stats_host, sizeof(PlanStats), hipHostMallocDefault));
    }
    if (ctx->plan_deep_cap < (size_t)n_loci) {
        PCHK(hipStreamSynchronize(st));
        (void)hipFree(ctx->plan_deep); ctx->plan_deep = nullptr; ctx->plan_deep_cap = 0;
        PCHK(hipMalloc(&ctx->plan_deep, sizeof(PlanDeep) * (size_t)n_loci));
        ctx->plan_deep_cap = (size_t)n_loci;
    }
    PlanStats* d_st = (PlanStats*)ctx->plan_stats;
    if (ctx->plan_fill_ev) PCHK(hipStreamWaitEvent(st, ctx->plan_fill_ev, 0));
    if (!ctx->plan_stats_clean) PCHK(hipMemsetAsync(d_st, 0, sizeof(PlanStats), st));
    ctx->plan_stats_clean = false;
    hipLaunchKernelGGL(k_plan_classify, dim3((unsigned)((n_loci + PLAN_BLOCK - 1) / PLAN_BLOCK)), dim3(PLAN_BLOCK), 0, st, d_loci, (int)n_loci, C, d_st,
                       (PlanDeep*)ctx->plan_deep, p->d_flt_list);
    PCHK(hipGetLastError());
    p->flt_clean = true;                                               // (k_plan_classify has zeroed both worklists' counts)
    return SMC_OK;
}
// Their epilogue, in two steps (smc_plan_create_dev makes its deep class's lists between them).  Behind k_plan_fill / k_plan_fill_spec,
// whose last workgroup zeroes the record: the event the next plan's kernels wait for.
static int plan_fill_launched(PlanBuild& B, hipStream_t st) {
    smc_ctx* ctx = B.p->ctx;
    if (!ctx->plan_fill_ev) PCHK(hipEventCreateWithFlags(&ctx->plan_fill_ev, hipEventDisableTiming));
    PCHK(hipEventRecord(ctx->plan_fill_ev, st));
    ctx->plan_stats_clean = true;
    return SMC_OK;
}
// Behind the last kernel that writes the plan's lists: the bins to the plan, and the event a plan destroyed unrun waits for.
static int plan_lists_launched(PlanBuild& B, hipStream_t st) {
    smc_plan* p = B.p;
    B.hand_over();
    PCHK(hipEventCreateWithFlags(&p->done_ev, hipEventDisableTiming));
    PCHK(hipEventRecord(p->done_ev, st));
    return SMC_OK;
}

// calProb's likelihoods all carry the factor rightP (smCounter.py:62-91), so the posteriors depend on the odds
// e / (1 - e) of the fragments only: P(barcode | allele k) / rightP = pcr_no_error * prod(odds of the fragments that do not
// show k) + pcrP term, and the pcrP term is >= 1e-6 (:79-81).  An included read has bq >= minBQ (:378-431), an unpaired
// fragment e = 0.1 (:65-68): every odds value is <= rho = max(1/9, e(minBQ) / (1 - e(minBQ))).  From K reference-allele
// fragments with rho^K < 1e-24 on, the product in the term of every OTHER allele is below a quarter ulp of 1e-6: it does
// not change the sum, and the general path does not have to visit the reference fragments (merged pairs: their
// qualities) at all.  INT_MAX when the bound is useless (minBQ so low that e >= 0.5).
static int lite_from_for(int min_bq) {
    if (exp_env("SMC_NO_LITE")) return INT_MAX;                       // (diagnostic: every queued barcode takes the full walk)
    const double e = std::pow(10.0, -0.1 * (double)(min_bq < 0 ? 0 : min_bq));
    if (!(e < 0.5)) return INT_MAX;
    const double rho = std::max(1.0 / 9.0, e / (1.0 - e));
    return (int)std::ceil(24.0 / -std::log10(rho)) + 1;
}

// The per-count table and `lite` never form rightP: right while the reference's rightP is a normal double (it cancels), wrong
// once it is not - the reference's posteriors are then denormal rounding, the general path follows them down and flags the row
// (SMC_ST_UNDERFLOW).  A fragment contributes a factor 1 - e >= 1 - max(0.1, e(minBQ)) (an unpaired fragment 0.1, a merged pair its
// smaller quality, >= minBQ), so rightP >= 2^-1000 while nf <= 1000 ln 2 / -ln(1 - e): barcodes from that count on (less one, for
// the rounding of the products) take the general path.  At minBQ >= 9 that is beyond SMC_SIMPLE_N (0.9^n: n = 6,578) and nothing
// changes; at minBQ 3 it is 995.
static int simple_to_for(int min_bq) {
    const double e = std::max(0.1, std::pow(10.0, -0.1 * (double)(min_bq < 0 ? 0 : min_bq)));
    if (!(e < 1.0)) return 1;                                         // (minBQ 0: a merged pair of quality 0 makes rightP 0)
    const double lim = std::floor(1000.0 * std::log(2.0) / -std::log1p(-e)) - 1.0;
    return (int)std::min((double)SMC_SIMPLE_N, std::max(1.0, lim));
}

template <int BLOCK, bool W16>
static hipError_t launch_bin(const Bin& b, const KParams& kp, const smc_plan* p, uint32_t* flt_list, const uint32_t* words, const uint32_t* umi_start,
                             smc_row* rows, hipStream_t st) {
    auto kern = k_call_v2<BLOCK, W16>;
    if (b.lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b.lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3((unsigned)b.n_parts), dim3(BLOCK), b.lds_bytes, st, kp, b.d_desc, b.d_parts, b.a_cap,
                       b.fcap, b.ucap, words, umi_start, p->ctx->lut, p->ctx->simple, p->ctx->pcr, rows, b.d_acc, b.d_flags, b.d_flags_off,
                       flt_list, b.d_launch_n);
    return hipGetLastError();
}

extern "C" {

int smc_abi_version(void) { return SMC_ABI_VERSION; }
const char* smc_last_error(void) { return g_err.c_str(); }
int smc_row_size(void) { return (int)sizeof(smc_row); }
int smc_locus_size(void) { return (int)sizeof(smc_locus); }

int smc_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// read class -> what the read adds to its allele's tallies (include/smcounter_hip.h: smc_read_class).  out[2c], out[2c+1]:
// nine 5-bit increments in SMC_T_* order (six in the first word, three in the second), second word bit 31 = incCond.
void smc_class_table(uint32_t* out /* [64] */) {
    uint32_t cls[32][2];
    memset(cls, 0, sizeof cls);
    for (int kind = 0; kind < 4; ++kind)
        for (int bits = 0; bits < 64; ++bits) {
            const int rev = bits & 1, r2 = (bits >> 1) & 1, inc = (bits >> 2) & 1, bq_ok = (bits >> 3) & 1,
                      le20 = (bits >> 4) & 1, prle = (bits >> 5) & 1;
            if (kind == SMC_KIND_BASE && inc && !bq_ok) continue;           // included implies bq >= minBQ
            const uint32_t c_ = smc_read_class(kind, rev, r2, inc, bq_ok, le20, prle);
            uint32_t f[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            f[SMC_T_CNT] = 1;                                                // :379,401,459
            if (kind != SMC_KIND_GAP) f[rev ? SMC_T_REV : SMC_T_FWD] = 1;    // :386-389,408-411,454-457
            if (kind == SMC_KIND_BASE) {
                if (!bq_ok) f[SMC_T_LOWQ] = 1;                               // :428-429
                if (inc && !r2) { f[SMC_T_R1N] = 1; f[SMC_T_R1LE] = (uint32_t)le20; }                  // :432-440
                if (inc && r2) { f[SMC_T_R2N] = 1; f[SMC_T_R2BCLE] = (uint32_t)le20; f[SMC_T_R2PRLE] = (uint32_t)prle; }   // :441-452
            }
            uint32_t lo = 0, hi = 0;
            for (int t = 0; t < 6; ++t) lo |= f[t] << (5 * t);
            for (int t = 6; t < 9; ++t) hi |= f[t] << (5 * (t - 6));
            hi |= (inc ? CLS_INC : 0u) | CLS_VALID;
            cls[c_][0] = lo; cls[c_][1] = hi;
        }
    memcpy(out, cls, sizeof cls);
}

int smc_create(int device, smc_ctx** out) {
    if (!out) return fail(SMC_E_ARG, "smc_create: out is NULL");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return fail(SMC_E_NOGPU, "no HIP device visible");
    if (device < 0 || device >= n) return fail(SMC_E_ARG, "smc_create: device index out of range");
    HIPCHK(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(SMC_E_NOGPU, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    smc_ctx* c = new smc_ctx();
    c->device = device;
    c->max_lds = 160 * 1024;
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    double h[256 + 32 + 32];
    for (int q = 0; q < 256; ++q) h[q] = pow(10.0, -q / 10.0);   // smCounter.py:469
    smc_class_table((uint32_t*)&h[256]);
    {   // the same table by smc_class16's code (16-bit read words: k_call_v2<., true>)
        const uint64_t* by_cls = (const uint64_t*)&h[256];
        uint64_t* by_c16 = (uint64_t*)&h[288];
        for (uint32_t c16 = 0; c16 < 32; ++c16) { const uint32_t c = smc_class16_inv(c16); by_c16[c16] = c < SMC_N_READ_CLASS ? by_cls[c] : 0ull; }
    }
    HIPCHK(hipMalloc(&c->lut, sizeof h));
    HIPCHK(hipMemcpy(c->lut, h, sizeof h, hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&c->simple, sizeof(double) * 2 * SMC_SIMPLE_N));
    hipLaunchKernelGGL(k_simple_table, dim3(SMC_SIMPLE_N / 256), dim3(256), 0, 0, c->simple, SMC_SIMPLE_N);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMalloc(&c->pcr, sizeof(double) * SMC_PCR_N * SMC_PCR_N));
    hipLaunchKernelGGL(k_pcr_table, dim3(SMC_PCR_N), dim3(SMC_PCR_N), 0, 0, c->pcr);
    HIPCHK(hipMalloc(&c->lfact, sizeof(double) * SMC_LFACT_N));
    hipLaunchKernelGGL(k_lfact_table, dim3(SMC_LFACT_N / 256), dim3(256), 0, 0, c->lfact);
    HIPCHK(hipGetLastError());
    HIPCHK(hipDeviceSynchronize());
    *out = c;
    return SMC_OK;
}

void smc_destroy(smc_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipFree(c->lut);
    (void)hipFree(c->simple);
    (void)hipFree(c->pcr);
    (void)hipFree(c->lfact);
    (void)hipFree(c->bp_scratch);
    (void)hipFree(c->sel_scratch);
    (void)hipFree(c->lod_scratch);
    (void)hipFree(c->af_scratch);
    (void)hipFree(c->spi_scratch);
    (void)hipFree(c->bl_scratch);
    (void)hipFree(c->chk_scratch);
    {
        std::vector<smc_ctx::VmmBlock> left;
        { std::lock_guard<std::mutex> g(c->vmm_mu); left.swap(c->vmm); }
        if (!left.empty()) (void)hipDeviceSynchronize();
        for (auto& b : left) { (void)hipMemUnmap(b.va, b.total); for (auto h : b.handles) (void)hipMemRelease(h); (void)hipMemAddressFree(b.va, b.total); }
    }
    plan_pool_collect(c, true);
    for (auto& b : c->plan_pool) (void)hipFree(b.second);
    (void)hipFree(c->plan_stats); (void)hipFree(c->plan_deep); (void)hipFree(c->d_spec_fail);
    if (c->plan_stats_host) (void)hipHostFree(c->plan_stats_host);
    for (void* h : c->spec_host_free) (void)hipHostFree(h);
    if (c->plan_fill_ev) (void)hipEventDestroy(c->plan_fill_ev);
    if (c->bp_done_ev) (void)hipEventDestroy(c->bp_done_ev);
    if (c->bl_done_ev) (void)hipEventDestroy(c->bl_done_ev);
    for (auto& sg : c->seg_stage) { if (sg.host) (void)hipHostFree(sg.host); if (sg.ev) (void)hipEventDestroy(sg.ev); }
    for (auto e : c->bp_ev0) (void)hipEventDestroy(e);
    for (auto e : c->bp_ev1) (void)hipEventDestroy(e);
    delete c;
}

void smc_plan_destroy(smc_plan* p) {
    if (!p) return;
    (void)hipSetDevice(p->ctx->device);
    // the device blocks go back to the context's pool - once the plan's last run is through (its event): nothing here waits
    smc_ctx::PendingFree q;
    q.ev = p->done_ev;
    auto give = [&](void* ptr, size_t bytes) { if (ptr) q.blocks.emplace_back(plan_size_class(bytes), ptr); };
    if (p->own_loci) give(p->d_loci, p->loci_bytes);
    give(p->d_flt_list, p->flt_bytes);
    give(p->d_words, p->words_bytes);
    give(p->d_spec, 256);
    // (the page-locked record may still be the target of the plan's copy: the next plan that takes it from the free list enqueues its
    // own copy behind the context's plan_fill_ev, which this plan recorded after its copy)
    if (p->spec_host) p->ctx->spec_host_free.push_back(p->spec_host);
    for (auto e : p->ev0) (void)hipEventDestroy(e);
    for (auto e : p->ev1) (void)hipEventDestroy(e);
    for (auto& b : p->bins) {
        give(b.d_parts, b.parts_bytes);
        give(b.d_desc, b.desc_bytes);
        give(b.d_flags_off, b.foff_bytes);
        give(b.d_flags, b.flags_bytes);
        give(b.d_acc, b.acc_bytes);
    }
    if (q.ev) p->ctx->plan_pending.push_back(std::move(q));
    else for (auto& b : q.blocks) plan_pool_put(p->ctx, b.first, b.second);
    delete p;
}

int smc_plan_create(smc_ctx* ctx, const smc_locus* loci, int64_t n_loci, smc_plan** out) {
    if (!ctx || !out || (n_loci > 0 && !loci)) return fail(SMC_E_ARG, "smc_plan_create: NULL argument");
    if (n_loci > 0x7fffffff) return fail(SMC_E_ARG, "smc_plan_create: more than 2^31-1 loci in one batch");
    HIPCHK(hipSetDevice(ctx->device));
    int deep_fcap;
    const PlanCfg C = plan_cfg_from_env(deep_fcap);
    PlanBuild B(ctx, n_loci);
    smc_plan* p = B.p;
    for (int64_t l = 0; l < n_loci; ++l) {
        const smc_locus& L = loci[l];
        if (L.n_alleles > SMC_MAX_ALLELES || L.n_reads < 0 || L.n_umi < 0 || L.n_frag < 0 || L.n_reads >= C.max_reads)
            return B.fail(SMC_E_INPUT, "smc_plan_create: locus " + std::to_string(l) +
                                           " violates the layout contract (alleles<=64, reads<2^24)");
        // one parameter set per batch, and it must be stated: the planes bake minBQ / minMQ / mismatchThr / primerDist in
        const uint16_t fp = (uint16_t)(L.flags >> SMC_LF_FP_SHIFT);
        if (fp == 0 || (l > 0 && fp != p->fp))
            return B.fail(SMC_E_INPUT, "smc_plan_create: locus " + std::to_string(l) + (fp == 0 ?
                          " carries no parameter fingerprint (smc_locus.flags bits 1-15 = smc_param_fingerprint(...))" :
                          " was built with different parameters than locus 0 (fingerprints differ)"));
        p->fp = fp;
        p->need_quads = std::max<int64_t>(p->need_quads, (int64_t)L.read_off4 + (L.n_reads + 3) / 4);
        int a_cap = (L.n_alleles + 7) & ~7;
        if (a_cap < 8) a_cap = 8;
        int c = SMC_CLS_DEEP;
        for (int k = 0; k < 4; ++k)
            if (L.n_reads <= C.cls_reads[k] && L.n_reads <= C.deep_from) { c = k; break; }
        // (many barcodes with few reads: the per-barcode tables, not the reads, size the workgroup's LDS)
        if (c < SMC_CLS_DEEP && whole_locus_lds(L, a_cap) > 64 * 1024) c = SMC_CLS_DEEP;
        Bin& b = B.bins[c];
        b.order.push_back((int)l);
        if (a_cap > b.a_cap) b.a_cap = a_cap;
        b.reads += L.n_reads;
    }
    p->flt_bytes = sizeof(uint32_t) * 2 * ((size_t)n_loci + 2);   // two worklists, each [0] = count, then locus indices (runs alternate)
    PCHK(plan_alloc(ctx, (void**)&p->d_flt_list, p->flt_bytes));
    if (n_loci) {
        p->loci_bytes = sizeof(smc_locus) * (size_t)n_loci;
        PCHK(plan_alloc(ctx, (void**)&p->d_loci, p->loci_bytes));
        PCHK(hipMemcpy(p->d_loci, loci, sizeof(smc_locus) * (size_t)n_loci, hipMemcpyHostToDevice));
    }
    int n_bins = 0;                                                // (a bin's place in the plan: classes without loci are left out)
    for (auto& b : B.bins) {
        if (b.order.empty()) continue;
        // heaviest loci first: the tail of the launch is then made of light blocks
        std::stable_sort(b.order.begin(), b.order.end(), [&](int x, int y) { return loci[x].n_reads > loci[y].n_reads; });
        if (b.cls < SMC_CLS_DEEP) {
            int mq = 0, mu = 0;
            for (int l : b.order) {
                mq = std::max(mq, (loci[l].n_reads + 3) / 4 + 2);
                mu = std::max(mu, loci[l].n_umi);
                b.parts.push_back(V2Part{l, 0, 1, 0});
            }
            b.fcap = mq; b.ucap = mu > 0 ? mu : 1;
            if (int rc = bin_blocks(B, b, b.parts.size())) return rc;
        } else {
            b.fcap = deep_fcap; b.ucap = C.deep_ucap;
            std::vector<int64_t> foff;
            int n_acc = 0;
            int64_t fdw = 0;
            for (int l : b.order) {
                const smc_locus& L = loci[l];
                const int np = plan_deep_parts(C, L.n_reads, L.n_umi);
                const int acc = np > 1 ? n_acc++ : 0;
                for (int q = 0; q < np; ++q) {
                    b.parts.push_back(V2Part{l, q, np, acc});
                    foff.push_back(fdw + 2 * q);
                }
                fdw += plan_deep_fdw(L.n_reads, np);
            }
            if (int rc = deep_bin_blocks(B, b, b.parts.size(), (size_t)n_acc, (uint64_t)fdw)) return rc;
            PCHK(hipMemcpy(b.d_flags_off, foff.data(), sizeof(int64_t) * foff.size(), hipMemcpyHostToDevice));
        }
        PCHK(hipMemcpy(b.d_parts, b.parts.data(), sizeof(V2Part) * b.parts.size(), hipMemcpyHostToDevice));
        std::vector<smc_locus> dl(b.parts.size());
        for (size_t k = 0; k < dl.size(); ++k) dl[k] = loci[b.parts[k].li];
        PCHK(hipMemcpy(b.d_desc, dl.data(), b.desc_bytes, hipMemcpyHostToDevice));
        if (b.reads > p->dom_reads) { p->dom_reads = b.reads; p->dom_loci = (int64_t)b.order.size(); p->dom_bin = n_bins; }
        ++n_bins;
    }
    *out = B.commit();
    return SMC_OK;
}

// The same plan from descriptors that are already on the device (smc_build_planes has just written them): classes, launch lists
// and table sizes are made there (k_plan.inc); only a small record and the few deep loci come back.  `d_loci` stays the
// caller's: it must outlive the plan.
int smc_plan_create_dev(smc_ctx* ctx, const smc_locus* d_loci, int64_t n_loci, void* stream, smc_plan** out) {
    if (!ctx || !out || (n_loci > 0 && !d_loci)) return fail(SMC_E_ARG, "smc_plan_create_dev: NULL argument");
    if (n_loci > 0x7fffffff) return fail(SMC_E_ARG, "smc_plan_create_dev: more than 2^31-1 loci in one batch");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    int deep_fcap;
    const PlanCfg C = plan_cfg_from_env(deep_fcap);
    PlanBuild B(ctx, n_loci);
    smc_plan* p = B.p;
    p->own_loci = false; p->d_loci = const_cast<smc_locus*>(d_loci);
    p->flt_bytes = sizeof(uint32_t) * 2 * ((size_t)n_loci + 2);   // two worklists, each [0] = count, then locus indices (runs alternate)
    hipError_t e = plan_alloc(ctx, (void**)&p->d_flt_list, p->flt_bytes);
    if (e != hipSuccess) return B.fail(SMC_E_HIP, std::string("smc_plan_create_dev: ") + hipGetErrorString(e));
    if (n_loci == 0) { *out = B.commit(); return SMC_OK; }
    if (int rc = plan_classify(B, d_loci, C, st)) return rc;
    PlanStats* d_st = (PlanStats*)ctx->plan_stats;
    PlanStats& S = *(PlanStats*)ctx->plan_stats_host;
    PCHK(hipMemcpyAsync(&S, d_st, sizeof(PlanStats), hipMemcpyDeviceToHost, st));
    PCHK(hipStreamSynchronize(st));
    if (S.bad) return B.fail(SMC_E_INPUT, "smc_plan_create_dev: " + std::to_string(S.bad) + " loci violate the layout contract (alleles<=64, reads<2^24)");
    if ((S.fp_or & S.fp_nor) != 0 || S.fp_or == 0)
        return B.fail(SMC_E_INPUT, S.fp_or == 0 ? "smc_plan_create_dev: the loci carry no parameter fingerprint (smc_locus.flags bits 1-15)"
                                               : "smc_plan_create_dev: loci built with different parameters in one batch (fingerprints differ)");
    p->fp = (uint16_t)S.fp_or;
    p->need_quads = (int64_t)S.max_quad;
    PlanLists PL;
    memset(&PL, 0, sizeof PL);
    for (int c = 0; c < 4; ++c) {
        Bin& b = B.bins[c];
        if (!S.count[c]) continue;
        b.a_cap = (int)std::max<uint32_t>(8, S.maxa[c]);
        b.fcap = (int)S.maxq[c]; b.ucap = (int)std::max<uint32_t>(1, S.maxu[c]);
        b.reads = (int64_t)S.reads[c];
        if (int rc = bin_blocks(B, b, S.count[c])) return rc;
        PL.parts[c] = b.d_parts; PL.desc[c] = b.d_desc;
        uint32_t run = 0;
        for (int k = 0; k < PLAN_NB; ++k) { PL.base[c][k] = run; run += S.bucket[c][k]; }
    }
    hipLaunchKernelGGL(k_plan_fill, dim3((unsigned)((n_loci + PLAN_BLOCK - 1) / PLAN_BLOCK)), dim3(PLAN_BLOCK), 0, st, d_loci, (int)n_loci, C, d_st, PL);
    PCHK(hipGetLastError());
    if (int rc = plan_fill_launched(B, st)) return rc;
    // the deep class: its launch list is made on the device too (k_plan_deep), sized by what k_plan_classify has summed
    if (S.n_deep) {
        Bin& b = B.bins[SMC_CLS_DEEP];
        b.fcap = deep_fcap; b.ucap = C.deep_ucap;
        b.a_cap = (int)std::max<uint32_t>(8, S.maxa[4]);
        b.reads = (int64_t)S.reads[4];
        if (int rc = deep_bin_blocks(B, b, S.deep_parts, S.deep_acc, S.deep_fdw)) return rc;
        hipLaunchKernelGGL(k_plan_deep, dim3(1), dim3(1024), 0, st, (const PlanDeep*)ctx->plan_deep, S.n_deep, C, d_loci, b.d_parts, b.d_flags_off, b.d_desc);
        PCHK(hipGetLastError());
        PCHK(hipEventRecord(ctx->plan_fill_ev, st));                      // (the context's list of deep loci is free for the next plan only now)
    }
    int n_bins = 0;                                                       // (a bin's place in the plan: classes without loci are left out)
    for (const Bin& b : B.bins) {
        if (!b.n_parts) continue;
        if (b.reads > p->dom_reads) { p->dom_reads = b.reads; p->dom_loci = b.cls < SMC_CLS_DEEP ? (int64_t)b.n_parts : (int64_t)S.n_deep; p->dom_bin = n_bins; }
        ++n_bins;
    }
    if (int rc = plan_lists_launched(B, st)) return rc;                    // (k_plan_fill writes the lists: a plan destroyed unrun waits for it)
    *out = B.commit();
    return SMC_OK;
}

// ---- the plan without the host in the loop (k_plan.inc, second half)
int smc_plan_create_dev_spec(smc_ctx* ctx, const smc_params* prm, const smc_locus* d_loci, int64_t n_loci, void* stream, smc_plan** out) {
    if (!ctx || !prm || !out || (n_loci > 0 && !d_loci)) return fail(SMC_E_ARG, "smc_plan_create_dev_spec: NULL argument");
    if (n_loci > 0x7fffffff) return fail(SMC_E_ARG, "smc_plan_create_dev_spec: more than 2^31-1 loci in one batch");
    const uint32_t fp = smc_param_fingerprint(prm->min_bq, prm->min_mq, prm->mismatch_thr, prm->primer_dist);
    // nothing to size the launches from (the context's first plan, or the last such plan did not fit), or an empty batch: the exact way
    // - whose record is what the next plan is sized from
    if (!ctx->hint_ok || n_loci == 0 || ctx->hint_stats.fp_or != fp || exp_env("SMC_PLAN_NO_SPEC")) {
        const int rc = smc_plan_create_dev(ctx, d_loci, n_loci, stream, out);
        if (rc == SMC_OK && n_loci > 0) {
            ctx->hint_stats = *(const PlanStats*)ctx->plan_stats_host; ctx->hint_loci = n_loci; ctx->hint_ok = true; ctx->spec_exact++;
        }
        return rc;
    }
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const PlanStats& Hn = ctx->hint_stats;
    int deep_fcap;
    const PlanCfg C = plan_cfg_from_env(deep_fcap);
    // ---- what the launches are sized for: the last record, scaled to this batch's loci, with room
    PlanCaps K;
    memset(&K, 0, sizeof K);
    K.fp = fp;
    const double scale = (double)n_loci / (double)std::max<int64_t>(1, ctx->hint_loci);
    auto grow = [&](uint64_t v, double f, uint64_t add) -> uint64_t { return v ? (uint64_t)std::ceil((double)v * scale * f) + add : 0ull; };
    for (int c = 0; c < 4; ++c) {
        if (!Hn.count[c]) continue;
        K.count[c] = (uint32_t)std::min<uint64_t>((uint64_t)n_loci, scale == 1.0 ? Hn.count[c] + (uint64_t)Hn.count[c] / 64 + 16 : grow(Hn.count[c], 1.125, 64));
        K.acap[c] = std::max<uint32_t>(8, Hn.maxa[c]);
        // the tables: as much more than the last batch needed as leaves the workgroups per CU what they were (the LDS decides them)
        const size_t q_max = (size_t)C.cls_reads[c] / 4 + 3;
        size_t fcap = Hn.maxq[c], ucap = std::max<uint32_t>(1, Hn.maxu[c]);
        const size_t lds0 = bin_lds_bytes((int)K.acap[c], fcap, ucap);
        const size_t per_cu = std::max<size_t>(1, (size_t)160 * 1024 / lds0);
        const size_t room = (size_t)160 * 1024 / per_cu;                   // bytes a workgroup may take without costing one per CU
        size_t fq = std::min(q_max, fcap + fcap / 8 + 8), uq = ucap + ucap / 4 + 16;
        while (bin_lds_bytes((int)K.acap[c], fq, uq) > std::max(room, lds0) && (fq > fcap || uq > ucap)) {
            if (fq > fcap) fq -= std::min<size_t>(fq - fcap, 8);
            if (uq > ucap) uq -= std::min<size_t>(uq - ucap, 4);
        }
        K.fcap[c] = (uint32_t)fq; K.ucap[c] = (uint32_t)std::min<size_t>(uq, 32767);
    }
    if (Hn.n_deep) {
        K.n_deep = (uint32_t)std::min<uint64_t>((uint64_t)n_loci, grow(Hn.n_deep, 1.25, 16));
        K.count[4] = (uint32_t)grow(Hn.deep_parts, 1.25, 64);
        K.deep_acc = (uint32_t)grow(std::max<uint32_t>(1, Hn.deep_acc), 1.25, 16);
        K.deep_fdw = grow(Hn.deep_fdw, 1.25, 4096);
        K.acap[4] = std::max<uint32_t>(8, Hn.maxa[4]);
    }
    PlanBuild B(ctx, n_loci);
    smc_plan* p = B.p;
    p->own_loci = false; p->d_loci = const_cast<smc_locus*>(d_loci);
    p->spec = true; p->caps = K; p->fp = (uint16_t)fp;
    p->flt_bytes = sizeof(uint32_t) * 2 * ((size_t)n_loci + 2);
    PCHK(plan_alloc(ctx, (void**)&p->d_flt_list, p->flt_bytes));
    PCHK(plan_alloc(ctx, (void**)&p->d_spec, 256));
    if (!ctx->spec_host_free.empty()) { p->spec_host = ctx->spec_host_free.back(); ctx->spec_host_free.pop_back(); }
    else PCHK(hipHostMalloc(&p->spec_host, sizeof(PlanStats), hipHostMallocDefault));
    if (!ctx->d_spec_fail) { PCHK(hipMalloc((void**)&ctx->d_spec_fail, 256)); PCHK(hipMemsetAsync(ctx->d_spec_fail, 0, 256, st)); }
    if (int rc = plan_classify(B, d_loci, C, st)) return rc;
    PlanStats* d_st = (PlanStats*)ctx->plan_stats;                      // (there since the exact plan that came first)
    PCHK(hipMemcpyAsync(p->spec_host, d_st, sizeof(PlanStats), hipMemcpyDeviceToHost, st));   // (for smc_plan_spec_ok; nobody waits for it here)
    PlanLists PL;
    memset(&PL, 0, sizeof PL);
    for (int c = 0; c < 4; ++c) {
        Bin& b = B.bins[c];
        if (!K.count[c]) continue;
        b.a_cap = (int)K.acap[c]; b.fcap = (int)K.fcap[c]; b.ucap = (int)K.ucap[c];
        b.reads = (int64_t)((double)Hn.reads[c] * scale);
        if (int rc = bin_blocks(B, b, K.count[c])) return rc;
        b.d_launch_n = &p->d_spec->n[c];
        PL.parts[c] = b.d_parts; PL.desc[c] = b.d_desc;
    }
    if (K.n_deep) {
        Bin& b = B.bins[SMC_CLS_DEEP];
        b.fcap = deep_fcap; b.ucap = C.deep_ucap;
        b.a_cap = (int)K.acap[4];
        b.reads = (int64_t)((double)Hn.reads[4] * scale);
        if (int rc = deep_bin_blocks(B, b, K.count[4], K.deep_acc, K.deep_fdw)) return rc;
        b.d_launch_n = &p->d_spec->n[4];
        hipLaunchKernelGGL(k_plan_deep_spec, dim3(1), dim3(1024), 0, st, (const PlanDeep*)ctx->plan_deep, (const PlanStats*)d_st, K, C, d_loci, b.d_parts,
                           b.d_flags_off, b.d_desc);
        PCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_plan_fill_spec, dim3((unsigned)((n_loci + PLAN_BLOCK - 1) / PLAN_BLOCK)), dim3(PLAN_BLOCK), 0, st, d_loci, (int)n_loci, C, d_st, K, PL,
                       p->d_spec, ctx->d_spec_fail);
    PCHK(hipGetLastError());
    if (int rc = plan_fill_launched(B, st)) return rc;
    int n_bins = 0;
    for (const Bin& b : B.bins) {
        if (!b.n_parts) continue;
        if (b.reads >= p->dom_reads) { p->dom_reads = b.reads; p->dom_loci = (int64_t)b.n_parts; p->dom_bin = n_bins; }
        ++n_bins;
    }
    if (int rc = plan_lists_launched(B, st)) return rc;
    ctx->spec_made++;
    *out = B.commit();
    return SMC_OK;
}

// After the plan's stream has been synchronised (the caller has waited for the rows): did the batch fit what the launches were sized
// for?  *ok = 0: the run launched nothing - the rows are not this batch's; make the plan with smc_plan_create_dev (or this function
// again: it goes the exact way once) and run it again.  A plan made the exact way always answers 1.
int smc_plan_spec_ok(smc_plan* p, int* ok) {
    if (!p || !ok) return fail(SMC_E_ARG, "smc_plan_spec_ok: NULL argument");
    *ok = 1;
    if (!p->spec) return SMC_OK;
    if (p->spec_checked < 0) {
        if (p->done_ev && hipEventQuery(p->done_ev) != hipSuccess)
            return fail(SMC_E_ARG, "smc_plan_spec_ok: the plan's kernels are still in flight (synchronise its stream first)");
        const PlanStats& S = *(const PlanStats*)p->spec_host;
        p->spec_checked = plan_spec_fits(S, p->caps) ? 1 : 0;
        smc_ctx* ctx = p->ctx;
        if (p->spec_checked) { ctx->hint_stats = S; ctx->hint_loci = p->n_loci; ctx->hint_ok = true; }   // (the sizes follow the data)
        else { ctx->hint_ok = false; ctx->spec_failed++; }
    }
    *ok = p->spec_checked;
    return SMC_OK;
}
// forget what the context's plans are sized from: the next smc_plan_create_dev_spec goes the exact way (a caller that knows its next
// batch is of another kind than the last - another file, another panel - saves the misfit)
int smc_plan_hint_reset(smc_ctx* ctx) {
    if (!ctx) return fail(SMC_E_ARG, "smc_plan_hint_reset: NULL context");
    ctx->hint_ok = false;
    return SMC_OK;
}
// plans made without the host by this context, how many of them went the exact way (nothing to size them from), and how many the
// DEVICE found not to fit (a counter there: synchronises the device) - a caller that destroys its plans unchecked asks here
int smc_plan_spec_counts(smc_ctx* ctx, int64_t* made, int64_t* exact, int64_t* not_fitting) {
    if (!ctx) return fail(SMC_E_ARG, "smc_plan_spec_counts: NULL context");
    HIPCHK(hipSetDevice(ctx->device));
    uint32_t nf = 0;
    if (ctx->d_spec_fail) HIPCHK(hipMemcpy(&nf, ctx->d_spec_fail, 4, hipMemcpyDeviceToHost));
    if (made) *made = ctx->spec_made;
    if (exact) *exact = ctx->spec_exact;
    if (not_fitting) *not_fitting = (int64_t)nf;
    return SMC_OK;
}

// The non-parity down-sampling of loci over the barcode cap on the device (k_philox_marks.inc): marks in umi_start + SMC_LF_SAMPLED in
// the descriptors, as the host's reference-exact sampling leaves them.  Before the plan of the batch is made or run.
int smc_philox_marks(smc_ctx* ctx, const smc_params* prm, smc_locus* d_loci, int64_t n_loci, const int64_t* d_pos, const void* d_words,
                     int word_bits, uint32_t* d_umi_start, const uint64_t* d_ident, const uint32_t* d_ident_index, uint64_t seed,
                     uint32_t* d_status, void* stream) {
    if (!ctx || !prm) return fail(SMC_E_ARG, "smc_philox_marks: NULL argument");
    if (n_loci <= 0) return SMC_OK;
    if (!d_loci || !d_pos || !d_words || !d_umi_start || !d_status || (word_bits != 16 && word_bits != 32) || n_loci > 0x7fffffff ||
        (d_ident_index && !d_ident))
        return fail(SMC_E_ARG, "smc_philox_marks: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_philox_marks, dim3((unsigned)n_loci), dim3(PHX_BLOCK), 0, (hipStream_t)stream, d_loci, d_pos, (const uint32_t*)d_words,
                       word_bits == 16 ? 1 : 0, d_umi_start, (const unsigned long long*)d_ident, d_ident_index, prm->ds, (unsigned long long)seed, d_status);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}
// (no GPU needed) the generator itself, for known-answer tests of the binding
void smc_philox4x32_10_host(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) { smc_philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1], out); }

int smc_select_alignments_keyed(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0,
                                int32_t key, int64_t n_bc, int64_t n_pair, const uint32_t* d_keep_mask, const uint64_t* d_ident, int64_t n_ids,
                                uint64_t seed, double frac, smc_dev_aln* d_aln_out, uint32_t* d_orig_index, smc_dev_locus* d_loc_out,
                                uint32_t* d_summary, void* stream) {
    if (!ctx) return fail(SMC_E_ARG, "smc_select_alignments: NULL context");
    if (key != SMC_SEL_KEY_BARCODE && key != SMC_SEL_KEY_READ) return fail(SMC_E_ARG, "smc_select_alignments_keyed: unknown key level");
    const bool renum = key == SMC_SEL_KEY_READ;          // (the read level renumbers the kept ids: n_bc / n_pair size its tables)
    if (renum && (n_bc < 0 || n_pair < 0 || n_bc + n_pair >= (int64_t)0xFFFFFFFF))
        return fail(SMC_E_ARG, "smc_select_alignments_keyed: bad id counts");
    if (n_aln < 0 || n_loci < 0 || n_ids < 0 || n_aln >= (int64_t)0xFFFFF000 || n_loci >= (int64_t)0x7FFFFFFF ||
        n_ids > (int64_t)0xFFFFFFFF || (!d_keep_mask && !d_ident && n_ids > 0) || !(frac >= 0.0))
        return fail(SMC_E_ARG, "smc_select_alignments: bad argument");
    if ((n_aln && (!d_aln || !d_aln_out || !d_orig_index)) || (n_loci && !d_loc_out) || !d_summary)
        return fail(SMC_E_ARG, "smc_select_alignments: NULL device pointer");
    (void)d_loc;                          // (the input windows are not needed: the decoder's rules are applied to the kept alignments)
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n_blk = (uint32_t)((n_aln + SEL_ITEMS - 1) / SEL_ITEMS), nl = (uint32_t)n_loci;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_off = carve(4 * ((size_t)n_blk + 1)), o_max = carve(4 * ((size_t)n_blk + 1)), o_diff = carve(4 * ((size_t)nl + 1));
    const size_t n_idw = renum ? (size_t)(n_bc + n_pair) : 0;
    const size_t o_rcnt = carve(renum ? 8 * ((size_t)n_blk + 1) : 0), o_rsum = carve(renum ? 16 : 0), o_first = carve(4 * n_idw), o_map = carve(4 * n_idw);
    if (int rc = grow_scratch(ctx->sel_scratch, ctx->sel_bytes, off, off + off / 8, "smc_select_alignments", &st)) return rc;
    char* sc = (char*)ctx->sel_scratch;
    uint32_t* blk_off = (uint32_t*)(sc + o_off);
    int32_t* blk_max = (int32_t*)(sc + o_max);
    int32_t* diff = (int32_t*)(sc + o_diff);
    SelRule R;
    R.mask = d_keep_mask; R.ident = (const unsigned long long*)d_ident; R.seed = (unsigned long long)seed; R.n_ids = (uint32_t)n_ids;
    R.thr = frac >= 1.0 ? (1ull << 32) : (unsigned long long)std::floor(frac * 4294967296.0);
    R.by_read = key == SMC_SEL_KEY_READ ? 1u : 0u;
    if (n_blk) hipLaunchKernelGGL(k_sel_count, dim3(n_blk), dim3(SEL_BLOCK), 0, st, d_aln, (uint32_t)n_aln, R, blk_off);
    hipLaunchKernelGGL(k_sel_offsets, dim3(1), dim3(SEL_SCAN), 0, st, blk_off, n_blk, diff, nl + 1u, d_summary);
    if (n_blk) hipLaunchKernelGGL(k_sel_scatter, dim3(n_blk), dim3(SEL_BLOCK), 0, st, d_aln, (uint32_t)n_aln, R, (const uint32_t*)blk_off,
                                  start0, nl, d_aln_out, d_orig_index, diff, blk_max);
    hipLaunchKernelGGL(k_sel_loci, dim3(1), dim3(SEL_SCAN), 0, st, blk_max, n_blk, (const int32_t*)diff, nl, d_loc_out, d_summary);
    if (nl) hipLaunchKernelGGL(k_sel_windows, dim3((nl + SEL_BLOCK / WAVE - 1) / (SEL_BLOCK / WAVE)), dim3(SEL_BLOCK), 0, st, (const smc_dev_aln*)d_aln_out,
                               (const uint32_t*)blk_off, (const int32_t*)blk_max, n_blk, start0, nl, d_loc_out);
    if (renum && n_blk) {
        // the kept ids renumbered by first kept appearance (k_select_aln.inc): first kept index per id, per-block counts of the firsts,
        // their exclusive scans (barcodes, read names), the new id of every first, the kept records' ids rewritten
        SelIds I;
        I.first = (uint32_t*)(sc + o_first); I.map = (uint32_t*)(sc + o_map); I.n_bc = (uint32_t)n_bc; I.n_pair = (uint32_t)n_pair;
        uint32_t* rcnt = (uint32_t*)(sc + o_rcnt);
        uint32_t* rsum = (uint32_t*)(sc + o_rsum);
        if (n_idw) HIPCHK(hipMemsetAsync(I.first, 0xFF, 4 * n_idw, st));
        hipLaunchKernelGGL(k_sel_first, dim3(n_blk), dim3(SEL_BLOCK), 0, st, (const smc_dev_aln*)d_aln_out, (const uint32_t*)d_summary, I);
        hipLaunchKernelGGL(k_sel_rcount, dim3(n_blk), dim3(SEL_BLOCK), 0, st, (const smc_dev_aln*)d_aln_out, (const uint32_t*)d_summary, I, n_blk, rcnt);
        hipLaunchKernelGGL(k_sel_offsets, dim3(1), dim3(SEL_SCAN), 0, st, rcnt, n_blk, (int32_t*)nullptr, 0u, rsum);
        hipLaunchKernelGGL(k_sel_offsets, dim3(1), dim3(SEL_SCAN), 0, st, rcnt + n_blk + 1, n_blk, (int32_t*)nullptr, 0u, rsum + 1);
        hipLaunchKernelGGL(k_sel_rank, dim3(n_blk), dim3(SEL_BLOCK), 0, st, (const smc_dev_aln*)d_aln_out, (const uint32_t*)d_summary, I, n_blk,
                           (const uint32_t*)rcnt);
        hipLaunchKernelGGL(k_sel_regid, dim3(n_blk), dim3(SEL_BLOCK), 0, st, d_aln_out, (const uint32_t*)d_summary, I);
    }
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (ABI 9) the barcode-level rule
int smc_select_alignments(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0,
                          const uint32_t* d_keep_mask, const uint64_t* d_ident, int64_t n_ids, uint64_t seed, double frac,
                          smc_dev_aln* d_aln_out, uint32_t* d_orig_index, smc_dev_locus* d_loc_out, uint32_t* d_summary, void* stream) {
    return smc_select_alignments_keyed(ctx, d_aln, n_aln, d_loc, n_loci, start0, SMC_SEL_KEY_BARCODE, 0, 0, d_keep_mask, d_ident, n_ids, seed, frac,
                                       d_aln_out, d_orig_index, d_loc_out, d_summary, stream);
}

// (ABI 11, additive) the philox selections of n_copies copies of a run at n_fracs fractions: the five stages of the single call with
// the selection as a grid dimension (k_select_aln.inc), the scratch once per selection.  Nothing waits.
int smc_select_alignments_copies(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t aln_stride_bytes, int32_t n_copies, int64_t n_aln,
                                 const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0, const uint64_t* d_ident, int64_t n_ids,
                                 const uint64_t* seeds, const double* fracs, int32_t n_fracs, smc_dev_aln* d_aln_out, uint32_t* d_orig_index,
                                 smc_dev_locus* d_loc_out, uint32_t* d_summary, void* stream) {
    const std::string who = "smc_select_alignments_copies";
    if (!ctx) return fail(SMC_E_ARG, who + ": NULL context");
    if (n_aln < 0 || n_loci < 0 || n_ids < 0 || n_aln >= (int64_t)0xFFFFF000 || n_loci >= (int64_t)0x7FFFFFFF || n_ids > (int64_t)0xFFFFFFFF ||
        (!d_ident && n_ids > 0) || (n_aln && !d_aln))
        return fail(SMC_E_ARG, who + ": bad argument");
    if (n_copies < 1 || n_fracs < 1 || (int64_t)n_copies * (int64_t)n_fracs > SMC_SEL_MAX_SELECTIONS)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies x " + std::to_string(n_fracs) + " fractions, 1 .. " +
                                 std::to_string(SMC_SEL_MAX_SELECTIONS) + " selections expected");
    if (!seeds || !fracs) return fail(SMC_E_ARG, who + ": NULL argument");
    for (int32_t f = 0; f < n_fracs; ++f)
        if (!(fracs[f] > 0.0 && fracs[f] <= 1.0))
            return fail(SMC_E_INPUT, who + ": fraction " + std::to_string(f) + " is " + std::to_string(fracs[f]) + ", not in (0, 1]");
    if (aln_stride_bytes < 0 || (aln_stride_bytes & 3))
        return fail(SMC_E_INPUT, who + ": a record stride of " + std::to_string(aln_stride_bytes) + " bytes (0 or a positive multiple of 4 expected)");
    if (!d_aln_out || !d_orig_index || !d_loc_out || !d_summary) return fail(SMC_E_INPUT, who + ": NULL output");
    (void)d_loc;                          // (as the single call: the input windows are not needed)
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n_blk = (uint32_t)((n_aln + SEL_ITEMS - 1) / SEL_ITEMS), nl = (uint32_t)n_loci;
    const uint32_t C = (uint32_t)n_copies, F = (uint32_t)n_fracs, S = C * F;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_off = carve(4 * ((size_t)n_blk + 1) * S), o_max = carve(4 * ((size_t)n_blk + 1) * S), o_diff = carve(4 * ((size_t)nl + 1) * S);
    if (int rc = grow_scratch(ctx->sel_scratch, ctx->sel_bytes, off, off + off / 8, who.c_str(), &st)) return rc;
    char* sc = (char*)ctx->sel_scratch;
    uint32_t* blk_off = (uint32_t*)(sc + o_off);
    int32_t* blk_max = (int32_t*)(sc + o_max);
    int32_t* diff = (int32_t*)(sc + o_diff);
    // the two record stages: a launch per group of SEL_CP_COPIES copies x SEL_CP_FRACS fractions (one launch for a usual batch)
    auto records = [&](bool scatter) {
        for (uint32_t c0 = 0; c0 < C; c0 += SEL_CP_COPIES)
            for (uint32_t f0 = 0; f0 < F; f0 += SEL_CP_FRACS) {
                SelCopies K;
                memset(&K, 0, sizeof K);
                const uint32_t nc = std::min<uint32_t>(SEL_CP_COPIES, C - c0);
                K.c0 = c0; K.f0 = f0; K.n_f = std::min<uint32_t>(SEL_CP_FRACS, F - f0); K.n_copies = C;
                for (uint32_t c = 0; c < nc; ++c) K.seed[c] = (unsigned long long)seeds[c0 + c];
                // (the single call's conversion)
                for (uint32_t f = 0; f < K.n_f; ++f)
                    K.thr[f] = fracs[f0 + f] >= 1.0 ? (1ull << 32) : (unsigned long long)std::floor(fracs[f0 + f] * 4294967296.0);
                if (!scatter)
                    hipLaunchKernelGGL(k_selc_count, dim3(n_blk, nc), dim3(SEL_BLOCK), 0, st, (const char*)d_aln, (unsigned long long)aln_stride_bytes,
                                       (uint32_t)n_aln, (const unsigned long long*)d_ident, (uint32_t)n_ids, K, n_blk, blk_off);
                else
                    hipLaunchKernelGGL(k_selc_scatter, dim3(n_blk, nc), dim3(SEL_BLOCK), 0, st, (const char*)d_aln, (unsigned long long)aln_stride_bytes,
                                       (uint32_t)n_aln, (const unsigned long long*)d_ident, (uint32_t)n_ids, K, n_blk, (const uint32_t*)blk_off, start0,
                                       nl, d_aln_out, d_orig_index, diff, blk_max);
            }
    };
    if (n_blk) records(false);
    hipLaunchKernelGGL(k_selc_offsets, dim3(S), dim3(SEL_SCAN), 0, st, blk_off, n_blk, diff, nl + 1u, d_summary);
    if (n_blk) records(true);
    hipLaunchKernelGGL(k_selc_loci, dim3(S), dim3(SEL_SCAN), 0, st, blk_max, n_blk, (const int32_t*)diff, nl, d_loc_out, d_summary);
    if (nl) hipLaunchKernelGGL(k_selc_windows, dim3((nl + SEL_BLOCK / WAVE - 1) / (SEL_BLOCK / WAVE), S), dim3(SEL_BLOCK), 0, st,
                               (const smc_dev_aln*)d_aln_out, (uint32_t)n_aln, (const uint32_t*)blk_off, (const int32_t*)blk_max, n_blk, start0,
                               nl, d_loc_out);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (ABI 11, additive) the read-level selections of n_copies copies of a run under n_masks keep masks each: the ten stages of
// smc_select_alignments_keyed at SMC_SEL_KEY_READ with the selection as a grid dimension (k_select_aln.inc), the scratch once per
// selection.  Nothing waits.
int smc_select_alignments_reads_copies(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t aln_stride_bytes, int32_t n_copies, int64_t n_aln,
                                       const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0, int64_t n_bc, int64_t n_pair,
                                       const uint32_t* d_masks, int64_t mask_words, int64_t mask_copy_stride_words, int32_t n_masks,
                                       int64_t n_ids, smc_dev_aln* d_aln_out, uint32_t* d_orig_index, smc_dev_locus* d_loc_out,
                                       uint32_t* d_summary, void* stream) {
    const std::string who = "smc_select_alignments_reads_copies";
    if (!ctx) return fail(SMC_E_ARG, who + ": NULL context");
    if (n_aln < 0 || n_loci < 0 || n_aln >= (int64_t)0xFFFFF000 || n_loci >= (int64_t)0x7FFFFFFF || n_ids > (int64_t)0xFFFFFFFF ||
        n_bc + n_pair >= (int64_t)0xFFFFFFFF || (n_aln && !d_aln))
        return fail(SMC_E_ARG, who + ": bad argument");
    if (n_copies < 1 || n_masks < 1 || (int64_t)n_copies * (int64_t)n_masks > SMC_SEL_MAX_SELECTIONS)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies x " + std::to_string(n_masks) + " masks, 1 .. " +
                                 std::to_string(SMC_SEL_MAX_SELECTIONS) + " selections expected");
    if (aln_stride_bytes < 0 || (aln_stride_bytes & 3))
        return fail(SMC_E_INPUT, who + ": a record stride of " + std::to_string(aln_stride_bytes) + " bytes (0 or a positive multiple of 4 expected)");
    if (n_bc < 0 || n_pair < 0 || n_ids < 0)
        return fail(SMC_E_INPUT, who + ": negative id counts (" + std::to_string(n_bc) + " barcodes, " + std::to_string(n_pair) + " read names, " +
                                 std::to_string(n_ids) + " mask ids)");
    if (mask_copy_stride_words < 0 || mask_words < (n_ids + 31) / 32)
        return fail(SMC_E_INPUT, who + ": masks of " + std::to_string(mask_words) + " words at a copy stride of " +
                                 std::to_string(mask_copy_stride_words) + " for " + std::to_string(n_ids) + " ids");
    if (!d_masks) return fail(SMC_E_INPUT, who + ": NULL masks");
    if (!d_aln_out || !d_orig_index || !d_loc_out || !d_summary) return fail(SMC_E_INPUT, who + ": NULL output");
    (void)d_loc;                          // (as the single call: the input windows are not needed)
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const uint32_t n_blk = (uint32_t)((n_aln + SEL_ITEMS - 1) / SEL_ITEMS), nl = (uint32_t)n_loci;
    const uint32_t C = (uint32_t)n_copies, M = (uint32_t)n_masks, S = C * M;
    const size_t n_idw = (size_t)(n_bc + n_pair);
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_off = carve(4 * ((size_t)n_blk + 1) * S), o_max = carve(4 * ((size_t)n_blk + 1) * S), o_diff = carve(4 * ((size_t)nl + 1) * S);
    const size_t o_rcnt = carve(8 * ((size_t)n_blk + 1) * S), o_rsum = carve(8 * (size_t)S), o_first = carve(4 * n_idw * S), o_map = carve(4 * n_idw * S);
    if (int rc = grow_scratch(ctx->sel_scratch, ctx->sel_bytes, off, off + off / 8, who.c_str(), &st)) return rc;
    char* sc = (char*)ctx->sel_scratch;
    uint32_t* blk_off = (uint32_t*)(sc + o_off);
    int32_t* blk_max = (int32_t*)(sc + o_max);
    int32_t* diff = (int32_t*)(sc + o_diff);
    // the two record stages: a launch per group of SEL_CP_FRACS masks (a bit of a register each; one launch for a usual batch)
    auto records = [&](bool scatter) {
        for (uint32_t m0 = 0; m0 < M; m0 += SEL_CP_FRACS) {
            SelReadCopies K;
            K.masks = d_masks; K.mask_words = (unsigned long long)mask_words; K.copy_stride = (unsigned long long)mask_copy_stride_words;
            K.n_ids = (uint32_t)n_ids; K.m0 = m0; K.n_m = std::min<uint32_t>(SEL_CP_FRACS, M - m0); K.n_copies = C;
            if (!scatter)
                hipLaunchKernelGGL(k_selr_count, dim3(n_blk, C), dim3(SEL_BLOCK), 0, st, (const char*)d_aln, (unsigned long long)aln_stride_bytes,
                                   (uint32_t)n_aln, K, n_blk, blk_off);
            else
                hipLaunchKernelGGL(k_selr_scatter, dim3(n_blk, C), dim3(SEL_BLOCK), 0, st, (const char*)d_aln, (unsigned long long)aln_stride_bytes,
                                   (uint32_t)n_aln, K, n_blk, (const uint32_t*)blk_off, start0, nl, d_aln_out, d_orig_index, diff, blk_max);
        }
    };
    if (n_blk) records(false);
    hipLaunchKernelGGL(k_selc_offsets, dim3(S), dim3(SEL_SCAN), 0, st, blk_off, n_blk, diff, nl + 1u, d_summary);
    if (n_blk) records(true);
    hipLaunchKernelGGL(k_selc_loci, dim3(S), dim3(SEL_SCAN), 0, st, blk_max, n_blk, (const int32_t*)diff, nl, d_loc_out, d_summary);
    if (nl) hipLaunchKernelGGL(k_selc_windows, dim3((nl + SEL_BLOCK / WAVE - 1) / (SEL_BLOCK / WAVE), S), dim3(SEL_BLOCK), 0, st,
                               (const smc_dev_aln*)d_aln_out, (uint32_t)n_aln, (const uint32_t*)blk_off, (const int32_t*)blk_max, n_blk, start0,
                               nl, d_loc_out);
    if (n_blk) {
        // the kept ids of every selection renumbered by first kept appearance: the single call's five stages, the selection on blockIdx.y
        SelIds I;
        I.first = (uint32_t*)(sc + o_first); I.map = (uint32_t*)(sc + o_map); I.n_bc = (uint32_t)n_bc; I.n_pair = (uint32_t)n_pair;
        uint32_t* rcnt = (uint32_t*)(sc + o_rcnt);
        uint32_t* rsum = (uint32_t*)(sc + o_rsum);
        const smc_dev_aln* kept = d_aln_out;
        const uint32_t* sum = d_summary;
        if (n_idw) HIPCHK(hipMemsetAsync(I.first, 0xFF, 4 * n_idw * S, st));
        hipLaunchKernelGGL(k_selr_first, dim3(n_blk, S), dim3(SEL_BLOCK), 0, st, kept, (uint32_t)n_aln, sum, I);
        hipLaunchKernelGGL(k_selr_rcount, dim3(n_blk, S), dim3(SEL_BLOCK), 0, st, kept, (uint32_t)n_aln, sum, I, n_blk, rcnt);
        hipLaunchKernelGGL(k_selr_offsets, dim3(2 * S), dim3(SEL_SCAN), 0, st, rcnt, n_blk, rsum);
        hipLaunchKernelGGL(k_selr_rank, dim3(n_blk, S), dim3(SEL_BLOCK), 0, st, kept, (uint32_t)n_aln, sum, I, n_blk, (const uint32_t*)rcnt);
        hipLaunchKernelGGL(k_selr_regid, dim3(n_blk, S), dim3(SEL_BLOCK), 0, st, d_aln_out, (uint32_t)n_aln, sum, I);
    }
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// ---- (ABI 11) the read-level philox sampler's file-wide table (k_read_groups.inc)
struct smc_read_groups {
    smc_ctx* ctx = nullptr;
    struct Chunk { smc_read_key* d = nullptr; int64_t n = 0, ord0 = 0; };
    std::vector<Chunk> chunks;          // the records added, in HBM until _finish inserts them
    int64_t n_records = 0, next_ord = 0;
    bool finished = false;
    void* mem = nullptr;                // both tables, the info / count words, status, counters, kept counts
    RgTable G{};
    unsigned long long* d_kept = nullptr;
    unsigned long long* d_frac = nullptr;   // (--dsGrid) RG_F_N counters per fraction
    int64_t counts[SMC_RG_N_COUNTS] = {0};
};

static int rg_grid(unsigned long long n) { return (int)std::max<unsigned long long>(1, std::min<unsigned long long>((n + RG_BLOCK - 1) / RG_BLOCK, 8192)); }

static int rg_thresholds(const uint64_t* thr, int32_t n_thr, RgThr& T) {
    if (n_thr < 0 || n_thr > SMC_RG_MAX_TARGETS || (n_thr && !thr)) return fail(SMC_E_ARG, "smc_read_groups: bad thresholds");
    memset(&T, 0, sizeof T);
    for (int t = 0; t < n_thr; ++t) {
        if (thr[t] > (1ull << 32)) return fail(SMC_E_ARG, "smc_read_groups: a threshold above 2^32");
        T.t[t] = thr[t];
    }
    return SMC_OK;
}

int smc_read_groups_create(smc_ctx* ctx, smc_read_groups** out) {
    if (!ctx || !out) return fail(SMC_E_ARG, "smc_read_groups_create: bad argument");
    *out = new smc_read_groups();
    (*out)->ctx = ctx;
    return SMC_OK;
}

int smc_read_groups_add(smc_read_groups* g, const smc_read_key* keys, int64_t n, int64_t first_ordinal) {
    if (!g || n < 0 || (n && !keys) || first_ordinal < 0) return fail(SMC_E_ARG, "smc_read_groups_add: bad argument");
    if (g->finished) return fail(SMC_E_ARG, "smc_read_groups_add: the table is finished");
    if (first_ordinal < g->next_ord) return fail(SMC_E_ARG, "smc_read_groups_add: ordinals must grow from chunk to chunk");
    if (first_ordinal + n >= (int64_t)0xFFFFFFFF) return fail(SMC_E_ARG, "smc_read_groups_add: ordinals beyond 2^32 - 2");
    if (!n) return SMC_OK;
    HIPCHK(hipSetDevice(g->ctx->device));
    smc_read_groups::Chunk c;
    c.n = n; c.ord0 = first_ordinal;
    HIPCHK(hipMalloc((void**)&c.d, sizeof(smc_read_key) * (size_t)n));
    const hipError_t e = hipMemcpy(c.d, keys, sizeof(smc_read_key) * (size_t)n, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(c.d); return fail(SMC_E_HIP, std::string("smc_read_groups_add: ") + hipGetErrorString(e)); }
    g->chunks.push_back(c);
    g->n_records += n;
    g->next_ord = first_ordinal + n;
    return SMC_OK;
}

int smc_read_groups_finish(smc_read_groups* g, int64_t* counts) {
    if (!g || !counts) return fail(SMC_E_ARG, "smc_read_groups_finish: bad argument");
    if (g->finished) return fail(SMC_E_ARG, "smc_read_groups_finish: finished already");
    HIPCHK(hipSetDevice(g->ctx->device));
    // capacity: a power of two >= 2 x the records (names and barcodes are each at most that many)
    unsigned long long cap = 2;
    while (cap < 2ull * (unsigned long long)g->n_records) cap <<= 1;
    if (cap > (1ull << 31)) return fail(SMC_E_ARG, "smc_read_groups_finish: too many records");
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_name = carve(16 * cap), o_info = carve(4 * cap), o_bc = carve(16 * cap), o_cnt = carve(4 * cap),
                 o_st = carve(4), o_ctr = carve(8 * RG_N_CTR), o_kept = carve(8 * SMC_RG_MAX_TARGETS),
                 o_frac = carve(8 * RG_F_N * SMC_RG_MAX_TARGETS);
    HIPCHK(hipMalloc(&g->mem, off));
    char* m = (char*)g->mem;
    RgTable& G = g->G;
    G.name = (RgSlot*)(m + o_name); G.name_info = (uint32_t*)(m + o_info); G.bc = (RgSlot*)(m + o_bc); G.bc_cnt = (uint32_t*)(m + o_cnt);
    G.n_mask = G.b_mask = cap - 1;
    G.status = (uint32_t*)(m + o_st); G.ctr = (unsigned long long*)(m + o_ctr);
    g->d_kept = (unsigned long long*)(m + o_kept);
    g->d_frac = (unsigned long long*)(m + o_frac);
    HIPCHK(hipMemsetAsync(m + o_st, 0, off - o_st, 0));
    hipLaunchKernelGGL(k_rg_init, dim3(rg_grid(cap)), dim3(RG_BLOCK), 0, 0, G);
    for (const auto& c : g->chunks)
        hipLaunchKernelGGL(k_rg_insert, dim3(rg_grid(c.n)), dim3(RG_BLOCK), 0, 0, G, (const smc_read_key*)c.d, (uint32_t)c.n, (uint32_t)c.ord0);
    for (const auto& c : g->chunks)
        hipLaunchKernelGGL(k_rg_verify, dim3(rg_grid(c.n)), dim3(RG_BLOCK), 0, 0, G, (const smc_read_key*)c.d, (uint32_t)c.n);
    hipLaunchKernelGGL(k_rg_link, dim3(rg_grid(cap)), dim3(RG_BLOCK), 0, 0, G);
    hipLaunchKernelGGL(k_rg_reduce, dim3(rg_grid(cap)), dim3(RG_BLOCK), 0, 0, G);
    HIPCHK(hipGetLastError());
    unsigned long long ctr[RG_N_CTR];
    HIPCHK(hipMemcpy(ctr, G.ctr, sizeof ctr, hipMemcpyDeviceToHost));
    for (auto& c : g->chunks) (void)hipFree(c.d);
    g->chunks.clear();
    g->finished = true;
    g->counts[0] = g->n_records;
    g->counts[1] = (int64_t)ctr[RG_C_NAMES]; g->counts[2] = (int64_t)ctr[RG_C_BARCODES]; g->counts[3] = (int64_t)ctr[RG_C_ONE];
    g->counts[4] = (int64_t)ctr[RG_C_MULTI]; g->counts[5] = (int64_t)ctr[RG_C_MULTI_NAMES]; g->counts[6] = (int64_t)ctr[RG_C_FIRST];
    for (int k = 0; k < SMC_RG_N_COUNTS; ++k) counts[k] = g->counts[k];
    return SMC_OK;
}

int smc_read_groups_masks(smc_read_groups* g, const uint64_t* d_idents, int64_t n_ids, uint64_t seed, const uint64_t* thr, int32_t n_thr,
                          uint32_t* d_masks, void* stream) {
    if (!g || n_ids < 0 || n_ids >= (int64_t)0xFFFFFF00 || (n_ids && (!d_idents || !d_masks))) return fail(SMC_E_ARG, "smc_read_groups_masks: bad argument");
    if (!g->finished) return fail(SMC_E_ARG, "smc_read_groups_masks: the table is not finished");
    RgThr T;
    { const int rc = rg_thresholds(thr, n_thr, T); if (rc) return rc; }
    if (!n_ids || !n_thr) return SMC_OK;
    HIPCHK(hipSetDevice(g->ctx->device));
    const uint32_t n_words = (uint32_t)((n_ids + 31) / 32);
    hipLaunchKernelGGL(k_rg_masks, dim3((unsigned)((n_ids + RG_BLOCK - 1) / RG_BLOCK)), dim3(RG_BLOCK), 0, (hipStream_t)stream, g->G,
                       (const unsigned long long*)d_idents, (uint32_t)n_ids, (unsigned long long)seed, T, (int)n_thr, d_masks, n_words);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

int smc_read_groups_kept(smc_read_groups* g, uint64_t seed, const uint64_t* thr, int32_t n_thr, int64_t* kept) {
    if (!g || (n_thr && !kept)) return fail(SMC_E_ARG, "smc_read_groups_kept: bad argument");
    if (!g->finished) return fail(SMC_E_ARG, "smc_read_groups_kept: the table is not finished");
    RgThr T;
    { const int rc = rg_thresholds(thr, n_thr, T); if (rc) return rc; }
    if (!n_thr) return SMC_OK;
    HIPCHK(hipSetDevice(g->ctx->device));
    HIPCHK(hipMemsetAsync(g->d_kept, 0, 8 * SMC_RG_MAX_TARGETS, 0));
    hipLaunchKernelGGL(k_rg_kept, dim3(rg_grid(g->G.n_mask + 1)), dim3(RG_BLOCK), 0, 0, g->G, (unsigned long long)seed, T, (int)n_thr, g->d_kept);
    HIPCHK(hipGetLastError());
    unsigned long long k[SMC_RG_MAX_TARGETS];
    HIPCHK(hipMemcpy(k, g->d_kept, 8 * (size_t)n_thr, hipMemcpyDeviceToHost));
    for (int t = 0; t < n_thr; ++t) kept[t] = (int64_t)k[t];
    return SMC_OK;
}

// (--lod) the table of one `needed`: k_lod_table over d = 0 .. max_depth on the null stream, the roots and the iteration counts back
int smc_lod_table(smc_ctx* ctx, int needed, int max_depth, double* roots, int32_t* iters) {
    if (!ctx || !roots) return fail(SMC_E_ARG, "smc_lod_table: NULL argument");
    if (needed < 1) return fail(SMC_E_INPUT, "smc_lod_table: needed = " + std::to_string(needed) + ", at least 1 barcode expected");
    if (max_depth < 0 || max_depth > SMC_LOD_MAX_DEPTH)
        return fail(SMC_E_INPUT, "smc_lod_table: max_depth = " + std::to_string(max_depth) + " outside 0 .. " + std::to_string(SMC_LOD_MAX_DEPTH));
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = (size_t)max_depth + 1, o_iters = (8 * n + 255) & ~(size_t)255, bytes = o_iters + 4 * n;
    // (no stream to wait for: no table kernel is in flight - the entry waits for its own)
    if (int rc = grow_scratch(ctx->lod_scratch, ctx->lod_bytes, bytes, bytes + bytes / 8, "smc_lod_table", nullptr)) return rc;
    double* d_roots = (double*)ctx->lod_scratch;
    int32_t* d_iters = (int32_t*)((char*)ctx->lod_scratch + o_iters);
    hipLaunchKernelGGL(k_lod_table, dim3((unsigned)((n + LOD_BLOCK - 1) / LOD_BLOCK)), dim3(LOD_BLOCK), 0, 0, needed, max_depth, d_roots, d_iters);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(roots, d_roots, 8 * n, hipMemcpyDeviceToHost));       // (null stream: ordered behind the kernel)
    if (iters) HIPCHK(hipMemcpy(iters, d_iters, 4 * n, hipMemcpyDeviceToHost));
    return SMC_OK;
}

// ---- checking entries: the Fisher tests' device arithmetic on arguments of the caller's choice (k_filter_loci.inc, its end)
// (their scratch grows to exactly what a call needs; the entries wait for their own kernels)
#define SMC_CHK_MAX_N ((int64_t)1 << 24)
int smc_fisher_tables(smc_ctx* ctx, const int64_t* tables, int64_t n, double* oddsratio, double* pvalue) {
    if (!ctx || n < 0) return fail(SMC_E_ARG, "smc_fisher_tables: bad argument");
    if (n == 0) return SMC_OK;
    if (!tables || !oddsratio || !pvalue) return fail(SMC_E_ARG, "smc_fisher_tables: NULL argument");
    if (n > SMC_CHK_MAX_N) return fail(SMC_E_ARG, "smc_fisher_tables: more than 2^24 tables in one call");
    for (int64_t i = 0; i < n; ++i) {
        const int64_t* T = tables + 4 * i;
        int64_t tot = 0;
        for (int k = 0; k < 4; ++k) {
            if (T[k] < 0) return fail(SMC_E_INPUT, "smc_fisher_tables: table " + std::to_string(i) + " has the negative count " + std::to_string(T[k]));
            if (T[k] > INT32_MAX || (tot += T[k]) > INT32_MAX)
                return fail(SMC_E_INPUT, "smc_fisher_tables: the counts of table " + std::to_string(i) + " add up to more than 2^31 - 1 (the tallies are int)");
        }
    }
    HIPCHK(hipSetDevice(ctx->device));
    const size_t N = (size_t)n;
    if (int rc = grow_scratch(ctx->chk_scratch, ctx->chk_bytes, 48 * N, 48 * N, "smc_fisher_tables", nullptr)) return rc;
    long long* d_tab = (long long*)ctx->chk_scratch;
    double* d_or = (double*)((char*)ctx->chk_scratch + 32 * N);
    double* d_p = d_or + N;
    HIPCHK(hipMemcpy(d_tab, tables, 32 * N, hipMemcpyHostToDevice));
    constexpr unsigned per_block = SMC_FISHER_BLOCK / WAVE;
    hipLaunchKernelGGL(k_fisher_tables, dim3((unsigned)((N + per_block - 1) / per_block)), dim3(SMC_FISHER_BLOCK), 0, 0, d_tab, (long long)n, ctx->lfact, d_or, d_p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(oddsratio, d_or, 8 * N, hipMemcpyDeviceToHost));      // (null stream: ordered behind the kernel)
    HIPCHK(hipMemcpy(pvalue, d_p, 8 * N, hipMemcpyDeviceToHost));
    return SMC_OK;
}

int smc_lfact_values(smc_ctx* ctx, const int64_t* n_values, int64_t n, double* out) {
    if (!ctx || n < 0) return fail(SMC_E_ARG, "smc_lfact_values: bad argument");
    if (n == 0) return SMC_OK;
    if (!n_values || !out) return fail(SMC_E_ARG, "smc_lfact_values: NULL argument");
    if (n > SMC_CHK_MAX_N) return fail(SMC_E_ARG, "smc_lfact_values: more than 2^24 values in one call");
    HIPCHK(hipSetDevice(ctx->device));
    const size_t N = (size_t)n;
    if (int rc = grow_scratch(ctx->chk_scratch, ctx->chk_bytes, 16 * N, 16 * N, "smc_lfact_values", nullptr)) return rc;
    long long* d_v = (long long*)ctx->chk_scratch;
    double* d_out = (double*)ctx->chk_scratch + N;
    HIPCHK(hipMemcpy(d_v, n_values, 8 * N, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_lfact_values, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, 0, d_v, (long long)n, ctx->lfact, d_out);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(out, d_out, 8 * N, hipMemcpyDeviceToHost));
    return SMC_OK;
}

// (--dsAF) the covers / carries bits of a run's listed variants: the counters zeroed, k_af_count over every variant's window, k_af_bits
int smc_allele_carriers(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, const uint8_t* d_bq,
                        const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0, int64_t n_bc, const smc_af_variant* d_var,
                        const smc_af_variant* var_host, int32_t n_var, const uint8_t* d_ins, int64_t n_ins, uint32_t* d_covers, uint32_t* d_carries,
                        uint32_t* d_counts, void* stream) {
    if (!ctx || n_aln < 0 || n_loci < 0 || n_bc < 0 || n_var < 0 || n_ins < 0) return fail(SMC_E_ARG, "smc_allele_carriers: bad argument");
    if (n_var > SMC_AF_MAX_VARIANTS) return fail(SMC_E_INPUT, "smc_allele_carriers: " + std::to_string(n_var) + " variants, at most " + std::to_string(SMC_AF_MAX_VARIANTS));
    if (!n_var || !n_bc) return SMC_OK;
    if (!d_aln || !d_cig || !d_bq || !d_loc || !d_var || !var_host || !d_covers || !d_carries) return fail(SMC_E_ARG, "smc_allele_carriers: NULL argument");
    if (n_aln >= (int64_t)0xFFFFFF00 || n_bc >= (int64_t)0x7FFFFF00) return fail(SMC_E_ARG, "smc_allele_carriers: run too large");
    if ((((uintptr_t)d_covers | (uintptr_t)d_carries | (uintptr_t)d_counts) & 7u) != 0) return fail(SMC_E_ARG, "smc_allele_carriers: outputs must be 8-byte aligned");
    for (int32_t v = 0; v < n_var; ++v) {
        const smc_af_variant& V = var_host[v];
        if ((int64_t)V.locus >= n_loci) return fail(SMC_E_INPUT, "smc_allele_carriers: variant " + std::to_string(v) + " names locus " + std::to_string(V.locus) + " of " + std::to_string(n_loci));
        if (V.kind > SMC_AF_NONE) return fail(SMC_E_INPUT, "smc_allele_carriers: variant " + std::to_string(v) + " has kind " + std::to_string(V.kind));
        if (V.kind == SMC_AF_INS && (V.len > SMC_AF_MAX_INS || (int64_t)V.ins_off + V.len > n_ins || (V.len && !d_ins)))
            return fail(SMC_E_INPUT, "smc_allele_carriers: variant " + std::to_string(v) + ": " + std::to_string(V.len) + " inserted letters at " +
                                     std::to_string(V.ins_off) + " (at most " + std::to_string(SMC_AF_MAX_INS) + ", pool of " + std::to_string(n_ins) + ")");
    }
    HIPCHK(hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const size_t n_cnt = 2 * (size_t)n_bc * (size_t)n_var;
    if (n_cnt >= (size_t)0xFFFFFF00) return fail(SMC_E_INPUT, "smc_allele_carriers: " + std::to_string(n_var) + " variants x " + std::to_string(n_bc) + " barcodes: too many counters for one call");
    if (!d_counts) {
        // (no stream to wait for: freeing the old block synchronises the device - no earlier call's kernels are in flight)
        if (int rc = grow_scratch(ctx->af_scratch, ctx->af_bytes, 4 * n_cnt, 4 * n_cnt + n_cnt / 2 + 256, "smc_allele_carriers", nullptr)) return rc;
        d_counts = (uint32_t*)ctx->af_scratch;
    }
    const uint32_t n_words64 = (uint32_t)((n_bc + 63) / 64);
    hipLaunchKernelGGL(k_bp_zero_words, dim3((unsigned)std::min<size_t>((n_cnt + 255) / 256, 4096)), dim3(256), 0, st, d_counts, (uint32_t)n_cnt);
    if (n_aln)
        hipLaunchKernelGGL(k_af_count, dim3((unsigned)std::min<int64_t>((n_aln + AF_BLOCK - 1) / AF_BLOCK, 64), (unsigned)n_var), dim3(AF_BLOCK), 0, st,
                           d_aln, (uint32_t)n_aln, d_cig, d_bq, d_loc, start0, d_var, d_ins, (uint32_t)n_bc, d_counts);
    hipLaunchKernelGGL(k_af_bits, dim3((n_words64 * WAVE + AF_BLOCK - 1) / AF_BLOCK, (unsigned)n_var), dim3(AF_BLOCK), 0, st,
                       (const uint32_t*)d_counts, (uint32_t)n_bc, n_words64, (unsigned long long*)d_covers, (unsigned long long*)d_carries);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--spikeAF, --spikeReps) what both rewrite entries check of the run and the listed variants, the variants on their host copy
// (`own_thr`: the variants' own thresholds count - smc_spike_alleles_reps takes one per copy instead)
static int spk_check(const std::string& who, smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, const uint8_t* d_bq,
                     int64_t n_pairs, const smc_spike_variant* d_var, const smc_spike_variant* var_host, int32_t n_var, const uint64_t* d_idents,
                     int64_t n_bc, const int32_t* d_nm, const int32_t* d_n_indel, const void* d_aln_out, const void* d_bq_out,
                     const uint32_t* d_stats, bool own_thr) {
    if (!ctx || n_aln < 0 || n_pairs < 0 || n_var < 0 || n_bc < 0) return fail(SMC_E_ARG, who + ": bad argument");
    if (n_var > SMC_AF_MAX_VARIANTS) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_var) + " variants, at most " + std::to_string(SMC_AF_MAX_VARIANTS));
    if (n_var && !var_host) return fail(SMC_E_ARG, who + ": NULL argument");
    auto acgt = [](uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; };
    for (int32_t v = 0; v < n_var; ++v) {
        const smc_spike_variant& V = var_host[v];
        const std::string w = who + ": variant " + std::to_string(v);
        if (v && var_host[v - 1].pos0 >= V.pos0) return fail(SMC_E_INPUT, w + ": the positions are not strictly ascending");
        if (!acgt(V.ref) || !acgt(V.alt)) return fail(SMC_E_INPUT, w + ": a letter outside ACGT");
        if (V.ref == V.alt) return fail(SMC_E_INPUT, w + ": ref equals alt");
        if (own_thr && V.thr > (1ull << 32)) return fail(SMC_E_INPUT, w + ": a threshold above 2^32");
        if ((int32_t)V.lead > v) return fail(SMC_E_INPUT, w + ": lead " + std::to_string(V.lead) + " points in front of the array");
        if (V.lead && var_host[v - (int32_t)V.lead].lead) return fail(SMC_E_INPUT, w + ": its leader has a lead of its own");
    }
    if (n_aln >= (int64_t)0xFFFFFF00 || n_bc >= (int64_t)0x7FFFFF00) return fail(SMC_E_ARG, who + ": run too large");
    if ((n_var && (!d_var || !d_stats)) || (n_aln && (!d_aln || !d_cig || !d_nm || !d_n_indel || !d_aln_out)) || (n_pairs && (!d_bq || !d_bq_out)) ||
        (n_bc && !d_idents))
        return fail(SMC_E_ARG, who + ": NULL argument");
    return SMC_OK;
}

// (--spikeAF) a run's records and pair pool copied, then k_spike_rewrite over the one copy, every variant at its own threshold
int smc_spike_alleles(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, const uint8_t* d_bq, int64_t n_pairs,
                      const smc_spike_variant* d_var, const smc_spike_variant* var_host, int32_t n_var, const uint64_t* d_idents,
                      int64_t n_bc, uint64_t seed, double mismatch_thr, const int32_t* d_nm, const int32_t* d_n_indel,
                      smc_dev_aln* d_aln_out, uint8_t* d_bq_out, uint32_t* d_stats, void* stream) {
    if (int rc = spk_check("smc_spike_alleles", ctx, d_aln, n_aln, d_cig, d_bq, n_pairs, d_var, var_host, n_var, d_idents, n_bc, d_nm, d_n_indel,
                           d_aln_out, d_bq_out, d_stats, true)) return rc;
    SpkCopies C;
    memset(&C, 0, sizeof C);
    C.seed[0] = seed;
    HIPCHK(hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    if (n_pairs) HIPCHK(hipMemcpyAsync(d_bq_out, d_bq, 2 * (size_t)n_pairs, hipMemcpyDeviceToDevice, st));
    if (n_var) hipLaunchKernelGGL(k_bp_zero_words, dim3((unsigned)((2 * n_var + 255) / 256)), dim3(256), 0, st, d_stats, (uint32_t)(2 * n_var));
    if (n_aln)
        hipLaunchKernelGGL(k_spike_rewrite, dim3((unsigned)((n_aln + SPK_BLOCK - 1) / SPK_BLOCK)), dim3(SPK_BLOCK), 0, st, d_aln, (uint32_t)n_aln,
                           d_cig, (unsigned long long)n_pairs, d_var, (int)n_var, (const unsigned long long*)d_idents, (uint32_t)n_bc, C, 1,
                           mismatch_thr, d_nm, d_n_indel, (uint8_t*)d_aln_out, 0ull, d_bq_out, 0ull, d_stats);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--spikeIndels, --spikeIndelReps) what the entries check of the listed variants, on their host copy.  `own_thr`: the variants' own
// thresholds count; `d_ins` / `n_ins`: the pool of inserted letters, not looked at without `with_ins` (smc_spike_indel_touch);
// `with_lead`: the entry draws, so `lead` must point at a leader inside the array (smc_spike_indel_touch does not read it)
static int spi_check_variants(const std::string& who, const smc_spike_indel_variant* var_host, int32_t n_var, const uint8_t* d_ins, int64_t n_ins,
                              bool with_ins, bool own_thr, bool with_lead) {
    if (n_var > SMC_AF_MAX_VARIANTS) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_var) + " variants, at most " + std::to_string(SMC_AF_MAX_VARIANTS));
    if (n_var && !var_host) return fail(SMC_E_ARG, who + ": NULL argument");
    auto acgt = [](uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; };
    auto fp_end = [](const smc_spike_indel_variant& V) {        // the last position of the footprint
        return (int64_t)V.pos0 + (V.kind == SMC_AF_SNV ? 0 : V.kind == SMC_AF_INS ? 1 : (int64_t)V.len + 1);
    };
    for (int32_t v = 0; v < n_var; ++v) {
        const smc_spike_indel_variant& V = var_host[v];
        const std::string w = who + ": variant " + std::to_string(v);
        if (V.kind > SMC_AF_DEL) return fail(SMC_E_INPUT, w + " has kind " + std::to_string(V.kind));
        if (v && var_host[v - 1].pos0 >= V.pos0) return fail(SMC_E_INPUT, w + ": the positions are not strictly ascending");
        if (!acgt(V.ref) || !acgt(V.alt)) return fail(SMC_E_INPUT, w + ": a letter outside ACGT");
        if (V.kind == SMC_AF_SNV ? V.ref == V.alt : V.ref != V.alt)
            return fail(SMC_E_INPUT, w + (V.kind == SMC_AF_SNV ? ": ref equals alt" : ": the anchor of an insertion / a deletion stands in ref and alt"));
        if (V.kind == SMC_AF_SNV ? V.len != 0 : (V.len < 1 || V.len > SMC_AF_MAX_INS))
            return fail(SMC_E_INPUT, w + ": a length of " + std::to_string(V.len) + " (1 .. " + std::to_string(SMC_AF_MAX_INS) + " for an insertion / a deletion, 0 for an SNV)");
        if (with_ins && V.kind == SMC_AF_INS && ((int64_t)V.ins_off + V.len > n_ins || !d_ins))
            return fail(SMC_E_INPUT, w + ": " + std::to_string(V.len) + " inserted letters at " + std::to_string(V.ins_off) + " (pool of " + std::to_string(n_ins) + ")");
        if (own_thr && V.thr > (1ull << 32)) return fail(SMC_E_INPUT, w + ": a threshold above 2^32");
        if (v && fp_end(var_host[v - 1]) >= (int64_t)V.pos0) return fail(SMC_E_INPUT, w + ": its footprint overlaps that of the variant before it");
        if (with_lead) {                                         // (--spikeIndelPhase: spk_check's two lines)
            if ((int32_t)V.lead > v) return fail(SMC_E_INPUT, w + ": lead " + std::to_string(V.lead) + " points in front of the array");
            if (V.lead && var_host[v - (int32_t)V.lead].lead) return fail(SMC_E_INPUT, w + ": its leader has a lead of its own");
        }
    }
    return SMC_OK;
}

// (--spikeIndels, --spikeIndelReps) the body of both rewrite entries: n_copies copies at byte strides (one copy, `own_thr`, strides 0:
// smc_spike_indels).  The pools reach the copies - hipMemcpyAsync for one, k_spike_pool for several -, then k_spi_count -> k_spi_scan ->
// k_spi_scatter with a row of the grid (a workgroup of the scan) per copy.
static int spi_copies(const std::string& who, smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, int64_t n_cig_words,
                      const uint8_t* d_bq, int64_t n_pairs, const smc_spike_indel_variant* d_var, const smc_spike_indel_variant* var_host,
                      int32_t n_var, const uint8_t* d_ins, int64_t n_ins, const uint64_t* d_idents, int64_t n_bc, const SpkCopies& C,
                      int32_t n_copies, bool own_thr, double mismatch_thr, const int32_t* d_nm, const int32_t* d_n_indel, int64_t cap_pairs,
                      int64_t cap_cig, uint8_t* d_aln_out, int64_t aln_stride, uint8_t* d_bq_out, int64_t bq_stride, uint8_t* d_cig_out,
                      int64_t cig_stride, int32_t* d_nm_out, int32_t* d_n_indel_out, uint32_t* d_stats, uint64_t* d_totals, void* stream) {
    if (!ctx || n_aln < 0 || n_pairs < 0 || n_cig_words < 0 || n_var < 0 || n_bc < 0 || n_ins < 0) return fail(SMC_E_ARG, who + ": bad argument");
    if (int rc = spi_check_variants(who, var_host, n_var, d_ins, n_ins, true, own_thr, true)) return rc;
    if (n_aln >= (int64_t)0xFFFFFF00 || n_bc >= (int64_t)0x7FFFFF00) return fail(SMC_E_ARG, who + ": run too large");
    if (cap_pairs < n_pairs || cap_cig < n_cig_words || cap_pairs > (int64_t)0xFFFFFFFF || cap_cig > (int64_t)0xFFFFFFFF)
        return fail(SMC_E_INPUT, who + ": capacities of " + std::to_string(cap_pairs) + " pairs / " + std::to_string(cap_cig) + " CIGAR words for a run of " +
                                 std::to_string(n_pairs) + " / " + std::to_string(n_cig_words) + " (at least the run's, below 2^32)");
    if ((n_var && (!d_var || !d_stats)) || (n_aln && (!d_aln || !d_cig || !d_nm || !d_n_indel || !d_aln_out || !d_nm_out || !d_n_indel_out)) ||
        (n_pairs && (!d_bq || !d_bq_out)) || (n_cig_words && (!d_cig || !d_cig_out)) || (n_bc && !d_idents) || !d_totals)
        return fail(SMC_E_ARG, who + ": NULL argument");
    if (((uintptr_t)d_totals & 7u) != 0) return fail(SMC_E_ARG, who + ": d_totals must be 8-byte aligned");
    HIPCHK(hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const size_t nb = ((size_t)n_aln + SPI_BLOCK - 1) / SPI_BLOCK;
    const size_t cnt_bytes = (8 * (size_t)n_aln * (size_t)n_copies + 15) & ~(size_t)15, need = cnt_bytes + 16 * std::max<size_t>(nb, 1) * (size_t)n_copies;
    if (int rc = grow_scratch(ctx->spi_scratch, ctx->spi_bytes, need, need + need / 8, who.c_str(), &st)) return rc;
    uint32_t* const cnt = (uint32_t*)ctx->spi_scratch;
    unsigned long long* const bsum = (unsigned long long*)((uint8_t*)ctx->spi_scratch + cnt_bytes);
    if (n_copies == 1) {
        if (n_pairs) HIPCHK(hipMemcpyAsync(d_bq_out, d_bq, 2 * (size_t)n_pairs, hipMemcpyDeviceToDevice, st));
        if (n_cig_words) HIPCHK(hipMemcpyAsync(d_cig_out, d_cig, 4 * (size_t)n_cig_words, hipMemcpyDeviceToDevice, st));
    } else {
        // (each pool read once and stored to every copy in 16-byte chunks, before the scatter appends behind it)
        auto pool = [&](const uint8_t* src, size_t n_bytes, uint8_t* dst, int64_t stride) {
            if (!n_bytes) return;
            hipLaunchKernelGGL(k_spike_pool, dim3((unsigned)std::min<size_t>(((n_bytes + 15) / 16 + SPR_BLOCK - 1) / SPR_BLOCK, 2048)), dim3(SPR_BLOCK), 0, st,
                               src, (unsigned long long)n_bytes, dst, (unsigned long long)stride, (int)n_copies);
        };
        pool(d_bq, 2 * (size_t)n_pairs, d_bq_out, bq_stride);
        pool((const uint8_t*)d_cig, 4 * (size_t)n_cig_words, d_cig_out, cig_stride);
    }
    const size_t n_st = 2 * (size_t)n_var * (size_t)n_copies;
    if (n_st) hipLaunchKernelGGL(k_bp_zero_words, dim3((unsigned)std::min<size_t>((n_st + 255) / 256, 4096)), dim3(256), 0, st, d_stats, (uint32_t)n_st);
    if (n_aln)
        hipLaunchKernelGGL(k_spi_count, dim3((unsigned)nb, (unsigned)n_copies), dim3(SPI_BLOCK), 0, st, d_aln, (uint32_t)n_aln, d_cig,
                           (unsigned long long)n_pairs, (unsigned long long)n_cig_words, d_var, (int)n_var, (const unsigned long long*)d_idents,
                           (uint32_t)n_bc, C, own_thr ? 1 : 0, cnt, bsum);
    hipLaunchKernelGGL(k_spi_scan, dim3((unsigned)n_copies), dim3(SPI_BLOCK), 0, st, bsum, (uint32_t)nb, (unsigned long long)n_pairs,
                       (unsigned long long)n_cig_words, (unsigned long long)cap_pairs, (unsigned long long)cap_cig, (unsigned long long*)d_totals);
    if (n_aln)
        hipLaunchKernelGGL(k_spi_scatter, dim3((unsigned)nb, (unsigned)n_copies), dim3(SPI_BLOCK), 0, st, d_aln, (uint32_t)n_aln, d_cig, d_bq,
                           (unsigned long long)n_pairs, (unsigned long long)n_cig_words, d_var, (int)n_var, d_ins, (const unsigned long long*)d_idents,
                           (uint32_t)n_bc, C, own_thr ? 1 : 0, mismatch_thr, d_nm, d_n_indel, (const uint32_t*)cnt, (const unsigned long long*)bsum,
                           (unsigned long long)cap_pairs, (unsigned long long)cap_cig, d_aln_out, (unsigned long long)aln_stride, d_bq_out,
                           (unsigned long long)bq_stride, d_cig_out, (unsigned long long)cig_stride, d_nm_out, d_n_indel_out, d_stats);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--spikeIndels) the run's records, pair pool and CIGAR pool copied; k_spi_count -> k_spi_scan -> k_spi_scatter behind the copies
int smc_spike_indels(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, int64_t n_cig_words, const uint8_t* d_bq,
                     int64_t n_pairs, const smc_spike_indel_variant* d_var, const smc_spike_indel_variant* var_host, int32_t n_var,
                     const uint8_t* d_ins, int64_t n_ins, const uint64_t* d_idents, int64_t n_bc, uint64_t seed, double mismatch_thr,
                     const int32_t* d_nm, const int32_t* d_n_indel, int64_t cap_pairs, int64_t cap_cig, smc_dev_aln* d_aln_out,
                     uint8_t* d_bq_out, uint32_t* d_cig_out, int32_t* d_nm_out, int32_t* d_n_indel_out, uint32_t* d_stats,
                     uint64_t* d_totals, void* stream) {
    SpkCopies C;
    memset(&C, 0, sizeof C);
    C.seed[0] = seed;
    return spi_copies("smc_spike_indels", ctx, d_aln, n_aln, d_cig, n_cig_words, d_bq, n_pairs, d_var, var_host, n_var, d_ins, n_ins, d_idents, n_bc,
                      C, 1, true, mismatch_thr, d_nm, d_n_indel, cap_pairs, cap_cig, (uint8_t*)d_aln_out, 0, d_bq_out, 0, (uint8_t*)d_cig_out, 0,
                      d_nm_out, d_n_indel_out, d_stats, d_totals, stream);
}

// (--spikeIndelReps) n_copies copies of smc_spike_indels from one call, every variant at the copy's threshold
int smc_spike_indels_reps(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, int64_t n_cig_words, const uint8_t* d_bq,
                          int64_t n_pairs, const smc_spike_indel_variant* d_var, const smc_spike_indel_variant* var_host, int32_t n_var,
                          const uint8_t* d_ins, int64_t n_ins, const uint64_t* d_idents, int64_t n_bc, const uint64_t* seeds, const uint64_t* thr,
                          int32_t n_copies, double mismatch_thr, const int32_t* d_nm, const int32_t* d_n_indel, int64_t cap_pairs,
                          int64_t cap_cig, uint8_t* d_aln_out, int64_t aln_stride, uint8_t* d_bq_out, int64_t bq_stride, uint8_t* d_cig_out,
                          int64_t cig_stride, int32_t* d_nm_out, int32_t* d_n_indel_out, uint32_t* d_stats, uint64_t* d_totals, void* stream) {
    const std::string who = "smc_spike_indels_reps";
    if (n_copies < 1 || n_copies > SMC_SPIKE_MAX_COPIES)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies, 1 .. " + std::to_string(SMC_SPIKE_MAX_COPIES) + " expected");
    if (!seeds || !thr) return fail(SMC_E_ARG, who + ": NULL argument");
    SpkCopies C;
    memset(&C, 0, sizeof C);
    for (int32_t c = 0; c < n_copies; ++c) {
        if (thr[c] > (1ull << 32)) return fail(SMC_E_INPUT, who + ": copy " + std::to_string(c) + ": a threshold above 2^32");
        C.seed[c] = seeds[c]; C.thr[c] = thr[c];
    }
    if (n_aln < 0 || cap_pairs < 0 || cap_cig < 0) return fail(SMC_E_ARG, who + ": bad argument");
    if (aln_stride < n_aln * (int64_t)sizeof(smc_dev_aln) || bq_stride < 2 * cap_pairs || cig_stride < 4 * cap_cig)
        return fail(SMC_E_INPUT, who + ": strides of " + std::to_string(aln_stride) + ", " + std::to_string(bq_stride) + " and " + std::to_string(cig_stride) +
                                 " bytes are smaller than a copy (" + std::to_string(n_aln * (int64_t)sizeof(smc_dev_aln)) + ", " +
                                 std::to_string(2 * cap_pairs) + " and " + std::to_string(4 * cap_cig) + " bytes)");
    if ((aln_stride & 3) || (bq_stride & 15) || (cig_stride & 15) ||
        (((uintptr_t)d_bq | (uintptr_t)d_bq_out | (uintptr_t)d_cig | (uintptr_t)d_cig_out) & 15u) || ((uintptr_t)d_aln_out & 3u))
        return fail(SMC_E_ARG, who + ": the record stride must be a multiple of 4 bytes, the pools' strides and addresses of 16");
    if ((double)n_copies * (double)n_var * 2.0 >= (double)0xFFFFFF00u)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies x " + std::to_string(n_var) + " variants: too many statistics words for one call");
    return spi_copies(who, ctx, d_aln, n_aln, d_cig, n_cig_words, d_bq, n_pairs, d_var, var_host, n_var, d_ins, n_ins, d_idents, n_bc, C, n_copies,
                      false, mismatch_thr, d_nm, d_n_indel, cap_pairs, cap_cig, d_aln_out, aln_stride, d_bq_out, bq_stride, d_cig_out, cig_stride,
                      d_nm_out, d_n_indel_out, d_stats, d_totals, stream);
}

// (--spikeIndelReps) per listed insertion / deletion and barcode of the run the records the rewrite changes when the barcode is spiked
int smc_spike_indel_touch(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, int64_t n_cig_words, int64_t n_pairs,
                          const smc_spike_indel_variant* d_var, const smc_spike_indel_variant* var_host, int32_t n_var, int64_t n_bc,
                          uint32_t* d_out, void* stream) {
    const std::string who = "smc_spike_indel_touch";
    if (!ctx || n_aln < 0 || n_pairs < 0 || n_cig_words < 0 || n_var < 0 || n_bc < 0) return fail(SMC_E_ARG, who + ": bad argument");
    if (int rc = spi_check_variants(who, var_host, n_var, nullptr, 0, false, false, false)) return rc;
    if (n_aln >= (int64_t)0xFFFFFF00 || n_bc >= (int64_t)0x7FFFFF00) return fail(SMC_E_ARG, who + ": run too large");
    if ((double)n_var * (double)n_bc >= (double)0xFFFFFF00u)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_var) + " variants x " + std::to_string(n_bc) + " barcodes: too many counters for one call");
    const size_t n_out = (size_t)n_var * (size_t)n_bc;
    if (!n_out) return SMC_OK;
    if (!d_var || !d_out || (n_aln && (!d_aln || !d_cig))) return fail(SMC_E_ARG, who + ": NULL argument");
    HIPCHK(hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_bp_zero_words, dim3((unsigned)std::min<size_t>((n_out + 255) / 256, 4096)), dim3(256), 0, st, d_out, (uint32_t)n_out);
    if (n_aln)
        hipLaunchKernelGGL(k_spi_touch, dim3((unsigned)(((size_t)n_aln + SPI_BLOCK - 1) / SPI_BLOCK)), dim3(SPI_BLOCK), 0, st, d_aln, (uint32_t)n_aln, d_cig,
                           (unsigned long long)n_pairs, (unsigned long long)n_cig_words, d_var, (int)n_var, (uint32_t)n_bc, d_out);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--spikeReps) n_copies spiked copies of a run: k_spike_pool stores the pair pool to every copy, k_spike_rewrite rewrites behind it,
// every variant at the copy's threshold
int smc_spike_alleles_reps(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, const uint8_t* d_bq, int64_t n_pairs,
                           const smc_spike_variant* d_var, const smc_spike_variant* var_host, int32_t n_var, const uint64_t* d_idents,
                           int64_t n_bc, const uint64_t* seeds, const uint64_t* thr, int32_t n_copies, double mismatch_thr,
                           const int32_t* d_nm, const int32_t* d_n_indel, uint8_t* d_aln_out, int64_t aln_stride, uint8_t* d_bq_out,
                           int64_t bq_stride, uint32_t* d_stats, void* stream) {
    const std::string who = "smc_spike_alleles_reps";
    if (int rc = spk_check(who, ctx, d_aln, n_aln, d_cig, d_bq, n_pairs, d_var, var_host, n_var, d_idents, n_bc, d_nm, d_n_indel, d_aln_out,
                           d_bq_out, d_stats, false)) return rc;
    if (n_copies < 1 || n_copies > SMC_SPIKE_MAX_COPIES)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies, 1 .. " + std::to_string(SMC_SPIKE_MAX_COPIES) + " expected");
    if (!seeds || !thr) return fail(SMC_E_ARG, who + ": NULL argument");
    SpkCopies C;
    memset(&C, 0, sizeof C);
    for (int32_t c = 0; c < n_copies; ++c) {
        if (thr[c] > (1ull << 32)) return fail(SMC_E_INPUT, who + ": copy " + std::to_string(c) + ": a threshold above 2^32");
        C.seed[c] = seeds[c]; C.thr[c] = thr[c];
    }
    if (aln_stride < n_aln * (int64_t)sizeof(smc_dev_aln) || bq_stride < 2 * n_pairs)
        return fail(SMC_E_INPUT, who + ": strides of " + std::to_string(aln_stride) + " and " + std::to_string(bq_stride) + " bytes are smaller than a copy (" +
                                 std::to_string(n_aln * (int64_t)sizeof(smc_dev_aln)) + " and " + std::to_string(2 * n_pairs) + " bytes)");
    if ((aln_stride & 3) || (bq_stride & 15) || (((uintptr_t)d_bq | (uintptr_t)d_bq_out) & 15u) || ((uintptr_t)d_aln_out & 3u))
        return fail(SMC_E_ARG, who + ": the record stride must be a multiple of 4 bytes, the pool stride and the pools' addresses of 16");
    if ((double)n_copies * (double)n_var * 2.0 >= (double)0xFFFFFF00u)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies x " + std::to_string(n_var) + " variants: too many statistics words for one call");
    HIPCHK(hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    if (n_pairs) {
        const size_t n_chunks = (2 * (size_t)n_pairs + 15) / 16;
        hipLaunchKernelGGL(k_spike_pool, dim3((unsigned)std::min<size_t>((n_chunks + SPR_BLOCK - 1) / SPR_BLOCK, 2048)), dim3(SPR_BLOCK), 0, st, d_bq,
                           2ull * (unsigned long long)n_pairs, d_bq_out, (unsigned long long)bq_stride, (int)n_copies);
    }
    const size_t n_st = 2 * (size_t)n_var * (size_t)n_copies;
    if (n_st) hipLaunchKernelGGL(k_bp_zero_words, dim3((unsigned)std::min<size_t>((n_st + 255) / 256, 4096)), dim3(256), 0, st, d_stats, (uint32_t)n_st);
    if (n_aln)
        hipLaunchKernelGGL(k_spike_rewrite, dim3((unsigned)((n_aln + SPK_BLOCK - 1) / SPK_BLOCK), (unsigned)n_copies), dim3(SPK_BLOCK), 0, st, d_aln,
                           (uint32_t)n_aln, d_cig, (unsigned long long)n_pairs, d_var, (int)n_var, (const unsigned long long*)d_idents, (uint32_t)n_bc,
                           C, 0, mismatch_thr, d_nm, d_n_indel, d_aln_out, (unsigned long long)aln_stride, d_bq_out, (unsigned long long)bq_stride, d_stats);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// What spk_cell_counts and spr_cell_counts check first, the axes both have: rows (`rows`: " variants" or " sets"), spike targets,
// replicates, and with `has_second` a second axis of the cells (`second`: " fractions" or " read thresholds"; second_thr its thresholds) -
// the limits, the NULL seeds and thresholds, then T filled from thr.  `bad`: what else makes the call a bad argument.
static int spk_axes(const std::string& who, const smc_ctx* ctx, bool bad, const std::string& rows, int32_t n_rows, const uint64_t* d_seeds,
                    int32_t n_reps, const uint64_t* thr, int32_t n_targets, bool has_second, const char* second, const uint64_t* second_thr,
                    int32_t n_second, SpkThr& T) {
    if (!ctx || n_rows < 0 || n_reps < 0 || n_targets < 0 || bad) return fail(SMC_E_ARG, who + ": bad argument");
    if (n_rows > SMC_AF_MAX_VARIANTS) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_rows) + rows + ", at most " + std::to_string(SMC_AF_MAX_VARIANTS));
    if (n_targets > SMC_SPIKE_REP_MAX_TARGETS)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_targets) + " targets, at most " + std::to_string(SMC_SPIKE_REP_MAX_TARGETS));
    if (n_reps > SMC_AF_REP_MAX_REPS) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_reps) + " replicates, at most " + std::to_string(SMC_AF_REP_MAX_REPS));
    if (has_second && n_second < 1) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_second) + second + ", at least 1 expected");
    if ((n_reps && !d_seeds) || (n_targets && !thr) || (has_second && !second_thr)) return fail(SMC_E_ARG, who + ": NULL argument");
    if (has_second && (int64_t)n_targets * (int64_t)n_second > SMC_AF_DEPTH_MAX_CELLS)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_targets) + " targets x " + std::to_string(n_second) + second + ", at most " +
                                 std::to_string(SMC_AF_DEPTH_MAX_CELLS) + " cells");
    memset(&T, 0, sizeof T);
    for (int32_t t = 0; t < n_targets; ++t) {
        if (thr[t] > (1ull << 32)) return fail(SMC_E_INPUT, who + ": target " + std::to_string(t) + ": a threshold above 2^32");
        T.t[t] = thr[t];
    }
    return SMC_OK;
}

// (--spikeReps, --spikeDepth, --spikePhase) what the three counts entries check, on the host copies and before anything is enqueued,
// then the counters zeroed and k_spike_cells.  A row is a listed variant, or with `sets` a phase set of set_m_host[g] members whose
// counters start at d_cnt_off[g].  Without `has_fracs` (smc_spike_rep_counts) the cells are those of one fraction that keeps every
// barcode.  `want`: k_spike_cells' mask of the counters the entry stores.
static int spk_cell_counts(const std::string& who, smc_ctx* ctx, const uint64_t* d_ident, const uint32_t* d_cnt, const uint32_t* d_off,
                           const uint32_t* off_host, bool sets, const uint32_t* d_set_m, const uint32_t* set_m_host, const uint32_t* d_cnt_off,
                           const uint32_t* d_pos1, int32_t n_rows, const uint64_t* d_seeds, int32_t n_reps, const uint64_t* thr,
                           int32_t n_targets, bool has_fracs, const uint64_t* depth_thr, int32_t n_fracs, uint32_t want, uint32_t* d_out,
                           void* stream, uint32_t cs = 3, uint32_t i_alt1 = 2, uint32_t i_touch = 2) {
    const std::string rows = sets ? " sets" : " variants", row = sets ? "set " : "variant ";
    const int n_want = __builtin_popcount(want);
    SpkThr T;
    if (int rc = spk_axes(who, ctx, false, rows, n_rows, d_seeds, n_reps, thr, n_targets, has_fracs, " fractions", depth_thr, n_fracs, T)) return rc;
    AfdThr D;
    memset(&D, 0, sizeof D);
    int with_depth = 0;
    if (!has_fracs) { n_fracs = 1; D.f[0] = 1ull << 32; }
    for (int32_t f = 0; has_fracs && f < n_fracs; ++f) {
        if (depth_thr[f] > (1ull << 32)) return fail(SMC_E_INPUT, who + ": depth threshold " + std::to_string(f) + " is above 2^32");
        if (f < SMC_AF_DEPTH_MAX_CELLS) D.f[f] = depth_thr[f];     // (more of them pass the cells' limit only without a target: nothing is launched)
        with_depth |= depth_thr[f] < (1ull << 32);
    }
    if ((double)n_rows * (double)n_reps * (double)n_targets * (double)n_fracs * (double)n_want >= (double)0xFFFFFF00u)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_rows) + rows + " x " + std::to_string(n_reps) + " replicates x " + std::to_string(n_targets) +
                                 " targets" + (has_fracs ? " x " + std::to_string(n_fracs) + " fractions" : "") + ": too many counters for one call");
    if (!n_rows || !n_reps || !n_targets) return SMC_OK;
    if (!off_host || !d_off || !d_pos1 || !d_out || (sets && (!set_m_host || !d_set_m || !d_cnt_off))) return fail(SMC_E_ARG, who + ": NULL argument");
    uint32_t widest = 0;
    double cnt_words = 0.0;
    for (int32_t g = 0; g < n_rows; ++g) {
        const uint32_t m = sets ? set_m_host[g] : 1u;
        if (m < 1 || m > SMC_SPIKE_PHASE_MAX_MEMBERS)
            return fail(SMC_E_INPUT, who + ": set " + std::to_string(g) + " has " + std::to_string(m) + " members, 1 .. " +
                                     std::to_string(SMC_SPIKE_PHASE_MAX_MEMBERS) + " expected");
        if (off_host[g + 1] < off_host[g]) return fail(SMC_E_INPUT, who + ": the offsets decrease at " + row + std::to_string(g));
        widest = std::max(widest, off_host[g + 1] - off_host[g]);
        cnt_words += (double)cs * (double)m * (double)(off_host[g + 1] - off_host[g]);
    }
    // (without sets and with three counters cnt_words is 3 * off_host[n_rows], below 2^32 - 256 with the first limit)
    if (off_host[n_rows] >= 0x55555500u || cnt_words >= (double)0xFFFFFF00u)
        return fail(SMC_E_INPUT, who + ": too many " + (sets ? "joint" : "covering") + " barcodes for one call");
    if (off_host[n_rows] && (!d_ident || !d_cnt)) return fail(SMC_E_ARG, who + (sets ? ": NULL joint barcodes" : ": NULL covers"));
    HIPCHK(hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const size_t n_out = (size_t)n_want * (size_t)n_rows * (size_t)n_reps * (size_t)n_targets * (size_t)n_fracs;
    hipLaunchKernelGGL(k_bp_zero_words, dim3((unsigned)std::min<size_t>((n_out + 255) / 256, 4096)), dim3(256), 0, st, d_out, (uint32_t)n_out);
    if (widest)
        hipLaunchKernelGGL(k_spike_cells, dim3((unsigned)std::min<uint32_t>((widest + SPR_BLOCK - 1) / SPR_BLOCK, 256u), (unsigned)n_rows,
                                               (unsigned)std::min<int32_t>(n_reps, 64)), dim3(SPR_BLOCK), 0, st,
                           (const unsigned long long*)d_ident, d_cnt, cs, i_alt1, i_touch, d_off, sets ? d_set_m : nullptr, sets ? d_cnt_off : nullptr, d_pos1, T,
                           (int)n_targets, D, (int)n_fracs, with_depth, (const unsigned long long*)d_seeds, (int)n_reps, want, d_out);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--spikeReps) (S, READS, V1) of every listed variant, replicate and target
int smc_spike_rep_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint32_t* d_cov_cnt, const uint32_t* d_cov_off,
                         const uint32_t* cov_off_host, const uint32_t* d_pos1, int32_t n_var, const uint64_t* d_seeds, int32_t n_reps,
                         const uint64_t* thr, int32_t n_targets, uint32_t* d_out, void* stream) {
    return spk_cell_counts("smc_spike_rep_counts", ctx, d_cov_ident, d_cov_cnt, d_cov_off, cov_off_host, false, nullptr, nullptr, nullptr, d_pos1,
                           n_var, d_seeds, n_reps, thr, n_targets, false, nullptr, 1, 0x1Cu, d_out, stream);
}

// (--spikeDepth) (N', V0', S', READS', V1') of every listed variant, replicate and cell (target x barcode fraction)
int smc_spike_depth_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint32_t* d_cov_cnt, const uint32_t* d_cov_off,
                           const uint32_t* cov_off_host, const uint32_t* d_pos1, int32_t n_var, const uint64_t* d_seeds, int32_t n_reps,
                           const uint64_t* thr, int32_t n_targets, const uint64_t* depth_thr, int32_t n_fracs, uint32_t* d_out, void* stream) {
    return spk_cell_counts("smc_spike_depth_counts", ctx, d_cov_ident, d_cov_cnt, d_cov_off, cov_off_host, false, nullptr, nullptr, nullptr,
                           d_pos1, n_var, d_seeds, n_reps, thr, n_targets, true, depth_thr, n_fracs, 0x1Fu, d_out, stream);
}

// (--spikeIndelReps, --spikeIndelDepth) smc_spike_rep_counts' numbers (depth_thr NULL) or smc_spike_depth_counts' from FOUR counters per
// covering barcode, (reads, alt0, alt1, touch): k_spike_cells with stride 4, car1 from column 2 and READS' from column 3
int smc_spike_indel_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint32_t* d_cov_cnt, const uint32_t* d_cov_off,
                           const uint32_t* cov_off_host, const uint32_t* d_pos1, int32_t n_var, const uint64_t* d_seeds, int32_t n_reps,
                           const uint64_t* thr, int32_t n_targets, const uint64_t* depth_thr, int32_t n_fracs, uint32_t* d_out, void* stream) {
    const bool cells = depth_thr != nullptr;
    return spk_cell_counts("smc_spike_indel_counts", ctx, d_cov_ident, d_cov_cnt, d_cov_off, cov_off_host, false, nullptr, nullptr, nullptr,
                           d_pos1, n_var, d_seeds, n_reps, thr, n_targets, cells, depth_thr, cells ? n_fracs : 1, cells ? 0x1Fu : 0x1Cu, d_out,
                           stream, 4, 2, 3);
}

// (--spikePhase) (N_ALL', V0_ALL', S_ALL', V1_ALL') of every phase set, replicate and cell
int smc_spike_phase_counts(smc_ctx* ctx, const uint64_t* d_joint_ident, const uint32_t* d_joint_cnt, const uint32_t* d_joint_off,
                           const uint32_t* joint_off_host, const uint32_t* d_set_m, const uint32_t* set_m_host, const uint32_t* d_cnt_off,
                           const uint32_t* d_pos1, int32_t n_sets, const uint64_t* d_seeds, int32_t n_reps, const uint64_t* thr,
                           int32_t n_targets, const uint64_t* depth_thr, int32_t n_fracs, uint32_t* d_out, void* stream) {
    return spk_cell_counts("smc_spike_phase_counts", ctx, d_joint_ident, d_joint_cnt, d_joint_off, joint_off_host, true, d_set_m, set_m_host,
                           d_cnt_off, d_pos1, n_sets, d_seeds, n_reps, thr, n_targets, true, depth_thr, n_fracs, 0x17u, d_out, stream);
}

// (--spikeIndelPhase) smc_spike_phase_counts' numbers from FOUR counters per joint barcode and member, (reads, alt0, alt1, touch):
// k_spike_cells with stride 4 and car1 from column 2 (READS' is not wanted: column 3 is not read for a set)
int smc_spike_indel_phase_counts(smc_ctx* ctx, const uint64_t* d_joint_ident, const uint32_t* d_joint_cnt, const uint32_t* d_joint_off,
                                 const uint32_t* joint_off_host, const uint32_t* d_set_m, const uint32_t* set_m_host, const uint32_t* d_cnt_off,
                                 const uint32_t* d_pos1, int32_t n_sets, const uint64_t* d_seeds, int32_t n_reps, const uint64_t* thr,
                                 int32_t n_targets, const uint64_t* depth_thr, int32_t n_fracs, uint32_t* d_out, void* stream) {
    return spk_cell_counts("smc_spike_indel_phase_counts", ctx, d_joint_ident, d_joint_cnt, d_joint_off, joint_off_host, true, d_set_m, set_m_host,
                           d_cnt_off, d_pos1, n_sets, d_seeds, n_reps, thr, n_targets, true, depth_thr, n_fracs, 0x17u, d_out, stream, 4, 2, 3);
}

// (--spikeRpb) per listed SNV of a run and alignment one byte: covers / shows ALT / single-letter key.  One launch, every byte written
int smc_spike_read_bits(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, int64_t n_cig_words, const uint8_t* d_bq,
                        int64_t n_pairs, const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0, const smc_af_variant* d_var,
                        const smc_af_variant* var_host, int32_t n_var, uint8_t* d_out, void* stream) {
    const std::string who = "smc_spike_read_bits";
    if (!ctx || n_aln < 0 || n_cig_words < 0 || n_pairs < 0 || n_loci < 0 || n_var < 0) return fail(SMC_E_ARG, who + ": bad argument");
    if (n_var > SMC_AF_MAX_VARIANTS) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_var) + " variants, at most " + std::to_string(SMC_AF_MAX_VARIANTS));
    if (n_var && !var_host) return fail(SMC_E_ARG, who + ": NULL argument");
    for (int32_t v = 0; v < n_var; ++v) {
        const smc_af_variant& V = var_host[v];
        if ((int64_t)V.locus >= n_loci)
            return fail(SMC_E_INPUT, who + ": variant " + std::to_string(v) + " names locus " + std::to_string(V.locus) + " of " + std::to_string(n_loci));
        if (V.kind != SMC_AF_SNV) return fail(SMC_E_INPUT, who + ": variant " + std::to_string(v) + " has kind " + std::to_string(V.kind) + ", an SNV expected");
    }
    if (n_aln >= (int64_t)0xFFFFFF00) return fail(SMC_E_ARG, who + ": run too large");
    if (!n_var || !n_aln) return SMC_OK;
    if (!d_aln || !d_cig || !d_bq || !d_loc || !d_var || !d_out) return fail(SMC_E_ARG, who + ": NULL argument");
    HIPCHK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_spr_bits, dim3((unsigned)std::min<int64_t>((n_aln + SPB_BLOCK - 1) / SPB_BLOCK, 1024), (unsigned)n_var), dim3(SPB_BLOCK), 0,
                       (hipStream_t)stream, d_aln, (uint32_t)n_aln, d_cig, (unsigned long long)n_cig_words, d_bq, (unsigned long long)n_pairs, d_loc,
                       start0, d_var, d_out);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--spikeScan) one verdict per (copy, listed locus) of a called batch: everything checked on the host copy before anything is
// enqueued, then the cursor zeroed and one launch (none for an empty list or no copy)
int smc_scan_detect(smc_ctx* ctx, const smc_row* d_rows, int32_t n_copies, int64_t n_loci, const smc_scan_locus* d_listed,
                    const smc_scan_locus* listed_host, int32_t n_listed, double thr, smc_scan_verdict* d_out, uint32_t* d_host_list,
                    uint32_t* d_n_host, void* stream) {
    const std::string who = "smc_scan_detect";
    static_assert(sizeof(smc_scan_verdict) == 16 && sizeof(smc_scan_locus) == 8, "smc_scan_detect's records");
    if (!ctx || n_copies < 0 || n_loci < 0 || n_listed < 0 || !d_n_host) return fail(SMC_E_ARG, who + ": bad argument");
    if (n_listed && !listed_host) return fail(SMC_E_ARG, who + ": NULL argument");
    if (!std::isfinite(thr)) return fail(SMC_E_INPUT, who + ": a threshold that is not finite");
    if (n_copies > 65535) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies, at most 65535");
    if ((int64_t)n_copies * (int64_t)n_listed >= (1ll << 31) || (int64_t)n_copies * n_loci >= (1ll << 31))
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies of " + std::to_string(n_loci) + " loci, " +
                                 std::to_string(n_listed) + " listed: 2^31 records or rows, or more");
    for (int32_t g = 0; g < n_listed; ++g) {
        if ((int64_t)listed_host[g].offset >= n_loci)
            return fail(SMC_E_INPUT, who + ": listed locus " + std::to_string(g) + " names offset " + std::to_string(listed_host[g].offset) +
                                     " of " + std::to_string(n_loci));
        if (listed_host[g].alt > 3u)
            return fail(SMC_E_INPUT, who + ": listed locus " + std::to_string(g) + " has allele id " + std::to_string(listed_host[g].alt) +
                                     ", one of 0 .. 3 expected");
    }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemsetAsync(d_n_host, 0, sizeof(uint32_t), (hipStream_t)stream));
    if (!n_listed || !n_copies) return SMC_OK;
    if (!d_rows || !d_listed || !d_out || !d_host_list) return fail(SMC_E_ARG, who + ": NULL argument");
    const double edge = thr - 0.005;
    hipLaunchKernelGGL(k_scan_detect, dim3((unsigned)std::min<int64_t>(((int64_t)n_listed + SCD_BLOCK - 1) / SCD_BLOCK, 1024), (unsigned)n_copies),
                       dim3(SCD_BLOCK), 0, (hipStream_t)stream, d_rows, (uint32_t)n_loci, d_listed, (uint32_t)n_listed, edge - 1e-6, edge + 1e-6,
                       d_out, d_host_list, d_n_host);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--spikeScanMnv) smc_scan_detect with the listed records tiled by phase sets: smc_scan_detect's checks and those of the offsets on
// the host copies before anything is enqueued, then the cursor zeroed and one launch (none for an empty list or no copy)
int smc_scan_detect_sets(smc_ctx* ctx, const smc_row* d_rows, int32_t n_copies, int64_t n_loci, const smc_scan_locus* d_listed,
                         const smc_scan_locus* listed_host, int32_t n_listed, const uint32_t* d_set_off, const uint32_t* set_off_host,
                         int32_t n_sets, double thr, smc_scan_verdict* d_out, uint32_t* d_joint, uint32_t* d_host_list, uint32_t* d_n_host,
                         void* stream) {
    const std::string who = "smc_scan_detect_sets";
    if (!ctx || n_copies < 0 || n_loci < 0 || n_listed < 0 || n_sets < 0 || !d_n_host || !set_off_host) return fail(SMC_E_ARG, who + ": bad argument");
    if (n_listed && !listed_host) return fail(SMC_E_ARG, who + ": NULL argument");
    if (!std::isfinite(thr)) return fail(SMC_E_INPUT, who + ": a threshold that is not finite");
    if (n_copies > 65535) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies, at most 65535");
    if ((int64_t)n_copies * (int64_t)n_listed >= (1ll << 31) || (int64_t)n_copies * n_loci >= (1ll << 31) ||
        (int64_t)n_copies * (int64_t)n_sets >= (1ll << 31))
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies of " + std::to_string(n_loci) + " loci, " +
                                 std::to_string(n_listed) + " listed in " + std::to_string(n_sets) + " sets: 2^31 records, rows or sets, or more");
    for (int32_t g = 0; g < n_listed; ++g) {
        if ((int64_t)listed_host[g].offset >= n_loci)
            return fail(SMC_E_INPUT, who + ": listed locus " + std::to_string(g) + " names offset " + std::to_string(listed_host[g].offset) +
                                     " of " + std::to_string(n_loci));
        if (listed_host[g].alt > 3u)
            return fail(SMC_E_INPUT, who + ": listed locus " + std::to_string(g) + " has allele id " + std::to_string(listed_host[g].alt) +
                                     ", one of 0 .. 3 expected");
    }
    if (set_off_host[0] != 0u || (int64_t)set_off_host[n_sets] != (int64_t)n_listed)
        return fail(SMC_E_INPUT, who + ": the sets' offsets run from " + std::to_string(set_off_host[0]) + " to " + std::to_string(set_off_host[n_sets]) +
                                 ", they must tile the " + std::to_string(n_listed) + " listed records");
    for (int32_t s = 0; s < n_sets; ++s) {
        const int64_t m = (int64_t)set_off_host[s + 1] - (int64_t)set_off_host[s];
        if (m < 1 || m > SMC_SPIKE_PHASE_MAX_MEMBERS)
            return fail(SMC_E_INPUT, who + ": set " + std::to_string(s) + " has " + std::to_string(m) + " members, 1 .. " +
                                     std::to_string(SMC_SPIKE_PHASE_MAX_MEMBERS) + " expected");
    }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemsetAsync(d_n_host, 0, sizeof(uint32_t), (hipStream_t)stream));
    if (!n_listed || !n_copies) return SMC_OK;
    if (!d_rows || !d_listed || !d_set_off || !d_out || !d_joint || !d_host_list) return fail(SMC_E_ARG, who + ": NULL argument");
    const double edge = thr - 0.005;
    const int64_t per_block = SCD_BLOCK / SCD_SET_LANES;
    hipLaunchKernelGGL(k_scan_detect_sets, dim3((unsigned)std::min<int64_t>(((int64_t)n_sets + per_block - 1) / per_block, 1024), (unsigned)n_copies),
                       dim3(SCD_BLOCK), 0, (hipStream_t)stream, d_rows, (uint32_t)n_loci, d_listed, (uint32_t)n_listed, d_set_off, (uint32_t)n_sets,
                       edge - 1e-6, edge + 1e-6, d_out, d_joint, d_host_list, d_n_host);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--spikeScanFilter) the FILTER word per (copy, listed locus) of a called batch: everything checked on the host copies before
// anything is enqueued, then one launch (none for an empty list or no copy)
int smc_scan_filter(smc_ctx* ctx, const smc_row* d_rows, int32_t n_copies, int64_t n_loci, const uint32_t* d_offsets,
                    const uint32_t* offsets_host, const uint32_t* d_gate, const uint32_t* gate_host, const uint32_t* d_always,
                    const uint32_t* always_host, int32_t n_listed, uint32_t* d_out, void* stream) {
    const std::string who = "smc_scan_filter";
    if (!ctx || n_copies < 0 || n_loci < 0 || n_listed < 0) return fail(SMC_E_ARG, who + ": bad argument");
    if (n_listed && (!d_rows || !d_offsets || !offsets_host || !d_gate || !gate_host || !d_always || !always_host || !d_out))
        return fail(SMC_E_INPUT, who + ": NULL argument with " + std::to_string(n_listed) + " listed loci");
    if (n_copies > 65535) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies, at most 65535");
    if ((int64_t)n_copies * (int64_t)n_listed >= (1ll << 31) || (int64_t)n_copies * n_loci >= (1ll << 31))
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies of " + std::to_string(n_loci) + " loci, " +
                                 std::to_string(n_listed) + " listed: 2^31 words or rows, or more");
    const uint32_t gate_ok = SMC_F_HP | SMC_F_LOWC, always_ok = SMC_F_LOWC | SMC_F_REPT | SMC_F_REPS | SMC_F_SL | SMC_F_OTHER_REPEAT;
    for (int32_t g = 0; g < n_listed; ++g) {
        if ((int64_t)offsets_host[g] >= n_loci)
            return fail(SMC_E_INPUT, who + ": listed locus " + std::to_string(g) + " names offset " + std::to_string(offsets_host[g]) +
                                     " of " + std::to_string(n_loci));
        if (gate_host[g] & ~gate_ok)
            return fail(SMC_E_INPUT, who + ": listed locus " + std::to_string(g) + " has gate bits " + std::to_string(gate_host[g]) +
                                     ", HP and LowC expected");
        if (always_host[g] & ~always_ok)
            return fail(SMC_E_INPUT, who + ": listed locus " + std::to_string(g) + " has always bits " + std::to_string(always_host[g]) +
                                     ", LowC and the repeat names expected");
    }
    if (!n_listed || !n_copies) return SMC_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const double edge = 4.995;
    hipLaunchKernelGGL(k_scan_filter, dim3((unsigned)std::min<int64_t>(((int64_t)n_listed + SCD_BLOCK - 1) / SCD_BLOCK, 1024), (unsigned)n_copies),
                       dim3(SCD_BLOCK), 0, (hipStream_t)stream, d_rows, (uint32_t)n_loci, d_offsets, d_gate, d_always, (uint32_t)n_listed,
                       edge - 1e-6, edge + 1e-6, d_out);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--spikeScanMnvFilter) smc_scan_filter with the listed loci tiled by phase sets: smc_scan_filter's checks and smc_scan_detect_sets'
// of the offsets on the host copies before anything is enqueued, then one launch (none for an empty list or no copy)
int smc_scan_filter_sets(smc_ctx* ctx, const smc_row* d_rows, int32_t n_copies, int64_t n_loci, const uint32_t* d_offsets,
                         const uint32_t* offsets_host, const uint32_t* d_gate, const uint32_t* gate_host, const uint32_t* d_always,
                         const uint32_t* always_host, int32_t n_listed, const uint32_t* d_set_off, const uint32_t* set_off_host,
                         int32_t n_sets, uint32_t* d_members, uint32_t* d_joint_flt, void* stream) {
    const std::string who = "smc_scan_filter_sets";
    if (!ctx || n_copies < 0 || n_loci < 0 || n_listed < 0 || n_sets < 0) return fail(SMC_E_ARG, who + ": bad argument");
    if (!set_off_host) return fail(SMC_E_INPUT, who + ": NULL argument: the sets' offsets");
    if (n_listed && (!d_rows || !d_offsets || !offsets_host || !d_gate || !gate_host || !d_always || !always_host || !d_set_off ||
                     !d_members || !d_joint_flt))
        return fail(SMC_E_INPUT, who + ": NULL argument with " + std::to_string(n_listed) + " listed loci");
    if (n_copies > 65535) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies, at most 65535");
    if ((int64_t)n_copies * (int64_t)n_listed >= (1ll << 31) || (int64_t)n_copies * n_loci >= (1ll << 31) ||
        (int64_t)n_copies * (int64_t)n_sets >= (1ll << 31))
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies of " + std::to_string(n_loci) + " loci, " +
                                 std::to_string(n_listed) + " listed in " + std::to_string(n_sets) + " sets: 2^31 words, rows or sets, or more");
    const uint32_t gate_ok = SMC_F_HP | SMC_F_LOWC, always_ok = SMC_F_LOWC | SMC_F_REPT | SMC_F_REPS | SMC_F_SL | SMC_F_OTHER_REPEAT;
    for (int32_t g = 0; g < n_listed; ++g) {
        if ((int64_t)offsets_host[g] >= n_loci)
            return fail(SMC_E_INPUT, who + ": listed locus " + std::to_string(g) + " names offset " + std::to_string(offsets_host[g]) +
                                     " of " + std::to_string(n_loci));
        if (gate_host[g] & ~gate_ok)
            return fail(SMC_E_INPUT, who + ": listed locus " + std::to_string(g) + " has gate bits " + std::to_string(gate_host[g]) +
                                     ", HP and LowC expected");
        if (always_host[g] & ~always_ok)
            return fail(SMC_E_INPUT, who + ": listed locus " + std::to_string(g) + " has always bits " + std::to_string(always_host[g]) +
                                     ", LowC and the repeat names expected");
    }
    if (set_off_host[0] != 0u || (int64_t)set_off_host[n_sets] != (int64_t)n_listed)
        return fail(SMC_E_INPUT, who + ": the sets' offsets run from " + std::to_string(set_off_host[0]) + " to " + std::to_string(set_off_host[n_sets]) +
                                 ", they must tile the " + std::to_string(n_listed) + " listed loci");
    for (int32_t s = 0; s < n_sets; ++s) {
        const int64_t m = (int64_t)set_off_host[s + 1] - (int64_t)set_off_host[s];
        if (m < 1 || m > SMC_SPIKE_PHASE_MAX_MEMBERS)
            return fail(SMC_E_INPUT, who + ": set " + std::to_string(s) + " has " + std::to_string(m) + " members, 1 .. " +
                                     std::to_string(SMC_SPIKE_PHASE_MAX_MEMBERS) + " expected");
    }
    if (!n_listed || !n_copies) return SMC_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const double edge = 4.995;
    const int64_t per_block = SCD_BLOCK / SCD_SET_LANES;
    hipLaunchKernelGGL(k_scan_filter_sets, dim3((unsigned)std::min<int64_t>(((int64_t)n_sets + per_block - 1) / per_block, 1024), (unsigned)n_copies),
                       dim3(SCD_BLOCK), 0, (hipStream_t)stream, d_rows, (uint32_t)n_loci, d_offsets, d_gate, d_always, (uint32_t)n_listed,
                       d_set_off, (uint32_t)n_sets, edge - 1e-6, edge + 1e-6, d_members, d_joint_flt);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--spikeScanIndel) smc_scan_detect for lists whose members are allele keys: the same checks, and those of the listed records, of the
// strides and of the pool, on the host copies before anything is enqueued; then the cursor zeroed and three launches (none for an
// empty list or no copy)
int smc_scan_detect_keys(smc_ctx* ctx, const smc_row* d_rows, int32_t n_copies, int64_t n_loci, const smc_af_variant* d_var,
                         const smc_af_variant* var_host, int32_t n_listed, const uint8_t* d_ins, int64_t n_ins, const smc_dev_aln* d_aln,
                         int64_t aln_stride, const uint32_t* d_cig, int64_t cig_stride, const uint8_t* d_bq, int64_t bq_stride, int64_t n_aln,
                         int64_t cap_pairs, const uint32_t* d_x, int64_t x_stride, const uint32_t* d_xcount, int64_t xcount_stride,
                         int64_t xcap, double thr, uint32_t* d_alt_id, smc_scan_verdict* d_out, uint32_t* d_host_list, uint32_t* d_n_host,
                         void* stream) {
    const std::string who = "smc_scan_detect_keys";
    if (!ctx || n_copies < 0 || n_loci < 0 || n_listed < 0 || n_ins < 0 || n_aln < 0 || cap_pairs < 0 || xcap < 0 || !d_n_host)
        return fail(SMC_E_ARG, who + ": bad argument");
    if (n_listed && !var_host) return fail(SMC_E_ARG, who + ": NULL argument");
    if (!std::isfinite(thr)) return fail(SMC_E_INPUT, who + ": a threshold that is not finite");
    if (n_copies > 65535) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies, at most 65535");
    if ((int64_t)n_copies * (int64_t)n_listed >= (1ll << 31) || (int64_t)n_copies * n_loci >= (1ll << 31))
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies of " + std::to_string(n_loci) + " loci, " +
                                 std::to_string(n_listed) + " listed: 2^31 records or rows, or more");
    if (n_aln >= (int64_t)0xFFFFFF00 || xcap >= (1ll << 31)) return fail(SMC_E_INPUT, who + ": run too large");
    // (a byte stride keeps its array aligned: records and CIGAR words 4 bytes, pairs 2; 0: the copies share the array)
    if (aln_stride < 0 || aln_stride % 4 || cig_stride < 0 || cig_stride % 4 || bq_stride < 0 || bq_stride % 2 || x_stride < 0 || xcount_stride < 0)
        return fail(SMC_E_INPUT, who + ": strides of " + std::to_string(aln_stride) + " / " + std::to_string(cig_stride) + " / " +
                                 std::to_string(bq_stride) + " bytes: multiples of 4 / 4 / 2 expected, none negative");
    bool keys = false;
    for (int32_t g = 0; g < n_listed; ++g) {
        const smc_af_variant& V = var_host[g];
        const std::string w = who + ": listed variant " + std::to_string(g);
        if ((int64_t)V.locus >= n_loci) return fail(SMC_E_INPUT, w + " names locus " + std::to_string(V.locus) + " of " + std::to_string(n_loci));
        if (g && V.locus < var_host[g - 1].locus) return fail(SMC_E_INPUT, w + ": locus " + std::to_string(V.locus) + " behind " +
                                                                           std::to_string(var_host[g - 1].locus) + ", ascending expected");
        if (V.kind > SMC_AF_NONE) return fail(SMC_E_INPUT, w + " has kind " + std::to_string(V.kind));
        if (V.kind == SMC_AF_SNV && V.letter != 'A' && V.letter != 'T' && V.letter != 'G' && V.letter != 'C')
            return fail(SMC_E_INPUT, w + ": an SNV to letter " + std::to_string(V.letter) + ", one of A, C, G, T expected");
        if (V.kind == SMC_AF_INS || V.kind == SMC_AF_DEL) {
            keys = true;
            if (V.len < 1 || V.len > SMC_AF_MAX_INS)
                return fail(SMC_E_INPUT, w + ": a length of " + std::to_string(V.len) + ", 1 .. " + std::to_string(SMC_AF_MAX_INS) + " expected");
            if (V.kind == SMC_AF_INS && ((int64_t)V.ins_off + V.len > n_ins || !d_ins))
                return fail(SMC_E_INPUT, w + ": " + std::to_string(V.len) + " inserted letters at " + std::to_string(V.ins_off) +
                                         " of a pool of " + std::to_string(n_ins));
        }
    }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemsetAsync(d_n_host, 0, sizeof(uint32_t), (hipStream_t)stream));
    if (!n_listed || !n_copies) return SMC_OK;
    if (!d_rows || !d_var || !d_alt_id || !d_out || !d_host_list) return fail(SMC_E_ARG, who + ": NULL argument");
    if (keys && xcap && (!d_aln || !d_bq || !d_x || !d_xcount)) return fail(SMC_E_ARG, who + ": NULL argument");
    const unsigned gx = (unsigned)std::min<int64_t>(((int64_t)n_listed + SCD_BLOCK - 1) / SCD_BLOCK, 1024);
    hipLaunchKernelGGL(k_sdk_init, dim3(gx, (unsigned)n_copies), dim3(SCD_BLOCK), 0, (hipStream_t)stream, d_var, (uint32_t)n_listed, d_alt_id);
    if (keys && xcap) {
        (void)d_cig;                    // (an entry holds the query position and the indel the walk resolved: no CIGAR is read)
        SdkCopies C;
        C.aln = (const uint8_t*)d_aln; C.aln_stride = (unsigned long long)aln_stride;
        C.bq = d_bq; C.bq_stride = (unsigned long long)bq_stride;
        C.n_aln = (uint32_t)n_aln; C.cap_pairs = (unsigned long long)cap_pairs;
        C.x = d_x; C.x_stride = (unsigned long long)x_stride;
        C.xcount = d_xcount; C.xcount_stride = (unsigned long long)xcount_stride;
        C.xcap = (uint32_t)xcap;
        hipLaunchKernelGGL(k_sdk_resolve, dim3((unsigned)std::min<int64_t>((xcap + SCD_BLOCK - 1) / SCD_BLOCK, 1024), (unsigned)n_copies),
                           dim3(SCD_BLOCK), 0, (hipStream_t)stream, C, d_var, (uint32_t)n_listed, d_ins, d_alt_id);
    }
    const double edge = thr - 0.005;
    hipLaunchKernelGGL(k_sdk_detect, dim3(gx, (unsigned)n_copies), dim3(SCD_BLOCK), 0, (hipStream_t)stream, d_rows, (uint32_t)n_loci, d_var,
                       (uint32_t)n_listed, d_alt_id, edge - 1e-6, edge + 1e-6, d_out, d_host_list, d_n_host);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// What spr_cell_counts and smc_spike_grid_counts check of the rows and their record segments, on the host copies -> `widest`: the most
// barcodes a row has.
static int spr_check_segments(const std::string& who, bool sets, const uint64_t* d_ident, const uint32_t* d_off, const uint32_t* off_host,
                              const uint32_t* d_set_m, const uint32_t* set_m_host, const uint32_t* d_seg_base, const uint32_t* seg_base_host,
                              const uint32_t* d_rec_off, const uint32_t* rec_off_host, const uint64_t* d_rec_name, const uint8_t* d_rec_flag,
                              int64_t n_rec, const uint32_t* d_pos1, int32_t n_rows, const uint32_t* d_out, uint32_t& widest) {
    const std::string row = sets ? "set " : "variant ";
    if (!off_host || !d_off || !d_pos1 || !d_out || (sets && (!set_m_host || !d_set_m || !seg_base_host || !d_seg_base)))
        return fail(SMC_E_ARG, who + ": NULL argument");
    widest = 0;
    uint64_t n_seg = 0;
    for (int32_t g = 0; g < n_rows; ++g) {
        const uint32_t m = sets ? set_m_host[g] : 1u;
        if (m < 1 || m > SMC_SPIKE_PHASE_MAX_MEMBERS)
            return fail(SMC_E_INPUT, who + ": set " + std::to_string(g) + " has " + std::to_string(m) + " members, 1 .. " +
                                     std::to_string(SMC_SPIKE_PHASE_MAX_MEMBERS) + " expected");
        if (off_host[g + 1] < off_host[g]) return fail(SMC_E_INPUT, who + ": the offsets decrease at " + row + std::to_string(g));
        if (sets && (uint64_t)seg_base_host[g] != n_seg)
            return fail(SMC_E_INPUT, who + ": the segments of set " + std::to_string(g) + " start at " + std::to_string(seg_base_host[g]) + ", " +
                                     std::to_string(n_seg) + " expected");
        widest = std::max(widest, off_host[g + 1] - off_host[g]);
        n_seg += (uint64_t)m * (uint64_t)(off_host[g + 1] - off_host[g]);
    }
    if (!sets) n_seg = off_host[n_rows];                           // (a variant's segment is its barcode's index in the covers, whatever off_host[0] is)
    if (off_host[n_rows] >= 0x55555500u || n_seg >= 0xFFFFFF00ull)
        return fail(SMC_E_INPUT, who + ": too many " + (sets ? "joint" : "covering") + " barcodes for one call");
    if (n_seg) {
        if (!d_ident || !d_rec_off || !rec_off_host) return fail(SMC_E_ARG, who + (sets ? ": NULL joint barcodes" : ": NULL covers"));
        for (uint64_t s = 0; s < n_seg; ++s)
            if (rec_off_host[s + 1] < rec_off_host[s])
                return fail(SMC_E_INPUT, who + ": the record offsets decrease at " + (sets ? "segment " : "covering barcode ") + std::to_string(s));
        if ((int64_t)rec_off_host[n_seg] > n_rec)
            return fail(SMC_E_INPUT, who + ": the record offsets end at " + std::to_string(rec_off_host[n_seg]) + ", beyond the " + std::to_string(n_rec) + " records");
        if (n_rec && (!d_rec_name || !d_rec_flag)) return fail(SMC_E_ARG, who + ": NULL records");
    }
    return SMC_OK;
}

// (the counts entries over records) the two axes of the cells - spk_axes' checks, the read thresholds into `Q`, the counters' limit
static int spr_cells(const std::string& who, const smc_ctx* ctx, bool bad, const std::string& rows, size_t n_counters, int32_t n_rows,
                     const uint64_t* d_seeds, int32_t n_reps, const uint64_t* thr, int32_t n_targets, const uint64_t* read_thr,
                     int32_t n_read_thr, SpkThr& T, RgThr& Q) {
    if (int rc = spk_axes(who, ctx, bad, rows, n_rows, d_seeds, n_reps, thr, n_targets, true, " read thresholds", read_thr, n_read_thr, T)) return rc;
    memset(&Q, 0, sizeof Q);
    for (int32_t r = 0; r < n_read_thr; ++r) {
        if (read_thr[r] > (1ull << 32)) return fail(SMC_E_INPUT, who + ": read threshold " + std::to_string(r) + " is above 2^32");
        if (r < SMC_RG_MAX_TARGETS) Q.t[r] = read_thr[r];         // (more of them pass the cells' limit only without a target: nothing is launched)
    }
    if ((double)n_rows * (double)n_reps * (double)n_targets * (double)n_read_thr * (double)n_counters >= (double)0xFFFFFF00u)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_rows) + rows + " x " + std::to_string(n_reps) + " replicates x " + std::to_string(n_targets) +
                                 " targets x " + std::to_string(n_read_thr) + " read thresholds: too many counters for one call");
    return SMC_OK;
}

// (--spikeRpb, --spikeIndelRpb, --spikePhaseRpb) what the three counts entries check, on the host copies and before anything is
// enqueued, then the counters zeroed and k_spr_counts.  A row is a listed variant: (N', V0', S', READS', V1') per replicate and cell
// (spike target x read threshold) from the records of its covering barcodes, segment e the records of barcode e - with `four` the
// instance that reads alt1 and touch from flag bits 2 and 3, else the one in which bit 2 is both.  Or with `sets` a phase set of
// set_m_host[g] members: (N_ALL', V0_ALL', S_ALL', V1_ALL') from the records of every (joint barcode, member); the segment bases are
// the running sums of (joint barcodes x members), so no lane reads an offset beyond the n_seg + 1 there are.
static int spr_cell_counts(const std::string& who, bool four, bool sets, smc_ctx* ctx, const uint64_t* d_ident, const uint32_t* d_off,
                           const uint32_t* off_host, const uint32_t* d_set_m, const uint32_t* set_m_host, const uint32_t* d_seg_base,
                           const uint32_t* seg_base_host, const uint32_t* d_rec_off, const uint32_t* rec_off_host, const uint64_t* d_rec_name,
                           const uint8_t* d_rec_flag, int64_t n_rec, const uint32_t* d_pos1, int32_t n_rows, const uint64_t* d_seeds,
                           int32_t n_reps, const uint64_t* thr, int32_t n_targets, const uint64_t* read_thr, int32_t n_read_thr,
                           uint32_t* d_out, void* stream) {
    const std::string rows = sets ? " sets" : " variants";
    const size_t n_counters = sets ? SPP_COUNTERS : SPC_COUNTERS;
    SpkThr T;
    RgThr Q;
    if (int rc = spr_cells(who, ctx, n_rec < 0, rows, n_counters, n_rows, d_seeds, n_reps, thr, n_targets, read_thr, n_read_thr, T, Q)) return rc;
    if (n_rec >= (int64_t)0xFFFFFF00) return fail(SMC_E_INPUT, who + ": too many covering records for one call");
    if (!n_rows || !n_reps || !n_targets) return SMC_OK;
    uint32_t widest = 0;
    if (int rc = spr_check_segments(who, sets, d_ident, d_off, off_host, d_set_m, set_m_host, d_seg_base, seg_base_host, d_rec_off, rec_off_host,
                                    d_rec_name, d_rec_flag, n_rec, d_pos1, n_rows, d_out, widest)) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const size_t n_out = n_counters * (size_t)n_rows * (size_t)n_reps * (size_t)n_targets * (size_t)n_read_thr;
    hipLaunchKernelGGL(k_bp_zero_words, dim3((unsigned)std::min<size_t>((n_out + 255) / 256, 4096)), dim3(256), 0, st, d_out, (uint32_t)n_out);
    const bool few = n_read_thr <= 8;
    const auto kernel = sets   ? (few ? k_spr_counts<8, false, true> : k_spr_counts<SMC_RG_MAX_TARGETS, false, true>)
                        : four ? (few ? k_spr_counts<8, true, false> : k_spr_counts<SMC_RG_MAX_TARGETS, true, false>)
                               : (few ? k_spr_counts<8, false, false> : k_spr_counts<SMC_RG_MAX_TARGETS, false, false>);
    if (widest)
        hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<uint32_t>((widest + SPB_BLOCK - 1) / SPB_BLOCK, 256u), (unsigned)n_rows,
                                        (unsigned)std::min<int32_t>(n_reps, 64)), dim3(SPB_BLOCK), 0, st,
                           (const unsigned long long*)d_ident, d_off, sets ? d_set_m : nullptr, sets ? d_seg_base : nullptr, d_rec_off,
                           (const unsigned long long*)d_rec_name, d_rec_flag, (uint32_t)n_rec, d_pos1, T, (int)n_targets, Q, (int)n_read_thr,
                           (const unsigned long long*)d_seeds, (int)n_reps, d_out);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--spikeRpb) flag bit 2 of a record is `single`
int smc_spike_rpb_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint32_t* d_cov_off, const uint32_t* cov_off_host,
                         const uint32_t* d_rec_off, const uint32_t* rec_off_host, const uint64_t* d_rec_name, const uint8_t* d_rec_flag,
                         int64_t n_rec, const uint32_t* d_pos1, int32_t n_var, const uint64_t* d_seeds, int32_t n_reps, const uint64_t* thr,
                         int32_t n_targets, const uint64_t* read_thr, int32_t n_read_thr, uint32_t* d_out, void* stream) {
    return spr_cell_counts("smc_spike_rpb_counts", false, false, ctx, d_cov_ident, d_cov_off, cov_off_host, nullptr, nullptr, nullptr, nullptr,
                           d_rec_off, rec_off_host, d_rec_name, d_rec_flag, n_rec, d_pos1, n_var, d_seeds, n_reps, thr, n_targets, read_thr,
                           n_read_thr, d_out, stream);
}

// (--spikeGrid) smc_spike_rpb_counts' numbers per cell (spike target x barcode fraction x read threshold): the barcode rule's
// thresholds by value, the read thresholds per replicate in device memory (rd_thr_host: the same words on the host, for the checks).
// A pair (fraction, read threshold) takes the place of smc_spike_rpb_counts' read threshold; k_spg_counts for 8 pairs or for 32.
int smc_spike_grid_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint32_t* d_cov_off, const uint32_t* cov_off_host,
                          const uint32_t* d_rec_off, const uint32_t* rec_off_host, const uint64_t* d_rec_name, const uint8_t* d_rec_flag,
                          int64_t n_rec, const uint32_t* d_pos1, int32_t n_var, const uint64_t* d_seeds, int32_t n_reps, const uint64_t* thr,
                          int32_t n_targets, const uint64_t* bc_thr, int32_t n_fracs, const uint64_t* d_rd_thr, const uint64_t* rd_thr_host,
                          int32_t n_read_thr, uint32_t* d_out, void* stream) {
    const std::string who = "smc_spike_grid_counts";
    if (n_fracs < 0 || n_read_thr < 0) return fail(SMC_E_ARG, who + ": bad argument");
    if (n_fracs < 1) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_fracs) + " fractions, at least 1 expected");
    if (n_read_thr < 1) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_read_thr) + " read thresholds, at least 1 expected");
    const int64_t n_pairs = (int64_t)n_fracs * (int64_t)n_read_thr;
    SpkThr T;
    if (int rc = spk_axes(who, ctx, n_rec < 0, " variants", n_var, d_seeds, n_reps, thr, n_targets, true, " fraction x read-threshold pairs", bc_thr,
                          (int32_t)std::min<int64_t>(n_pairs, INT32_MAX), T)) return rc;
    AfdThr D;
    memset(&D, 0, sizeof D);
    for (int32_t f = 0; f < n_fracs; ++f) {
        if (bc_thr[f] > (1ull << 32)) return fail(SMC_E_INPUT, who + ": depth threshold " + std::to_string(f) + " is above 2^32");
        if (f < SMC_AF_DEPTH_MAX_CELLS) D.f[f] = bc_thr[f];          // (more of them pass the cells' limit only without a target: nothing is launched)
    }
    if ((double)n_var * (double)n_reps * (double)n_targets * (double)n_pairs * (double)SPC_COUNTERS >= (double)0xFFFFFF00u)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_var) + " variants x " + std::to_string(n_reps) + " replicates x " + std::to_string(n_targets) +
                                 " targets x " + std::to_string(n_fracs) + " fractions x " + std::to_string(n_read_thr) + " read thresholds: too many counters for one call");
    if (n_rec >= (int64_t)0xFFFFFF00) return fail(SMC_E_INPUT, who + ": too many covering records for one call");
    if (!n_var || !n_reps || !n_targets) return SMC_OK;
    if (!d_rd_thr || !rd_thr_host) return fail(SMC_E_ARG, who + ": NULL argument");
    for (int64_t k = 0; k < (int64_t)n_reps * n_pairs; ++k)         // (n_pairs <= SMC_AF_DEPTH_MAX_CELLS here: a target there is)
        if (rd_thr_host[k] > (1ull << 32))
            return fail(SMC_E_INPUT, who + ": read threshold " + std::to_string(k % n_pairs) + " of replicate " + std::to_string(k / n_pairs) + " is above 2^32");
    uint32_t widest = 0;
    if (int rc = spr_check_segments(who, false, d_cov_ident, d_cov_off, cov_off_host, nullptr, nullptr, nullptr, nullptr, d_rec_off, rec_off_host,
                                    d_rec_name, d_rec_flag, n_rec, d_pos1, n_var, d_out, widest)) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const size_t n_out = (size_t)SPC_COUNTERS * (size_t)n_var * (size_t)n_reps * (size_t)n_targets * (size_t)n_pairs;
    hipLaunchKernelGGL(k_bp_zero_words, dim3((unsigned)std::min<size_t>((n_out + 255) / 256, 4096)), dim3(256), 0, st, d_out, (uint32_t)n_out);
    const auto kernel = n_pairs <= 8 ? k_spg_counts<8> : k_spg_counts<SMC_AF_DEPTH_MAX_CELLS>;
    if (widest)
        hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<uint32_t>((widest + SPB_BLOCK - 1) / SPB_BLOCK, 256u), (unsigned)n_var,
                                        (unsigned)std::min<int32_t>(n_reps, 64)), dim3(SPB_BLOCK), 0, st,
                           (const unsigned long long*)d_cov_ident, d_cov_off, d_rec_off, (const unsigned long long*)d_rec_name, d_rec_flag,
                           (uint32_t)n_rec, d_pos1, T, (int)n_targets, D, (int)n_fracs, (int)n_read_thr, (const unsigned long long*)d_rd_thr,
                           (const unsigned long long*)d_seeds, (int)n_reps, d_out);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--spikeIndelRpb) the same from FOUR bits per record: flag bit 2 = alt1, bit 3 = touch (smc_spike_indel_read_bits' bits 2 and 3)
int smc_spike_indel_rpb_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint32_t* d_cov_off, const uint32_t* cov_off_host,
                               const uint32_t* d_rec_off, const uint32_t* rec_off_host, const uint64_t* d_rec_name, const uint8_t* d_rec_flag,
                               int64_t n_rec, const uint32_t* d_pos1, int32_t n_var, const uint64_t* d_seeds, int32_t n_reps,
                               const uint64_t* thr, int32_t n_targets, const uint64_t* read_thr, int32_t n_read_thr, uint32_t* d_out,
                               void* stream) {
    return spr_cell_counts("smc_spike_indel_rpb_counts", true, false, ctx, d_cov_ident, d_cov_off, cov_off_host, nullptr, nullptr, nullptr,
                           nullptr, d_rec_off, rec_off_host, d_rec_name, d_rec_flag, n_rec, d_pos1, n_var, d_seeds, n_reps, thr, n_targets,
                           read_thr, n_read_thr, d_out, stream);
}

// (--spikePhaseRpb) the joint numbers of every phase set
int smc_spike_phase_rpb_counts(smc_ctx* ctx, const uint64_t* d_joint_ident, const uint32_t* d_joint_off, const uint32_t* joint_off_host,
                               const uint32_t* d_set_m, const uint32_t* set_m_host, const uint32_t* d_seg_base, const uint32_t* seg_base_host,
                               const uint32_t* d_rec_off, const uint32_t* rec_off_host, const uint64_t* d_rec_name, const uint8_t* d_rec_flag,
                               int64_t n_rec, const uint32_t* d_pos1, int32_t n_sets, const uint64_t* d_seeds, int32_t n_reps,
                               const uint64_t* thr, int32_t n_targets, const uint64_t* read_thr, int32_t n_read_thr, uint32_t* d_out,
                               void* stream) {
    return spr_cell_counts("smc_spike_phase_rpb_counts", false, true, ctx, d_joint_ident, d_joint_off, joint_off_host, d_set_m, set_m_host,
                           d_seg_base, seg_base_host, d_rec_off, rec_off_host, d_rec_name, d_rec_flag, n_rec, d_pos1, n_sets, d_seeds, n_reps,
                           thr, n_targets, read_thr, n_read_thr, d_out, stream);
}

// (--spikeScanMnvRpb) smc_spike_phase_rpb_counts' words from the run in barcode-major order and the read bits in HBM: no record CSR.
// Everything is checked on the host copies before anything is enqueued; what only the device holds (d_bm_aln, d_joint_gid) is bounded
// by the kernel itself.
int smc_scan_phase_rpb_counts(smc_ctx* ctx, const uint32_t* d_bm_aln, const uint64_t* d_bm_name, const uint8_t* d_bm_first, int64_t n_aln,
                              const uint32_t* d_bc_start, const uint32_t* bc_start_host, const uint64_t* d_idents, int64_t n_bc,
                              const uint8_t* d_bits, int32_t n_var, const uint32_t* d_row_off, const uint32_t* row_off_host,
                              const uint32_t* d_row_var, const uint32_t* row_var_host, const uint32_t* d_joint_off,
                              const uint32_t* joint_off_host, const uint32_t* d_joint_gid, const uint32_t* d_pos1, int32_t n_rows,
                              const uint64_t* d_seeds, int32_t n_reps, const uint64_t* thr, int32_t n_targets, const uint64_t* read_thr,
                              int32_t n_read_thr, uint32_t* d_out, void* stream) {
    const std::string who = "smc_scan_phase_rpb_counts";
    SpkThr T;
    RgThr Q;
    if (int rc = spr_cells(who, ctx, n_aln < 0 || n_bc < 0 || n_var < 0, " rows", SPP_COUNTERS, n_rows, d_seeds, n_reps, thr, n_targets, read_thr,
                           n_read_thr, T, Q)) return rc;
    if (n_aln >= (int64_t)0xFFFFFF00 || n_bc >= (int64_t)0xFFFFFF00) return fail(SMC_E_INPUT, who + ": run too large for one call");
    if (!n_rows || !n_reps || !n_targets) return SMC_OK;
    if (!row_off_host || !d_row_off || !joint_off_host || !d_joint_off || !d_pos1 || !d_out || !bc_start_host || !d_bc_start)
        return fail(SMC_E_ARG, who + ": NULL argument");
    uint32_t widest = 0;
    for (int32_t g = 0; g < n_rows; ++g) {
        if (row_off_host[g + 1] < row_off_host[g]) return fail(SMC_E_INPUT, who + ": the row offsets decrease at row " + std::to_string(g));
        const uint32_t m = row_off_host[g + 1] - row_off_host[g];
        if (m < 1 || m > SMC_SPIKE_PHASE_MAX_MEMBERS)
            return fail(SMC_E_INPUT, who + ": row " + std::to_string(g) + " has " + std::to_string(m) + " members, 1 .. " +
                                     std::to_string(SMC_SPIKE_PHASE_MAX_MEMBERS) + " expected");
        if (joint_off_host[g + 1] < joint_off_host[g]) return fail(SMC_E_INPUT, who + ": the joint offsets decrease at row " + std::to_string(g));
        widest = std::max(widest, joint_off_host[g + 1] - joint_off_host[g]);
    }
    if (!row_var_host || !d_row_var) return fail(SMC_E_ARG, who + ": NULL members");
    for (uint32_t k = row_off_host[0]; k < row_off_host[n_rows]; ++k)
        if ((int64_t)row_var_host[k] >= (int64_t)n_var)
            return fail(SMC_E_INPUT, who + ": member " + std::to_string(k) + " names bit row " + std::to_string(row_var_host[k]) + " of " + std::to_string(n_var));
    for (int64_t b = 0; b < n_bc; ++b)
        if (bc_start_host[b + 1] < bc_start_host[b]) return fail(SMC_E_INPUT, who + ": the barcode starts decrease at barcode " + std::to_string(b));
    if ((int64_t)bc_start_host[n_bc] != n_aln)
        return fail(SMC_E_INPUT, who + ": the barcode starts end at " + std::to_string(bc_start_host[n_bc]) + ", not at the " + std::to_string(n_aln) + " alignments");
    if (widest && (!d_joint_gid || (n_bc && !d_idents) || (n_aln && (!d_bm_aln || !d_bm_name || !d_bm_first || !d_bits))))
        return fail(SMC_E_ARG, who + ": NULL run");
    HIPCHK(hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const size_t n_out = (size_t)SPP_COUNTERS * (size_t)n_rows * (size_t)n_reps * (size_t)n_targets * (size_t)n_read_thr;
    hipLaunchKernelGGL(k_bp_zero_words, dim3((unsigned)std::min<size_t>((n_out + 255) / 256, 4096)), dim3(256), 0, st, d_out, (uint32_t)n_out);
    SprRun src;
    memset(&src, 0, sizeof src);
    src.bm_aln = d_bm_aln; src.bm_name = (const unsigned long long*)d_bm_name; src.bm_first = d_bm_first; src.bc_start = d_bc_start;
    src.idents = (const unsigned long long*)d_idents; src.bits = d_bits; src.row_off = d_row_off; src.row_var = d_row_var;
    src.joint_gid = d_joint_gid; src.n_aln = (uint32_t)n_aln; src.n_bc = (uint32_t)n_bc;
    const auto kernel = n_read_thr <= 8 ? k_spr_run_counts<8> : k_spr_run_counts<SMC_RG_MAX_TARGETS>;     // (as spr_cell_counts chooses)
    if (widest)
        hipLaunchKernelGGL(kernel, dim3((unsigned)std::min<uint32_t>((widest + SPB_BLOCK - 1) / SPB_BLOCK, 256u), (unsigned)n_rows,
                                        (unsigned)std::min<int32_t>(n_reps, 64)), dim3(SPB_BLOCK), 0, st,
                           src, d_joint_off, d_pos1, T, (int)n_targets, Q, (int)n_read_thr, (const unsigned long long*)d_seeds, (int)n_reps, d_out);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--spikeIndelRpb) per listed variant of a run - an SNV, an insertion, a deletion - and alignment one byte: covers / shows the key /
// alt1 / touch.  One launch, every byte written
int smc_spike_indel_read_bits(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, int64_t n_cig_words,
                              const uint8_t* d_bq, int64_t n_pairs, const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0,
                              const smc_spike_indel_variant* d_var, const smc_spike_indel_variant* var_host, int32_t n_var,
                              const uint8_t* d_ins, int64_t n_ins, uint8_t* d_out, void* stream) {
    const std::string who = "smc_spike_indel_read_bits";
    if (!ctx || n_aln < 0 || n_cig_words < 0 || n_pairs < 0 || n_loci < 0 || n_var < 0 || n_ins < 0) return fail(SMC_E_ARG, who + ": bad argument");
    // (kinds, ascending positions, letters, lengths, the inserted letters inside the pool, disjoint footprints; no draw: thr and lead are not read)
    if (int rc = spi_check_variants(who, var_host, n_var, d_ins, n_ins, true, false, false)) return rc;
    for (int32_t v = 0; v < n_var; ++v) {
        const int64_t locus = (int64_t)var_host[v].pos0 - (int64_t)start0;
        if (locus < 0 || locus >= n_loci)
            return fail(SMC_E_INPUT, who + ": variant " + std::to_string(v) + " names locus " + std::to_string(locus) + " of " + std::to_string(n_loci));
    }
    if (n_aln >= (int64_t)0xFFFFFF00) return fail(SMC_E_ARG, who + ": run too large");
    if (!n_var || !n_aln) return SMC_OK;
    if (!d_aln || !d_cig || !d_bq || !d_loc || !d_var || !d_out) return fail(SMC_E_ARG, who + ": NULL argument");
    HIPCHK(hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_spr_indel_bits, dim3((unsigned)std::min<int64_t>((n_aln + SPB_BLOCK - 1) / SPB_BLOCK, 1024), (unsigned)n_var), dim3(SPB_BLOCK), 0,
                       (hipStream_t)stream, d_aln, (uint32_t)n_aln, d_cig, (unsigned long long)n_cig_words, d_bq, (unsigned long long)n_pairs, d_loc,
                       start0, d_var, (int)n_var, d_ins, d_out);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

// (--dsAFReps, --dsAFDepth) what the four entries check of the carrier table, on its host copy, and of the fractions' thresholds
// (host memory), which go into the kernels' argument -> `with_depth`: a fraction is below 2^32, so the depth draw decides something
static int afd_check_table(const std::string& w, const uint64_t* d_car, const uint64_t* d_car_thr, const uint64_t* car_host,
                           const uint64_t* car_thr_host, int64_t n_car, int32_t n_targets, const uint64_t* depth_thr, int32_t n_fracs,
                           const uint64_t* d_seeds, int32_t n_reps, AfdThr& D, int& with_depth) {
    if (n_car < 0 || n_car >= (int64_t)0x7FFFFF00 || n_targets < 0 || n_reps < 0) return fail(SMC_E_ARG, w + ": bad argument");
    if (n_targets > SMC_AF_REP_MAX_TARGETS) return fail(SMC_E_INPUT, w + ": " + std::to_string(n_targets) + " targets, at most " + std::to_string(SMC_AF_REP_MAX_TARGETS));
    if (n_reps > SMC_AF_REP_MAX_REPS) return fail(SMC_E_INPUT, w + ": " + std::to_string(n_reps) + " replicates, at most " + std::to_string(SMC_AF_REP_MAX_REPS));
    if (n_reps && !d_seeds) return fail(SMC_E_ARG, w + ": NULL seeds");
    if (n_car && (!d_car || !car_host || (n_targets && (!d_car_thr || !car_thr_host)))) return fail(SMC_E_ARG, w + ": NULL carrier table");
    for (int64_t c = 1; c < n_car; ++c)
        if (car_host[c - 1] >= car_host[c])
            return fail(SMC_E_INPUT, w + ": the carrier table is not strictly ascending at entry " + std::to_string(c));
    for (int64_t k = 0; k < n_car * (int64_t)n_targets; ++k)
        if (car_thr_host[k] > (1ull << 32))
            return fail(SMC_E_INPUT, w + ": threshold " + std::to_string(k) + " of the carrier table is above 2^32");
    if (n_fracs < 0 || (n_fracs && !depth_thr)) return fail(SMC_E_ARG, w + ": bad depth thresholds");
    if ((int64_t)n_targets * (int64_t)n_fracs > SMC_AF_DEPTH_MAX_CELLS)
        return fail(SMC_E_INPUT, w + ": " + std::to_string(n_targets) + " targets x " + std::to_string(n_fracs) + " fractions, at most " +
                                 std::to_string(SMC_AF_DEPTH_MAX_CELLS) + " cells");
    memset(&D, 0, sizeof D);
    with_depth = 0;
    for (int f = 0; f < n_fracs; ++f) {
        if (depth_thr[f] > (1ull << 32)) return fail(SMC_E_INPUT, w + ": depth threshold " + std::to_string(f) + " is above 2^32");
        D.f[f] = depth_thr[f];
        with_depth |= depth_thr[f] < (1ull << 32);
    }
    return SMC_OK;
}

// The replicate entries are the depth entries at one fraction of 2^32 (every barcode passes the depth rule): one body per call.
// `who`: the entry, for the messages; `frac_text`: whether they name the fractions (the replicate entries have none to name).
static const uint64_t AFR_ONE_FRACTION[1] = {1ull << 32};
static std::string afd_fracs_text(bool frac_text, int32_t n_fracs) { return frac_text ? " x " + std::to_string(n_fracs) + " fractions" : std::string(); }

static int af_cell_masks(const char* who, bool frac_text, smc_ctx* ctx, const uint64_t* d_idents, int64_t n_ids, const uint64_t* d_car,
                         const uint64_t* d_car_thr, const uint64_t* car_host, const uint64_t* car_thr_host, int64_t n_car, int32_t n_targets,
                         const uint64_t* depth_thr, int32_t n_fracs, const uint64_t* d_seeds, int32_t n_reps, uint32_t* d_masks,
                         int64_t n_words, uint32_t* d_draws_af, uint32_t* d_draws_depth, void* stream) {
    const std::string w(who);
    if (!ctx || n_ids < 0 || n_ids >= (int64_t)0x7FFFFF00 || n_words < 0) return fail(SMC_E_ARG, w + ": bad argument");
    AfdThr D;
    int with_depth;
    { const int rc = afd_check_table(w, d_car, d_car_thr, car_host, car_thr_host, n_car, n_targets, depth_thr, n_fracs, d_seeds, n_reps, D, with_depth); if (rc) return rc; }
    if (n_words < (n_ids + 31) / 32)
        return fail(SMC_E_INPUT, w + ": " + std::to_string(n_words) + " words per mask for " + std::to_string(n_ids) + " ids");
    if ((double)n_reps * (double)n_targets * (double)n_fracs * (double)n_words >= (double)0xFFFFFF00u)
        return fail(SMC_E_INPUT, w + ": " + std::to_string(n_reps) + " replicates x " + std::to_string(n_targets) + " targets" +
                                 afd_fracs_text(frac_text, n_fracs) + " x " + std::to_string(n_words) + " words: too many mask words for one call");
    if (!n_reps || !n_targets || !n_fracs || !n_words) return SMC_OK;
    if (!d_masks || (n_ids && !d_idents)) return fail(SMC_E_ARG, w + ": NULL argument");
    HIPCHK(hipSetDevice(ctx->device));
    const unsigned gx = (unsigned)(((n_words + 1) / 2 * WAVE + AFR_BLOCK - 1) / AFR_BLOCK);      // (two words per wave)
    hipLaunchKernelGGL(k_afd_masks, dim3(gx, (unsigned)std::min<int32_t>(n_reps, 64)), dim3(AFR_BLOCK), 0, (hipStream_t)stream,
                       (const unsigned long long*)d_idents, (uint32_t)n_ids, (const unsigned long long*)d_car, (const unsigned long long*)d_car_thr,
                       (uint32_t)n_car, (int)n_targets, D, (int)n_fracs, (int)(with_depth || d_draws_depth), (const unsigned long long*)d_seeds,
                       (int)n_reps, d_masks, (uint32_t)n_words, d_draws_af, d_draws_depth);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

static int af_cell_counts(const char* who, bool frac_text, smc_ctx* ctx, const uint64_t* d_cov_ident, const uint8_t* d_cov_carry,
                          const uint32_t* d_cov_off, const uint32_t* cov_off_host, int32_t n_var, const uint64_t* d_car, const uint64_t* d_car_thr,
                          const uint64_t* car_host, const uint64_t* car_thr_host, int64_t n_car, int32_t n_targets, const uint64_t* depth_thr,
                          int32_t n_fracs, const uint64_t* d_seeds, int32_t n_reps, uint32_t* d_out, void* stream) {
    const std::string w(who);
    if (!ctx || n_var < 0) return fail(SMC_E_ARG, w + ": bad argument");
    if (n_var > SMC_AF_MAX_VARIANTS) return fail(SMC_E_INPUT, w + ": " + std::to_string(n_var) + " variants, at most " + std::to_string(SMC_AF_MAX_VARIANTS));
    AfdThr D;
    int with_depth;
    { const int rc = afd_check_table(w, d_car, d_car_thr, car_host, car_thr_host, n_car, n_targets, depth_thr, n_fracs, d_seeds, n_reps, D, with_depth); if (rc) return rc; }
    if ((double)n_var * (double)n_reps * (double)n_targets * (double)n_fracs * 2.0 >= (double)0xFFFFFF00u)
        return fail(SMC_E_INPUT, w + ": " + std::to_string(n_var) + " variants x " + std::to_string(n_reps) + " replicates x " +
                                 std::to_string(n_targets) + " targets" + afd_fracs_text(frac_text, n_fracs) + ": too many counters for one call");
    if (!n_var || !n_reps || !n_targets || !n_fracs) return SMC_OK;
    if (!cov_off_host || !d_cov_off || !d_out) return fail(SMC_E_ARG, w + ": NULL argument");
    uint32_t widest = 0;
    for (int32_t v = 0; v < n_var; ++v) {
        if (cov_off_host[v + 1] < cov_off_host[v]) return fail(SMC_E_INPUT, w + ": the offsets decrease at variant " + std::to_string(v));
        widest = std::max(widest, cov_off_host[v + 1] - cov_off_host[v]);
    }
    if (cov_off_host[n_var] >= 0xFFFFFF00u) return fail(SMC_E_INPUT, w + ": too many covering barcodes for one call");
    if (cov_off_host[n_var] && (!d_cov_ident || !d_cov_carry)) return fail(SMC_E_ARG, w + ": NULL covers");
    HIPCHK(hipSetDevice(ctx->device));
    const hipStream_t st = (hipStream_t)stream;
    const size_t n_out = 2 * (size_t)n_var * (size_t)n_reps * (size_t)n_targets * (size_t)n_fracs;
    hipLaunchKernelGGL(k_bp_zero_words, dim3((unsigned)std::min<size_t>((n_out + 255) / 256, 4096)), dim3(256), 0, st, d_out, (uint32_t)n_out);
    if (widest)
        hipLaunchKernelGGL(k_afd_counts, dim3((unsigned)std::min<uint32_t>((widest + AFR_BLOCK - 1) / AFR_BLOCK, 256u), (unsigned)n_var,
                                              (unsigned)std::min<int32_t>(n_reps, 64)), dim3(AFR_BLOCK), 0, st,
                           (const unsigned long long*)d_cov_ident, d_cov_carry, d_cov_off, (const unsigned long long*)d_car,
                           (const unsigned long long*)d_car_thr, (uint32_t)n_car, (int)n_targets, D, (int)n_fracs, with_depth,
                           (const unsigned long long*)d_seeds, (int)n_reps, d_out);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

int smc_af_rep_masks(smc_ctx* ctx, const uint64_t* d_idents, int64_t n_ids, const uint64_t* d_car, const uint64_t* d_car_thr,
                     const uint64_t* car_host, const uint64_t* car_thr_host, int64_t n_car, int32_t n_targets, const uint64_t* d_seeds,
                     int32_t n_reps, uint32_t* d_masks, int64_t n_words, uint32_t* d_draws, void* stream) {
    return af_cell_masks("smc_af_rep_masks", false, ctx, d_idents, n_ids, d_car, d_car_thr, car_host, car_thr_host, n_car, n_targets,
                         AFR_ONE_FRACTION, 1, d_seeds, n_reps, d_masks, n_words, d_draws, nullptr, stream);
}

int smc_af_rep_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint8_t* d_cov_carry, const uint32_t* d_cov_off,
                      const uint32_t* cov_off_host, int32_t n_var, const uint64_t* d_car, const uint64_t* d_car_thr,
                      const uint64_t* car_host, const uint64_t* car_thr_host, int64_t n_car, int32_t n_targets, const uint64_t* d_seeds,
                      int32_t n_reps, uint32_t* d_out, void* stream) {
    return af_cell_counts("smc_af_rep_counts", false, ctx, d_cov_ident, d_cov_carry, d_cov_off, cov_off_host, n_var, d_car, d_car_thr,
                          car_host, car_thr_host, n_car, n_targets, AFR_ONE_FRACTION, 1, d_seeds, n_reps, d_out, stream);
}

int smc_af_depth_masks(smc_ctx* ctx, const uint64_t* d_idents, int64_t n_ids, const uint64_t* d_car, const uint64_t* d_car_thr,
                       const uint64_t* car_host, const uint64_t* car_thr_host, int64_t n_car, int32_t n_targets,
                       const uint64_t* depth_thr, int32_t n_fracs, const uint64_t* d_seeds, int32_t n_reps, uint32_t* d_masks,
                       int64_t n_words, uint32_t* d_draws, void* stream) {
    return af_cell_masks("smc_af_depth_masks", true, ctx, d_idents, n_ids, d_car, d_car_thr, car_host, car_thr_host, n_car, n_targets,
                         depth_thr, n_fracs, d_seeds, n_reps, d_masks, n_words, nullptr, d_draws, stream);
}

int smc_af_depth_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint8_t* d_cov_carry, const uint32_t* d_cov_off,
                        const uint32_t* cov_off_host, int32_t n_var, const uint64_t* d_car, const uint64_t* d_car_thr,
                        const uint64_t* car_host, const uint64_t* car_thr_host, int64_t n_car, int32_t n_targets,
                        const uint64_t* depth_thr, int32_t n_fracs, const uint64_t* d_seeds, int32_t n_reps, uint32_t* d_out, void* stream) {
    return af_cell_counts("smc_af_depth_counts", true, ctx, d_cov_ident, d_cov_carry, d_cov_off, cov_off_host, n_var, d_car, d_car_thr,
                          car_host, car_thr_host, n_car, n_targets, depth_thr, n_fracs, d_seeds, n_reps, d_out, stream);
}

// (--dsGrid) the cells' thresholds: bc_thr[c] (sel_keep's: floor(f * 2^32), 2^32 keeps every barcode) and rd_thr[c], each <= 2^32
static int rg_grid_thresholds(const uint64_t* bc_thr, const uint64_t* rd_thr, int32_t n, RgGridThr& T) {
    if (n < 0 || n > SMC_RG_MAX_TARGETS || (n && (!bc_thr || !rd_thr))) return fail(SMC_E_ARG, "smc_read_groups: bad grid thresholds");
    memset(&T, 0, sizeof T);
    for (int c = 0; c < n; ++c) {
        if (bc_thr[c] > (1ull << 32) || rd_thr[c] > (1ull << 32)) return fail(SMC_E_ARG, "smc_read_groups: a threshold above 2^32");
        T.bc[c] = bc_thr[c];
        T.rd[c] = rd_thr[c];
    }
    return SMC_OK;
}

int smc_read_groups_counts_frac(smc_read_groups* g, uint64_t seed, const uint64_t* bc_thr, int32_t n_frac, int64_t* counts) {
    if (!g || (n_frac && !counts)) return fail(SMC_E_ARG, "smc_read_groups_counts_frac: bad argument");
    if (!g->finished) return fail(SMC_E_ARG, "smc_read_groups_counts_frac: the table is not finished");
    RgThr F;
    { const int rc = rg_thresholds(bc_thr, n_frac, F); if (rc) return rc; }
    if (!n_frac) return SMC_OK;
    HIPCHK(hipSetDevice(g->ctx->device));
    HIPCHK(hipMemsetAsync(g->d_frac, 0, 8 * RG_F_N * SMC_RG_MAX_TARGETS, 0));
    hipLaunchKernelGGL(k_rg_reduce_frac, dim3(std::min(rg_grid(g->G.b_mask + 1), RG_RED_GRID)), dim3(RG_BLOCK), 0, 0, g->G, (unsigned long long)seed, F, (int)n_frac,
                       g->d_frac);
    HIPCHK(hipGetLastError());
    unsigned long long k[RG_F_N * SMC_RG_MAX_TARGETS];
    HIPCHK(hipMemcpy(k, g->d_frac, 8 * RG_F_N * (size_t)n_frac, hipMemcpyDeviceToHost));
    for (int f = 0; f < n_frac; ++f) {
        const unsigned long long* a = k + f * RG_F_N;
        int64_t* c = counts + (size_t)f * SMC_RG_N_COUNTS;
        c[0] = 0;                                                          // (records: not counted per barcode)
        c[1] = (int64_t)(a[RG_F_ONE] + a[RG_F_MULTI_NAMES]);               // names: one per single-name barcode, multi_names
        c[2] = (int64_t)a[RG_F_BARCODES]; c[3] = (int64_t)a[RG_F_ONE]; c[4] = (int64_t)a[RG_F_MULTI]; c[5] = (int64_t)a[RG_F_MULTI_NAMES];
        c[6] = (int64_t)a[RG_F_BARCODES];                                  // first names: one per barcode
        c[7] = 0;
    }
    return SMC_OK;
}

// (--spikeGrid) smc_read_groups_counts_frac's four counters for n_seeds seeds in ONE launch: counts[(j * n_frac + f) * 4 + k], k =
// barcodes, one, multi, multi_names of the barcodes seeds[j] keeps at bc_thr[f].  The seeds and the counters live in one allocation of
// the call's own (R can be 1000: more than the table's scratch holds).
int smc_read_groups_counts_frac_seeds(smc_read_groups* g, const uint64_t* seeds, int32_t n_seeds, const uint64_t* bc_thr, int32_t n_frac,
                                      uint64_t* counts) {
    const std::string who = "smc_read_groups_counts_frac_seeds";
    if (!g || n_seeds < 0 || (n_seeds && !seeds) || (n_seeds && n_frac > 0 && !counts)) return fail(SMC_E_ARG, who + ": bad argument");
    if (!g->finished) return fail(SMC_E_ARG, who + ": the table is not finished");
    if (n_seeds > SMC_AF_REP_MAX_REPS) return fail(SMC_E_INPUT, who + ": " + std::to_string(n_seeds) + " seeds, at most " + std::to_string(SMC_AF_REP_MAX_REPS));
    RgThr F;
    { const int rc = rg_thresholds(bc_thr, n_frac, F); if (rc) return rc; }
    if (!n_frac || !n_seeds) return SMC_OK;
    HIPCHK(hipSetDevice(g->ctx->device));
    const size_t n_out = (size_t)n_seeds * (size_t)n_frac * RG_F_N;
    unsigned long long* d = nullptr;
    HIPCHK(hipMalloc((void**)&d, 8 * ((size_t)n_seeds + n_out)));
    hipError_t e = hipMemcpy(d, seeds, 8 * (size_t)n_seeds, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemsetAsync(d + n_seeds, 0, 8 * n_out, 0);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rg_reduce_frac_seeds, dim3(std::min(rg_grid(g->G.b_mask + 1), RG_RED_GRID), (unsigned)std::min<int32_t>(n_seeds, 64)),
                           dim3(RG_BLOCK), 0, 0, g->G, d, (int)n_seeds, F, (int)n_frac, d + n_seeds);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(counts, d + n_seeds, 8 * n_out, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    HIPCHK(e);
    return SMC_OK;
}

int smc_read_groups_masks_grid(smc_read_groups* g, const uint64_t* d_idents, int64_t n_ids, uint64_t seed, const uint64_t* bc_thr,
                               const uint64_t* rd_thr, int32_t n_cells, uint32_t* d_masks, void* stream) {
    if (!g || n_ids < 0 || n_ids >= (int64_t)0xFFFFFF00 || (n_ids && (!d_idents || !d_masks)))
        return fail(SMC_E_ARG, "smc_read_groups_masks_grid: bad argument");
    if (!g->finished) return fail(SMC_E_ARG, "smc_read_groups_masks_grid: the table is not finished");
    RgGridThr T;
    { const int rc = rg_grid_thresholds(bc_thr, rd_thr, n_cells, T); if (rc) return rc; }
    if (!n_ids || !n_cells) return SMC_OK;
    HIPCHK(hipSetDevice(g->ctx->device));
    const uint32_t n_words = (uint32_t)((n_ids + 31) / 32);
    hipLaunchKernelGGL(k_rg_masks_grid, dim3((unsigned)((n_ids + RG_BLOCK - 1) / RG_BLOCK)), dim3(RG_BLOCK), 0, (hipStream_t)stream, g->G,
                       (const unsigned long long*)d_idents, (uint32_t)n_ids, (unsigned long long)seed, T, (int)n_cells, d_masks, n_words);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

int smc_read_groups_kept_grid(smc_read_groups* g, uint64_t seed, const uint64_t* bc_thr, const uint64_t* rd_thr, int32_t n_cells,
                              int64_t* kept) {
    if (!g || (n_cells && !kept)) return fail(SMC_E_ARG, "smc_read_groups_kept_grid: bad argument");
    if (!g->finished) return fail(SMC_E_ARG, "smc_read_groups_kept_grid: the table is not finished");
    RgGridThr T;
    { const int rc = rg_grid_thresholds(bc_thr, rd_thr, n_cells, T); if (rc) return rc; }
    if (!n_cells) return SMC_OK;
    HIPCHK(hipSetDevice(g->ctx->device));
    HIPCHK(hipMemsetAsync(g->d_kept, 0, 8 * SMC_RG_MAX_TARGETS, 0));
    hipLaunchKernelGGL(k_rg_kept_grid, dim3(std::min(rg_grid(g->G.n_mask + 1), RG_RED_GRID)), dim3(RG_BLOCK), 0, 0, g->G, (unsigned long long)seed, T, (int)n_cells,
                       g->d_kept);
    HIPCHK(hipGetLastError());
    unsigned long long k[SMC_RG_MAX_TARGETS];
    HIPCHK(hipMemcpy(k, g->d_kept, 8 * (size_t)n_cells, hipMemcpyDeviceToHost));
    for (int c = 0; c < n_cells; ++c) kept[c] = (int64_t)k[c];
    return SMC_OK;
}

int smc_read_groups_status(smc_read_groups* g, uint32_t* status) {
    if (!g || !status) return fail(SMC_E_ARG, "smc_read_groups_status: bad argument");
    *status = 0;
    if (!g->mem) return SMC_OK;
    HIPCHK(hipSetDevice(g->ctx->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(status, g->G.status, 4, hipMemcpyDeviceToHost));
    return SMC_OK;
}

void smc_read_groups_destroy(smc_read_groups* g) {
    if (!g) return;
    if (hipSetDevice(g->ctx->device) == hipSuccess) {
        (void)hipDeviceSynchronize();           // (a _masks launch on another stream may still read the table)
        for (auto& c : g->chunks) (void)hipFree(c.d);
        if (g->mem) (void)hipFree(g->mem);
    }
    delete g;
}

int smc_plan_set_timing(smc_plan* p, int slots) {
    if (!p || slots < 0) return fail(SMC_E_ARG, "smc_plan_set_timing: bad argument");
    HIPCHK(hipSetDevice(p->ctx->device));
    for (auto e : p->ev0) (void)hipEventDestroy(e);
    for (auto e : p->ev1) (void)hipEventDestroy(e);
    p->ev0.assign((size_t)slots, nullptr);
    p->ev1.assign((size_t)slots, nullptr);
    for (int k = 0; k < slots; ++k) { HIPCHK(hipEventCreate(&p->ev0[k])); HIPCHK(hipEventCreate(&p->ev1[k])); }
    p->timing = slots;
    p->n_timed = 0;
    return SMC_OK;
}

int smc_plan_kernel_ms(smc_plan* p, float* avg_ms, int32_t* n_samples, int64_t* n_loci, int64_t* n_reads) {
    if (!p || !avg_ms) return fail(SMC_E_ARG, "smc_plan_kernel_ms: NULL argument");
    const int64_t ns = p->n_timed < p->timing ? p->n_timed : p->timing;
    if (ns <= 0) return fail(SMC_E_ARG, "smc_plan_kernel_ms: no timed run (smc_plan_set_timing(plan, slots) then smc_plan_run)");
    double tot = 0;
    for (int64_t k = 0; k < ns; ++k) {
        float ms = 0;
        HIPCHK(hipEventSynchronize(p->ev1[k]));
        HIPCHK(hipEventElapsedTime(&ms, p->ev0[k], p->ev1[k]));
        tot += ms;
    }
    *avg_ms = (float)(tot / ns);
    if (n_samples) *n_samples = (int32_t)ns;
    if (n_loci) *n_loci = p->dom_loci;
    if (n_reads) *n_reads = p->dom_reads;
    return SMC_OK;
}


int smc_plan_info(const smc_plan* p, int32_t* n_launches, int64_t* scratch_bytes) {
    if (!p) return fail(SMC_E_ARG, "smc_plan_info: NULL plan");
    if (n_launches) *n_launches = (int32_t)p->bins.size() + (p->n_loci ? 1 : 0);
    if (scratch_bytes) {
        int64_t s = 0;
        for (auto& b : p->bins) s += (int64_t)(b.acc_bytes + b.flags_bytes);
        *scratch_bytes = s;
    }
    return SMC_OK;
}

static int plan_run_words_impl(smc_plan* p, const smc_params* prm, const uint32_t* words, bool w16, const uint32_t* umi_start, smc_row* rows, void* stream);
int smc_plan_run_words(smc_plan* p, const smc_params* prm, const uint32_t* words, const uint32_t* umi_start, smc_row* rows, void* stream) {
    return plan_run_words_impl(p, prm, words, false, umi_start, rows, stream);
}
int smc_plan_run_words16(smc_plan* p, const smc_params* prm, const uint16_t* words16, const uint32_t* umi_start, smc_row* rows, void* stream) {
    return plan_run_words_impl(p, prm, (const uint32_t*)words16, true, umi_start, rows, stream);
}
static int plan_run_words_impl(smc_plan* p, const smc_params* prm, const uint32_t* words, bool w16, const uint32_t* umi_start, smc_row* rows, void* stream) {
    if (!p || !prm) return fail(SMC_E_ARG, "smc_plan_run_words: NULL argument");
    if (p->n_loci == 0) return SMC_OK;
    if (!words || !umi_start || !rows) return fail(SMC_E_ARG, "smc_plan_run_words: NULL device pointer");
    {
        const uint16_t fp = smc_param_fingerprint(prm->min_bq, prm->min_mq, prm->mismatch_thr, prm->primer_dist);
        if (fp != p->fp)
            return fail(SMC_E_INPUT, "smc_plan_run_words: the planes were built with other parameters than this run's (minBQ " +
                                         std::to_string(prm->min_bq) + ", minMQ " + std::to_string(prm->min_mq) + ", mismatchThr " +
                                         std::to_string(prm->mismatch_thr) + ", primerDist " + std::to_string(prm->primer_dist) +
                                         " -> fingerprint " + std::to_string(fp) + ", batch has " + std::to_string(p->fp) +
                                         "): the read class, the mismatch flag and the in-deletion quality bake them in");
    }
    HIPCHK(hipSetDevice(p->ctx->device));
    hipStream_t st = (hipStream_t)stream;
    // (a batch with loci of the deep class: the filter-only tallies of the queued loci are k_filter_tallies' - below)
    bool deep_bins = false;
    for (const Bin& b : p->bins) deep_bins |= b.cls >= SMC_CLS_DEEP;
    if (const char* v = exp_env("SMC_TALLIES_LATER")) deep_bins = atoi(v) != 0;          // (measurements: 1 always, 0 never)
    KParams kp{prm->min_bq, prm->min_mq, prm->mt_drop, prm->primer_dist, prm->ds, prm->smt, lite_from_for(prm->min_bq), exp_env("SMC_NO_ALT") ? 0 : 1,
               deep_bins ? 1 : 0, simple_to_for(prm->min_bq)};
    // Two filter worklists, taken in turn: this run's k_filter_loci zeroes the OTHER list's count (the run before has long
    // finished with it) - no memset per run, a tenth of a 10,000-locus batch's time (C2).  Both counts are zeroed here before a
    // plan's first run (its blocks come from the context's pool; smc_plan_create_dev has k_plan_classify do it) and after a run
    // that did not get as far as k_filter_loci.
    const size_t flt_stride = (size_t)p->n_loci + 2;
    if (!p->flt_clean) {
        HIPCHK(hipMemsetAsync(p->d_flt_list, 0, 4, st));
        HIPCHK(hipMemsetAsync(p->d_flt_list + flt_stride, 0, 4, st));
    }
    uint32_t* const flt_cur = p->d_flt_list + (p->flt_parity ? flt_stride : 0);
    uint32_t* const flt_other = p->d_flt_list + (p->flt_parity ? 0 : flt_stride);
    p->flt_clean = false;
    for (size_t bi = 0; bi < p->bins.size(); ++bi) {
        const Bin& b = p->bins[bi];
        if (b.d_acc) HIPCHK(hipMemsetAsync(b.d_acc, 0, b.acc_bytes, st));   // the multi-part loci's accumulators and tickets
        const bool timed = p->timing > 0 && (int)bi == p->dom_bin;
        const size_t slot = timed ? (size_t)(p->n_timed % p->timing) : 0;
        if (timed) HIPCHK(hipEventRecord(p->ev0[slot], st));
        hipError_t e = hipSuccess;
        if (w16) switch (b.cls) {
            case 0: e = launch_bin<64, true>(b, kp, p, flt_cur, words, umi_start, rows, st); break;
            case 1: e = launch_bin<128, true>(b, kp, p, flt_cur, words, umi_start, rows, st); break;
            case 2: e = launch_bin<256, true>(b, kp, p, flt_cur, words, umi_start, rows, st); break;
            case 3: e = launch_bin<512, true>(b, kp, p, flt_cur, words, umi_start, rows, st); break;
            default: e = launch_bin<SMC_DEEP_BLOCK, true>(b, kp, p, flt_cur, words, umi_start, rows, st); break;
        } else switch (b.cls) {
            case 0: e = launch_bin<64, false>(b, kp, p, flt_cur, words, umi_start, rows, st); break;
            case 1: e = launch_bin<128, false>(b, kp, p, flt_cur, words, umi_start, rows, st); break;
            case 2: e = launch_bin<256, false>(b, kp, p, flt_cur, words, umi_start, rows, st); break;
            case 3: e = launch_bin<512, false>(b, kp, p, flt_cur, words, umi_start, rows, st); break;
            default: e = launch_bin<SMC_DEEP_BLOCK, false>(b, kp, p, flt_cur, words, umi_start, rows, st); break;
        }
        if (e != hipSuccess) return fail(SMC_E_HIP, std::string("k_call_v2 launch: ") + hipGetErrorString(e));
        if (timed) { HIPCHK(hipEventRecord(p->ev1[slot], st)); p->n_timed++; }
    }
    const unsigned fgrid = (unsigned)(p->n_loci < 2048 ? p->n_loci : 2048);   // four-wavefront workgroups, eight per CU; each walks the worklist
    if (deep_bins) {
        // the filter-only tallies of the loci the locus kernels have just queued: 16 wavefront-items per locus over the whole chip, each
        // taking every 16th slice of 4,096 reads
        const int split = 16;
        if (w16) hipLaunchKernelGGL(k_filter_tallies<true>, dim3(2048), dim3(256), 0, st, p->d_loci, rows, flt_cur, words, p->ctx->lut, split);
        else hipLaunchKernelGGL(k_filter_tallies<false>, dim3(2048), dim3(256), 0, st, p->d_loci, rows, flt_cur, words, p->ctx->lut, split);
    }
    hipLaunchKernelGGL(k_filter_loci, dim3(fgrid), dim3(SMC_FLT_BLOCK), 0, st, kp, p->d_loci, rows, flt_cur, flt_other, p->ctx->lfact);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SMC_E_HIP, std::string("k_filter_loci launch: ") + hipGetErrorString(e));
    p->flt_clean = true; p->flt_parity ^= 1;
    // behind the run: when this event has fired the plan's lists and scratch may be handed to another plan (smc_plan_destroy)
    if (!p->done_ev) HIPCHK(hipEventCreateWithFlags(&p->done_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(p->done_ev, st));
    return SMC_OK;
}

// one word per read from the raw-field planes: allele and quality from the meta word, class from the frag word, "first read of
// its fragment" from the fragment slots - whose order and density (first slot 0, steps of 0 or 1, last slot n_frag - 1: the batch
// contract) are checked here: a read that breaks them gets the class nobody has, and the locus's row SMC_ST_BAD_INPUT
int smc_pack_words(smc_plan* p, const uint32_t* meta, const uint32_t* frag, uint32_t* words, void* stream) {
    if (!p) return fail(SMC_E_ARG, "smc_pack_words: NULL argument");
    if (p->n_loci == 0) return SMC_OK;
    if (p->spec && p->spec_checked != 1) return fail(SMC_E_ARG, "smc_pack_words: a plan made by smc_plan_create_dev_spec packs no words until smc_plan_spec_ok has answered 1 (its launch lists may be empty)");
    if (!meta || !frag || !words) return fail(SMC_E_ARG, "smc_pack_words: NULL device pointer");
    HIPCHK(hipSetDevice(p->ctx->device));
    const unsigned grid = (unsigned)std::min<int64_t>(p->n_loci, 65536 * 4);
    hipLaunchKernelGGL(k_pack_words, dim3(grid), dim3(256), 0, (hipStream_t)stream, p->d_loci, (int)p->n_loci, meta, frag, words);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(SMC_E_HIP, std::string("k_pack_words launch: ") + hipGetErrorString(e));
    if (!p->done_ev) HIPCHK(hipEventCreateWithFlags(&p->done_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(p->done_ev, (hipStream_t)stream));
    return SMC_OK;
}

int smc_plan_run(smc_plan* p, const smc_params* prm, const uint32_t* meta, const uint32_t* umi, const uint32_t* frag,
                 const uint32_t* dist, const uint32_t* umi_start, smc_row* rows, void* stream) {
    if (!p || !prm) return fail(SMC_E_ARG, "smc_plan_run: NULL argument");
    if (p->n_loci == 0) return SMC_OK;
    // (a plan made without the host does not know how many quads of read words its batch spans - the array this call packs them into)
    if (p->spec) return fail(SMC_E_ARG, "smc_plan_run: a plan made by smc_plan_create_dev_spec runs read words (smc_plan_run_words / _words16), not raw-field planes");
    (void)umi; (void)dist;   // not read by the kernels (the read class and umi_start carry what they need)
    if (!meta || !frag || !umi_start || !rows) return fail(SMC_E_ARG, "smc_plan_run: NULL device pointer");
    HIPCHK(hipSetDevice(p->ctx->device));
    if (!p->d_words) { p->words_bytes = 16 * (size_t)std::max<int64_t>(1, p->need_quads); HIPCHK(plan_alloc(p->ctx, (void**)&p->d_words, p->words_bytes)); }
    int rc = smc_pack_words(p, meta, frag, p->d_words, stream);
    if (rc) return rc;
    return smc_plan_run_words(p, prm, p->d_words, umi_start, rows, stream);
}

int smc_call_batch_host(smc_ctx* ctx, const smc_params* prm, const smc_locus* loci, int64_t n_loci, const uint32_t* meta,
                        const uint32_t* umi, const uint32_t* frag, const uint32_t* dist, int64_t n_slots,
                        const uint32_t* umi_start, int64_t n_umi_start, smc_row* rows_out) {
    if (!ctx || !prm || (n_loci && (!loci || !rows_out))) return fail(SMC_E_ARG, "smc_call_batch_host: NULL argument");
    if (n_loci == 0) return SMC_OK;
    // the descriptors must stay inside the buffers handed over (the kernels trust them for addressing)
    for (int64_t l = 0; l < n_loci; ++l) {
        const smc_locus& L = loci[l];
        if (L.n_reads < 0 || L.n_umi < 0 || 4ll * L.read_off4 + L.n_reads > n_slots ||
            (int64_t)L.umi_off + L.n_umi + 1 > n_umi_start)
            return fail(SMC_E_INPUT, "smc_call_batch_host: locus " + std::to_string(l) + " points outside the planes / umi_start");
    }
    HIPCHK(hipSetDevice(ctx->device));
    smc_plan* plan = nullptr;
    int rc = smc_plan_create(ctx, loci, n_loci, &plan);
    if (rc) return rc;
    uint32_t* d[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    const uint32_t* h[5] = {meta, umi, frag, dist, umi_start};
    const int64_t hn[5] = {n_slots, n_slots, n_slots, n_slots, n_umi_start};
    smc_row* d_rows = nullptr;

    auto cleanup = [&]() {
        for (auto q : d) (void)hipFree(q);
        (void)hipFree(d_rows);
        smc_plan_destroy(plan);
    };
    // the read words are made of the meta and frag planes (smc_plan_run packs them on the device): the umi and dist planes
    // never cross PCIe
    (void)umi; (void)dist;
    for (int k = 0; k < 5; ++k) {
        if (k == 1 || k == 3) continue;
        hipError_t e = hipMalloc(&d[k], sizeof(uint32_t) * (size_t)(hn[k] > 0 ? hn[k] : 1));
        if (e == hipSuccess && hn[k] > 0) e = hipMemcpy(d[k], h[k], sizeof(uint32_t) * (size_t)hn[k], hipMemcpyHostToDevice);
        if (e != hipSuccess) { cleanup(); return fail(SMC_E_HIP, std::string("plane upload: ") + hipGetErrorString(e)); }
    }
    hipError_t e = hipMalloc(&d_rows, sizeof(smc_row) * (size_t)n_loci);
    if (e != hipSuccess) { cleanup(); return fail(SMC_E_HIP, std::string("rows alloc: ") + hipGetErrorString(e)); }
    rc = smc_plan_run(plan, prm, d[0], d[1], d[2], d[3], d[4], d_rows, nullptr);
    if (rc == SMC_OK) {
        e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(rows_out, d_rows, sizeof(smc_row) * (size_t)n_loci, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(SMC_E_HIP, std::string("run/download: ") + hipGetErrorString(e));
    }
    cleanup();
    return rc;
}

int smc_build_max_depth(void) { return (1 << 24) - 1; }

static int build_planes_impl(smc_ctx* ctx, const smc_params* prm, const smc_build_in* in, uint32_t slot_base, uint32_t umi_base,
                             uint32_t* words, bool w16, uint32_t* meta, uint32_t* umi, uint32_t* frag, uint32_t* dist, uint32_t* umi_start,
                             uint32_t* u_gid, uint32_t* u_finc, smc_locus* loci, uint32_t* xlist, uint32_t xcap, uint32_t* counters, void* stream);
int smc_build_planes(smc_ctx* ctx, const smc_params* prm, const smc_build_in* in, uint32_t slot_base, uint32_t umi_base,
                     uint32_t* words, uint32_t* meta, uint32_t* umi, uint32_t* frag, uint32_t* dist, uint32_t* umi_start,
                     uint32_t* u_gid, uint32_t* u_finc, smc_locus* loci, uint32_t* xlist, uint32_t xcap, uint32_t* counters, void* stream) {
    return build_planes_impl(ctx, prm, in, slot_base, umi_base, words, false, meta, umi, frag, dist, umi_start, u_gid, u_finc, loci, xlist, xcap, counters, stream);
}
int smc_build_planes_w16(smc_ctx* ctx, const smc_params* prm, const smc_build_in* in, uint32_t slot_base, uint32_t umi_base,
                         uint16_t* words16, uint32_t* umi_start, uint32_t* u_gid, uint32_t* u_finc, smc_locus* loci,
                         uint32_t* xlist, uint32_t xcap, uint32_t* counters, void* stream) {
    if (!words16) return fail(SMC_E_ARG, "smc_build_planes_w16: NULL device pointer");
    if (prm && (prm->min_bq < 0 || prm->min_bq > 63)) return fail(SMC_E_INPUT, "smc_build_planes_w16: minBQ " + std::to_string(prm->min_bq) + " has no room in a 16-bit read word (0 .. 63)");
    return build_planes_impl(ctx, prm, in, slot_base, umi_base, (uint32_t*)words16, true, nullptr, nullptr, nullptr, nullptr, umi_start, u_gid, u_finc, loci, xlist, xcap, counters, stream);
}
static int build_planes_impl(smc_ctx* ctx, const smc_params* prm, const smc_build_in* in, uint32_t slot_base, uint32_t umi_base,
                             uint32_t* words, bool w16, uint32_t* meta, uint32_t* umi, uint32_t* frag, uint32_t* dist, uint32_t* umi_start,
                             uint32_t* u_gid, uint32_t* u_finc, smc_locus* loci, uint32_t* xlist, uint32_t xcap, uint32_t* counters, void* stream) {
    if (!ctx || !prm || !in || !counters) return fail(SMC_E_ARG, "smc_build_planes: NULL argument");
    if (in->n_loci <= 0) return SMC_OK;
    if (!in->aln || !in->cig || !in->bq || !in->loc || !in->refseq || !(words || (meta && frag)) || !umi_start ||
        !u_gid || !u_finc || !loci || !xlist) return fail(SMC_E_ARG, "smc_build_planes: NULL device pointer");
    if (in->max_depth < 0 || in->max_depth > smc_build_max_depth())
        return fail(SMC_E_INPUT, "smc_build_planes: a locus of " + std::to_string(in->max_depth) + " reads (limit " + std::to_string(smc_build_max_depth()) + ")");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const int n_loci = in->n_loci, n_tiles = (n_loci + BP_TILE - 1) / BP_TILE;
    // the per-locus windows on the host: they size the sort, the grids and the scratch (the segment table itself is made on the
    // device by the same formulas, k_bp_segtab)
    std::vector<smc_dev_locus> loc_copy;
    const smc_dev_locus* lh = in->loc_host;
    if (!lh) {
        loc_copy.resize((size_t)n_loci);
        HIPCHK(hipMemcpy(loc_copy.data(), in->loc, sizeof(smc_dev_locus) * (size_t)n_loci, hipMemcpyDeviceToHost));
        lh = loc_copy.data();
    }
    // one tile per segment where every tile's window fits the one-workgroup sort (k_build_planes.inc: BP_SEG_TILES_DEEP)
    int tiles_per_seg = 1;
    for (int t = 0; t < n_tiles && tiles_per_seg == 1; ++t) {
        const int l0 = t * BP_TILE, l1 = std::min(n_loci, l0 + BP_TILE) - 1;
        if (lh[l1].w1 > lh[l0].w0 && lh[l1].w1 - lh[l0].w0 > BP_LSORT_MAX) tiles_per_seg = BP_SEG_TILES_DEEP;
    }
    { const char* v = exp_env("SMC_BP_SEG_TILES"); if (v && atoi(v) >= 1) tiles_per_seg = atoi(v); }
    const int seg_loci = tiles_per_seg * BP_TILE, n_seg = (n_loci + seg_loci - 1) / seg_loci;
    uint64_t ntot = 0, work = 0, reads = 0;
    std::vector<uint32_t> seg_cnt((size_t)n_seg), seg_tiles((size_t)n_seg);
    for (int s = 0; s < n_seg; ++s) {
        const int l0 = s * seg_loci, l1 = std::min(n_loci, l0 + seg_loci) - 1;
        const uint32_t w0 = lh[l0].w0, w1 = std::max(w0, lh[l1].w1);
        if (in->n_aln >= 0 && (int64_t)w1 > (int64_t)in->n_aln)
            return fail(SMC_E_INPUT, "smc_build_planes: locus window beyond the run's " + std::to_string(in->n_aln) + " alignments");
        seg_cnt[(size_t)s] = w1 - w0; seg_tiles[(size_t)s] = (uint32_t)((l1 - l0) / BP_TILE + 1);
        ntot += w1 - w0; work += (uint64_t)(w1 - w0) * seg_tiles[(size_t)s];
    }
    // deep runs: the walks behind the sort run on one list per tile (k_bp_tile_count / k_bp_tile_scatter: the tile's own window of
    // the file in the segment's order), the sort on the segments
    const bool tile_lists = tiles_per_seg > 1 && !exp_env("SMC_BP_NO_TILE_LISTS");
    std::vector<uint32_t> wcnt;
    uint64_t ntot_w = 0;
    int nch = 1;
    if (tile_lists) {
        wcnt.resize((size_t)n_tiles);
        for (int t = 0; t < n_tiles; ++t) {
            const int l0 = t * BP_TILE, l1 = std::min(n_loci, l0 + BP_TILE) - 1;
            const uint32_t w0 = lh[l0].w0, w1 = std::max(w0, lh[l1].w1);
            wcnt[(size_t)t] = w1 - w0; ntot_w += w1 - w0;
        }
        for (int s = 0; s < n_seg; ++s) nch = std::max(nch, (int)((seg_cnt[(size_t)s] + BP_TL_CH - 1) / BP_TL_CH));
        work = ntot_w;
        if (ntot_w >= (1ull << 31)) return fail(SMC_E_INPUT, "smc_build_planes: run too large (entries of the tiles' lists " + std::to_string(ntot_w) + ")");
    }
    for (int l = 0; l < n_loci; ++l) reads += lh[l].n;
    int64_t n_aln = in->n_aln;
    if (n_aln < 0) { n_aln = 0; for (int l = 0; l < n_loci; ++l) n_aln = std::max<int64_t>(n_aln, lh[l].w1); }
    if (ntot >= (1ull << 31) || reads >= (1ull << 32)) return fail(SMC_E_INPUT, "smc_build_planes: run too large (sorted entries " + std::to_string(ntot) + ", reads " + std::to_string(reads) + ")");
    // entries of the sorted list per wavefront.  Many short parts: the wavefronts of a tile then write adjacent stretches of its
    // loci's words at about the same time - on one XCD (k_bp_emit2's mapping), so that its L2 completes lines before it evicts
    // them - and a part's state before its first row (the open barcode's earlier rows) is cheap to replay.  Measured on the
    // 3000x shape (4500 rows per tile), round 4's first walk: 128 rows 1.77 ms, 192 1.72, 256 1.85, 448 2.09, 896 2.25, 1792 2.38, 3584 2.88;
    // with the pool on tile lines and the indel positions in the fast path: 128 1.43, 192 1.44, 256 1.32, 320 1.37, 384 1.36, 512 1.37
    uint32_t part = (uint32_t)std::min<uint64_t>(4096, std::max<uint64_t>(256, (work / 81920 + 63) / 64 * 64));
    { const char* v = exp_env("SMC_BP_PART"); if (v && atoi(v) >= 64) part = (uint32_t)std::min(4096, atoi(v)) / 64u * 64u; }   // (at most 64 stretches of 64 rows per count wavefront: k_bp_count)
    int rs_maxblk = BP_RS_MAXBLK;
    { const char* v = exp_env("SMC_BP_RS_MAXBLK"); if (v && atoi(v) > 0) rs_maxblk = atoi(v); }
    const uint32_t max_blk = (uint32_t)std::max(1, rs_maxblk / n_seg);
    uint64_t total_blk = 0, total_parts = 0, total_cparts = 0;     // total_parts: wavefronts of BP_SUB rows (k_bp_emit2); total_cparts: k_bp_count's
    for (int s = 0; s < n_seg; ++s) {
        total_blk += bp_seg_blocks(seg_cnt[(size_t)s], max_blk);
        if (tile_lists) continue;
        total_parts += (uint64_t)((seg_cnt[(size_t)s] + BP_SUB - 1) / BP_SUB) * seg_tiles[(size_t)s];
        total_cparts += (uint64_t)((seg_cnt[(size_t)s] + part - 1) / part) * seg_tiles[(size_t)s];
    }
    if (tile_lists)
        for (int t = 0; t < n_tiles; ++t) {
            total_parts += (uint64_t)((wcnt[(size_t)t] + BP_SUB - 1) / BP_SUB);
            total_cparts += (uint64_t)((wcnt[(size_t)t] + part - 1) / part);
        }
    if (total_parts >= (1ull << 31)) return fail(SMC_E_INPUT, "smc_build_planes: too many (tile, part) wavefronts");
    int bc_bits = 1, pair_bits = 1;
    while (bc_bits < 32 && (1ll << bc_bits) < (int64_t)std::max(1, in->n_bc)) ++bc_bits;
    while (pair_bits < 32 && (1ll << pair_bits) < (int64_t)std::max(1, in->n_pair)) ++pair_bits;
    const int passes = (bc_bits + pair_bits + 7) / 8;
    const uint32_t xraw_cap = (uint32_t)std::min<uint64_t>(1u << 28, reads / 32 + 65536);
    // scratch, carved in 256-byte steps
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    // (behind each segment table its segments' live row counts, BpArgs.n_live: one copy brings both)
    const size_t o_seg = carve((sizeof(BpSeg) + 4) * (size_t)n_seg);
    const size_t o_wseg = carve(tile_lists ? (sizeof(BpSeg) + 4) * (size_t)n_tiles : 0), o_sorted2 = carve(tile_lists ? 4 * (size_t)ntot_w : 0),
                 o_tc = carve(tile_lists ? 4 * (size_t)n_tiles * (size_t)nch : 0);
    const size_t o_k0 = carve(8 * (size_t)ntot), o_k1 = carve(8 * (size_t)ntot), o_v0 = carve(4 * (size_t)ntot), o_v1 = carve(4 * (size_t)ntot);
    const size_t o_hist = carve(4 * 256 * (size_t)total_blk), o_dtot = carve(4 * 256 * (size_t)n_seg);
    const size_t o_cnt = carve(768 * (size_t)total_cparts), o_cntp = carve(256 * (size_t)total_parts), o_pstate = carve(16 * (size_t)total_parts);
    // the transposed walk (k_bp_emit2.inc): a 32-byte row record per alignment, and for the general CIGARs a linearised copy of
    // their bases and qualities (a (letter, quality) pair per reference position; an alignment the pool has no room for keeps the exact path)
    const uint32_t n_rblk = (uint32_t)((std::max<int64_t>(1, n_aln) + 255) / 256);
    const size_t lin_cap = (size_t)std::min<uint64_t>(0xFFFF0000ull, ((uint64_t)1 << 20) + 24ull * (uint64_t)std::max<int64_t>(1, n_aln));
    const size_t o_rows = carve(32 * (size_t)std::max<int64_t>(1, n_aln)), o_need = carve(4 * (size_t)std::max<int64_t>(1, n_aln));
    const size_t o_bsum = carve(128 * BP_NCUR + 256), o_lin = carve(2 * lin_cap + 256);            // (k_bp_rows_write's cursors)
    // (the list of general CIGARs in BP_NCUR parts: workgroup b appends to part b % BP_NCUR - at most its 256 alignments)
    const uint32_t glist_stride = 256u * ((n_rblk + BP_NCUR - 1) / BP_NCUR) + 64u;
    const size_t o_glist = carve(4 * (size_t)glist_stride * BP_NCUR), o_k8 = carve(8 * (size_t)std::max<int64_t>(1, n_aln));
    const size_t o_kend = carve(4 * (size_t)std::max<int64_t>(1, n_aln));
    const size_t o_zero = off;                                                // [o_zero, o_zend): cleared before every run
    const size_t o_xcnt = carve(4 * (size_t)n_loci), o_tcnt = carve(4 * ((size_t)n_tiles + 1)), o_tcur = carve(4 * (size_t)n_tiles), o_xn = carve(4);
    const size_t o_zend = off;
    const size_t o_xraw = carve(4 * BP_XW * (size_t)xraw_cap), o_gidx = carve(4 * ((size_t)xraw_cap + 4)), o_gidx2 = carve(4 * ((size_t)xraw_cap + 4));
    if (int rc = grow_scratch(ctx->bp_scratch, ctx->bp_bytes, off, off + off / 8, "smc_build_planes", &st)) return rc;
    char* sc = (char*)ctx->bp_scratch;
    // one scratch per context: a build issued on another stream than the one before waits for that one's last kernel (ADVICE r4)
    if (ctx->bp_done_ev) HIPCHK(hipStreamWaitEvent(st, ctx->bp_done_ev, 0));
    // (debugging and tests: SMC_BP_POISON_SCRATCH=<byte> fills the scratch before every run - does anything read what this run has not
    // written?  A fresh allocation is zero, a recycled one is not: the soak of round 5 found a read with bq = minBQ - 1 included
    // because of a stale byte next to it)
    if (const char* v = exp_env("SMC_BP_POISON_SCRATCH")) HIPCHK(hipMemsetAsync(sc, atoi(v) & 0xFF, ctx->bp_bytes, st));
    if (!total_parts) {                                                       // (else k_bp_rows_need clears both)
        HIPCHK(hipMemsetAsync(sc + o_zero, 0, o_zend - o_zero, st));
        HIPCHK(hipMemsetAsync(counters, 0, 8, st));
    }
    BpArgs A;
    A.aln = in->aln; A.cig = in->cig; A.bq = in->bq; A.loc = in->loc; A.refseq = in->refseq;
    A.start0 = in->start0; A.n_loci = n_loci; A.n_seg = n_seg; A.part = (int32_t)part; A.seg_tiles = tiles_per_seg;
    A.min_bq = prm->min_bq; A.min_mq = prm->min_mq; A.primer_dist = prm->primer_dist; A.ds = prm->ds;
    A.fp = (uint32_t)smc_param_fingerprint(prm->min_bq, prm->min_mq, prm->mismatch_thr, prm->primer_dist) << SMC_LF_FP_SHIFT;
    A.slot_base = slot_base; A.umi_base = umi_base;
    { const char* v = exp_env("SMC_BP_XCD_ROT"); A.xcd_rot = v ? (uint32_t)atoi(v) & 7u : 0u; }
    { const char* v = exp_env("SMC_BP_XCD_GROUP"); if (v && atoi(v) > 0) A.xcd_rot |= (uint32_t)atoi(v) << 8; }
    A.words = words; A.w16 = w16 ? 1u : 0u; A.meta = meta; A.umi = umi; A.frag = frag; A.dist = dist; A.umi_start = umi_start; A.u_gid = u_gid; A.u_finc = u_finc;
    A.loci = loci;
    BpSeg* d_seg = (BpSeg*)(sc + o_seg);
    uint32_t* d_nlive = (uint32_t*)(d_seg + n_seg);
    A.seg = d_seg; A.n_live = d_nlive;
    // the sort of a one-tile segment drops the window rows that end before the tile (k_bp_sort_seg); SMC_BP_KEEP_DEAD_ROWS keeps
    // them - the planes are the same bytes either way (a dead row's coverage mask is empty in both walks)
    const bool live_rows = tiles_per_seg == 1 && !exp_env("SMC_BP_KEEP_DEAD_ROWS");
    A.cnt = (uint32_t*)(sc + o_cnt); A.cntp = (uint32_t*)(sc + o_cntp); A.pstate = (uint32_t*)(sc + o_pstate);
    A.xraw = (uint32_t*)(sc + o_xraw); A.xraw_cap = xraw_cap; A.xraw_n = (uint32_t*)(sc + o_xn);
    A.xcnt = (uint32_t*)(sc + o_xcnt); A.tcnt = (uint32_t*)(sc + o_tcnt); A.tcur = (uint32_t*)(sc + o_tcur); A.gidx = (uint32_t*)(sc + o_gidx); A.gidx2 = (uint32_t*)(sc + o_gidx2);
    A.xlist = xlist; A.xcap = xcap; A.xcount = counters; A.status = counters + 1;
    BpSeg* d_wseg = (BpSeg*)(sc + o_wseg);
    if (tile_lists || (in->loc_host && !exp_env("SMC_BP_SEGTAB_DEV"))) {
        // the segment table from the host's copy of the windows (the same formulas as k_bp_segtab: a 23 us one-workgroup kernel at the
        // head of every run otherwise): a stream-ordered copy of 32 bytes per segment
        smc_ctx::SegStage& SG = ctx->seg_stage[ctx->seg_next];
        ctx->seg_next = (ctx->seg_next + 1) % 4;
        if (SG.used) HIPCHK(hipEventSynchronize(SG.ev));                      // (four builds ago: long done)
        const size_t n_stage = (size_t)n_seg + (tile_lists ? (size_t)n_tiles : 0);
        if (SG.cap < (sizeof(BpSeg) + 4) * n_stage) {
            if (SG.host) (void)hipHostFree(SG.host);
            SG.host = nullptr; SG.cap = 0;
            const size_t want = std::max<size_t>(4096, (sizeof(BpSeg) + 4) * n_stage * 2);
            HIPCHK(hipHostMalloc(&SG.host, want, hipHostMallocDefault));
            SG.cap = want;
        }
        if (!SG.ev) HIPCHK(hipEventCreateWithFlags(&SG.ev, hipEventDisableTiming));
        BpSeg* hs = (BpSeg*)SG.host;
        uint32_t* hn = (uint32_t*)(hs + n_seg);                               // every row of the window: the sort writes the live count where it filters
        uint32_t off_run = 0, part_run = 0, blk_run = 0, cpart_run = 0;
        for (int sgi = 0; sgi < n_seg; ++sgi) {
            BpSeg S{};
            const int l0 = sgi * seg_loci, l1 = std::min(n_loci, l0 + seg_loci) - 1;
            S.w0 = lh[l0].w0;
            S.w1 = std::max(S.w0, lh[l1].w1);
            const uint32_t cnt = S.w1 - S.w0;
            S.n_tiles = (uint32_t)((l1 - l0) / BP_TILE + 1);
            S.ppt = (cnt + BP_SUB - 1) / BP_SUB;
            S.cppt = (cnt + part - 1) / part;
            S.n_blk = bp_seg_blocks(cnt, max_blk);
            S.off = off_run; S.part_base = part_run; S.blk_base = blk_run; S.cpart_base = cpart_run;
            off_run += cnt; part_run += S.ppt * S.n_tiles; blk_run += S.n_blk; cpart_run += S.cppt * S.n_tiles;
            hs[(size_t)sgi] = S; hn[(size_t)sgi] = cnt;
        }
        HIPCHK(hipMemcpyAsync(d_seg, hs, (sizeof(BpSeg) + 4) * (size_t)n_seg, hipMemcpyHostToDevice, st));
        if (tile_lists) {                                                     // the walks' table: a segment per tile, its own window and list
            BpSeg* hw = (BpSeg*)(hn + n_seg);
            uint32_t* hwn = (uint32_t*)(hw + n_tiles);                        // (a deep run's tile lists keep every window row)
            uint32_t woff = 0, wpart = 0, wcpart = 0;
            for (int t = 0; t < n_tiles; ++t) {
                BpSeg S{};
                const int l0 = t * BP_TILE, l1 = std::min(n_loci, l0 + BP_TILE) - 1;
                S.w0 = lh[l0].w0; S.w1 = std::max(S.w0, lh[l1].w1);
                const uint32_t cnt = S.w1 - S.w0;
                S.n_tiles = 1u; S.ppt = (cnt + BP_SUB - 1) / BP_SUB; S.cppt = (cnt + part - 1) / part; S.n_blk = 0u;
                S.off = woff; S.part_base = wpart; S.blk_base = 0u; S.cpart_base = wcpart;
                woff += cnt; wpart += S.ppt; wcpart += S.cppt;
                hw[(size_t)t] = S; hwn[(size_t)t] = cnt;
            }
            HIPCHK(hipMemcpyAsync(d_wseg, hw, (sizeof(BpSeg) + 4) * (size_t)n_tiles, hipMemcpyHostToDevice, st));
        }
        HIPCHK(hipEventRecord(SG.ev, st));
        SG.used = true;
    } else
        hipLaunchKernelGGL(k_bp_segtab, dim3(1), dim3(1024), 0, st, in->loc, n_loci, n_seg, seg_loci, part, max_blk, d_seg, d_nlive);
    HIPCHK(hipGetLastError());
    const bool raw = meta || umi || frag || dist;
    BpRow* d_rows = (BpRow*)(sc + o_rows);
    uint8_t* d_lin = (uint8_t*)(sc + o_lin);
    uint2* d_k8 = (uint2*)(sc + o_k8);
    int32_t* d_kend = (int32_t*)(sc + o_kend);
    uint32_t* const sort_nlive = live_rows ? d_nlive : nullptr;
    uint32_t* d_bsum = (uint32_t*)(sc + o_bsum);
    uint32_t* d_glist = (uint32_t*)(sc + o_glist);
    if (total_parts) {      // the row records first: they do not depend on the order, and leave the sort its keys as a compact array
        hipLaunchKernelGGL(k_bp_zero_words, dim3(8), dim3(256), 0, st, d_bsum, 32u * BP_NCUR);   // (its cursors: pool pairs handed out, general CIGARs listed)
        hipLaunchKernelGGL(k_bp_rows_write, dim3(n_rblk), dim3(256), 0, st, A, (uint32_t)n_aln, d_bsum, d_glist, glist_stride, d_rows, (uint32_t)lin_cap, raw ? 1 : 0, d_k8, d_kend,
                           (uint32_t*)(sc + o_zero), (uint32_t)((o_zend - o_zero) / 4), counters);
    }
    unsigned long long* kb[2] = {(unsigned long long*)(sc + o_k0), (unsigned long long*)(sc + o_k1)};
    uint32_t* vb[2] = {(uint32_t*)(sc + o_v0), (uint32_t*)(sc + o_v1)};
    uint32_t* d_hist = (uint32_t*)(sc + o_hist);
    int cur = 0;
    bool any_small = false, any_mid = false;
    for (int s = 0; s < n_seg; ++s) {
        any_small |= seg_cnt[(size_t)s] > 0 && seg_cnt[(size_t)s] <= BP_LSORT_MAX;
        any_mid |= seg_cnt[(size_t)s] > BP_SORT_LDS_MAX && seg_cnt[(size_t)s] <= BP_LSORT_MAX;
    }
    if (any_small) {        // segments one workgroup sorts, every pass in this launch (the result lands where the passes below leave theirs)
        // (a run with segments of 6,145 ... 16,384 entries takes the instantiation that keeps 16 entries per thread: 146 KB of LDS)
        // and the small one the segments up to 6,144 where there are any: a run with both kinds launches both)
        const bool big = any_mid && !exp_env("SMC_BP_SORT_SMALL");
        bool any_le = false;
        for (int s = 0; s < n_seg; ++s) any_le |= seg_cnt[(size_t)s] > 0 && seg_cnt[(size_t)s] <= BP_SORT_LDS_MAX;
        if (any_le || !big)
            hipLaunchKernelGGL((k_bp_sort_seg<BP_SORT_REG, BP_SORT_WAVES_SMALL, false>), dim3((unsigned)n_seg), dim3(64 * BP_SORT_WAVES_SMALL), 0, st, d_seg, d_k8, pair_bits, passes, kb[0], kb[1], vb[0], vb[1],
                               0u, big ? (uint32_t)BP_SORT_LDS_MAX : (uint32_t)BP_LSORT_MAX, d_kend, in->start0, sort_nlive);
        if (big)
            hipLaunchKernelGGL((k_bp_sort_seg<BP_SORT_REG_BIG, BP_SORT_WAVES, true>), dim3((unsigned)n_seg), dim3(64 * BP_SORT_WAVES), 0, st, d_seg, d_k8, pair_bits, passes, kb[0], kb[1], vb[0], vb[1],
                               (uint32_t)BP_SORT_LDS_MAX, (uint32_t)BP_LSORT_MAX, d_kend, in->start0, sort_nlive);
    }
    if (total_blk) {
        for (int ps = 0; ps < passes; ++ps) {
            const int shift = 8 * ps;
            if (ps == 0) hipLaunchKernelGGL(k_bp_hist<true>, dim3((unsigned)total_blk), dim3(64), 0, st, d_seg, n_seg, d_k8, pair_bits, kb[0], vb[0], shift, d_hist);
            else hipLaunchKernelGGL(k_bp_hist<false>, dim3((unsigned)total_blk), dim3(64), 0, st, d_seg, n_seg, d_k8, pair_bits, kb[cur], vb[cur], shift, d_hist);
            hipLaunchKernelGGL(k_bp_rowscan, dim3(256u * (unsigned)n_seg), dim3(64), 0, st, d_seg, d_hist, (uint32_t*)(sc + o_dtot));
            hipLaunchKernelGGL(k_bp_scatter, dim3((unsigned)total_blk), dim3(64), 0, st, d_seg, n_seg, kb[cur], vb[cur], kb[cur ^ 1], vb[cur ^ 1], shift, d_hist,
                               (const uint32_t*)(sc + o_dtot));
            cur ^= 1;
        }
        HIPCHK(hipGetLastError());
    }
    A.sorted = vb[passes & 1];
    if (tile_lists && total_parts) {
        uint32_t* d_tc = (uint32_t*)(sc + o_tc);
        uint32_t* d_sorted2 = (uint32_t*)(sc + o_sorted2);
        const unsigned tgrid = (unsigned)((size_t)n_tiles * (size_t)nch);
        hipLaunchKernelGGL(k_bp_tile_count, dim3(tgrid), dim3(256), 0, st, d_seg, tiles_per_seg, d_wseg, n_tiles, nch, A.sorted, d_tc);
        hipLaunchKernelGGL(k_bp_tile_scatter, dim3(tgrid), dim3(256), 0, st, d_seg, tiles_per_seg, d_wseg, n_tiles, nch, A.sorted, d_tc, d_sorted2);
        A.sorted = d_sorted2; A.seg = d_wseg; A.n_live = (const uint32_t*)(d_wseg + n_tiles); A.n_seg = n_tiles; A.seg_tiles = 1;
    }
    if (total_parts) {
        int64_t lin_grid = 2048;                                              // (workgroups of 16 teams of 16 lanes, a team per general CIGAR at a time)
        { const char* v = exp_env("SMC_BP_LIN_GRID"); if (v && atoi(v) > 0) lin_grid = atoi(v); }
        // (a whole number of workgroups per part of the list, at least one: k_bp_lin deals them g -> part g % BP_NCUR)
        const int64_t lin_wgs = std::max<int64_t>(BP_NCUR, std::min<int64_t>(lin_grid, (n_aln + 15) / 16) / BP_NCUR * BP_NCUR);
        if (!raw) hipLaunchKernelGGL(k_bp_lin, dim3((unsigned)lin_wgs), dim3(256), 0, st, A, d_glist, glist_stride, d_bsum, d_rows, d_lin);
        hipLaunchKernelGGL(k_bp_count, dim3((unsigned)total_cparts), dim3(64), 0, st, A);
    }
    hipLaunchKernelGGL(k_bp_scan_tiles, dim3((unsigned)n_tiles), dim3(256), 0, st, A);
    if (total_parts) {
        const bool timed = !ctx->bp_ev0.empty();
        const size_t ev = timed ? (size_t)(ctx->bp_timed % (int64_t)ctx->bp_ev0.size()) : 0;
        if (timed) HIPCHK(hipEventRecord(ctx->bp_ev0[ev], st));
        size_t lds_pad = 0;                                                      // (experiments: LDS a wavefront claims on top of its own - bounds the wavefronts per CU)
        { const char* v = exp_env("SMC_BP_LDS_PAD"); if (v) lds_pad = (size_t)std::max(0, atoi(v)); }
        if (raw) hipLaunchKernelGGL((k_bp_emit2<true, false>), dim3((unsigned)total_parts), dim3(64), lds_pad, st, A, d_rows, d_lin);
        else if (w16) hipLaunchKernelGGL((k_bp_emit2<false, true>), dim3((unsigned)total_parts), dim3(64), lds_pad, st, A, d_rows, d_lin);
        else hipLaunchKernelGGL((k_bp_emit2<false, false>), dim3((unsigned)total_parts), dim3(64), lds_pad, st, A, d_rows, d_lin);
        if (timed) { HIPCHK(hipEventRecord(ctx->bp_ev1[ev], st)); ctx->bp_timed++; }
        hipLaunchKernelGGL(k_bp_scan, dim3(1), dim3(1024), 0, st, A.tcnt, (uint32_t)n_tiles + 1u, (const uint32_t*)nullptr);
        hipLaunchKernelGGL(k_bp_xgroup, dim3(256), dim3(256), 0, st, A);
        hipLaunchKernelGGL(k_bp_xfix2, dim3((unsigned)n_tiles), dim3(64), 0, st, A);
        hipLaunchKernelGGL(k_bp_xfix, dim3((unsigned)n_tiles), dim3(64 * BP_XF_WAVES), 0, st, A);
    }
    HIPCHK(hipGetLastError());
    ctx->bp_nlive_off = (size_t)((const char*)A.n_live - sc); ctx->bp_nlive_n = A.n_seg;
    if (!ctx->bp_done_ev) HIPCHK(hipEventCreateWithFlags(&ctx->bp_done_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ctx->bp_done_ev, st));
    return SMC_OK;
}

// (--spikeScanBuild listed) the listed loci of B copies of a run as a dense batch: everything checked on the host before anything is
// enqueued, then five launches for the whole batch (k_build_listed.inc)
int smc_build_listed(smc_ctx* ctx, const smc_params* prm, const smc_listed_copy* d_copies, int32_t n_copies, int32_t flags,
                     int32_t start0, int32_t n_loci, const uint8_t* d_refseq, const uint32_t* offsets, const uint32_t* caps,
                     int32_t n_listed, int32_t word_bits, uint32_t slot_base, uint32_t umi_base, void* words, uint32_t* umi_start,
                     uint32_t* u_gid, uint32_t* u_finc, smc_locus* loci, uint32_t* xlist, uint32_t xcap, uint32_t* counters,
                     void* stream) {
    const std::string who = "smc_build_listed";
    static_assert(sizeof(smc_listed_copy) == 48, "smc_build_listed's copy record");
    static_assert(SMC_LISTED_MAX_LOCI == BL_MAX_LOCI && SMC_LISTED_MAX_COPIES == BL_MAX_COPIES && SMC_LISTED_UNFLAGGED == BL_ST_UNFLAGGED, "smc_build_listed's limits");
    if (!ctx || !prm) return fail(SMC_E_ARG, who + ": NULL argument");
    if (n_copies < 0 || n_copies > SMC_LISTED_MAX_COPIES)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies, 0 .. " + std::to_string(SMC_LISTED_MAX_COPIES) + " expected");
    if (n_listed < 0 || n_listed > SMC_LISTED_MAX_LOCI)
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_listed) + " listed loci, 0 .. " + std::to_string(SMC_LISTED_MAX_LOCI) + " expected");
    if (word_bits != 16 && word_bits != 32) return fail(SMC_E_INPUT, who + ": read words of " + std::to_string(word_bits) + " bits, 16 or 32 expected");
    if (word_bits == 16 && (prm->min_bq < 0 || prm->min_bq > 63))
        return fail(SMC_E_INPUT, who + ": minBQ " + std::to_string(prm->min_bq) + " has no room in a 16-bit read word (0 .. 63)");
    if (n_loci < 0) return fail(SMC_E_INPUT, who + ": a run of " + std::to_string(n_loci) + " loci");
    if (flags & ~(SMC_LISTED_SHARED_ORDER | SMC_LISTED_DENSE_LOCUS)) return fail(SMC_E_INPUT, who + ": flags " + std::to_string(flags) + ", bits 0 and 1 expected");
    const bool shared_order = (flags & SMC_LISTED_SHARED_ORDER) != 0;
    if (!n_copies) return SMC_OK;
    if (!d_copies || !counters) return fail(SMC_E_ARG, who + ": NULL device pointer");
    if (n_listed && (!offsets || !caps)) return fail(SMC_E_ARG, who + ": NULL argument with " + std::to_string(n_listed) + " listed loci");
    if (n_listed && (!d_refseq || !words || !umi_start || !u_gid || !u_finc || !loci || !xlist)) return fail(SMC_E_ARG, who + ": NULL device pointer");
    if (slot_base & 3u) return fail(SMC_E_INPUT, who + ": slot_base " + std::to_string(slot_base) + " is not on a 4-read boundary");
    BlArgs A{};
    uint64_t stride = 0;
    uint32_t cap_max = 0;
    for (int32_t g = 0; g < n_listed; ++g) {
        if ((int64_t)offsets[g] >= (int64_t)n_loci)
            return fail(SMC_E_INPUT, who + ": listed locus " + std::to_string(g) + " names offset " + std::to_string(offsets[g]) + " of " + std::to_string(n_loci));
        if (g && offsets[g] <= offsets[g - 1]) return fail(SMC_E_INPUT, who + ": the listed offsets do not ascend at entry " + std::to_string(g));
        if ((caps[g] & 3u) || caps[g] > (uint32_t)smc_build_max_depth() + 1u)
            return fail(SMC_E_INPUT, who + ": listed locus " + std::to_string(g) + " has a capacity of " + std::to_string(caps[g]) +
                                     " slots (a multiple of 4, at most " + std::to_string(smc_build_max_depth() + 1) + ")");
        A.off[g] = offsets[g]; A.capoff[g] = (uint32_t)stride;
        stride += caps[g];
        cap_max = std::max(cap_max, caps[g]);
    }
    A.capoff[n_listed] = (uint32_t)stride;
    const uint64_t G = (uint64_t)n_listed, B = (uint64_t)n_copies;
    if ((uint64_t)slot_base + B * stride >= (1ull << 32) || (uint64_t)umi_base + B * (stride + G) + 1ull >= (1ull << 32))
        return fail(SMC_E_INPUT, who + ": " + std::to_string(n_copies) + " copies of " + std::to_string(stride) + " slots: 2^32 slots or more");
    HIPCHK(hipSetDevice(ctx->device));
    hipStream_t st = (hipStream_t)stream;
    const uint64_t Bo = shared_order ? 1ull : B;
    size_t off = 0;
    auto carve = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_k0 = carve(8 * Bo * stride), o_k1 = carve(8 * Bo * stride), o_v0 = carve(4 * Bo * stride), o_v1 = carve(4 * Bo * stride);
    const size_t o_ord = carve(4 * Bo * stride), o_hi = carve(4 * Bo * stride), o_meta = carve(16 * Bo * G);
    const size_t o_cstat = carve(4 * B), o_st = carve(4 * B * G), o_nx = carve(4 * B * G), o_xtmp = carve(20 * (size_t)BL_XMAX * B * G);
    if (int rc = grow_scratch(ctx->bl_scratch, ctx->bl_bytes, off, off + off / 8, who.c_str(), &st)) return rc;
    if (ctx->bl_done_ev) HIPCHK(hipStreamWaitEvent(st, ctx->bl_done_ev, 0));
    char* sc = (char*)ctx->bl_scratch;
    A.copies = d_copies; A.refseq = d_refseq;
    A.n_copies = n_copies; A.n_listed = n_listed; A.shared = shared_order ? 1 : 0; A.dense = (flags & SMC_LISTED_DENSE_LOCUS) ? 1 : 0; A.start0 = start0;
    A.min_bq = prm->min_bq; A.min_mq = prm->min_mq; A.primer_dist = prm->primer_dist; A.ds = prm->ds;
    A.fp = (uint32_t)smc_param_fingerprint(prm->min_bq, prm->min_mq, prm->mismatch_thr, prm->primer_dist) << SMC_LF_FP_SHIFT;
    A.w16 = word_bits == 16 ? 1u : 0u; A.slot_base = slot_base; A.umi_base = umi_base; A.stride = (uint32_t)stride;
    A.words = words; A.umi_start = umi_start; A.u_gid = u_gid; A.u_finc = u_finc; A.loci = loci; A.xlist = xlist; A.xcap = xcap; A.counters = counters;
    A.key[0] = (unsigned long long*)(sc + o_k0); A.key[1] = (unsigned long long*)(sc + o_k1);
    A.val[0] = (uint32_t*)(sc + o_v0); A.val[1] = (uint32_t*)(sc + o_v1);
    A.order = (uint32_t*)(sc + o_ord); A.hinfo = (uint32_t*)(sc + o_hi); A.meta = (uint32_t*)(sc + o_meta);
    A.cstat = (uint32_t*)(sc + o_cstat); A.st = (uint32_t*)(sc + o_st); A.nx = (uint32_t*)(sc + o_nx); A.xtmp = (uint32_t*)(sc + o_xtmp);
    hipLaunchKernelGGL(k_bl_check, dim3((unsigned)n_copies), dim3(256), 0, st, A);
    if (n_listed) {
        hipLaunchKernelGGL(k_bl_sort, dim3((unsigned)n_listed, (unsigned)Bo), dim3(64 * BL_SORT_WAVES), 0, st, A);
        if (cap_max) hipLaunchKernelGGL(k_bl_words, dim3((cap_max + 255u) / 256u, (unsigned)n_listed, (unsigned)n_copies), dim3(256), 0, st, A);
        hipLaunchKernelGGL(k_bl_finish, dim3((unsigned)n_listed, (unsigned)n_copies), dim3(256), 0, st, A);
    }
    hipLaunchKernelGGL(k_bl_gather, dim3((unsigned)n_copies), dim3(64), 0, st, A);
    HIPCHK(hipGetLastError());
    if (!ctx->bl_done_ev) HIPCHK(hipEventCreateWithFlags(&ctx->bl_done_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(ctx->bl_done_ev, st));
    return SMC_OK;
}

int smc_build_live_rows(smc_ctx* ctx, uint32_t* live, int32_t cap, int32_t* n_lists) {
    if (!ctx || !n_lists || cap < 0 || (cap > 0 && !live)) return fail(SMC_E_ARG, "smc_build_live_rows: bad argument");
    if (!ctx->bp_scratch || !ctx->bp_done_ev || ctx->bp_nlive_n <= 0) return fail(SMC_E_ARG, "smc_build_live_rows: no build on this context yet");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipEventSynchronize(ctx->bp_done_ev));
    *n_lists = ctx->bp_nlive_n;
    const int32_t n = std::min(cap, ctx->bp_nlive_n);
    if (n > 0) HIPCHK(hipMemcpy(live, (const char*)ctx->bp_scratch + ctx->bp_nlive_off, 4 * (size_t)n, hipMemcpyDeviceToHost));
    return SMC_OK;
}

int smc_build_set_timing(smc_ctx* ctx, int slots) {
    if (!ctx || slots < 0) return fail(SMC_E_ARG, "smc_build_set_timing: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    for (auto e : ctx->bp_ev0) (void)hipEventDestroy(e);
    for (auto e : ctx->bp_ev1) (void)hipEventDestroy(e);
    ctx->bp_ev0.assign((size_t)slots, nullptr);
    ctx->bp_ev1.assign((size_t)slots, nullptr);
    for (int k = 0; k < slots; ++k) { HIPCHK(hipEventCreate(&ctx->bp_ev0[(size_t)k])); HIPCHK(hipEventCreate(&ctx->bp_ev1[(size_t)k])); }
    ctx->bp_timed = 0;
    return SMC_OK;
}
int smc_build_kernel_ms(smc_ctx* ctx, float* avg_ms, int32_t* n_samples) {
    if (!ctx || !avg_ms) return fail(SMC_E_ARG, "smc_build_kernel_ms: NULL argument");
    const int64_t ns = std::min<int64_t>(ctx->bp_timed, (int64_t)ctx->bp_ev0.size());
    if (ns <= 0) return fail(SMC_E_ARG, "smc_build_kernel_ms: no timed run (smc_build_set_timing(ctx, slots) then smc_build_planes)");
    double tot = 0;
    for (int64_t k = 0; k < ns; ++k) {
        float ms = 0;
        HIPCHK(hipEventSynchronize(ctx->bp_ev1[(size_t)k]));
        HIPCHK(hipEventElapsedTime(&ms, ctx->bp_ev0[(size_t)k], ctx->bp_ev1[(size_t)k]));
        tot += ms;
    }
    *avg_ms = (float)(tot / ns);
    if (n_samples) *n_samples = (int32_t)ns;
    return SMC_OK;
}

int smc_wire_row_size(void) { return (int)sizeof(smc_wire_row); }

int smc_pack_rows(smc_ctx* ctx, const smc_row* rows, int64_t n, smc_wire_row* wire, void* stream) {
    if (!ctx || n < 0 || (n > 0 && (!rows || !wire))) return fail(SMC_E_ARG, "smc_pack_rows: bad argument");
    if (n == 0) return SMC_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const long long words = (long long)n * WIRE_WORDS;
    hipLaunchKernelGGL(k_pack_rows, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rows, (uint32_t*)wire, words);
    HIPCHK(hipGetLastError());
    return SMC_OK;
}

int smc_unpack_rows(const smc_wire_row* wire, int64_t n, smc_row* rows) {
    if (n < 0 || (n > 0 && (!wire || !rows))) return fail(SMC_E_ARG, "smc_unpack_rows: bad argument");
    for (int64_t i = 0; i < n; ++i) {
        const smc_wire_row& W = wire[i];
        smc_row& R = rows[i];
        memset(&R, 0, sizeof R);
        R.status = (int32_t)(W.status & 0xFFFFu);
        R.biallelic = (W.status & SMC_WIRE_BIALLELIC) ? 1 : 0;
        R.cvg = W.cvg; R.all_frag = W.all_frag; R.all_mt = W.all_mt; R.used_frag = W.used_frag; R.used_mt = W.used_mt;
        R.mt3 = W.mt3; R.mt5 = W.mt5; R.mt7 = W.mt7; R.mt10 = W.mt10;
        R.max_allele = R.second_allele = -1;
        for (int a = 0; a < 4; ++a) { R.dp[a] = W.dp[a]; R.umt[a] = W.umt[a]; R.vsm[a] = W.vsm[a]; R.pi[a] = W.pi[a]; }
        for (int c = 0; c < 2; ++c) {
            const smc_wire_cand& wc = W.cand[c];
            smc_cand& C = R.cand[c];
            C.allele = wc.allele;
            C.flt = wc.flags & SMC_WIRE_FLT_MASK;
            C.flt_applied = (wc.flags & SMC_WIRE_FLT_APPLIED) ? 1 : 0;
            C.vmf_lt_099 = (wc.flags & SMC_WIRE_VMF_LT_099) ? 1 : 0;
            C.vdp = wc.vdp; C.vmt = wc.vmt; C.vsm = wc.vsm; C.pi = wc.pi;
            C.p_sb = C.p_r1 = C.p_r2 = C.p_pr = NAN;
        }
    }
    return SMC_OK;
}

int smc_pool_trim(smc_ctx* ctx) {
    if (!ctx) return fail(SMC_E_ARG, "smc_pool_trim: NULL context");
    HIPCHK(hipSetDevice(ctx->device));
    plan_pool_collect(ctx, true);
    for (auto& b : ctx->plan_pool) (void)hipFree(b.second);
    ctx->plan_pool.clear();
    return SMC_OK;
}

// Large blocks (the read words of a batch, umi_start and its companions: gigabytes) are NOT taken from hipMalloc: which physical
// pages back the read words moves the walk that writes them by 10 % (k_bp_emit2: 1.29 ... 1.48 ms for the same 2.4 GB in different
// hipMalloc allocations of one process - the same from launch to launch, whatever the offset inside the allocation; translation
// misses, L2 hits and request counts are the same in a fast and a slow one: profiles/r05_place_*).  A virtual range backed by
// separately created physical handles of 64 MB each measured 1.20-1.26 ms in every process tried, below the best of thirty
// hipMalloc allocations (DESIGN.md section 5) - so that is what a caller of this library gets, with no trial at run time.
// SMC_VMM_CHUNK_MB overrides the handle size (0: plain hipMalloc for everything); blocks below SMC_VMM_MIN_MB stay with hipMalloc.
#ifndef SMC_VMM_CHUNK_MB
#define SMC_VMM_CHUNK_MB 64
#endif
#ifndef SMC_VMM_MIN_MB
#define SMC_VMM_MIN_MB 256
#endif
// NOT USED BY DEFAULT since the end of round 5.  On this ROCm (7.2) a range mapped over freshly created handles can LOSE what is
// written to it: scripts/vmm_stress.py allocates a 576 MB block this way, copies a pattern into it, reads it back after 0 / 10 /
// 30 / 100 ms with kernels running in between, frees it and starts over - every second block read back as ZEROS from some point
// on (123-159 bad read-backs in 40 blocks; whole 64 MB handles at a time; never the first block of a process, never a plain
// hipMalloc block, nor a hipMalloc block that follows the free of such a range: scripts/vmm_stress2.py).  The pages a released
// handle gives back are wiped asynchronously, and a new handle can be made of them before that has happened.  In the product it
// showed as a batch's umi_start - a fresh block of 576 MB once the batches had grown to 128 M reads - coming back zero on some
// boxes (tests/test_gpu_devplanes.py failing after other tests).  Kept for measurements: SMC_VMM_CHUNK_MB=<MB> for smc_mem_alloc,
// SMC_ALLOC_VMM=1 for smc_mem_alloc_best's candidates.
static hipError_t vmm_alloc(smc_ctx* ctx, size_t bytes, size_t chunk, void** out) {
    hipMemAllocationProp prop = {};
    prop.type = hipMemAllocationTypePinned; prop.location.type = hipMemLocationTypeDevice; prop.location.id = ctx->device;
    size_t gran = 0;
    hipError_t e = hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityRecommended);
    if (e != hipSuccess) return e;
    if (gran == 0) gran = 4096;
    chunk = (chunk + gran - 1) / gran * gran;
    const size_t total = (bytes + chunk - 1) / chunk * chunk;
    void* va = nullptr;
    e = hipMemAddressReserve(&va, total, (size_t)2 << 20, nullptr, 0);
    if (e != hipSuccess) return e;
    size_t mapped = 0;
    std::vector<hipMemGenericAllocationHandle_t> handles;
    const bool early_release = exp_env("SMC_VMM_EARLY_RELEASE") != nullptr;   // (experiments: round 5's first form - see below)
    for (; mapped < total; mapped += chunk) {
        hipMemGenericAllocationHandle_t h;
        e = hipMemCreate(&h, chunk, &prop, 0);
        if (e != hipSuccess) break;
        e = hipMemMap((char*)va + mapped, chunk, 0, h, 0);
        // (the handle stays until the range is unmapped; releasing it right after the map, as round 5's first form did, makes no
        // difference to what follows)
        if (early_release || e != hipSuccess) (void)hipMemRelease(h); else handles.push_back(h);
        if (e != hipSuccess) break;
    }
    if (e == hipSuccess) {
        hipMemAccessDesc ad = {};
        ad.location.type = hipMemLocationTypeDevice; ad.location.id = ctx->device; ad.flags = hipMemAccessFlagsProtReadWrite;
        e = hipMemSetAccess(va, total, &ad, 1);
    }
    if (e != hipSuccess) {
        if (mapped) (void)hipMemUnmap(va, mapped);
        for (auto h : handles) (void)hipMemRelease(h);
        (void)hipMemAddressFree(va, total);
        return e;
    }
    if (exp_env("SMC_VMM_CLEAR")) { (void)hipMemset(va, 0, total); (void)hipDeviceSynchronize(); }   // (experiments)
    {
        std::lock_guard<std::mutex> g(ctx->vmm_mu);
        ctx->vmm.push_back({va, total, handles});
    }
    *out = va;
    return hipSuccess;
}
int smc_mem_alloc(smc_ctx* ctx, int64_t bytes, void** out) {
    if (!ctx || !out || bytes < 0) return fail(SMC_E_ARG, "smc_mem_alloc: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    // (virtual-memory backing only on request: see vmm_alloc)
    size_t chunk_mb = 0;
    { const char* v = exp_env("SMC_VMM_CHUNK_MB"); if (v && *v) chunk_mb = (size_t)std::max(0, atoi(v)); }
    if (chunk_mb > 0 && (size_t)bytes >= ((size_t)SMC_VMM_MIN_MB << 20)) {
        if (vmm_alloc(ctx, (size_t)bytes, chunk_mb << 20, out) == hipSuccess) return SMC_OK;
        (void)hipGetLastError();                                 // (a runtime without the virtual-memory calls: hipMalloc below)
    }
    HIPCHK(hipMalloc(out, (size_t)(bytes > 0 ? bytes : 1)));
    return SMC_OK;
}
void smc_mem_free(smc_ctx* ctx, void* p) {
    if (!ctx || !p) return;
    (void)hipSetDevice(ctx->device);
    size_t total = 0;
    std::vector<hipMemGenericAllocationHandle_t> handles;
    {
        std::lock_guard<std::mutex> g(ctx->vmm_mu);
        for (size_t i = 0; i < ctx->vmm.size(); ++i)
            if (ctx->vmm[i].va == p) { total = ctx->vmm[i].total; handles.swap(ctx->vmm[i].handles); ctx->vmm.erase(ctx->vmm.begin() + (long)i); break; }
    }
    if (total) {
        (void)hipDeviceSynchronize();                            // (hipFree waits for the device by itself; an unmap does not)
        (void)hipMemUnmap(p, total);
        for (auto h : handles) (void)hipMemRelease(h);
        (void)hipMemAddressFree(p, total);
        return;
    }
    (void)hipFree(p);
}
// The write pattern of the plane builder's walk into [p, p + bytes), timed with HIP events (the fastest of three launches)
int smc_mem_write_probe(smc_ctx* ctx, void* p, int64_t bytes, float* ms) {
    if (!ctx || !p || !ms || bytes < (1 << 20)) return fail(SMC_E_ARG, "smc_mem_write_probe: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    // a 3000x panel: rows of 3000 words, 18 parts of 4 batches, 43 of a batch's 64 alignments cover a locus
    // (no arithmetic between the stores: with the walk's ~ 24 multiply-adds per store the probe stops telling the allocations
    // apart - it is the memory side that differs, and only a kernel bound by it shows that; measured over 40 allocations the
    // write-only probe's time correlates 0.92 with the walk's and its best pick was the walk's second best: profiles/r05_place_*)
    uint32_t row_words = 3000, parts = 18, batches = 4, run = 41, spin = 0;
    { const char* v = exp_env("SMC_PROBE_SPIN"); if (v) spin = (uint32_t)atoi(v); }
    { const char* v = exp_env("SMC_PROBE_SHAPE"); if (v) sscanf(v, "%u,%u,%u", &parts, &batches, &run); }   // (experiments: parts per tile, batches per part, words per run)
    // (a shape whose runs do not fit a row would store past it - for the last tile past the block: ADVICE r5)
    if (!parts || !batches || !run || run > 64u || (uint64_t)parts * batches * run > row_words)
        return fail(SMC_E_ARG, "smc_mem_write_probe: SMC_PROBE_SHAPE parts * batches * run must be 1 ... 3000 words, run <= 64");
    const uint32_t n_tiles = (uint32_t)std::min<int64_t>(1 << 20, bytes / (4ll * 64 * row_words));
    if (!n_tiles) return fail(SMC_E_ARG, "smc_mem_write_probe: block too small");
    // on a stream of its own, between its own events: a caller's kernels on the NULL stream (a prefetch thread's) are not timed with it
    hipStream_t ps;
    HIPCHK(hipStreamCreateWithFlags(&ps, hipStreamNonBlocking));
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0)); HIPCHK(hipEventCreate(&e1));
    float best = 1e30f;
    for (int rep = 0; rep < 4; ++rep) {
        HIPCHK(hipEventRecord(e0, ps));
        hipLaunchKernelGGL(k_mem_write_probe, dim3(n_tiles * parts), dim3(64), 0, ps, (uint32_t*)p, n_tiles, parts, batches, row_words, run, spin);
        HIPCHK(hipEventRecord(e1, ps));
        HIPCHK(hipEventSynchronize(e1));
        float t = 0;
        HIPCHK(hipEventElapsedTime(&t, e0, e1));
        if (rep && t < best) best = t;
    }
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipStreamDestroy(ps);
    HIPCHK(hipGetLastError());
    *ms = best;
    return SMC_OK;
}
// `bytes` of device memory for an array the plane builder's walk writes (the read words of a batch): up to `tries` allocations are
// made - virtual-memory ranges over physical handles of 64 / 32 / 128 / 16 / 256 MB and plain hipMalloc blocks in turn, all held
// until the end so that each gets other physical pages -, the walk's write pattern is timed into each (smc_mem_write_probe, ~ 4 ms
// per candidate + the allocation), the fastest is kept and the others go back.  Most allocations sit at one slow level (the walk
// 1.45 ms on the 3000x shape, probe 1.09 ms); about one in eight is of the fast kind (walk 1.16-1.26 ms, probe 0.75-0.85 ms): the
// search stops as soon as a candidate's probe is 20 % below the slowest seen.  info[0] / info[1]: the kept candidate's and the slowest candidate's probe time, info[2]: candidates
// tried.  tries <= 1 or a block below 256 MB: smc_mem_alloc.
int smc_mem_alloc_best(smc_ctx* ctx, int64_t bytes, int tries, void** out, float* info /* [3] or NULL */) {
    if (!ctx || !out || bytes < 0) return fail(SMC_E_ARG, "smc_mem_alloc_best: bad argument");
    if (info) info[0] = info[1] = info[2] = 0.f;
    if (tries <= 1 || (size_t)bytes < ((size_t)SMC_VMM_MIN_MB << 20)) return smc_mem_alloc(ctx, bytes, out);
    HIPCHK(hipSetDevice(ctx->device));
    {   // never more candidates than half of the free memory holds
        size_t fr = 0, tot = 0;
        if (hipMemGetInfo(&fr, &tot) == hipSuccess) tries = (int)std::max<size_t>(1, std::min<size_t>((size_t)tries, fr / 2 / (size_t)std::max<int64_t>(1, bytes)));
    }
    // (until the end of round 5 five of six candidates were virtual-memory ranges: hipMemCreate / hipMemMap hands out pages whose
    // wipe after an earlier release is still pending and LOSES what is written to them meanwhile - vmm_alloc above.  SMC_ALLOC_VMM=1
    // brings those candidates back for measurements.)
    static const size_t chunk_vmm[6] = {64, 64, 32, 64, 128, 0 /* hipMalloc */}, chunk_plain[6] = {0, 0, 0, 0, 0, 0};
    const size_t* chunk_mb = exp_env("SMC_ALLOC_VMM") ? chunk_vmm : chunk_plain;
    std::vector<void*> cand;
    std::vector<float> ms;
    int best = -1;
    float worst = 0.f;
    for (int t = 0; t < tries; ++t) {
        void* p = nullptr;
        const size_t cm = chunk_mb[t % 6];
        hipError_t e = cm ? vmm_alloc(ctx, (size_t)bytes, cm << 20, &p) : hipMalloc(&p, (size_t)bytes);
        if (e != hipSuccess) { (void)hipGetLastError(); if (cm && hipMalloc(&p, (size_t)bytes) != hipSuccess) { (void)hipGetLastError(); break; } if (!cm) break; }
        float t_ms = 0.f;
        if (smc_mem_write_probe(ctx, p, bytes, &t_ms) != SMC_OK) { smc_mem_free(ctx, p); break; }
        cand.push_back(p); ms.push_back(t_ms);
        if (best < 0 || t_ms < ms[(size_t)best]) best = (int)cand.size() - 1;
        worst = std::max(worst, t_ms);
        if (cand.size() >= 3 && ms[(size_t)best] <= 0.80f * worst) break;
    }
    if (best < 0) return smc_mem_alloc(ctx, bytes, out);
    for (size_t i = 0; i < cand.size(); ++i) if ((int)i != best) smc_mem_free(ctx, cand[i]);
    *out = cand[(size_t)best];
    if (info) { info[0] = ms[(size_t)best]; info[1] = worst; info[2] = (float)cand.size(); }
    return SMC_OK;
}
int smc_mem_alloc_host(smc_ctx* ctx, int64_t bytes, void** out) {
    if (!ctx || !out || bytes < 0) return fail(SMC_E_ARG, "smc_mem_alloc_host: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipHostMalloc(out, (size_t)(bytes > 0 ? bytes : 1), hipHostMallocDefault));
    return SMC_OK;
}
void smc_mem_free_host(smc_ctx* ctx, void* p) {
    if (!ctx || !p) return;
    (void)hipSetDevice(ctx->device);
    (void)hipHostFree(p);
}
int smc_mem_h2d(smc_ctx* ctx, void* dst, const void* src, int64_t bytes) {
    if (!ctx || bytes < 0 || (bytes > 0 && (!dst || !src))) return fail(SMC_E_ARG, "smc_mem_h2d: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    if (bytes) HIPCHK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyHostToDevice));
    return SMC_OK;
}
int smc_mem_d2h(smc_ctx* ctx, void* dst, const void* src, int64_t bytes) {
    if (!ctx || bytes < 0 || (bytes > 0 && (!dst || !src))) return fail(SMC_E_ARG, "smc_mem_d2h: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    if (bytes) HIPCHK(hipMemcpy(dst, src, (size_t)bytes, hipMemcpyDeviceToHost));
    return SMC_OK;
}
int smc_device_sync(smc_ctx* ctx) {
    if (!ctx) return fail(SMC_E_ARG, "smc_device_sync: NULL context");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipDeviceSynchronize());
    return SMC_OK;
}

int smc_event_create(void** ev) {
    hipEvent_t e;
    HIPCHK(hipEventCreate(&e));
    *ev = (void*)e;
    return SMC_OK;
}
int smc_event_record(void* ev, void* stream) {
    HIPCHK(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
    return SMC_OK;
}
int smc_event_elapsed_ms(void* start, void* stop, float* ms) {
    HIPCHK(hipEventSynchronize((hipEvent_t)stop));
    HIPCHK(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
    return SMC_OK;
}
void smc_event_destroy(void* ev) { (void)hipEventDestroy((hipEvent_t)ev); }

}  // extern "C"

