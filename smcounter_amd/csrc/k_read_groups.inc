// Included by smcounter_hip.hip after k_philox_marks.inc (it uses smc_philox4x32_10) and after k_select_aln.inc (the --dsGrid
// passes below use its sel_draw, the barcode draw of --dsMT's philox rule).
// ------------------------------------------------------------------------------------------
// the read-level philox sampler of --dsRpb (smc_read_groups_*): a file-wide table of read names and barcodes in HBM
// ------------------------------------------------------------------------------------------
// ds.reads.withinMT.py:37-58 groups the placed records of the whole file by barcode: per barcode its distinct full read names in
// order of first appearance, probKeep from the counts (one / multi / multi_names).  The reference then draws one Python 2 random()
// per name in dict order; this sampler keeps a name when it is its barcode's first, or when word 0 of Philox4x32-10(counter =
// (identity lo, identity hi, RG_DOMAIN, 0), key = (seed lo, seed hi)) < thr - a draw per name, so the kept sets of two targets are
// nested and nothing depends on how the file is cut into runs.
// The table: two power-of-two open-addressing tables (linear probing, load factor at most 0.5, sized from the placed-record count -
// an upper bound of both the names and the barcodes), a 16-byte slot each {identity, check word, first ordinal}; a name slot also
// has an info word, its barcode's slot (| RG_FIRST once it is known to be the barcode's first name).  Identity 0 marks an empty slot.
// Launches (one stream):
//   k_rg_init     empty slots
//   k_rg_insert   per record: the barcode slot, then the name slot - a 64-bit CAS claims an empty slot, an atomic minimum keeps
//                 the first ordinal; the claimant writes the check word (and, for a name, its barcode slot)
//   k_rg_verify   per record, after every insert: the slots' check words and the name's barcode slot against the record's - a
//                 difference is a hash collision (status bits; the host refuses the file)
//   k_rg_link     per name slot: the barcode's name count; first name iff the name's first ordinal is the barcode's
//   k_rg_reduce   per barcode slot: barcodes, one, multi, multi_names into 64-bit counters (names and first names by k_rg_link)
//   k_rg_masks    per run: a wave of 64 read-name ids looks up its names and writes two mask words per target (the bit layout
//                 smc_select_alignments_keyed takes at SMC_SEL_KEY_READ)
//   k_rg_kept     per name slot: the kept names of every target, for the run log
// and, for --dsGrid (below): k_rg_reduce_frac, k_rg_masks_grid, k_rg_kept_grid; for --spikeGrid: k_rg_reduce_frac_seeds.
// Every probe loop ends after `capacity` steps: a full table sets RG_FULL and the record is dropped (not met: load <= 0.5).
#define RG_BLOCK 256
#define RG_DOMAIN 0x64735250u               // counter word 2 of the read draw ("dsRP"); SEL_DOMAIN "dsMT" is the barcode draw's
#define RG_FIRST 0x80000000u                // (name info) the barcode's first name
#define RG_NONE 0xFFFFFFFFu

struct RgSlot {
    unsigned long long key;                 // identity (FNV-1a 64 of the text); 0: empty
    uint32_t chk;                           // check word (FNV-1a 32 of the same text)
    uint32_t first;                         // smallest ordinal of the records with this key
};
static_assert(sizeof(RgSlot) == 16, "RgSlot is one 16-byte slot");

struct RgTable {
    RgSlot* name;
    uint32_t* name_info;                    // barcode slot of the name | RG_FIRST
    RgSlot* bc;
    uint32_t* bc_cnt;                       // names per barcode
    unsigned long long n_mask, b_mask;      // capacities - 1
    uint32_t* status;                       // SMC_RG_* bits
    unsigned long long* ctr;                // RG_C_* counters
};
#define RG_C_NAMES 0
#define RG_C_BARCODES 1
#define RG_C_ONE 2
#define RG_C_MULTI 3
#define RG_C_MULTI_NAMES 4
#define RG_C_FIRST 5
#define RG_N_CTR 8

struct RgThr { unsigned long long t[SMC_RG_MAX_TARGETS]; };   // floor(probKeep * 2^32) per target, in [0, 2^32]

__device__ __forceinline__ unsigned long long rg_hash(unsigned long long x) {   // (splitmix64's finaliser: the home slot)
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// claim or find the slot of `key`, keep the smallest ordinal; *claimed: this thread wrote the key.  RG_NONE: the table is full.
__device__ __forceinline__ uint32_t rg_claim(RgSlot* __restrict__ T, unsigned long long mask, unsigned long long key, uint32_t chk,
                                             uint32_t ord, bool& claimed) {
    unsigned long long h = rg_hash(key) & mask;
    claimed = false;
    for (unsigned long long step = 0; step <= mask; ++step) {
        RgSlot* s = T + h;
        unsigned long long cur = __hip_atomic_load(&s->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (cur == 0ull) cur = atomicCAS(&s->key, 0ull, key);
        if (cur == 0ull) {
            s->chk = chk;
            claimed = true;
            atomicMin(&s->first, ord);
            return (uint32_t)h;
        }
        if (cur == key) {
            // (records come in file order: the slot's first ordinal is almost always below this one already - no atomic then)
            if (ord < __hip_atomic_load(&s->first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(&s->first, ord);
            return (uint32_t)h;
        }
        h = (h + 1) & mask;
    }
    return RG_NONE;
}

// the slot of `key`, or RG_NONE (read-only: after the inserts)
__device__ __forceinline__ uint32_t rg_find(const RgSlot* __restrict__ T, unsigned long long mask, unsigned long long key) {
    unsigned long long h = rg_hash(key) & mask;
    for (unsigned long long step = 0; step <= mask; ++step) {
        const unsigned long long cur = T[h].key;
        if (cur == key) return (uint32_t)h;
        if (cur == 0ull) return RG_NONE;
        h = (h + 1) & mask;
    }
    return RG_NONE;
}

// empty slots; first ordinals at the largest value (the atomic minimum brings them down)
__global__ __launch_bounds__(RG_BLOCK) void k_rg_init(RgTable G) {
    for (unsigned long long s = (unsigned long long)blockIdx.x * RG_BLOCK + threadIdx.x; s <= G.n_mask; s += (unsigned long long)gridDim.x * RG_BLOCK) {
        G.name[s] = RgSlot{0ull, 0u, RG_NONE};
        G.name_info[s] = 0u;
    }
    for (unsigned long long s = (unsigned long long)blockIdx.x * RG_BLOCK + threadIdx.x; s <= G.b_mask; s += (unsigned long long)gridDim.x * RG_BLOCK) {
        G.bc[s] = RgSlot{0ull, 0u, RG_NONE};
        G.bc_cnt[s] = 0u;
    }
}

__global__ __launch_bounds__(RG_BLOCK) void k_rg_insert(RgTable G, const smc_read_key* __restrict__ keys, uint32_t n, uint32_t ord0) {
    for (uint32_t i = blockIdx.x * RG_BLOCK + threadIdx.x; i < n; i += gridDim.x * RG_BLOCK) {
        const smc_read_key k = keys[i];
        if (k.name_id == 0ull || k.bc_id == 0ull) { atomicOr(G.status, SMC_RG_RESERVED); continue; }
        bool claimed;
        const uint32_t b = rg_claim(G.bc, G.b_mask, k.bc_id, k.bc_chk, ord0 + i, claimed);
        if (b == RG_NONE) { atomicOr(G.status, SMC_RG_FULL); continue; }
        const uint32_t s = rg_claim(G.name, G.n_mask, k.name_id, k.name_chk, ord0 + i, claimed);
        if (s == RG_NONE) { atomicOr(G.status, SMC_RG_FULL); continue; }
        if (claimed) G.name_info[s] = b;
    }
}

__global__ __launch_bounds__(RG_BLOCK) void k_rg_verify(RgTable G, const smc_read_key* __restrict__ keys, uint32_t n) {
    for (uint32_t i = blockIdx.x * RG_BLOCK + threadIdx.x; i < n; i += gridDim.x * RG_BLOCK) {
        const smc_read_key k = keys[i];
        if (k.name_id == 0ull || k.bc_id == 0ull) continue;
        const uint32_t b = rg_find(G.bc, G.b_mask, k.bc_id), s = rg_find(G.name, G.n_mask, k.name_id);
        if (b == RG_NONE || s == RG_NONE) continue;                // (full: reported by k_rg_insert)
        if (G.bc[b].chk != k.bc_chk) atomicOr(G.status, SMC_RG_BARCODE_COLLISION);
        // (one name identity whose records name two barcodes: two names behind it)
        if (G.name[s].chk != k.name_chk || G.name_info[s] != b) atomicOr(G.status, SMC_RG_NAME_COLLISION);
    }
}

__device__ __forceinline__ unsigned long long rg_wave_sum(unsigned long long v) {
    for (int o = WAVE / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, WAVE);
    return v;
}

// (grid-stride loops whose bound is wave-uniform: every lane of a wave takes part in each round's ballot / reduction)
__global__ __launch_bounds__(RG_BLOCK) void k_rg_link(RgTable G) {
    const unsigned long long n = G.n_mask + 1, stride = (unsigned long long)gridDim.x * RG_BLOCK;
    const int lane = threadIdx.x & (WAVE - 1);
    unsigned long long names = 0, firsts = 0;
    for (unsigned long long w = ((unsigned long long)blockIdx.x * RG_BLOCK + threadIdx.x) - lane; w < n; w += stride) {
        const unsigned long long s = w + lane;
        bool used = false, first = false;
        if (s < n && G.name[s].key != 0ull) {
            const uint32_t b = G.name_info[s] & ~RG_FIRST;
            used = true;
            atomicAdd(&G.bc_cnt[b], 1u);
            first = G.name[s].first == G.bc[b].first;
            G.name_info[s] = b | (first ? RG_FIRST : 0u);
        }
        names += used; firsts += first;
    }
    names = rg_wave_sum(names); firsts = rg_wave_sum(firsts);
    if (lane == 0) {
        if (names) atomicAdd(&G.ctr[RG_C_NAMES], names);
        if (firsts) atomicAdd(&G.ctr[RG_C_FIRST], firsts);
    }
}

__global__ __launch_bounds__(RG_BLOCK) void k_rg_reduce(RgTable G) {
    const unsigned long long n = G.b_mask + 1, stride = (unsigned long long)gridDim.x * RG_BLOCK;
    const int lane = threadIdx.x & (WAVE - 1);
    unsigned long long bcs = 0, one = 0, multi = 0, multi_names = 0;
    for (unsigned long long w = ((unsigned long long)blockIdx.x * RG_BLOCK + threadIdx.x) - lane; w < n; w += stride) {
        const unsigned long long s = w + lane;
        if (s < n && G.bc[s].key != 0ull) {
            const uint32_t c = G.bc_cnt[s];
            bcs += 1; one += c == 1u; multi += c >= 2u; multi_names += c >= 2u ? c : 0u;
        }
    }
    bcs = rg_wave_sum(bcs); one = rg_wave_sum(one); multi = rg_wave_sum(multi); multi_names = rg_wave_sum(multi_names);
    if (lane == 0 && bcs) {
        atomicAdd(&G.ctr[RG_C_BARCODES], bcs);
        if (one) atomicAdd(&G.ctr[RG_C_ONE], one);
        if (multi) atomicAdd(&G.ctr[RG_C_MULTI], multi);
        if (multi_names) atomicAdd(&G.ctr[RG_C_MULTI_NAMES], multi_names);
    }
}

__device__ __forceinline__ uint32_t rg_draw(unsigned long long id, unsigned long long seed) {
    uint32_t x[4];
    smc_philox4x32_10((uint32_t)id, (uint32_t)(id >> 32), RG_DOMAIN, 0u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
    return x[0];
}

// masks[t * n_words + (g >> 5)] bit (g & 31): read-name id g is kept at target t.  One thread per id, a wave writes two words per
// target; n_words = ceil(n_ids / 32) (the last wave's second word only when it exists).
__global__ __launch_bounds__(RG_BLOCK) void k_rg_masks(RgTable G, const unsigned long long* __restrict__ ident, uint32_t n_ids,
                                                       unsigned long long seed, RgThr T, int n_thr, uint32_t* __restrict__ masks,
                                                       uint32_t n_words) {
    const uint32_t g = blockIdx.x * RG_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    bool found = false, first = false;
    uint32_t u = 0;
    if (g < n_ids) {
        const unsigned long long id = ident[g];
        const uint32_t s = id ? rg_find(G.name, G.n_mask, id) : RG_NONE;
        if (s == RG_NONE) atomicOr(G.status, SMC_RG_MISS);
        else { found = true; first = (G.name_info[s] & RG_FIRST) != 0u; u = rg_draw(id, seed); }
    }
    const uint32_t word = (g - lane) >> 5;             // the wave's first word
    for (int t = 0; t < n_thr; ++t) {
        const unsigned long long m = __ballot(found && (first || (unsigned long long)u < T.t[t]));
        if (lane == 0) {
            if (word < n_words) masks[(size_t)t * n_words + word] = (uint32_t)m;
            if (word + 1 < n_words) masks[(size_t)t * n_words + word + 1] = (uint32_t)(m >> 32);
        }
    }
}

__global__ __launch_bounds__(RG_BLOCK) void k_rg_kept(RgTable G, unsigned long long seed, RgThr T, int n_thr, unsigned long long* __restrict__ kept) {
    const unsigned long long n = G.n_mask + 1, stride = (unsigned long long)gridDim.x * RG_BLOCK;
    const int lane = threadIdx.x & (WAVE - 1);
    for (unsigned long long w = ((unsigned long long)blockIdx.x * RG_BLOCK + threadIdx.x) - lane; w < n; w += stride) {
        const unsigned long long s = w + lane;
        bool used = false, first = false;
        uint32_t u = 0;
        if (s < n && G.name[s].key != 0ull) {
            used = true;
            first = (G.name_info[s] & RG_FIRST) != 0u;
            u = rg_draw(G.name[s].key, seed);
        }
        for (int t = 0; t < n_thr; ++t) {
            const unsigned long long m = __ballot(used && (first || (unsigned long long)u < T.t[t]));
            if (lane == 0 && m) atomicAdd(&kept[t], (unsigned long long)__popcll(m));
        }
    }
}

// ---- --dsGrid: the barcode rule of --dsMT (--dsSampler philox) and the read rule above composed, over the same table
// A name is kept in cell (f, r) when its barcode's draw - sel_draw (k_select_aln.inc: sel_keep's, over the barcode slot's identity) -
// is below thr_f, and it is its barcode's first name or its own draw (rg_draw) is below the cell's read threshold.  Three launches:
//   k_rg_reduce_frac  per barcode slot, per fraction: the kept barcodes' barcodes / one / multi / multi_names (probKeep of a cell is
//                     computed from them on the host).  Per wave ballots and one sum, per workgroup in LDS, then one global atomic
//                     per workgroup and counter (a per-wave atomic would be millions on a handful of lines at 32 fractions)
//   k_rg_masks_grid   per run: k_rg_masks with the barcode draw in front (the name slot's info word gives its barcode slot)
//   k_rg_kept_grid    per name slot: the kept names of every cell, for the run log (per workgroup in LDS as k_rg_reduce_frac)
// The two reducing passes run on at most RG_RED_GRID workgroups (grid-stride): one global atomic per workgroup and counter.
#define RG_F_BARCODES 0
#define RG_F_ONE 1
#define RG_F_MULTI 2
#define RG_F_MULTI_NAMES 3
#define RG_F_N 4                            // counters per fraction (names = one + multi_names)
#define RG_RED_GRID 1024                    // workgroups of k_rg_reduce_frac / k_rg_kept_grid (4 per CU)

struct RgGridThr {
    unsigned long long bc[SMC_RG_MAX_TARGETS];   // per cell: floor(f * 2^32), 2^32 at f >= 1 (sel_keep's thr)
    unsigned long long rd[SMC_RG_MAX_TARGETS];   // per cell: floor(probKeep * 2^32) in [0, 2^32]
};

// (the body of k_rg_reduce_frac and k_rg_reduce_frac_seeds: one seed's counters over the workgroup's share of the barcode slots;
// `acc`: SMC_RG_MAX_TARGETS * RG_F_N words of LDS; every thread of the workgroup calls it, it begins and ends with a barrier)
__device__ __forceinline__ void rg_reduce_frac_seed(const RgTable& G, unsigned long long seed, const RgThr& F, int n_frac,
                                                    unsigned long long* __restrict__ acc, unsigned long long* __restrict__ out) {
    for (int k = threadIdx.x; k < n_frac * RG_F_N; k += RG_BLOCK) acc[k] = 0ull;
    __syncthreads();
    const unsigned long long n = G.b_mask + 1, stride = (unsigned long long)gridDim.x * RG_BLOCK;
    const int lane = threadIdx.x & (WAVE - 1);
    for (unsigned long long w = ((unsigned long long)blockIdx.x * RG_BLOCK + threadIdx.x) - lane; w < n; w += stride) {
        const unsigned long long s = w + lane;
        bool used = false;
        uint32_t c = 0, u = 0;
        if (s < n && G.bc[s].key != 0ull) {
            used = true;
            c = G.bc_cnt[s];
            u = sel_draw(G.bc[s].key, seed);
        }
        if (__ballot(used) == 0ull) continue;                      // (wave-uniform)
        for (int f = 0; f < n_frac; ++f) {
            const bool kept = used && (unsigned long long)u < F.t[f];
            const unsigned long long bcs = __ballot(kept);
            if (bcs == 0ull) continue;                             // (wave-uniform)
            const unsigned long long one = __ballot(kept && c == 1u), multi = __ballot(kept && c >= 2u);
            const unsigned long long multi_names = rg_wave_sum(kept && c >= 2u ? (unsigned long long)c : 0ull);
            if (lane == 0) {
                unsigned long long* a = acc + f * RG_F_N;
                atomicAdd(&a[RG_F_BARCODES], (unsigned long long)__popcll(bcs));
                if (one) atomicAdd(&a[RG_F_ONE], (unsigned long long)__popcll(one));
                if (multi) {
                    atomicAdd(&a[RG_F_MULTI], (unsigned long long)__popcll(multi));
                    atomicAdd(&a[RG_F_MULTI_NAMES], multi_names);
                }
            }
        }
    }
    __syncthreads();
    for (int k = threadIdx.x; k < n_frac * RG_F_N; k += RG_BLOCK)
        if (acc[k]) atomicAdd(&out[k], acc[k]);
    __syncthreads();
}

__global__ __launch_bounds__(RG_BLOCK) void k_rg_reduce_frac(RgTable G, unsigned long long seed, RgThr F, int n_frac,
                                                             unsigned long long* __restrict__ out) {
    __shared__ unsigned long long acc[SMC_RG_MAX_TARGETS * RG_F_N];
    rg_reduce_frac_seed(G, seed, F, n_frac, acc, out);
}

// (--spikeGrid) k_rg_reduce_frac with the replicate as a grid dimension: blockIdx.y strides over the n_seeds seeds,
// out[(j * n_frac + f) * RG_F_N + k] the counters of seed j (zeroed before the launch) - one launch where --spikeReps R would make R
__global__ __launch_bounds__(RG_BLOCK) void k_rg_reduce_frac_seeds(RgTable G, const unsigned long long* __restrict__ seeds, int n_seeds, RgThr F,
                                                                   int n_frac, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long acc[SMC_RG_MAX_TARGETS * RG_F_N];
    for (int j = blockIdx.y; j < n_seeds; j += gridDim.y)
        rg_reduce_frac_seed(G, seeds[j], F, n_frac, acc, out + (size_t)j * n_frac * RG_F_N);
}

// masks[c * n_words + (g >> 5)] bit (g & 31): read-name id g is kept in cell c (k_rg_masks' layout, a mask per cell)
__global__ __launch_bounds__(RG_BLOCK) void k_rg_masks_grid(RgTable G, const unsigned long long* __restrict__ ident, uint32_t n_ids,
                                                            unsigned long long seed, RgGridThr T, int n_cells, uint32_t* __restrict__ masks,
                                                            uint32_t n_words) {
    const uint32_t g = blockIdx.x * RG_BLOCK + threadIdx.x;
    const int lane = threadIdx.x & (WAVE - 1);
    bool found = false, first = false;
    uint32_t ub = 0, un = 0;
    if (g < n_ids) {
        const unsigned long long id = ident[g];
        const uint32_t s = id ? rg_find(G.name, G.n_mask, id) : RG_NONE;
        if (s == RG_NONE) atomicOr(G.status, SMC_RG_MISS);
        else {
            const uint32_t info = G.name_info[s];
            found = true;
            first = (info & RG_FIRST) != 0u;
            ub = sel_draw(G.bc[info & ~RG_FIRST].key, seed);       // (the slot index is below the capacity: k_rg_insert wrote it)
            un = rg_draw(id, seed);
        }
    }
    const uint32_t word = (g - lane) >> 5;             // the wave's first word
    for (int c = 0; c < n_cells; ++c) {
        const unsigned long long m = __ballot(found && (unsigned long long)ub < T.bc[c] && (first || (unsigned long long)un < T.rd[c]));
        if (lane == 0) {
            if (word < n_words) masks[(size_t)c * n_words + word] = (uint32_t)m;
            if (word + 1 < n_words) masks[(size_t)c * n_words + word + 1] = (uint32_t)(m >> 32);
        }
    }
}

__global__ __launch_bounds__(RG_BLOCK) void k_rg_kept_grid(RgTable G, unsigned long long seed, RgGridThr T, int n_cells,
                                                           unsigned long long* __restrict__ kept) {
    __shared__ unsigned long long acc[SMC_RG_MAX_TARGETS];
    for (int c = threadIdx.x; c < n_cells; c += RG_BLOCK) acc[c] = 0ull;
    __syncthreads();
    const unsigned long long n = G.n_mask + 1, stride = (unsigned long long)gridDim.x * RG_BLOCK;
    const int lane = threadIdx.x & (WAVE - 1);
    for (unsigned long long w = ((unsigned long long)blockIdx.x * RG_BLOCK + threadIdx.x) - lane; w < n; w += stride) {
        const unsigned long long s = w + lane;
        bool used = false, first = false;
        uint32_t ub = 0, un = 0;
        if (s < n && G.name[s].key != 0ull) {
            const uint32_t info = G.name_info[s];
            used = true;
            first = (info & RG_FIRST) != 0u;
            ub = sel_draw(G.bc[info & ~RG_FIRST].key, seed);
            un = rg_draw(G.name[s].key, seed);
        }
        for (int c = 0; c < n_cells; ++c) {
            const unsigned long long m = __ballot(used && (unsigned long long)ub < T.bc[c] && (first || (unsigned long long)un < T.rd[c]));
            if (lane == 0 && m) atomicAdd(&acc[c], (unsigned long long)__popcll(m));
        }
    }
    __syncthreads();
    for (int c = threadIdx.x; c < n_cells; c += RG_BLOCK)
        if (acc[c]) atomicAdd(&kept[c], acc[c]);
}
