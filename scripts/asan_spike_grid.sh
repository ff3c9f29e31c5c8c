#!/bin/bash
# smc_spike_grid_counts' and smc_read_groups_counts_frac_seeds' host wrappers (argument checks, csrc/host_abi.inc) under
# AddressSanitizer and UBSan, in a stand-alone program: every call below is refused, or has nothing to do, BEFORE anything touches a
# device, so the program runs on a machine without a GPU.
# Usage: scripts/asan_spike_grid.sh   (needs hipcc; prints one line per refusal and "ok")
set -euo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
cat > "$T/main.hip" <<'EOS'
#include "smcounter_hip.hip"
static int n_bad = 0;
static void refused(const char* what, int rc, const char* needle) {
    const char* msg = smc_last_error();
    const bool ok = rc != SMC_OK && strstr(msg, needle) != nullptr;
    printf("%s %-34s rc %d: %s\n", ok ? "refused" : "NOT REFUSED", what, rc, msg);
    if (!ok) ++n_bad;
}
int main() {
    smc_ctx* ctx = new smc_ctx();
    ctx->device = 0;
    uint64_t buf[64] = {0};
    const uint64_t* d64 = buf;
    const uint32_t* d32 = (const uint32_t*)buf;
    const uint8_t* d8 = (const uint8_t*)buf;
    std::vector<uint64_t> half(2 * 1000 * 32, 1ull << 31), above(half);
    above[1] = (1ull << 32) + 1;
    const uint32_t off[3] = {0, 3, 5}, off_down[3] = {0, 3, 2};
    const uint32_t rec_off[6] = {0, 2, 2, 5, 6, 9}, rec_down[6] = {0, 2, 1, 5, 6, 9};
    auto call = [&](smc_ctx* c, const uint32_t* o, const uint32_t* ro, int64_t n_rec, int n_var, int n_reps, const uint64_t* thr, int n_tgt,
                    const uint64_t* bthr, int n_frac, const uint64_t* d_rthr, const uint64_t* rthr, int n_rr, uint32_t* out) {
        return smc_spike_grid_counts(c, d64, d32, o, d32, ro, d64, d8, n_rec, d32, n_var, d64, n_reps, thr, n_tgt, bthr, n_frac, d_rthr, rthr, n_rr,
                                     out, nullptr);
    };
    uint32_t* out = (uint32_t*)buf;
    const uint64_t* h = half.data();
    refused("no context", call(nullptr, off, rec_off, 9, 2, 2, h, 2, h, 2, d64, h, 2, out), "bad argument");
    refused("negative records", call(ctx, off, rec_off, -1, 2, 2, h, 2, h, 2, d64, h, 2, out), "bad argument");
    refused("negative fractions", call(ctx, off, rec_off, 9, 2, 2, h, 2, h, -1, d64, h, 2, out), "bad argument");
    refused("no fraction", call(ctx, off, rec_off, 9, 2, 2, h, 2, h, 0, d64, h, 2, out), "0 fractions");
    refused("no read threshold", call(ctx, off, rec_off, 9, 2, 2, h, 2, h, 2, d64, h, 0, out), "0 read thresholds");
    refused("too many variants", call(ctx, off, rec_off, 9, SMC_AF_MAX_VARIANTS + 1, 2, h, 2, h, 2, d64, h, 2, out), "variants, at most");
    refused("too many targets", call(ctx, off, rec_off, 9, 2, 2, h, 33, h, 1, d64, h, 1, out), "33 targets");
    refused("too many replicates", call(ctx, off, rec_off, 9, 2, SMC_AF_REP_MAX_REPS + 1, h, 2, h, 2, d64, h, 2, out), "replicates, at most");
    refused("33 cells", call(ctx, off, rec_off, 9, 2, 2, h, 3, h, 1, d64, h, 11, out), "at most 32 cells");
    refused("pairs beyond int32", call(ctx, off, rec_off, 9, 2, 2, h, 1, h, 1 << 20, d64, h, 1 << 20, out), "at most 32 cells");
    refused("no fraction thresholds", call(ctx, off, rec_off, 9, 2, 2, h, 2, nullptr, 2, d64, h, 2, out), "NULL");
    refused("a spike threshold above 2^32", call(ctx, off, rec_off, 9, 2, 2, above.data(), 2, h, 2, d64, h, 2, out), "target 1: a threshold above 2^32");
    refused("a barcode threshold above 2^32", call(ctx, off, rec_off, 9, 2, 2, h, 2, above.data(), 2, d64, h, 2, out), "depth threshold 1");
    refused("a read threshold above 2^32", call(ctx, off, rec_off, 9, 2, 2, h, 2, h, 2, d64, above.data(), 2, out), "read threshold 1 of replicate 0");
    refused("no device thresholds", call(ctx, off, rec_off, 9, 2, 2, h, 2, h, 2, nullptr, h, 2, out), "NULL");
    refused("no host thresholds", call(ctx, off, rec_off, 9, 2, 2, h, 2, h, 2, d64, nullptr, 2, out), "NULL");
    refused("no output", call(ctx, off, rec_off, 9, 2, 2, h, 2, h, 2, d64, h, 2, nullptr), "NULL");
    refused("offsets decrease", call(ctx, off_down, rec_off, 9, 2, 2, h, 2, h, 2, d64, h, 2, out), "offsets decrease");
    refused("record offsets decrease", call(ctx, off, rec_down, 9, 2, 2, h, 2, h, 2, d64, h, 2, out), "record offsets decrease");
    refused("records end beyond n_rec", call(ctx, off, rec_off, 8, 2, 2, h, 2, h, 2, d64, h, 2, out), "beyond the 8 records");
    // the largest shape the limits admit reads every host threshold: 1000 replicates x 32 pairs, then the offsets stop the call
    refused("1000 x 32 thresholds read", call(ctx, off_down, rec_off, 9, 2, SMC_AF_REP_MAX_REPS, h, 1, h, 4, d64, h, 8, out), "offsets decrease");
    // nothing to do is no refusal, and still no device call: no variant, no replicate, no target
    if (call(ctx, off, rec_off, 9, 0, 2, h, 2, h, 2, d64, h, 2, out) != SMC_OK || call(ctx, off, rec_off, 9, 2, 0, h, 2, h, 2, d64, h, 2, out) != SMC_OK ||
        call(ctx, off, rec_off, 9, 2, 2, h, 0, h, 40, d64, h, 40, out) != SMC_OK) { printf("an empty call refused\n"); ++n_bad; }

    smc_read_groups* g = new smc_read_groups();
    g->ctx = ctx;
    refused("seeds: no table", smc_read_groups_counts_frac_seeds(nullptr, d64, 1, h, 1, buf), "bad argument");
    refused("seeds: negative count", smc_read_groups_counts_frac_seeds(g, d64, -1, h, 1, buf), "bad argument");
    refused("seeds: no seeds", smc_read_groups_counts_frac_seeds(g, nullptr, 1, h, 1, buf), "bad argument");
    refused("seeds: no counters", smc_read_groups_counts_frac_seeds(g, d64, 1, h, 1, nullptr), "bad argument");
    refused("seeds: table not finished", smc_read_groups_counts_frac_seeds(g, d64, 1, h, 1, buf), "not finished");
    g->finished = true;
    refused("seeds: too many", smc_read_groups_counts_frac_seeds(g, d64, SMC_AF_REP_MAX_REPS + 1, h, 1, buf), "1001 seeds");
    refused("seeds: too many fractions", smc_read_groups_counts_frac_seeds(g, d64, 1, h, SMC_RG_MAX_TARGETS + 1, buf), "bad thresholds");
    refused("seeds: a threshold above 2^32", smc_read_groups_counts_frac_seeds(g, d64, 1, above.data(), 2, buf), "above 2^32");
    if (smc_read_groups_counts_frac_seeds(g, d64, 0, h, 2, buf) != SMC_OK || smc_read_groups_counts_frac_seeds(g, d64, 2, h, 0, buf) != SMC_OK) {
        printf("an empty seeds call refused\n"); ++n_bad;
    }
    delete g;
    delete ctx;
    printf(n_bad ? "FAILED: %d\n" : "ok\n", n_bad);
    return n_bad ? 1 : 0;
}
EOS
HIPCC=${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}
"$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -I"$R/include" -I"$R/smcounter_amd/csrc" -o "$T/prog" "$T/main.hip"
ASAN_OPTIONS=detect_leaks=0 "$T/prog"
