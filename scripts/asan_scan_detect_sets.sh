#!/bin/bash
# smc_scan_detect_sets' host wrapper (argument checks and the walk over the sets' offsets, csrc/host_abi.inc) under AddressSanitizer
# and UBSan, in a stand-alone program: every call below is refused BEFORE anything touches a device, so the program runs on a machine
# without a GPU.
# Usage: scripts/asan_scan_detect_sets.sh   (needs hipcc; prints one line per refusal and "ok")
set -euo pipefail
R=$(cd "$(dirname "$0")/.." && pwd)
T=$(mktemp -d)
trap 'rm -rf "$T"' EXIT
cat > "$T/main.hip" <<'EOS'
#include "smcounter_hip.hip"
static int n_bad = 0;
static void refused(const char* what, int rc, int want, const char* needle) {
    const char* msg = smc_last_error();
    const bool ok = rc == want && strstr(msg, needle) != nullptr;
    printf("%s %-30s rc %d: %s\n", ok ? "refused" : "NOT REFUSED", what, rc, msg);
    if (!ok) ++n_bad;
}
int main() {
    smc_ctx* ctx = new smc_ctx();
    ctx->device = 0;
    uint32_t buf[64] = {0};
    const smc_row* rows = (const smc_row*)buf;
    const int G = 14, NL = 70;
    std::vector<smc_scan_locus> listed(G);
    for (int g = 0; g < G; ++g) listed[g] = smc_scan_locus{(uint32_t)(5 * g), (uint32_t)(g % 4)};
    const std::vector<uint32_t> tile = {0, 1, 3, 6, 14};
    auto call = [&](smc_ctx* c, int B, int64_t nl, const smc_scan_locus* lh, int g, const uint32_t* off, int ns, double thr, uint32_t* cursor) {
        return smc_scan_detect_sets(c, rows, B, nl, (const smc_scan_locus*)buf, lh, g, buf, off, ns, thr, (smc_scan_verdict*)buf, buf, buf, cursor, nullptr);
    };
    refused("no context", call(nullptr, 3, NL, listed.data(), G, tile.data(), 4, 17.0, buf), SMC_E_ARG, "bad argument");
    refused("no cursor", call(ctx, 3, NL, listed.data(), G, tile.data(), 4, 17.0, nullptr), SMC_E_ARG, "bad argument");
    refused("no offsets", call(ctx, 3, NL, listed.data(), G, nullptr, 4, 17.0, buf), SMC_E_ARG, "bad argument");
    refused("no listed records", call(ctx, 3, NL, nullptr, G, tile.data(), 4, 17.0, buf), SMC_E_ARG, "NULL");
    refused("copies < 0", call(ctx, -1, NL, listed.data(), G, tile.data(), 4, 17.0, buf), SMC_E_ARG, "bad argument");
    refused("sets < 0", call(ctx, 3, NL, listed.data(), G, tile.data(), -1, 17.0, buf), SMC_E_ARG, "bad argument");
    refused("threshold NaN", call(ctx, 3, NL, listed.data(), G, tile.data(), 4, NAN, buf), SMC_E_INPUT, "not finite");
    refused("too many copies", call(ctx, 65536, NL, listed.data(), G, tile.data(), 4, 17.0, buf), SMC_E_INPUT, "at most 65535");
    refused("2^31 rows", call(ctx, 65535, 32769, listed.data(), G, tile.data(), 4, 17.0, buf), SMC_E_INPUT, "2^31");
    {   // 65535 copies x 32769 sets of one: 2^31 joint words or more
        std::vector<uint32_t> many(32770);
        for (size_t s = 0; s < many.size(); ++s) many[s] = (uint32_t)s;
        refused("2^31 joint words", call(ctx, 65535, NL, listed.data(), G, many.data(), 32769, 17.0, buf), SMC_E_INPUT, "2^31");
    }
    { auto w = listed; w[G - 1].offset = NL; refused("offset outside a copy", call(ctx, 3, NL, w.data(), G, tile.data(), 4, 17.0, buf), SMC_E_INPUT, "names offset 70 of 70"); }
    { auto w = listed; w[3].alt = 4; refused("allele id 4", call(ctx, 3, NL, w.data(), G, tile.data(), 4, 17.0, buf), SMC_E_INPUT, "allele id 4"); }
    { const uint32_t o[5] = {1, 1, 3, 6, 14}; refused("offsets start at 1", call(ctx, 3, NL, listed.data(), G, o, 4, 17.0, buf), SMC_E_INPUT, "must tile"); }
    { const uint32_t o[5] = {0, 1, 3, 6, 13}; refused("offsets end early", call(ctx, 3, NL, listed.data(), G, o, 4, 17.0, buf), SMC_E_INPUT, "must tile"); }
    { const uint32_t o[5] = {0, 1, 3, 6, 15}; refused("offsets end late", call(ctx, 3, NL, listed.data(), G, o, 4, 17.0, buf), SMC_E_INPUT, "must tile"); }
    { const uint32_t o[1] = {0}; refused("no set for the records", call(ctx, 3, NL, listed.data(), G, o, 0, 17.0, buf), SMC_E_INPUT, "must tile"); }
    { const uint32_t o[5] = {0, 0, 3, 6, 14}; refused("an empty set", call(ctx, 3, NL, listed.data(), G, o, 4, 17.0, buf), SMC_E_INPUT, "has 0 members"); }
    { const uint32_t o[5] = {0, 3, 2, 6, 14}; refused("offsets that decrease", call(ctx, 3, NL, listed.data(), G, o, 4, 17.0, buf), SMC_E_INPUT, "has -1 members"); }
    { const uint32_t o[4] = {0, 1, 5, 14}; refused("a set of nine", call(ctx, 3, NL, listed.data(), G, o, 3, 17.0, buf), SMC_E_INPUT, "has 9 members"); }
    { const uint32_t o[3] = {0, 0xFFFFFFFFu, 14}; refused("an offset at the top", call(ctx, 3, NL, listed.data(), G, o, 2, 17.0, buf), SMC_E_INPUT, "members"); }
    delete ctx;
    printf(n_bad ? "FAILED: %d\n" : "ok\n", n_bad);
    return n_bad ? 1 : 0;
}
EOS
HIPCC=${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}
"$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -I"$R/include" -I"$R/smcounter_amd/csrc" -o "$T/prog" "$T/main.hip"
ASAN_OPTIONS=detect_leaks=0 "$T/prog"
