#!/bin/bash
# smc_build_listed's host wrapper (argument checks and sizing arithmetic, csrc/host_abi.inc) under AddressSanitizer and UBSan, in a
# stand-alone program: every call below is refused BEFORE anything touches a device, so the program runs on a machine without a GPU.
# Usage: scripts/asan_build_listed.sh   (needs hipcc; prints one line per refusal and "ok")
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
    printf("%s %-28s rc %d: %s\n", ok ? "refused" : "NOT REFUSED", what, rc, msg);
    if (!ok) ++n_bad;
}
int main() {
    smc_ctx* ctx = new smc_ctx();
    ctx->device = 0;
    smc_params P{};
    P.min_bq = 20;
    uint32_t buf[64] = {0};
    const smc_listed_copy* copies = (const smc_listed_copy*)buf;
    const uint8_t* ref = (const uint8_t*)buf;
    std::vector<uint32_t> off(SMC_LISTED_MAX_LOCI + 1), cap(SMC_LISTED_MAX_LOCI + 1, 4u);
    for (size_t g = 0; g < off.size(); ++g) off[g] = (uint32_t)g;
    auto call = [&](smc_ctx* c, const smc_params* p, const smc_listed_copy* cp, int B, int nl, const uint32_t* o, const uint32_t* k, int G, int bits,
                    uint32_t slot_base, uint32_t umi_base, void* words, uint32_t* counters) {
        return smc_build_listed(c, p, cp, B, 0, 1000, nl, ref, o, k, G, bits, slot_base, umi_base, words, buf, buf, buf, (smc_locus*)buf, buf, 8, counters, nullptr);
    };
    refused("no context", call(nullptr, &P, copies, 1, 64, off.data(), cap.data(), 1, 32, 0, 0, buf, buf), "NULL");
    refused("no params", call(ctx, nullptr, copies, 1, 64, off.data(), cap.data(), 1, 32, 0, 0, buf, buf), "NULL");
    refused("no copies", call(ctx, &P, nullptr, 1, 64, off.data(), cap.data(), 1, 32, 0, 0, buf, buf), "NULL");
    refused("no counters", call(ctx, &P, copies, 1, 64, off.data(), cap.data(), 1, 32, 0, 0, buf, nullptr), "NULL");
    refused("no words", call(ctx, &P, copies, 1, 64, off.data(), cap.data(), 1, 32, 0, 0, nullptr, buf), "NULL");
    refused("no offsets", call(ctx, &P, copies, 1, 64, nullptr, cap.data(), 1, 32, 0, 0, buf, buf), "NULL");
    refused("no capacities", call(ctx, &P, copies, 1, 64, off.data(), nullptr, 1, 32, 0, 0, buf, buf), "NULL");
    refused("B < 0", call(ctx, &P, copies, -1, 64, off.data(), cap.data(), 1, 32, 0, 0, buf, buf), "copies");
    refused("B too large", call(ctx, &P, copies, SMC_LISTED_MAX_COPIES + 1, 64, off.data(), cap.data(), 1, 32, 0, 0, buf, buf), "copies");
    refused("G < 0", call(ctx, &P, copies, 1, 64, off.data(), cap.data(), -1, 32, 0, 0, buf, buf), "listed loci");
    refused("G too large", call(ctx, &P, copies, 1, 128, off.data(), cap.data(), SMC_LISTED_MAX_LOCI + 1, 32, 0, 0, buf, buf), "listed loci");
    refused("word width", call(ctx, &P, copies, 1, 64, off.data(), cap.data(), 1, 24, 0, 0, buf, buf), "bits");
    { smc_params Q = P; Q.min_bq = 64; refused("minBQ in 16 bits", call(ctx, &Q, copies, 1, 64, off.data(), cap.data(), 1, 16, 0, 0, buf, buf), "minBQ"); }
    refused("n_loci < 0", call(ctx, &P, copies, 1, -1, off.data(), cap.data(), 1, 32, 0, 0, buf, buf), "loci");
    refused("offset outside the run", call(ctx, &P, copies, 1, 3, off.data(), cap.data(), 4, 32, 0, 0, buf, buf), "offset 3 of 3");
    { const uint32_t o2[2] = {5, 5}; refused("offsets equal", call(ctx, &P, copies, 1, 64, o2, cap.data(), 2, 32, 0, 0, buf, buf), "ascend"); }
    { const uint32_t o2[2] = {5, 4}; refused("offsets descending", call(ctx, &P, copies, 1, 64, o2, cap.data(), 2, 32, 0, 0, buf, buf), "ascend"); }
    { const uint32_t c2[1] = {6}; refused("capacity not 4-aligned", call(ctx, &P, copies, 1, 64, off.data(), c2, 1, 32, 0, 0, buf, buf), "capacity"); }
    { const uint32_t c2[1] = {1u << 25}; refused("capacity too deep", call(ctx, &P, copies, 1, 64, off.data(), c2, 1, 32, 0, 0, buf, buf), "capacity"); }
    refused("unknown flag bit", smc_build_listed(ctx, &P, copies, 1, 4, 1000, 64, ref, off.data(), cap.data(), 1, 32, 0, 0, buf, buf, buf, buf, (smc_locus*)buf, buf, 8, buf, nullptr), "flags");
    refused("slot_base unaligned", call(ctx, &P, copies, 1, 64, off.data(), cap.data(), 1, 32, 2, 0, buf, buf), "boundary");
    {   // the sizing arithmetic at its limits: 64 loci of 2^24 slots x 1024 copies, bases at the top of the range
        std::vector<uint32_t> big(SMC_LISTED_MAX_LOCI, 1u << 24);
        refused("2^32 slots", call(ctx, &P, copies, SMC_LISTED_MAX_COPIES, 64, off.data(), big.data(), SMC_LISTED_MAX_LOCI, 32, 0, 0, buf, buf), "2^32");
        refused("slot_base at the top", call(ctx, &P, copies, 1, 64, off.data(), cap.data(), 1, 32, 0xFFFFFFFCu, 0, buf, buf), "2^32");
        refused("umi_base at the top", call(ctx, &P, copies, 1, 64, off.data(), cap.data(), 1, 32, 0, 0xFFFFFFFFu, buf, buf), "2^32");
    }
    // nothing to do is no refusal, and still no device call: no copy
    if (call(ctx, &P, copies, 0, 64, off.data(), cap.data(), 1, 32, 0, 0, buf, buf) != SMC_OK) { printf("B = 0 refused\n"); ++n_bad; }
    delete ctx;
    printf(n_bad ? "FAILED: %d\n" : "ok\n", n_bad);
    return n_bad ? 1 : 0;
}
EOS
HIPCC=${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}
"$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -I"$R/include" -I"$R/smcounter_amd/csrc" -o "$T/prog" "$T/main.hip"
ASAN_OPTIONS=detect_leaks=0 "$T/prog"
