#!/bin/bash
# smc_scan_phase_rpb_counts' host wrapper (argument checks and the walks over the rows', the joint lists' and the barcodes' offsets,
# csrc/host_abi.inc) under AddressSanitizer and UBSan, in a stand-alone program: every call below is refused BEFORE anything touches a
# device, so the program runs on a machine without a GPU.
# Usage: scripts/asan_scan_phase_rpb_counts.sh   (needs hipcc; prints one line per refusal and "ok")
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
    printf("%s %-34s rc %d: %s\n", ok ? "refused" : "NOT REFUSED", what, rc, msg);
    if (!ok) ++n_bad;
}
struct Args {
    std::vector<uint32_t> row_off{0, 2, 5}, row_var{0, 1, 2, 3, 4}, joint_off{0, 2, 3}, bc_start{0, 3, 3, 9};
    std::vector<uint64_t> thr = std::vector<uint64_t>(40, 1ull << 31), rthr = std::vector<uint64_t>(40, 1ull << 31);
    int64_t n_aln = 9, n_bc = 3;
    int32_t n_var = 5, n_rows = 2, n_reps = 2, n_targets = 2, n_rthr = 2;
};
int main() {
    smc_ctx* ctx = new smc_ctx();
    ctx->device = 0;
    uint64_t buf[64] = {0};
    const uint32_t* p32 = (const uint32_t*)buf;
    auto call = [&](smc_ctx* c, const Args& a, const uint32_t* row_var_host, const uint32_t* bc_host) {
        return smc_scan_phase_rpb_counts(c, p32, buf, (const uint8_t*)buf, a.n_aln, p32, bc_host, buf, a.n_bc, (const uint8_t*)buf, a.n_var, p32,
                                         a.row_off.data(), p32, row_var_host, p32, a.joint_off.data(), p32, p32, a.n_rows, buf, a.n_reps,
                                         a.thr.data(), a.n_targets, a.rthr.data(), a.n_rthr, (uint32_t*)buf, nullptr);
    };
    auto run = [&](const Args& a) { return call(ctx, a, a.row_var.data(), a.bc_start.data()); };
    { Args a; refused("no context", call(nullptr, a, a.row_var.data(), a.bc_start.data()), SMC_E_ARG, "bad argument"); }
    { Args a; refused("no member list", call(ctx, a, nullptr, a.bc_start.data()), SMC_E_ARG, "NULL members"); }
    { Args a; refused("no barcode starts", call(ctx, a, a.row_var.data(), nullptr), SMC_E_ARG, "NULL argument"); }
    { Args a; a.n_aln = -1; refused("alignments < 0", run(a), SMC_E_ARG, "bad argument"); }
    { Args a; a.n_var = -1; refused("bit rows < 0", run(a), SMC_E_ARG, "bad argument"); }
    { Args a; a.row_off = {0, 3, 2}; refused("row offsets that decrease", run(a), SMC_E_INPUT, "row offsets decrease at row 1"); }
    { Args a; a.joint_off = {0, 3, 2}; refused("joint offsets that decrease", run(a), SMC_E_INPUT, "joint offsets decrease at row 1"); }
    { Args a; a.row_off = {0, 2, 11}; refused("a row of nine", run(a), SMC_E_INPUT, "row 1 has 9 members"); }
    { Args a; a.row_off = {0, 0, 3}; refused("an empty row", run(a), SMC_E_INPUT, "row 0 has 0 members"); }
    { Args a; a.row_off = {0, 2, 0xFFFFFFFFu}; refused("a row offset at the top", run(a), SMC_E_INPUT, "members"); }
    { Args a; a.row_var[3] = 5; refused("a member beyond the bit rows", run(a), SMC_E_INPUT, "member 3 names bit row 5 of 5"); }
    { Args a; a.row_var[0] = 0xFFFFFFFFu; refused("a member at the top", run(a), SMC_E_INPUT, "member 0 names bit row 4294967295"); }
    { Args a; a.n_var = 0; refused("no bit rows", run(a), SMC_E_INPUT, "member 0 names bit row 0 of 0"); }
    { Args a; a.bc_start = {0, 4, 3, 9}; refused("barcode starts that decrease", run(a), SMC_E_INPUT, "barcode starts decrease at barcode 1"); }
    { Args a; a.bc_start = {0, 3, 3, 8}; refused("barcode starts end early", run(a), SMC_E_INPUT, "end at 8, not at the 9 alignments"); }
    { Args a; a.n_aln = 10; refused("barcode starts end early (n_aln)", run(a), SMC_E_INPUT, "end at 9, not at the 10 alignments"); }
    { Args a; a.n_bc = 0; a.bc_start = {0}; refused("no barcodes, alignments", run(a), SMC_E_INPUT, "end at 0, not at the 9 alignments"); }
    { Args a; a.thr[1] = (1ull << 32) + 1; refused("a target above 2^32", run(a), SMC_E_INPUT, "target 1: a threshold above 2^32"); }
    { Args a; a.rthr[1] = (1ull << 32) + 1; refused("a read threshold above 2^32", run(a), SMC_E_INPUT, "read threshold 1 is above 2^32"); }
    { Args a; a.n_rthr = 0; refused("no read threshold", run(a), SMC_E_INPUT, "0 read thresholds"); }
    { Args a; a.n_targets = 3; a.n_rthr = 11; refused("33 cells", run(a), SMC_E_INPUT, "at most 32 cells"); }
    { Args a; a.n_targets = 33; a.n_rthr = 1; refused("33 targets", run(a), SMC_E_INPUT, "33 targets, at most 32"); }
    { Args a; a.n_reps = 1001; refused("1001 replicates", run(a), SMC_E_INPUT, "1001 replicates, at most 1000"); }
    { Args a; a.n_rows = 4097; a.row_off.assign(4098, 0); a.joint_off.assign(4098, 0); refused("4097 rows", run(a), SMC_E_INPUT, "4097 rows, at most 4096"); }
    {   // the most rows there may be, every offset array read to its end: refused at the first row, which has no member
        Args a; a.n_rows = 4096; a.row_off.assign(4097, 0); a.joint_off.assign(4097, 0);
        refused("4096 rows without members", run(a), SMC_E_INPUT, "row 0 has 0 members");
    }
    delete ctx;
    printf(n_bad ? "FAILED: %d\n" : "ok\n", n_bad);
    return n_bad ? 1 : 0;
}
EOS
HIPCC=${HIPCC:-$(command -v hipcc || echo /opt/rocm/bin/hipcc)}
"$HIPCC" --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
    -I"$R/include" -I"$R/smcounter_amd/csrc" -o "$T/prog" "$T/main.hip"
ASAN_OPTIONS=detect_leaks=0 "$T/prog"
