"""Cost of --spikeScan (dev tool, GPU box).

On scripts/spike_reps_perf.py's shape (a synthetic BAM, `n_umi` barcodes x `rpb` reads per locus, 128 loci by default), three targets,
R replicates and stride S, wall time in process, after a warm-up run, medians of `REPEATS`:
(a) the run with --spikeScan, and the same run without it; the stage's own clock and its pass lines' sums from the run log;
(b) the workflow the flag replaces: every pass as a run of its own, --spikeAF --spikeVariants pass<k>.txt --spikeReps R.  A SUBSET of the
    passes is timed (`SUBSET` of them, evenly spread; each the median of `REPEATS`), and the sum over all passes is that subset's sum
    scaled by passes / subset - stated as such in the result; the subset's sensitivity lines are compared with the scan's;
(c) one batch's verdicts, device synchronised around each: smc_scan_detect over B copies of the file's rows in HBM (devplanes.scan_detect:
    the listed loci up, one launch, the 16-byte records and the list down) against the same batch downloaded whole and its listed rows
    decided by the host path (vc._strings, dsaf.replicate_entry, spike._called).  The batch is the full-depth rows of the file, B times:
    what a pass calls has the same shape.

usage: spike_scan_perf.py [n_loci] [n_umi] [rpb] [reps] [stride] [out.json]   -> one JSON line (also written to out.json when given)"""
import argparse
import collections
import contextlib
import io
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ds_af_restate  # noqa: E402
import ds_restate  # noqa: E402
from smcounter_amd import abi, cli, devplanes, fasta, spike, synth, vc, writers  # noqa: E402
from smcounter_amd.engine import DevBuf, Engine  # noqa: E402
from smcounter_amd.tools import spike_scan_lists as lists  # noqa: E402

TARGETS = (0.05, 0.02, 0.01)
SEED = 1234567
REPEATS = 5
SUBSET = 4
COPIES = 6


def verdicts(eng, bam, fa, loci, P, stride):
    """(c): smc_scan_detect against download + host path on one batch of COPIES x len(loci) rows."""
    ref = fasta.FastaFile(fa)
    parts, refs, tables = [], [], []
    for _, rb in devplanes.iter_resident_batches(bam, ref, [(c, str(p)) for c, p in loci], P, eng, all_planes=False):
        parts.append(vc.vc_resident_rows(rb, P, eng)); refs += list(rb.ref); tables += list(rb.alleles)
    rows = np.concatenate(parts)
    nl = len(rows)
    variants, _ = lists.scan_variants([(c, str(p)) for c, p in loci], ref, "transition")
    at = {(c, p): n for n, (c, p) in enumerate(loci)}
    mine = [v for v in variants if v.pos % stride == 0]
    listed = np.zeros(len(mine), abi.SCAN_LOCUS_DTYPE)
    for g, v in enumerate(mine):
        listed[g] = (at[(v.chrom, v.pos)], devplanes.SCAN_ALT_ID[v.alt])
    batch = np.tile(rows, COPIES)
    d_rows = DevBuf(eng, batch.nbytes + 256).upload(batch.view(np.uint8).reshape(-1))
    thr = writers.pi_threshold(P.mtDepth, 0)
    nothing = (collections.defaultdict(list), collections.defaultdict(list))
    sync = lambda: eng.L.smc_device_sync(eng.ctx)

    def device():
        return devplanes.scan_detect(eng, d_rows, COPIES, nl, listed, thr)

    def host():
        got = d_rows.download(abi.ROW_DTYPE, COPIES * nl)
        idx = [c * nl + int(o) for c in range(COPIES) for o in listed["offset"]]
        view = vc.LocusView([loci[i % nl][0] for i in idx], [loci[i % nl][1] for i in idx], [refs[i % nl] for i in idx], [tables[i % nl] for i in idx])
        text = vc._strings(got[idx].copy(), view, P, ref)
        return [devplanes.scan_called_host(t, mine[n % len(mine)], thr, nothing) for n, t in enumerate(text)]

    def median_ms(fn):
        fn(); sync()
        times = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            fn(); sync()
            times.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(times), 4)
    rec, todo = device()
    verdict = (rec["mt_verdict"] >> 30).reshape(-1)
    by_host = host()
    agree = all(bool(v == abi.SCAN_CALLED) == h for v, h in zip(verdict.tolist(), by_host) if v != abi.SCAN_HOST)
    out = {"copies": COPIES, "loci_per_copy": nl, "listed": len(mine), "batch_row_bytes": int(batch.nbytes),
           "verdicts_for_the_host": int(len(todo)), "device_and_host_agree": bool(agree),
           "scan_detect_ms": median_ms(device), "download_and_host_path_ms": median_ms(host)}
    out["host_over_device"] = round(out["download_and_host_path_ms"] / max(1e-9, out["scan_detect_ms"]), 1)
    d_rows.free()
    return out


def wall(tmp, bam, fa, bed, P, n_reps, stride):
    base = ["--bedTarget=%s" % bed, "--mtDepth=%d" % P.mtDepth, "--rpb=%g" % P.rpb, "--refGenome=%s" % fa, "--bamFile=%s" % bam,
            "--dsSeed=%d" % SEED]
    text = ",".join("%g" % t for t in TARGETS)
    scan = ["--spikeScan=" + text, "--spikeScanReps=%d" % n_reps, "--spikeScanStride=%d" % stride]
    parser = cli.build_parser()

    def run(prefix, *extra):
        log = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(log):
            cli.main(parser.parse_args(base + ["--outPrefix=%s" % os.path.join(tmp, prefix)] + list(extra)))
        return time.perf_counter() - t0, log.getvalue()
    run("warm", "--spikeScan=" + text, "--spikeScanReps=2", "--spikeScanStride=%d" % stride)
    with_, without, log = [], [], None
    for _ in range(REPEATS):
        t, log = run("scan", *scan)
        with_.append(t)
        without.append(run("plain")[0])
    closing = [l for l in log.splitlines() if l.startswith("--spikeScan:") and " stage " in l][-1]
    per_pass = re.findall(r"^--spikeScan pass \d+: (\d+) variants, (\d+) copies, (\d+) builds, (\d+) verdicts decided by the host, ([0-9.]+) s$",
                          log, re.M)
    res = {"reps": n_reps, "stride": stride, "repetitions": REPEATS, "with_spikeScan_s": round(statistics.median(with_), 3),
           "without_spikeScan_s": round(statistics.median(without), 3), "with_spikeScan_all_s": [round(x, 3) for x in with_],
           "stage_s": float(re.search(r"stage ([0-9.]+) s", closing).group(1)), "closing_line": closing, "passes": len(per_pass),
           "builds": sum(int(m[2]) for m in per_pass), "verdicts_decided_by_the_host": sum(int(m[3]) for m in per_pass)}
    res["flag_costs_s"] = round(res["with_spikeScan_s"] - res["without_spikeScan_s"], 3)
    res["ms_per_build"] = round(1e3 * res["stage_s"] / max(1, res["builds"]), 3)
    # (b) a subset of the passes as runs of their own
    names = lists.main(argparse.Namespace(runPath=None, bedTarget=bed, refGenome=fa, stride=stride, alt="transition",
                                          outPrefix=os.path.join(tmp, "lists")))
    step = max(1, len(names) // SUBSET)
    subset = names[::step][:SUBSET]
    mine = {}
    for line in open(os.path.join(tmp, "scan.spikeScan.sensitivity.txt")).read().splitlines()[1:]:
        f = line.split("\t")
        mine[(f[0], f[1], f[4])] = f
    total, same, compared = 0.0, True, 0
    n_sens = len(spike.SCAN_SENSITIVITY_HEADER)
    for n, name in enumerate(subset):
        extra = ("--spikeAF=" + text, "--spikeVariants=%s" % name, "--spikeReps=%d" % n_reps)
        run("passwarm%d" % n, *extra)
        total += statistics.median(run("pass%d" % n, *extra)[0] for _ in range(REPEATS))
        for line in open(os.path.join(tmp, "pass%d.spikeAF.sensitivity.txt" % n)).read().splitlines()[1:]:
            f = line.split("\t")
            same &= mine[(f[0], f[1], f[4])] == f[:n_sens]
            compared += 1
    res.update(separate_runs_subset=len(subset), separate_runs_subset_of=len(names), separate_runs_subset_sum_s=round(total, 3),
               separate_runs_all_passes_scaled_s=round(total * len(names) / len(subset), 3),
               separate_runs_note="a subset of the passes was timed; the figure for all passes is the subset's sum scaled by passes / subset",
               lines_compared=compared, scan_lines_equal_the_separate_runs=bool(same))
    res["separate_runs_scaled_over_flag_cost"] = round(res["separate_runs_all_passes_scaled_s"] / max(1e-9, res["flag_costs_s"]), 2)
    return res


def main():
    a = sys.argv[1:]
    n_loci = int(a[0]) if a else 128
    n_umi = int(a[1]) if len(a) > 1 else 2000
    rpb = int(a[2]) if len(a) > 2 else 10
    n_reps = int(a[3]) if len(a) > 3 else 32
    stride = int(a[4]) if len(a) > 4 else 16
    cfg = synth.SynthConfig("SPS", n_loci, n_umi, rpb, 20170502, alt_locus_frac=0.3, alt_af=0.1)
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, n_loci)
    bed = ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci)
    res = {"targets": list(TARGETS), "file": {"loci": n_loci, "barcodes_per_locus": n_umi, "reads_per_barcode": rpb, "records": len(A["aln"]),
                                              "make_s": round(time.perf_counter() - t0, 1)}}
    eng = Engine(0)
    res["verdicts"] = verdicts(eng, bam, fa, loci, P, stride)
    eng.close()
    res["wall"] = wall(tmp, bam, fa, bed, P, n_reps, stride)
    line = json.dumps(res)
    print(line)
    if len(a) > 5:
        with open(a[5], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
