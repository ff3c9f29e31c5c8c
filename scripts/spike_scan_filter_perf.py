"""Cost of --spikeScanFilter (dev tool, GPU box) -> profiles/spike_scan_filter_perf.json.

On scripts/spike_scan_perf.py's input (a synthetic BAM, 128 loci x 2000 barcodes x 10 reads, three targets, R = 32, S = 16).  Every
timed run is made in a FRESH process (this one starts them one at a time and never opens the GPU itself); a process makes a warm-up
run first (R = 2), then the timed one; a figure is the median of `REPEATS` processes:
(a) the scan with --spikeScanFilter against the same scan without it on this tree, alternating; the stage's clock, the smc_scan_filter
    calls (one per called batch) and the words they bring down, the log's closing lines;
(b) the plain --spikeScan run on this tree against a built checkout of the parent commit (`--parent DIR`; left out without it),
    alternating: the parent's runs give the run-to-run spread this tree's median is held against.
No number is fixed in advance; the JSON says what was measured and what was not.

usage: spike_scan_filter_perf.py [--parent DIR] [--out profiles/spike_scan_filter_perf.json]"""
import argparse
import contextlib
import io
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = (0.05, 0.02, 0.01)
SEED = 1234567
REPEATS = 5
N_LOCI, N_UMI, RPB, REPS, STRIDE = 128, 2000, 10, 32, 16


def _use(tree):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))


def child_cli(job):
    """One warm-up run and one timed run of the command line in the tree job["tree"] -> dict(seconds, log, calls, words)."""
    _use(job["tree"])
    from smcounter_amd import cli, devplanes
    parser = cli.build_parser()
    calls = []
    real = getattr(devplanes, "scan_filter", None)          # (the parent commit has none)
    if real is not None:
        def counted(*a, **kw):
            out = real(*a, **kw)
            calls.append(int(out.size))
            return out
        devplanes.scan_filter = counted

    def run(prefix, extra):
        log = io.StringIO()
        del calls[:]
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(log):
            cli.main(parser.parse_args(job["base"] + ["--outPrefix=%s" % os.path.join(job["tmp"], prefix)] + extra))
        return time.perf_counter() - t0, log.getvalue()
    run(job["prefix"] + ".warm", job["warm"])
    t, log = run(job["prefix"], job["extra"])
    return {"seconds": t, "log": log, "calls": len(calls), "words": sum(calls)}


def spawn(job):
    """A fresh process for one job -> its JSON answer."""
    print("[%s] %s" % (time.strftime("%H:%M:%S"), job["prefix"]), file=sys.stderr, flush=True)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(job)], stdout=subprocess.PIPE, check=True,
                         cwd=job["tree"])
    return json.loads(out.stdout.decode().splitlines()[-1])


def med(xs):
    return round(statistics.median(xs), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for measurement (b)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spike_scan_filter_perf.json"))
    args = ap.parse_args()
    if args.child:
        print(json.dumps(child_cli(json.loads(args.child))))
        return
    _use(ROOT)
    import ds_af_restate
    import ds_restate
    from smcounter_amd import synth
    cfg = synth.SynthConfig("SPS", N_LOCI, N_UMI, RPB, 20170502, alt_locus_frac=0.3, alt_af=0.1)
    tmp = tempfile.mkdtemp()
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, N_LOCI)
    bed = ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci)
    base = ["--bedTarget=%s" % bed, "--mtDepth=%d" % P.mtDepth, "--rpb=%g" % P.rpb, "--refGenome=%s" % fa, "--bamFile=%s" % bam, "--dsSeed=%d" % SEED]
    text = ",".join("%g" % t for t in TARGETS)
    scan = ["--spikeScan=" + text, "--spikeScanReps=%d" % REPS, "--spikeScanStride=%d" % STRIDE]
    warm = ["--spikeScan=" + text, "--spikeScanReps=2", "--spikeScanStride=%d" % STRIDE]
    job = lambda tree, prefix, extra, w: dict(tree=tree, tmp=tmp, base=base, prefix=prefix, extra=extra, warm=w)
    res = {"targets": list(TARGETS), "reps": REPS, "stride": STRIDE, "processes_per_figure": REPEATS,
           "file": {"loci": N_LOCI, "barcodes_per_locus": N_UMI, "reads_per_barcode": RPB, "records": len(A["aln"])}}
    with_, without, got = [], [], None
    for _ in range(REPEATS):                                                       # (alternating)
        got = spawn(job(ROOT, "filter", scan + ["--spikeScanFilter"], warm + ["--spikeScanFilter"]))
        with_.append(got["seconds"])
        without.append(spawn(job(ROOT, "scan", scan, warm))["seconds"])
    log = got["log"]
    closing = [l for l in log.splitlines() if l.startswith("--spikeScan:") and " stage " in l][-1]
    last = [l for l in log.splitlines() if l.startswith("--spikeScanFilter:")][-1]
    a = {"with_spikeScanFilter_s": med(with_), "without_s": med(without), "with_all_s": [round(x, 3) for x in with_],
         "without_all_s": [round(x, 3) for x in without], "without_spread_s": [round(min(without), 3), round(max(without), 3)],
         "stage_s": float(re.search(r"stage ([0-9.]+) s", closing).group(1)), "closing_line": closing, "filter_line": last,
         "builds": int(re.search(r"(\d+) copies built and called", closing).group(1)),
         "scan_filter_calls": got["calls"], "words_downloaded": got["words"], "bytes_downloaded": 4 * got["words"]}
    a["flag_costs_s"] = round(a["with_spikeScanFilter_s"] - a["without_s"], 3)
    a["flag_cost_within_the_spread_without_it"] = bool(statistics.median(with_) <= max(without))
    res["flag"] = a
    if args.parent:
        parent = os.path.abspath(args.parent)
        this, theirs = [], []
        for _ in range(REPEATS):
            this.append(spawn(job(ROOT, "plain_this", scan, warm))["seconds"])
            theirs.append(spawn(job(parent, "plain_parent", scan, warm))["seconds"])
        res["plain_scan_against_parent"] = {
            "this_tree_s": med(this), "parent_s": med(theirs), "this_tree_all_s": [round(x, 3) for x in this],
            "parent_all_s": [round(x, 3) for x in theirs], "parent_spread_s": [round(min(theirs), 3), round(max(theirs), 3)],
            "this_tree_within_the_parents_spread": bool(statistics.median(this) <= max(theirs))}
    else:
        res["plain_scan_against_parent"] = "not measured: no --parent checkout given"
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
