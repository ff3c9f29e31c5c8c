"""Cost of --spikeScanBuild listed against whole (dev tool, GPU box).

Three comparisons, each the scan run `whole` and `listed` on the same synthetic BAM, every timed run in a FRESH process (a warm-up scan
of two replicates first, then the timed run), medians of REPEATS with every run's time kept:
  deep      scripts/spike_scan_perf.py's standing fixture: 128 loci, 2000 barcodes x 10 reads (20,000x), three targets, R = 32, S = 16
  panel     a 512-position run at 3000x (300 barcodes x 10 reads), S = 256 - the default stride: two listed loci per pass -, R = 4
  depth     the deep fixture with --spikeScanDepth 0.5,0.25
Per mode: the wall time, the stage's own clock, builds, copies per pass line, whole fallbacks.  `listed` is "faster" where its median
lies below the fastest `whole` run.  The files of both modes are compared byte for byte once per comparison.
Two more entries:
  batch     the builds alone, on the deep fixture: inside one scan per mode every call of devplanes._build_copies (whole: B whole
            builds, one behind the other) or devplanes._build_listed (ONE smc_build_listed call for B copies) is clocked - both end in
            synchronous downloads -, and the library entries called and the downloads made inside it are counted
  launches  the builders' kernel launches of such a scan (4 replicates), counted from a rocprofv3 --kernel-trace run of its own per
            mode: the whole builder's k_bp_* dispatches per build, the listed builder's k_bl_* per call (named explicitly: not in the default set)
  plain     the scan with NO --spikeScanBuild on the deep fixture, on this tree and on a built checkout of the parent commit given
            with --parent DIR (and on further trees, --also NAME=DIR), 12 rounds of one process per tree with the order rotated: the
            default path must not have moved - this tree's median within the parent's fastest .. slowest, and the differences paired by round
A name given on the command line runs that entry alone; results are merged into an out.json that exists.

usage: spike_scan_build_perf.py [--parent DIR] [--also NAME=DIR ...] [out.json] [entry ...]      (children: --one / --batch <mode> <json of the shape>)"""
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
sys.path.insert(0, os.environ.get("SMC_PERF_TREE") or ROOT)        # (a child of `plain` imports the package of the tree it measures)
sys.path.insert(1, os.path.join(ROOT, "tests"))
PASS = re.compile(r"^--spikeScan pass \d+: (\d+) variants, (\d+) copies, (\d+) builds(?:, (\d+) of them whole)?,", re.M)

TARGETS = (0.05, 0.02, 0.01)
SEED = 1234567
REPEATS = 5
SHAPES = {"deep": dict(n_loci=128, n_umi=2000, rpb=10, reps=32, stride=16, extra=[]),
          "panel": dict(n_loci=512, n_umi=300, rpb=10, reps=4, stride=256, extra=[]),
          "depth": dict(n_loci=128, n_umi=2000, rpb=10, reps=32, stride=16, extra=["--spikeScanDepth=0.5,0.25"])}


def _scan(mode, shape):
    from smcounter_amd import cli
    base = ["--bedTarget=%s" % shape["bed"], "--mtDepth=%d" % shape["mtDepth"], "--rpb=%g" % shape["rpb_param"], "--refGenome=%s" % shape["fa"],
            "--bamFile=%s" % shape["bam"], "--dsSeed=%d" % SEED, "--spikeScan=" + ",".join("%g" % t for t in TARGETS),
            "--spikeScanStride=%d" % shape["stride"]] + list(shape["extra"]) + ([] if mode == "whole" else ["--spikeScanBuild=" + mode])
    parser = cli.build_parser()

    def run(prefix, reps):
        log = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(log):
            cli.main(parser.parse_args(base + ["--outPrefix=%s" % os.path.join(shape["tmp"], prefix), "--spikeScanReps=%d" % reps]))
        return time.perf_counter() - t0, log.getvalue()
    return run


def one(mode, shape):
    """(child) warm-up, then one timed scan -> a JSON line."""
    run = _scan(mode, shape)
    run("warm_" + mode, 2)
    t, log = run("scan_" + mode, shape["reps"])
    lines = PASS.findall(log)
    closing = [l for l in log.splitlines() if l.startswith("--spikeScan:") and " stage " in l][-1]
    print(json.dumps({"wall_s": round(t, 4), "stage_s": float(re.search(r"stage ([0-9.]+) s", closing).group(1)), "passes": len(lines),
                      "builds": sum(int(l[2]) for l in lines), "copies": sum(int(l[1]) for l in lines),
                      "whole_fallbacks": sum(int(l[3] or 0) for l in lines) if mode != "whole" else None}))


def batch(mode, shape):
    """(child) warm-up, then one scan in which the batch builder of `mode` is clocked and its entry calls and downloads counted."""
    from smcounter_amd import devplanes, engine
    n = dict(batches=0, copies=0, seconds=0.0, downloads=0, entries={})
    inside = [False]

    def counted(cls, name):
        f = getattr(cls, name)

        def g(*a, **k):
            if inside[0]:
                n["downloads"] += 1
            return f(*a, **k)
        setattr(cls, name, g)
    for cls in (engine.DevBuf, devplanes._BufView):
        if "download" in vars(cls):
            counted(cls, "download")

    class Lib(object):                          # the library's entries, those called inside a batch build counted by name
        def __init__(self, L):
            self._L = L

        def __getattr__(self, name):
            f = getattr(self._L, name)
            if not name.startswith("smc_") or name.startswith("smc_mem_"):
                return f

            def g(*a):
                if inside[0]:
                    n["entries"][name] = n["entries"].get(name, 0) + 1
                return f(*a)
            return g
    make = engine.Engine.__init__

    def init(self, *a, **k):
        make(self, *a, **k)
        self.L = Lib(self.L)
    engine.Engine.__init__ = init
    fname = "_build_copies" if mode == "whole" else "_build_listed"
    f = getattr(devplanes, fname)

    def clocked(eng, run, *a, **k):
        copies = a[0] if mode == "whole" else len(a[0])
        inside[0] = True
        t0 = time.perf_counter()
        try:
            return f(eng, run, *a, **k)
        finally:
            n["seconds"] += time.perf_counter() - t0
            inside[0] = False
            n["batches"] += 1
            n["copies"] += copies
    setattr(devplanes, fname, clocked)
    run = _scan(mode, shape)
    run("warm_" + mode, 2)
    warm = (n["batches"], n["copies"])
    n.update(batches=0, copies=0, seconds=0.0, downloads=0, entries={})
    run("scan_" + mode, shape["reps"])
    B = n["copies"] / max(1, n["batches"])
    print(json.dumps({"batches": n["batches"], "copies_per_batch": round(B, 2), "ms_per_batch": round(1e3 * n["seconds"] / max(1, n["batches"]), 4),
                      "ms_per_copy": round(1e3 * n["seconds"] / max(1, n["copies"]), 4), "downloads_per_batch": round(n["downloads"] / max(1, n["batches"]), 2),
                      "entry_calls_per_batch": {k: round(v / max(1, n["batches"]), 2) for k, v in sorted(n["entries"].items())},
                      "process_batches": warm[0] + n["batches"], "process_copies": warm[1] + n["copies"]}))


def _fixture(name):
    import ds_af_restate
    import ds_restate
    from smcounter_amd import synth
    sh = dict(SHAPES[name])
    tmp = tempfile.mkdtemp()
    cfg = synth.SynthConfig("SPB", sh["n_loci"], sh["n_umi"], sh["rpb"], 20170502, alt_locus_frac=0.3, alt_af=0.1)
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, sh["n_loci"])
    sh.update(tmp=tmp, bam=bam, fa=fa, bed=ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci), mtDepth=P.mtDepth, rpb_param=P.rpb)
    return sh


def _child(what, mode, sh, tree=None):
    env = dict(os.environ, SMC_PERF_TREE=tree) if tree else None
    out = subprocess.run([sys.executable, os.path.abspath(__file__), what, mode, json.dumps(sh)], check=True, capture_output=True, text=True, env=env)
    return json.loads(out.stdout.strip().splitlines()[-1])


def compare_batch():
    sh = _fixture("deep")
    runs = {m: [_child("--batch", m, sh) for _ in range(REPEATS)] for m in ("whole", "listed")}
    res = {m: dict(runs[m][-1], ms_per_batch_all=[r["ms_per_batch"] for r in runs[m]], ms_per_copy_all=[r["ms_per_copy"] for r in runs[m]],
                   ms_per_batch=statistics.median(r["ms_per_batch"] for r in runs[m]), ms_per_copy=statistics.median(r["ms_per_copy"] for r in runs[m]))
           for m in runs}
    res["whole_over_listed_per_copy"] = round(res["whole"]["ms_per_copy"] / max(1e-9, res["listed"]["ms_per_copy"]), 2)
    return res


def compare_launches():
    """The builders' kernel launches, counted: per mode ONE process of the `batch` child (a short scan: 4 replicates) under
    rocprofv3 --kernel-trace, a run of its own - nothing here is timed -; of the trace's dispatches those of the whole builder's
    kernels (k_bp_*) over the whole builds of the process, and those of the listed builder's (k_bl_*) over its calls."""
    import csv
    import glob
    sh = dict(_fixture("deep"), reps=4)
    res = {}
    for mode, prefix in (("whole", "k_bp_"), ("listed", "k_bl_")):
        out = tempfile.mkdtemp()
        got = subprocess.run(["rocprofv3", "--kernel-trace", "-f", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--batch", mode,
                              json.dumps(sh)], check=True, capture_output=True, text=True)
        child = json.loads([l for l in got.stdout.splitlines() if l.startswith('{"batches"')][-1])
        names = {}
        for f in glob.glob(out + "/**/*kernel_trace.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                k = re.search(r"k_[a-z0-9_]+", r["Kernel_Name"])
                if k and k.group(0).startswith(prefix):
                    names[k.group(0)] = names.get(k.group(0), 0) + 1
        total = sum(names.values())
        res[mode] = dict(builder_launches=total, by_kernel=dict(sorted(names.items())), batches=child["process_batches"], copies=child["process_copies"],
                         launches_per_batch=round(total / max(1, child["process_batches"]), 2), launches_per_copy=round(total / max(1, child["process_copies"]), 3))
    return res


PLAIN_ROUNDS = 12


def compare_plain(parent, also=()):
    """The no-flag scan on the parent's tree and on this one - and on every tree of `also` ((name, dir): e.g. the parent's Python
    files with this tree's library, which assigns a difference to one of the two) - PLAIN_ROUNDS rounds of one fresh process per
    tree, the order within a round rotated from round to round: a drift of the machine over the minutes this takes meets all alike."""
    sh = _fixture("deep")
    trees = [("parent", parent), ("this", ROOT)] + list(also)
    runs = {who: [] for who, _ in trees}
    for i in range(PLAIN_ROUNDS):
        k = i % len(trees)
        for who, tree in trees[k:] + trees[:k]:
            runs[who].append(_child("--one", "whole", sh, tree))
    res = {who: dict(stage_all_s=[r["stage_s"] for r in runs[who]], stage_s=round(statistics.median(r["stage_s"] for r in runs[who]), 4),
                     stage_mean_s=round(statistics.mean(r["stage_s"] for r in runs[who]), 4), wall_s=round(statistics.median(r["wall_s"] for r in runs[who]), 4))
           for who in runs}
    lo, hi = min(res["parent"]["stage_all_s"]), max(res["parent"]["stage_all_s"])
    for who in runs:
        if who != "parent":
            res[who]["median_within_parent_spread"] = lo <= res[who]["stage_s"] <= hi
            # (paired by round: the same minute of the machine)
            d = [x - y for x, y in zip(res[who]["stage_all_s"], res["parent"]["stage_all_s"])]
            res[who]["paired_minus_parent_s"] = dict(median=round(statistics.median(d), 4), mean=round(statistics.mean(d), 4),
                                                     sem=round(statistics.stdev(d) / len(d) ** 0.5, 4), slower_in=sum(x > 0 for x in d), rounds=len(d))
    res["this_median_within_parent_spread"] = res["this"]["median_within_parent_spread"]
    return res


def compare(name):
    sh = _fixture(name)
    tmp = sh["tmp"]
    res = {"shape": {k: SHAPES[name][k] for k in ("n_loci", "n_umi", "rpb", "reps", "stride", "extra")}, "targets": list(TARGETS)}
    for mode in ("whole", "listed"):
        runs = []
        for _ in range(REPEATS):
            runs.append(_child("--one", mode, sh))
        res[mode] = dict(runs[-1], wall_all_s=[r["wall_s"] for r in runs], stage_all_s=[r["stage_s"] for r in runs],
                         wall_s=round(statistics.median(r["wall_s"] for r in runs), 4), stage_s=round(statistics.median(r["stage_s"] for r in runs), 4))
        res[mode]["ms_per_build"] = round(1e3 * res[mode]["stage_s"] / max(1, res[mode]["builds"]), 4)
    files = {m: {f[len("scan_" + m):]: open(os.path.join(tmp, f), "rb").read() for f in os.listdir(tmp) if f.startswith("scan_%s." % m)}
             for m in ("whole", "listed")}
    # (the .cut.vcf names its prefix: every other file byte for byte)
    res["files_equal"] = sorted(files["whole"]) == sorted(files["listed"]) and all(
        files["whole"][f] == files["listed"][f] for f in files["whole"] if not f.endswith(".vcf"))
    res["listed_median_below_fastest_whole"] = res["listed"]["stage_s"] < min(res["whole"]["stage_all_s"])
    res["whole_over_listed_stage"] = round(res["whole"]["stage_s"] / max(1e-9, res["listed"]["stage_s"]), 2)
    return res


def main():
    a = sys.argv[1:]
    if a and a[0] in ("--one", "--batch"):
        return (one if a[0] == "--one" else batch)(a[1], json.loads(a[2]))
    parent, also = None, []
    while a and a[0] in ("--parent", "--also"):
        if a[0] == "--parent":
            parent = os.path.abspath(a[1])
        else:
            also.append((a[1].split("=", 1)[0], os.path.abspath(a[1].split("=", 1)[1])))
        a = a[2:]
    names = a[1:] or list(SHAPES) + ["batch"] + (["plain"] if parent else [])
    res = {}
    if a and os.path.exists(a[0]):
        with open(a[0]) as fh:
            res = json.load(fh)
    for n in names:
        res[n] = compare_batch() if n == "batch" else compare_launches() if n == "launches" else compare_plain(parent, also) if n == "plain" else compare(n)
        print("%s done" % n, file=sys.stderr, flush=True)
    line = json.dumps(res, indent=1)
    print(line)
    if a:
        with open(a[0], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
