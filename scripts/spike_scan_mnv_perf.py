"""Cost of --spikeScanMnv (dev tool, GPU box).

scripts/spike_scan_perf.py's standing fixture - a synthetic BAM of 128 loci at 20,000x (2000 barcodes x 10 reads), three targets,
R = 32, S = 16 - on one GPU; every timed run a FRESH process behind a warm-up scan of two replicates, medians of REPEATS with min .. max
and every run kept, the stage's own clock (the closing line's `stage`) beside the wall time.  Every child runs under a timeout of its own
with SMC_HOST_THREADS at most 16, and a child that fails ends the job (check=True).
  scan      --spikeScanMnv 2 under --spikeScanBuild whole and listed, and the SNV scan (whole) on the same tree; the files of the two
            MNV modes are compared byte for byte
  passes    the workflow the flag replaces: a pass as a run of its own, --spikeAF --spikeVariants pass<k>.txt --spikeReps 32 --spikePhase.
            A SUBSET of the 16 passes is timed (SUBSET of them, evenly spread) and the sum over all passes is that subset's sum SCALED by
            passes / subset - stated as such in the result; the subset's phase sensitivity lines are compared with the scan's
  detect    one batch's verdicts, device synchronised around each call: smc_scan_detect_sets (devplanes.scan_detect_sets: the joint
            words, the list and replicate 0's records come down) against smc_scan_detect plus the host's reduction of its records to
            joint verdicts (devplanes.scan_detect: every record comes down; abi.scan_joint_rule's reduction in numpy), and the bytes
            each brings down.  The batch is the full-depth rows of the file, COPIES times: what a pass calls has the same shape
  plain     the SNV scan with no new flag on this tree and on a built checkout of the parent commit given with --parent DIR,
            PLAIN_ROUNDS rounds of one fresh process per tree, the order rotated from round to round: the default path must not have
            moved - this tree's median within the parent's fastest .. slowest.  --also NAME=DIR[@LIB] adds a tree to the rounds, with
            LIB the HIP library it loads (SMC_HIP_LIB): the parent's Python files on this tree's library assign a difference to one of
            the two
A name given on the command line runs that entry alone; results are merged into an out.json that exists.

usage: spike_scan_mnv_perf.py [--parent DIR] [--also NAME=DIR[@LIB] ...] [out.json] [entry ...]      (children: --one <mode> <json> / --pass <list> <json>)"""
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

TARGETS = (0.05, 0.02, 0.01)
SEED = 1234567
REPEATS = 5
SUBSET = 2
COPIES = 6
PLAIN_ROUNDS = int(os.environ.get("SMC_PERF_PLAIN_ROUNDS", "5"))
L = 2
CHILD_TIMEOUT = 180             # seconds: a child is a warm-up and one scan of a few seconds
SHAPE = dict(n_loci=128, n_umi=2000, rpb=10, reps=32, stride=16)
MODES = {"mnv_whole": ["--spikeScanMnv=%d" % L], "mnv_listed": ["--spikeScanMnv=%d" % L, "--spikeScanBuild=listed"], "snv_whole": []}


def _cli(shape, extra):
    from smcounter_amd import cli
    base = ["--bedTarget=%s" % shape["bed"], "--mtDepth=%d" % shape["mtDepth"], "--rpb=%g" % shape["rpb_param"], "--refGenome=%s" % shape["fa"],
            "--bamFile=%s" % shape["bam"], "--dsSeed=%d" % SEED] + list(extra)
    parser = cli.build_parser()

    def run(prefix, *more):
        log = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(log):
            cli.main(parser.parse_args(base + ["--outPrefix=%s" % os.path.join(shape["tmp"], prefix)] + list(more)))
        return time.perf_counter() - t0, log.getvalue()
    return run


def one(mode, shape):
    """(child) warm-up, then one timed scan -> a JSON line."""
    text = ",".join("%g" % t for t in TARGETS)
    run = _cli(shape, ["--spikeScan=" + text, "--spikeScanStride=%d" % shape["stride"]] + MODES[mode])
    run("warm_" + mode, "--spikeScanReps=2")
    t, log = run("scan_" + mode, "--spikeScanReps=%d" % shape["reps"])
    closing = [l for l in log.splitlines() if l.startswith("--spikeScan:") and " stage " in l][-1]
    lines = re.findall(r"^--spikeScan pass \d+: (\d+) variants, (\d+) copies, (\d+) builds(?:, (\d+) of them whole)?, (\d+) verdicts", log, re.M)
    out = {"wall_s": round(t, 4), "stage_s": float(re.search(r"stage ([0-9.]+) s", closing).group(1)), "passes": len(lines),
           "member_variants": sum(int(l[0]) for l in lines), "builds": sum(int(l[2]) for l in lines),
           "whole_fallbacks": sum(int(l[3] or 0) for l in lines) if "listed" in mode else None,
           "member_verdicts_decided_by_the_host": sum(int(l[4]) for l in lines)}
    m = re.search(r"^--spikeScanMnv \d+: (\d+) sets scanned, (\d+) loci skipped, (\d+) of (\d+) joint verdicts decided by the host$", log, re.M)
    if m:
        out.update(sets=int(m.group(1)), skipped=int(m.group(2)), joint_verdicts_decided_by_the_host=int(m.group(3)), joint_verdicts=int(m.group(4)))
    print(json.dumps(out))


def one_pass(name, shape):
    """(child) a pass as a run of its own: warm-up (two replicates), then the timed run -> a JSON line."""
    text = ",".join("%g" % t for t in TARGETS)
    run = _cli(shape, ["--spikeAF=" + text, "--spikeVariants=%s" % name, "--spikePhase"])
    tag = os.path.basename(name).replace(".txt", "")
    run("warm_" + tag, "--spikeReps=2")
    t, _ = run("own_" + tag, "--spikeReps=%d" % shape["reps"])
    print(json.dumps({"wall_s": round(t, 4)}))


def _fixture():
    import ds_af_restate
    import ds_restate
    from smcounter_amd import synth
    sh = dict(SHAPE)
    tmp = tempfile.mkdtemp()
    cfg = synth.SynthConfig("SPS", sh["n_loci"], sh["n_umi"], sh["rpb"], 20170502, alt_locus_frac=0.3, alt_af=0.1)
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, sh["n_loci"])
    sh.update(tmp=tmp, bam=bam, fa=fa, bed=ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci), mtDepth=P.mtDepth, rpb_param=P.rpb,
              loci=[[c, int(p)] for c, p in loci])
    return sh


def _child(what, arg, sh, tree=None, lib=None):
    env = dict(os.environ, SMC_HOST_THREADS=str(min(16, int(os.environ.get("SMC_HOST_THREADS", "16") or 16))))
    if tree:
        env["SMC_PERF_TREE"] = tree
    if lib:
        env["SMC_HIP_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.abspath(__file__), what, arg, json.dumps(sh)], check=True, capture_output=True, text=True,
                         env=env, timeout=CHILD_TIMEOUT)
    return json.loads(out.stdout.strip().splitlines()[-1])


def _spread(runs, key):
    xs = [r[key] for r in runs]
    return {key: round(statistics.median(xs), 4), key.replace("_s", "_min_s"): min(xs), key.replace("_s", "_max_s"): max(xs),
            key.replace("_s", "_all_s"): xs}


def compare_scan(sh):
    res = {"shape": dict(SHAPE), "targets": list(TARGETS), "mnv_letters": L, "repetitions": REPEATS}
    for mode in MODES:
        runs = [_child("--one", mode, sh) for _ in range(REPEATS)]
        res[mode] = dict(runs[-1], **_spread(runs, "wall_s"), **_spread(runs, "stage_s"))
        res[mode]["ms_per_build"] = round(1e3 * res[mode]["stage_s"] / max(1, res[mode]["builds"]), 4)
    tmp = sh["tmp"]
    files = {m: {f[len("scan_" + m):]: open(os.path.join(tmp, f), "rb").read() for f in os.listdir(tmp) if f.startswith("scan_%s." % m)}
             for m in ("mnv_whole", "mnv_listed")}
    # (the .cut.vcf names its prefix: every other file byte for byte)
    res["mnv_files_equal"] = sorted(files["mnv_whole"]) == sorted(files["mnv_listed"]) and all(
        files["mnv_whole"][f] == files["mnv_listed"][f] for f in files["mnv_whole"] if not f.endswith(".vcf"))
    for m in ("mnv_whole", "mnv_listed"):
        res[m + "_over_snv_whole_stage"] = round(res[m]["stage_s"] / max(1e-9, res["snv_whole"]["stage_s"]), 2)
    return res


def compare_passes(sh):
    """A subset of the passes as --spikeReps --spikePhase runs of their own (after compare_scan: it holds their lines against the scan's)."""
    import argparse
    from smcounter_amd.tools import spike_scan_lists as lists
    tmp = sh["tmp"]
    names = lists.main(argparse.Namespace(runPath=None, bedTarget=sh["bed"], refGenome=sh["fa"], stride=sh["stride"], alt="transition", mnv=L,
                                          outPrefix=os.path.join(tmp, "lists")))
    step = max(1, len(names) // SUBSET)
    subset = names[::step][:SUBSET]
    total, per = 0.0, []
    for name in subset:
        runs = [_child("--pass", name, sh) for _ in range(REPEATS)]
        per.append(_spread(runs, "wall_s"))
        total += per[-1]["wall_s"]
    res = dict(subset=len(subset), subset_of=len(names), per_pass=per, subset_sum_s=round(total, 3),
               all_passes_scaled_s=round(total * len(names) / len(subset), 3),
               note="a subset of the passes was timed; the figure for all passes is the subset's sum scaled by passes / subset")
    page = os.path.join(tmp, "scan_mnv_whole.spikeScan.mnv.sensitivity.txt")
    if os.path.exists(page):
        mine = {(l.split("\t")[0], l.split("\t")[5]): l for l in open(page).read().splitlines()[1:]}
        same, compared = True, 0
        for name in subset:
            tag = os.path.basename(name).replace(".txt", "")
            for l in open(os.path.join(tmp, "own_%s.spikeAF.phase.sensitivity.txt" % tag)).read().splitlines()[1:]:
                same &= mine[(l.split("\t")[0], l.split("\t")[5])] == l
                compared += 1
        res.update(lines_compared=compared, scan_lines_equal_the_separate_runs=bool(same))
    return res


def compare_detect(sh):
    """One batch: smc_scan_detect_sets against smc_scan_detect plus the host's reduction, and the bytes each brings down."""
    import numpy as np
    from smcounter_amd import abi, devplanes, fasta, vc, writers
    from smcounter_amd.engine import DevBuf, Engine
    from smcounter_amd.params import VcParams
    from smcounter_amd.tools import spike_scan_lists as lists
    eng = Engine(0)
    loci = [(c, p) for c, p in sh["loci"]]
    ref = fasta.FastaFile(sh["fa"])
    P = VcParams(mtDepth=sh["mtDepth"], rpb=sh["rpb_param"])
    parts = [vc.vc_resident_rows(rb, P, eng) for _, rb in
             devplanes.iter_resident_batches(sh["bam"], ref, [(c, str(p)) for c, p in loci], P, eng, all_planes=False)]
    rows = np.concatenate(parts)
    nl = len(rows)
    mnvs, leaders, _ = lists.scan_mnvs([(c, str(p)) for c, p in loci], ref, L, "transition")
    at = {cp: n for n, cp in enumerate(loci)}
    sets = [s for s, (c, p) in zip(mnvs.sets, leaders) if p % sh["stride"] == 0]
    listed = np.zeros(L * len(sets), abi.SCAN_LOCUS_DTYPE)
    for g, k in enumerate(k for s in sets for k in s.members):
        listed[g] = (at[(mnvs[k].chrom, mnvs[k].pos)], devplanes.SCAN_ALT_ID[mnvs[k].alt])
    set_off = np.arange(0, len(listed) + 1, L, dtype=np.uint32)
    batch = np.tile(rows, COPIES)
    d_rows = DevBuf(eng, batch.nbytes + 256).upload(batch.view(np.uint8).reshape(-1))
    thr = writers.pi_threshold(P.mtDepth, 0)
    sync = lambda: eng.L.smc_device_sync(eng.ctx)

    def with_sets():
        return devplanes.scan_detect_sets(eng, d_rows, COPIES, nl, listed, set_off, thr, records_of=[0])

    def with_members():
        rec, todo = devplanes.scan_detect(eng, d_rows, COPIES, nl, listed, thr)
        return abi.scan_joint_rule(rec["mt_verdict"] >> 30, set_off) + (rec,)

    def median_ms(fn):
        fn(); sync()
        times = []
        for _ in range(25):
            t0 = time.perf_counter()
            fn(); sync()
            times.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4)}
    words, todo, rec0 = with_sets()
    want_words, want_todo, rec = with_members()
    G, S = len(listed), len(sets)
    out = {"copies": COPIES, "loci_per_copy": nl, "listed_records": G, "sets": S,
           "equal": bool(np.array_equal(words, want_words) and np.array_equal(todo, want_todo) and rec0[0].tobytes() == rec[0].tobytes()),
           "joint_verdicts_for_the_host": int(((words >> 30) == abi.SCAN_HOST).sum()),
           "scan_detect_sets": dict(median_ms(with_sets), bytes_down=4 + 4 * COPIES * S + 4 * len(todo) + 16 * G),
           "scan_detect_and_host_reduction": dict(median_ms(with_members), bytes_down=4 + 16 * COPIES * G + 4 * len(want_todo))}
    d_rows.free()
    eng.close()
    return out


def compare_plain(sh, parent, also=()):
    trees = [("parent", parent, None), ("this", ROOT, None)] + list(also)
    runs = {who: [] for who, _, _ in trees}
    for i in range(PLAIN_ROUNDS):
        k = i % len(trees)
        for who, tree, lib in trees[k:] + trees[:k]:
            runs[who].append(_child("--one", "snv_whole", sh, tree, lib))
    res = {who: dict(_spread(runs[who], "stage_s"), **_spread(runs[who], "wall_s")) for who in runs}
    lo, hi = res["parent"]["stage_min_s"], res["parent"]["stage_max_s"]
    res["rounds"] = PLAIN_ROUNDS
    res["this_median_within_parent_spread"] = bool(lo <= res["this"]["stage_s"] <= hi)
    for who in [w for w in runs if w != "parent"]:
        d = [x - y for x, y in zip(res[who]["stage_all_s"], res["parent"]["stage_all_s"])]
        res[who + "_minus_parent_paired_s"] = dict(median=round(statistics.median(d), 4), all=[round(x, 4) for x in d])
    return res


def main():
    a = sys.argv[1:]
    if a and a[0] == "--one":
        return one(a[1], json.loads(a[2]))
    if a and a[0] == "--pass":
        return one_pass(a[1], json.loads(a[2]))
    parent, also = None, []
    while a and a[0] in ("--parent", "--also"):
        if a[0] == "--parent":
            parent = os.path.abspath(a[1])
        else:
            name, where = a[1].split("=", 1)
            tree, _, lib = where.partition("@")
            also.append((name, os.path.abspath(tree), os.path.abspath(lib) if lib else None))
        a = a[2:]
    names = a[1:] or ["scan", "passes", "detect"] + (["plain"] if parent else [])
    res = {}
    if a and os.path.exists(a[0]):
        with open(a[0]) as fh:
            res = json.load(fh)
    sh = _fixture()
    for n in names:
        res[n] = compare_scan(sh) if n == "scan" else compare_passes(sh) if n == "passes" else compare_detect(sh) if n == "detect" else \
            compare_plain(sh, parent, also)
        print("%s done" % n, file=sys.stderr, flush=True)
    line = json.dumps(res, indent=1)
    print(line)
    if a:
        with open(a[0], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
