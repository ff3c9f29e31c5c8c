"""Cost of --spikeGrid (dev tool, GPU box).

On scripts/spike_rpb_perf.py's standing input (a synthetic BAM of 128 loci, 2000 barcodes x 10 reads per locus, four listed SNVs), with
two targets, the fractions 1 and 0.5, the reads-per-barcode targets 4 and 2 and R = 32 replicates.  Every timed command-line run is a
FRESH PROCESS (this script again, in --child mode): the child makes one warm-up run (R = 2) and then times the run asked for, so the
figure is the run's wall time in a process whose GPU runtime is up.  Medians of `REPEATS` children, the variants alternating:
(a) a run with --spikeGrid, --spikeDepth, --spikeRpb and --spikeReps R against the same run without the three flags, and from the
    difference the time per cell and replicate;
(b) in one child, device synchronised around each: one smc_spike_grid_counts call over all (variant, replicate, target, fraction, r),
    beside one smc_spike_rpb_counts call of the same records at F = 1; one ReadGroups.counts_frac_seeds call beside the R counts_frac
    calls it replaces;
(c) the two-step workflow the switch replaces, for the (target, replicate) pairs of `OFFLINE` - tools.spike_variants --af t --seed s,
    then the command line with --dsMT .. --dsRpb .. --dsGrid and both philox samplers on its output - timed ONCE each and scaled to the
    T x R pairs of (a): a stated subset.  The cells' files of (a) are compared with the workflow's for seed s_0;
(d) the plain --spikeRpb 4,2 --spikeReps R run on this tree and, with --parent DIR (a checkout of the parent commit, built), on the
    parent's: this tree's median has to lie inside the parent's own min .. max spread.

usage: spike_grid_perf.py [--parent DIR] [out.json]   -> one JSON line (also written to out.json, default
profiles/spike_grid_perf.json)"""
import argparse
import contextlib
import io
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (--child: the tree whose package and tests are imported - this one, or the parent commit's)
ROOT = sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else HERE
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

TARGETS = (0.05, 0.01)
FRACS = (1, 0.5)
RPBS = (4, 2)
REPS = 32
SEED = 1234567
REPEATS = 5
CHILD_TIMEOUT_S = 120                           # a child takes a few seconds
OFFLINE = ((0.05, 0), (0.01, 0), (0.01, 1))      # (target, replicate) pairs the two-step workflow is timed on
SUFFIXES = (".smCounter.all.txt", ".smCounter.cut.txt", ".smCounter.cut.vcf")
N_LOCI, N_UMI, RPB = 128, 2000, 10
text = lambda xs: ",".join("%g" % x for x in xs)


def fixture(tmp):
    import ds_af_restate
    import ds_restate
    import spike_restate
    from smcounter_amd import synth
    cfg = synth.SynthConfig("SPP", N_LOCI, N_UMI, RPB, 20170502, alt_locus_frac=0.3, alt_af=0.1)
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, N_LOCI)
    bed = ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci)
    variants = spike_restate.pick_positions(bam, fa, loci[N_LOCI // 2:N_LOCI // 2 + 24], 4)
    vfile = ds_af_restate.write_variants(os.path.join(tmp, "v.txt"), variants)
    with open(os.path.join(tmp, "fixture.json"), "w") as fh:
        json.dump(dict(bam=bam, fa=fa, bed=bed, vfile=vfile, mtDepth=P.mtDepth, rpb=P.rpb, records=len(A["aln"]),
                       variants=["%s:%d %s>%s" % (v.chrom, v.pos, v.ref, v.alt) for v in variants]), fh)


def cli_run(fx, tmp, prefix, extra, src=None, spike=True):
    """One command-line run in this process -> (seconds, its log)."""
    from smcounter_amd import cli
    base = ["--bedTarget=%s" % fx["bed"], "--mtDepth=%d" % fx["mtDepth"], "--rpb=%g" % fx["rpb"], "--refGenome=%s" % fx["fa"]]
    if spike:
        base += ["--spikeAF=" + text(TARGETS), "--spikeVariants=%s" % fx["vfile"]]
    log = io.StringIO()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(log):
        cli.main(cli.build_parser().parse_args(base + ["--bamFile=%s" % (src or fx["bam"]), "--outPrefix=%s" % os.path.join(tmp, prefix)] + list(extra)))
    return time.perf_counter() - t0, log.getvalue()


def child_wall(tmp, prefix, extra):
    fx = json.load(open(os.path.join(tmp, "fixture.json")))
    warm = [re.sub(r"^--spikeReps=\d+$", "--spikeReps=2", x) for x in extra]
    cli_run(fx, tmp, "warm." + prefix, warm)
    t, log = cli_run(fx, tmp, prefix, extra)
    m = re.search(r"--spikeReps: replicate stage ([0-9.]+) s", log)
    print(json.dumps({"s": t, "stage": float(m.group(1)) if m else None}))


def child_offline(tmp, t, j):
    """The two-step workflow for target t and replicate j, timed once, behind a plain run that brings the GPU runtime up (as the
    children of (a) have it up when their clock starts)."""
    from smcounter_amd import bamio, dsaf
    from smcounter_amd.tools import spike_variants as sv
    fx = json.load(open(os.path.join(tmp, "fixture.json")))
    cli_run(fx, tmp, "warm.off_%g_%d" % (t, j), [], spike=False)
    seed = dsaf.rep_seeds(SEED, REPS)[j]
    out = os.path.join(tmp, "off_%g_%d.bam" % (t, j))
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        sv.main(argparse.Namespace(runPath=None, inBam=fx["bam"], outBam=out, variants=fx["vfile"], af="%g" % t, seed=seed, refGenome=fx["fa"]))
        if not os.path.exists(out + ".bai"):
            bamio.write_bai(out)
    t_tool = time.perf_counter() - t0
    prefix = "off.spikeAF%g.s%d" % (t, j)
    t_run, _ = cli_run(fx, tmp, prefix, ["--dsMT=" + text(FRACS), "--dsRpb=" + text(RPBS), "--dsGrid", "--dsSampler=philox", "--dsRpbSampler=philox",
                                         "--dsSeed=%d" % seed], src=out, spike=False)
    os.remove(out)
    print(json.dumps({"s": t_tool + t_run, "prefix": prefix}))


def child_kernels(tmp):
    import numpy as np
    from smcounter_amd import devplanes, dsaf, fasta
    from smcounter_amd.engine import Engine
    from smcounter_amd.tools import spike_variants as sv
    fx = json.load(open(os.path.join(tmp, "fixture.json")))
    P = fixture_params()
    eng = Engine(0)
    variants = sv.parse_variants(fx["vfile"], "v.txt")
    keep = {}
    rpb = dict(targets=list(RPBS), fracs=list(FRACS), reps=REPS, flag="--spikeGrid", params=[P] * (len(TARGETS) * len(FRACS) * len(RPBS)))
    devplanes.spike_rules(fx["bam"], fasta.FastaFile(fx["fa"]), variants, list(TARGETS), [P] * len(TARGETS), SEED, eng, keep=keep, rpb=rpb)
    sync = lambda: eng.L.smc_device_sync(eng.ctx)
    pos, seeds, thr = [v.pos for v in variants], dsaf.rep_seeds(SEED, REPS), [sv.threshold(t) for t in TARGETS]
    bthr = [devplanes.frac_threshold(f) for f in FRACS]
    groups = rpb["rules"][0].groups

    def median_ms(fn):
        fn(); sync()                                              # (warm-up)
        times = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            fn(); sync()
            times.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(times), 4)
    full = [int(x) for x in rpb["rep_thr"][0, 0]]
    out = {"covering_barcodes": int(sum(len(c) for c in keep["covers"])), "covering_records": int(sum(len(r[1]) for r in keep["records"])),
           "cells_counted": len(variants) * REPS * len(TARGETS) * len(FRACS) * len(RPBS),
           "grid_counts_call_ms": median_ms(lambda: devplanes.spike_grid_counts(eng, pos, keep["covers"], keep["records"], seeds, thr, bthr, rpb["rep_thr"])),
           "rpb_counts_call_ms": median_ms(lambda: devplanes.spike_rpb_counts(eng, pos, keep["covers"], keep["records"], seeds, thr, full)),
           "counts_frac_seeds_call_ms": median_ms(lambda: groups.counts_frac_seeds(seeds, bthr)),
           "counts_frac_R_calls_ms": median_ms(lambda: [groups.counts_frac(s, bthr) for s in seeds]),
           "thresholds_differ_per_replicate": bool(len({rpb["rep_thr"][j].tobytes() for j in range(REPS)}) > 1)}
    assert np.array_equal(groups.counts_frac_seeds(seeds[:3], bthr)[:, :, 1].astype(np.int64),
                          np.array([[c["one"] for c in groups.counts_frac(s, bthr)] for s in seeds[:3]], np.int64))
    devplanes.free_af_runs(keep["runs"])
    devplanes.close_rules(rpb["rules"])
    eng.close()
    print(json.dumps(out))


def fixture_params():
    """The fixture's VcParams: the synthetic BAM's own (synth.params_for, what ds_af_restate.synth_bam calls it with)."""
    from smcounter_amd import synth
    return synth.params_for(synth.SynthConfig("SPP", N_LOCI, N_UMI, RPB, 20170502, alt_locus_frac=0.3, alt_af=0.1))


def spawn(tmp, root, *args):
    """A child of this script on the tree `root` -> its last output line, parsed."""
    # (every child has a limit of its own: one that hangs ends the script, it does not hang it)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", tmp, "--root", root] + [str(a) for a in args],
                         check=True, capture_output=True, text=True, cwd=root, timeout=CHILD_TIMEOUT_S).stdout
    return json.loads(out.strip().splitlines()[-1])


def main():
    a = [x for x in sys.argv[1:]]
    parent = None
    if "--parent" in a:
        parent = os.path.abspath(a[a.index("--parent") + 1])
        del a[a.index("--parent"):a.index("--parent") + 2]
    out_json = a[0] if a else os.path.join(HERE, "profiles", "spike_grid_perf.json")
    tmp = tempfile.mkdtemp()
    try:
        measure(tmp, parent, out_json)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def measure(tmp, parent, out_json):
    t0 = time.perf_counter()
    fixture(tmp)
    fx = json.load(open(os.path.join(tmp, "fixture.json")))
    res = {"targets": list(TARGETS), "fractions": list(FRACS), "rpb_targets": list(RPBS), "reps": REPS, "repetitions": REPEATS,
           "file": {"loci": N_LOCI, "barcodes_per_locus": N_UMI, "reads_per_barcode": RPB, "records": fx["records"], "variants": fx["variants"],
                    "make_s": round(time.perf_counter() - t0, 1)}}
    seed, reps = "--dsSeed=%d" % SEED, "--spikeReps=%d" % REPS
    grid = [seed, reps, "--spikeGrid", "--spikeDepth=" + text(FRACS), "--spikeRpb=" + text(RPBS)]
    with_, without, st_with, st_without = [], [], [], []
    for _ in range(REPEATS):
        r = spawn(tmp, HERE, "wall", "cells", *grid)
        with_.append(r["s"]); st_with.append(r["stage"])
        r = spawn(tmp, HERE, "wall", "plain", seed, reps)
        without.append(r["s"]); st_without.append(r["stage"])
    t_with, t_without = statistics.median(with_), statistics.median(without)
    n_cells = len(TARGETS) * len(FRACS) * len(RPBS)
    res["wall"] = {"with_spikeGrid_s": round(t_with, 3), "without_the_three_flags_s": round(t_without, 3),
                   "with_spikeGrid_all_s": [round(x, 3) for x in with_], "without_all_s": [round(x, 3) for x in without],
                   "switch_costs_s": round(t_with - t_without, 3), "replicate_stage_with_s": statistics.median(st_with),
                   "replicate_stage_without_s": statistics.median(st_without), "cells": n_cells,
                   "ms_per_cell_and_replicate": round(1e3 * (t_with - t_without) / (REPS * n_cells), 3)}
    res["kernels"] = spawn(tmp, HERE, "kernels")
    # (c) the two-step workflow on a stated subset of (target, replicate) pairs, scaled to all T x R
    total, same, compared = [], True, 0
    for t, j in OFFLINE:
        r = spawn(tmp, HERE, "offline", t, j)
        total.append(round(r["s"], 3))
        if j == 0:
            for f in FRACS:
                for q in RPBS:
                    mine = os.path.join(tmp, "cells.spikeAF%g.dsMT%g.dsRpb%g" % (t, f, q))
                    theirs = os.path.join(tmp, r["prefix"] + ".dsMT%g.dsRpb%g" % (f, q))
                    for s in SUFFIXES:
                        same &= open(mine + s, "rb").read() == open(theirs + s, "rb").read().replace(theirs.encode(), mine.encode())
                        compared += 1
    pairs = REPS * len(TARGETS)
    res["two_step"] = {"subset_of_pairs": [list(p) for p in OFFLINE], "pair_s": total, "timed": "once each, a subset scaled to all pairs",
                       "scaled_to_all_pairs_s": round(statistics.mean(total) * pairs, 1), "pairs": pairs,
                       "scaled_over_switch_cost": round(statistics.mean(total) * pairs / max(1e-9, t_with - t_without), 1),
                       "files_compared": compared, "cells_equal_the_two_step_workflow": bool(same)}
    # (d) the plain --spikeRpb run, this tree against the parent commit's
    rpb = [seed, reps, "--spikeRpb=" + text(RPBS)]
    mine, theirs = [], []
    for _ in range(REPEATS):
        mine.append(spawn(tmp, HERE, "wall", "rpb_here", *rpb)["s"])
        if parent:
            theirs.append(spawn(tmp, parent, "wall", "rpb_parent", *rpb)["s"])
    res["spikeRpb_run"] = {"this_tree_s": round(statistics.median(mine), 3), "this_tree_all_s": [round(x, 3) for x in mine]}
    if parent:
        res["spikeRpb_run"].update(parent_s=round(statistics.median(theirs), 3), parent_all_s=[round(x, 3) for x in theirs],
                                   inside_the_parents_spread=bool(min(theirs) <= statistics.median(mine) <= max(theirs)))
    line = json.dumps(res)
    print(line)
    with open(out_json, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    if "--child" in sys.argv:
        k = sys.argv.index("--child")
        tmp, rest = sys.argv[k + 1], sys.argv[k + 4:]           # (--child TMP --root ROOT what ...)
        if rest[0] == "wall":
            child_wall(tmp, rest[1], rest[2:])
        elif rest[0] == "offline":
            child_offline(tmp, float(rest[1]), int(rest[2]))
        else:
            child_kernels(tmp)
    else:
        main()
