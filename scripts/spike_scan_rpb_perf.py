"""Cost of --spikeScanRpb and of smc_select_alignments_reads_copies (dev tool, GPU box) -> profiles/spike_scan_rpb_perf.json.

On scripts/spike_scan_perf.py's input (a synthetic BAM, 128 loci x 2000 barcodes x 10 reads, three targets, R = 32, S = 16) with the
reads-per-barcode targets 4 and 2.  Every timed run is made in a FRESH process (this one starts them one at a time and never opens the
GPU itself); a process makes a warm-up run first (R = 2), then the timed one; a figure is the median of `REPEATS` processes:
(a) the run with --spikeScanRpb against the same --spikeScan run without it; the stage's clock, the builds, the selection calls and the
    host-decided verdicts from the log;
(b) one devplanes.select_copies_reads call of 8 copies x 2 masks against the 16 devplanes.select_run(level="read") calls it replaces
    (160 launches, 16 downloads), on the file's run spiked 8 times with the masks of 8 seeds; per process the median of `INNER`
    repetitions of each, alternating, the device synchronised around each; the selections compared byte for byte;
(c) the workflow the flag replaces: every pass as a run of its own, --spikeAF --spikeVariants pass<k>.txt --spikeReps R --spikeRpb
    <r...>.  A SUBSET of the passes is timed (`SUBSET` of them, evenly spread), and the sum over all passes is that subset's sum scaled
    by passes / subset - stated as such in the result; the subset's rpb sensitivity lines are compared with the scan's;
(d) the plain --spikeScan run and the --spikeScanDepth run on this tree against a built checkout of the parent commit (`--parent DIR`;
    left out without it), alternating: the parent's runs give the run-to-run spread this tree's medians are held against.
No ratio is fixed in advance; the JSON says whether the batched call was faster and whether the two scans stayed within the spread.
`--parts abcd` makes a subset of the measurements (the others keep what the JSON file already holds).

usage: spike_scan_rpb_perf.py [--parent DIR] [--parts abcd] [--out profiles/spike_scan_rpb_perf.json]"""
import argparse
import contextlib
import dataclasses
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
FRACS = (0.5, 0.25)            # (measurement (d): the --spikeScanDepth run)
RPBS = (4, 2)
SEED = 1234567
REPEATS = 5
SUBSET = 4
INNER = 10
COPIES = 8
N_LOCI, N_UMI, RPB, REPS, STRIDE = 128, 2000, 10, 32, 16


def _use(tree):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "tests"))


def child_cli(job):
    """One warm-up run and one timed run of the command line in the tree job["tree"] -> dict(seconds, log)."""
    _use(job["tree"])
    from smcounter_amd import cli
    parser = cli.build_parser()

    def run(prefix, extra):
        log = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(log):
            cli.main(parser.parse_args(job["base"] + ["--outPrefix=%s" % os.path.join(job["tmp"], prefix)] + extra))
        return time.perf_counter() - t0, log.getvalue()
    run(job["prefix"] + ".warm", job["warm"])
    t, log = run(job["prefix"], job["extra"])
    return {"seconds": t, "log": log}


def child_select(job):
    """(b) in one process: the run of the file uploaded, COPIES spiked copies of it (threshold 2^31: about half of the covering barcodes
    rewritten), the keep masks of COPIES seeds x the reads-per-barcode targets, then select_copies_reads against the select_run calls."""
    _use(job["tree"])
    import numpy as np
    from smcounter_amd import bamio, devplanes, dsaf, fasta
    from smcounter_amd.engine import Engine
    from smcounter_amd.params import VcParams
    from smcounter_amd.tools import spike_scan_lists as lists
    eng = Engine(0)
    P = VcParams(**job["params"])
    ref = fasta.FastaFile(job["fa"])
    loci = [(c, str(p)) for c, p in job["loci"]]
    variants, _ = lists.scan_variants(loci, ref, "transition")
    mine = [v for v in variants if v.pos % STRIDE == 0]
    run = devplanes.AfRun(mine[0].chrom, int(job["loci"][0][1]) - 1, int(job["loci"][-1][1]), [], 0)
    run.load(job["bam"], ref, eng, P, 128_000_000, bamio.host_threads(), mism=True)
    spikes = devplanes.SpikeSet(mine)
    svar, _ = spikes.chrom_variants(run.chrom, 0.5)
    seeds = dsaf.rep_seeds(SEED, COPIES)
    copies = devplanes._SpikedCopies(eng, run, svar, seeds, 1 << 31, P)
    M = len(RPBS)
    rules = devplanes.philox_read_rules(job["bam"], list(RPBS), [P] * M, SEED, eng, flag="--spikeScanRpb")
    masks = devplanes._scan_read_masks(eng, run, rules, seeds)
    d_masks, nw = masks["masks"].data_ptr(), masks["n_words"]
    sync = lambda: eng.L.smc_device_sync(eng.ctx)

    def batched():
        return devplanes.select_copies_reads(eng, copies.runs, run.A, run.lo, d_masks, nw, nw * M, M)

    def singles():
        return [[devplanes.select_run(eng, up, run.A, run.lo, level="read", d_mask=d_masks + 4 * nw * (c * M + m))
                 for c, up in enumerate(copies.runs)] for m in range(M)]

    def free_singles(got):
        for row in got:
            for sel, _, d_orig in row:
                sel.aln.free(); sel.loc.free(); d_orig.free()
    # the same selections
    a, b = batched(), singles()
    same = True
    for m in range(M):
        for c in range(COPIES):
            (s1, c1, o1), (s2, c2, o2) = a.of[m][c], b[m][c]
            k = s2.n_aln
            same &= s1.n_aln == k and c1["n_slots"] == c2["n_slots"] and c1["deepest"] == c2["deepest"]
            same &= s1.aln.download(np.uint8, 36 * k).tobytes() == s2.aln.download(np.uint8, 36 * k).tobytes()
            same &= o1.download(np.uint32, k).tobytes() == o2.download(np.uint32, k).tobytes()
            same &= s1.loc.download(np.uint8, 16 * run.nl).tobytes() == s2.loc.download(np.uint8, 16 * run.nl).tobytes()
    kept = [[int(x) for x in a.summary[m, :, 0]] for m in range(M)]
    a.free(); free_singles(b)
    tb, ts = [], []
    for _ in range(INNER):                                                     # (alternating)
        sync(); t0 = time.perf_counter(); got = batched(); sync(); tb.append((time.perf_counter() - t0) * 1e3); got.free()
        sync(); t0 = time.perf_counter(); got = singles(); sync(); ts.append((time.perf_counter() - t0) * 1e3); free_singles(got)
    out = {"alignments": int(run.up.n_aln), "loci": int(run.nl), "barcode_ids": int(run.A["n_bc"]), "read_name_ids": int(run.A["n_pair"]),
           "copies": COPIES, "rpb_targets": list(RPBS), "kept": kept, "selections_equal": bool(same),
           "select_copies_reads_ms": statistics.median(tb), "select_runs_ms": statistics.median(ts)}
    masks["masks"].free(); devplanes.close_rules(rules)
    copies.free(); run.free(); eng.close()
    return out


def spawn(job):
    """A fresh process for one job -> its JSON answer."""
    print("[%s] %s" % (time.strftime("%H:%M:%S"), job.get("prefix", job["kind"])), file=sys.stderr, flush=True)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", json.dumps(job)], stdout=subprocess.PIPE, check=True,
                         cwd=job["tree"])
    return json.loads(out.stdout.decode().splitlines()[-1])


def med(xs):
    return round(statistics.median(xs), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for measurement (d)")
    ap.add_argument("--parts", default="abcd", help="the measurements to make")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spike_scan_rpb_perf.json"))
    args = ap.parse_args()
    if args.child:
        job = json.loads(args.child)
        print(json.dumps(child_select(job) if job["kind"] == "select" else child_cli(job)))
        return
    _use(ROOT)
    import ds_af_restate
    import ds_restate
    from smcounter_amd import spike, synth
    from smcounter_amd.tools import spike_scan_lists as lists
    cfg = synth.SynthConfig("SPS", N_LOCI, N_UMI, RPB, 20170502, alt_locus_frac=0.3, alt_af=0.1)
    tmp = tempfile.mkdtemp()
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, N_LOCI)
    bed = ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci)
    base = ["--bedTarget=%s" % bed, "--mtDepth=%d" % P.mtDepth, "--rpb=%g" % P.rpb, "--refGenome=%s" % fa, "--bamFile=%s" % bam, "--dsSeed=%d" % SEED]
    text, rtext, ftext = ",".join("%g" % t for t in TARGETS), ",".join("%g" % r for r in RPBS), ",".join("%g" % f for f in FRACS)
    scan = ["--spikeScan=" + text, "--spikeScanReps=%d" % REPS, "--spikeScanStride=%d" % STRIDE]
    warm = ["--spikeScan=" + text, "--spikeScanReps=2", "--spikeScanStride=%d" % STRIDE]
    job = lambda tree, prefix, extra, w: dict(kind="cli", tree=tree, tmp=tmp, base=base, prefix=prefix, extra=extra, warm=w)
    res = json.load(open(args.out)) if os.path.exists(args.out) and set(args.parts) != set("abcd") else {}
    res.update({"targets": list(TARGETS), "rpb_targets": list(RPBS), "reps": REPS, "stride": STRIDE, "processes_per_figure": REPEATS,
                "file": {"loci": N_LOCI, "barcodes_per_locus": N_UMI, "reads_per_barcode": RPB, "records": len(A["aln"])}})
    if "a" in args.parts or "c" in args.parts:
        # (a) ((c) compares with the pages of a run with the flag)
        with_, without, log = [], [], None
        for n in range(REPEATS if "a" in args.parts else 1):
            got = spawn(job(ROOT, "rpb", scan + ["--spikeScanRpb=" + rtext], warm + ["--spikeScanRpb=" + rtext]))
            with_.append(got["seconds"]); log = got["log"]
            if "a" in args.parts:
                without.append(spawn(job(ROOT, "scan", scan, warm))["seconds"])
    if "a" in args.parts:
        closing = [l for l in log.splitlines() if l.startswith("--spikeScan:") and " stage " in l][-1]
        last = [l for l in log.splitlines() if l.startswith("--spikeScanRpb:")][-1]
        host = re.search(r"(\d+) of (\d+) verdicts decided by the host", closing)
        a = {"with_spikeScanRpb_s": med(with_), "without_s": med(without), "with_all_s": [round(x, 3) for x in with_],
             "without_all_s": [round(x, 3) for x in without], "stage_s": float(re.search(r"stage ([0-9.]+) s", closing).group(1)),
             "closing_line": closing, "rpb_line": last, "rule_lines": [l for l in log.splitlines() if re.match(r"--spikeScanRpb \S+: sampler", l)],
             "builds": int(re.search(r"(\d+) copies built and called", closing).group(1)),
             "select_copies_reads_calls": int(re.search(r"(\d+) select_copies_reads calls", last).group(1)),
             "host_decided_verdicts": int(host.group(1)), "verdicts": int(host.group(2))}
        a["rpb_axis_costs_s"] = round(a["with_spikeScanRpb_s"] - a["without_s"], 3)
        a["with_over_without"] = round(a["with_spikeScanRpb_s"] / a["without_s"], 2)
        a["cost_model_builds_ratio"] = 1 + len(RPBS)
        res["flag"] = a
    if "b" in args.parts:
        sel = [spawn(dict(kind="select", tree=ROOT, bam=bam, fa=fa, loci=loci, params=dataclasses.asdict(P)))
               for _ in range(REPEATS)]
        c = dict(sel[-1])
        c["select_copies_reads_ms"] = med([s["select_copies_reads_ms"] for s in sel])
        c["select_runs_ms"] = med([s["select_runs_ms"] for s in sel])
        c["select_copies_reads_all_ms"] = [round(s["select_copies_reads_ms"], 3) for s in sel]
        c["select_runs_all_ms"] = [round(s["select_runs_ms"], 3) for s in sel]
        c["selections_equal"] = all(s["selections_equal"] for s in sel)
        c["inner_repetitions"] = INNER
        c["select_runs_over_select_copies_reads"] = round(c["select_runs_ms"] / c["select_copies_reads_ms"], 2)
        c["batched_call_is_faster"] = bool(c["select_copies_reads_ms"] < c["select_runs_ms"])
        res["select_copies_reads"] = c
    if "c" in args.parts:
        names = lists.main(argparse.Namespace(runPath=None, bedTarget=bed, refGenome=fa, stride=STRIDE, alt="transition",
                                              outPrefix=os.path.join(tmp, "lists")))
        subset = names[::max(1, len(names) // SUBSET)][:SUBSET]
        mine = {}
        for line in open(os.path.join(tmp, "rpb.spikeScan.rpb.sensitivity.txt")).read().splitlines()[1:]:
            f = line.split("\t")
            mine[(f[0], f[1], f[4], f[5])] = f
        page = spike.cell_sensitivity_header(spike.RPB_AXIS)
        drop = [page.index(x) for x in ("PI_MEAN", "PI_MIN")]
        total, same, compared = 0.0, True, 0
        for n, name in enumerate(subset):
            extra = ["--spikeAF=" + text, "--spikeVariants=%s" % name, "--spikeRpb=" + rtext]
            times = [spawn(job(ROOT, "pass%d" % n, extra + ["--spikeReps=%d" % REPS], extra + ["--spikeReps=2"]))["seconds"] for _ in range(REPEATS)]
            total += statistics.median(times)
            for line in open(os.path.join(tmp, "pass%d.spikeAF.rpb.sensitivity.txt" % n)).read().splitlines()[1:]:
                f = line.split("\t")
                same &= mine[(f[0], f[1], f[4], f[5])] == [x for k, x in enumerate(f) if k not in drop]
                compared += 1
        res["separate_runs"] = {"subset": len(subset), "subset_of": len(names), "subset_sum_s": round(total, 3),
                                "all_passes_scaled_s": round(total * len(names) / len(subset), 3),
                                "note": "a subset of the passes was timed; the figure for all passes is the subset's sum scaled by passes / subset",
                                "lines_compared": compared, "scan_lines_equal_the_separate_runs": bool(same)}
        if "flag" in res:
            res["separate_runs"]["scaled_over_the_run_with_the_flag"] = round(res["separate_runs"]["all_passes_scaled_s"] /
                                                                              res["flag"]["with_spikeScanRpb_s"], 2)
    if "d" in args.parts:
        if args.parent:
            parent = os.path.abspath(args.parent)
            d = {}
            for what, more in (("plain_scan", []), ("depth_scan", ["--spikeScanDepth=" + ftext])):
                this, theirs = [], []
                for _ in range(REPEATS):
                    this.append(spawn(job(ROOT, what + "_this", scan + more, warm + more))["seconds"])
                    theirs.append(spawn(job(parent, what + "_parent", scan + more, warm + more))["seconds"])
                d[what] = {"this_tree_s": med(this), "parent_s": med(theirs), "this_tree_all_s": [round(x, 3) for x in this],
                           "parent_all_s": [round(x, 3) for x in theirs], "parent_spread_s": [round(min(theirs), 3), round(max(theirs), 3)],
                           "this_tree_within_the_parents_spread": bool(statistics.median(this) <= max(theirs))}
            res["scans_against_parent"] = d
        else:
            res["scans_against_parent"] = "not measured: no --parent checkout given"
    line = json.dumps(res)
    print(line)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
