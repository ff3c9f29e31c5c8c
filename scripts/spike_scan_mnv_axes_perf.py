"""Cost of --spikeScanMnvFilter and --spikeScanMnvDepth (dev tool, GPU box) -> profiles/spike_scan_mnv_axes_perf.json.

scripts/spike_scan_mnv_perf.py's fixture and method - 128 loci at 20,000x, three targets, R = 32, S = 16, L = 2; one GPU; every timed run
a FRESH process behind a warm-up scan of two replicates, medians of REPEATS with min .. max and every run kept, the stage's own clock
beside the wall time; every child under a timeout of its own, and a child that fails ends the job.  Its helpers are imported, not
copied.  The fixture is called at --rpb 2.9 where FILTER is measured: at the file's own 10 reads per barcode the switch's cost is the
same, but a --bedTandemRepeats track over the lower half of the loci makes the two halves differ, as in the test.
  scan      the MNV scan with and without --spikeScanMnvFilter under --spikeScanBuild whole and listed; the files of the two builds are
            compared byte for byte, and every file of the scan without the switch with the same file of the scan with it
  passes    a SUBSET of the 16 passes as --spikeAF --spikeVariants pass<k>.txt --spikeReps 32 --spikePhase runs of their own, the sum
            SCALED by passes / subset and stated as such; the lines of the filter page restated from the members' FILTER and CALLED
            columns of their .spikeAF.replicates.txt and compared with the scan's
  filter    one batch's joint FILTER words, device synchronised around each call: smc_scan_filter_sets (4 bytes per copy and set and
            replicate 0's member words come down) against smc_scan_filter plus the host's reduction (abi.scan_filter_joint_rule in
            numpy; 4 bytes per copy and member come down), in time and bytes
  depth     the MNV scan with --spikeScanMnvDepth 0.5,0.25, alone and beside the switch, whole and listed, the builds counted; a SUBSET
            of the passes as --spikeReps --spikePhase --spikeDepth runs, SCALED, their cell lines compared with the scan's
  plain     the plain MNV scan and the plain SNV scan WITHOUT the new switch on this tree and on a built checkout of the parent commit
            (--parent DIR), PLAIN_ROUNDS rounds of one fresh process per tree and scan, the order rotated from round to round: this
            tree's median must lie within the parent's fastest .. slowest

usage: spike_scan_mnv_axes_perf.py [--parent DIR] [out.json] [entry ...]      (children: --one <mode> <json> / --pass <list> <json>)"""
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.environ.get("SMC_PERF_TREE") or ROOT)        # (a child of `plain` imports the package of the tree it measures)
sys.path.insert(1, os.path.join(ROOT, "tests"))
sys.path.insert(2, os.path.join(ROOT, "scripts"))
import spike_scan_mnv_perf as base  # noqa: E402  (the fixture, the children's runner, the spreads)

TARGETS, L, REPEATS, SUBSET, COPIES = base.TARGETS, base.L, base.REPEATS, base.SUBSET, base.COPIES
PLAIN_ROUNDS = base.PLAIN_ROUNDS
MNV = ["--spikeScanMnv=%d" % L]
FRACS = "0.5,0.25"
MODES = {"mnv_whole": MNV, "mnv_filter_whole": MNV + ["--spikeScanMnvFilter"], "mnv_listed": MNV + ["--spikeScanBuild=listed"],
         "mnv_filter_listed": MNV + ["--spikeScanMnvFilter", "--spikeScanBuild=listed"], "snv_whole": [],
         "mnv_depth_whole": MNV + ["--spikeScanMnvDepth=" + FRACS], "mnv_depth_listed": MNV + ["--spikeScanMnvDepth=" + FRACS, "--spikeScanBuild=listed"],
         "mnv_both_whole": MNV + ["--spikeScanMnvDepth=" + FRACS, "--spikeScanMnvFilter"],
         "mnv_both_listed": MNV + ["--spikeScanMnvDepth=" + FRACS, "--spikeScanMnvFilter", "--spikeScanBuild=listed"]}
DEPTH_MODES = ("mnv_depth_whole", "mnv_depth_listed", "mnv_both_whole", "mnv_both_listed")
CLOSING = re.compile(r"^--spikeScanMnv \d+: (\d+) sets scanned, (\d+) loci skipped, (\d+) of (\d+) joint verdicts decided by the host"
                     r"(?:; --spikeScanMnvFilter: (\d+) of (\d+) called sets PASS, the FILTER of (\d+) decided by the host; (.*?))?"
                     r"(?:; --spikeScanMnvDepth: fractions \S+: (\d+) cells per pass, (\d+) builds \(S x R x T x \(1 \+ F\)\), (\d+) select_copies calls)?$",
                     re.M)


def _extra(shape):
    return ["--bedTandemRepeats=%s" % shape["trf"]] if shape.get("trf") else []


def one(mode, shape):
    """(child) warm-up, then one timed scan -> a JSON line."""
    text = ",".join("%g" % t for t in TARGETS)
    run = base._cli(shape, ["--spikeScan=" + text, "--spikeScanStride=%d" % shape["stride"]] + MODES[mode] + _extra(shape))
    run("warm_" + mode, "--spikeScanReps=2")
    t, log = run("scan_" + mode, "--spikeScanReps=%d" % shape["reps"])
    closing = [l for l in log.splitlines() if l.startswith("--spikeScan:") and " stage " in l][-1]
    lines = re.findall(r"^--spikeScan pass \d+: (\d+) variants, (\d+) copies, (\d+) builds(?:, (\d+) of them whole)?, (\d+) verdicts", log, re.M)
    out = {"wall_s": round(t, 4), "stage_s": float(re.search(r"stage ([0-9.]+) s", closing).group(1)), "passes": len(lines),
           "builds": sum(int(l[2]) for l in lines)}
    m = CLOSING.search(log)
    if m:
        out.update(sets=int(m.group(1)), joint_verdicts_decided_by_the_host=int(m.group(3)), joint_verdicts=int(m.group(4)))
        if m.group(5) is not None:
            out.update(called_sets_pass=int(m.group(5)), called_sets=int(m.group(6)), filter_decided_by_the_host=int(m.group(7)), names=m.group(8))
        if m.group(9) is not None:
            out.update(cells_per_pass=int(m.group(9)), builds_by_the_closing_line=int(m.group(10)), select_copies_calls=int(m.group(11)))
    print(json.dumps(out))


def one_pass(name, shape):
    """(child) a pass as a run of its own: warm-up (two replicates), then the timed run -> a JSON line."""
    text = ",".join("%g" % t for t in TARGETS)
    run = base._cli(shape, ["--spikeAF=" + text, "--spikeVariants=%s" % name, "--spikePhase"] + _extra(shape) +
                    (["--spikeDepth=" + shape["pass_depth"]] if shape.get("pass_depth") else []))
    tag = os.path.basename(name).replace(".txt", "")
    run("warm_" + tag, "--spikeReps=2")
    t, _ = run("own_" + tag, "--spikeReps=%d" % shape["reps"])
    print(json.dumps({"wall_s": round(t, 4)}))


def _fixture():
    sh = base._fixture()
    by = sorted(p for _, p in sh["loci"])
    sh["trf"] = os.path.join(sh["tmp"], "trf.bed")
    with open(sh["trf"], "w") as fh:              # (the lower half of the positions: its end falls between the members of one MNV)
        fh.write("%s\t%d\t%d\n" % (sh["loci"][0][0], by[0] - 1, by[(len(by) - 1) // 2]))
    sh["rpb_param"] = 2.9
    return sh


def _child(what, arg, sh, tree=None):
    # (the children are this script's: spike_scan_mnv_perf._child starts its own file)
    import subprocess
    env = dict(os.environ, SMC_HOST_THREADS=str(min(16, int(os.environ.get("SMC_HOST_THREADS", "16") or 16))))
    if tree:
        env["SMC_PERF_TREE"] = tree
    out = subprocess.run([sys.executable, os.path.abspath(__file__), what, arg, json.dumps(sh)], check=True, capture_output=True, text=True,
                         env=env, timeout=base.CHILD_TIMEOUT)
    return json.loads(out.stdout.strip().splitlines()[-1])


def _files(tmp, mode):
    return {f[len("scan_" + mode):]: open(os.path.join(tmp, f), "rb").read() for f in os.listdir(tmp) if f.startswith("scan_%s." % mode)}


def compare_scan(sh):
    res = {"shape": dict(base.SHAPE), "targets": list(TARGETS), "mnv_letters": L, "repetitions": REPEATS, "rpb": sh["rpb_param"]}
    modes = [m for m in MODES if m != "snv_whole" and m not in DEPTH_MODES]
    for mode in modes:
        runs = [_child("--one", mode, sh) for _ in range(REPEATS)]
        res[mode] = dict(runs[-1], **base._spread(runs, "wall_s"), **base._spread(runs, "stage_s"))
    files = {m: _files(sh["tmp"], m) for m in modes}
    same = lambda a, b, names: all(files[a][f] == files[b][f] for f in names if not f.endswith(".vcf"))      # (the .cut.vcf names its prefix)
    res["filter_files_equal_whole_and_listed"] = sorted(files["mnv_filter_whole"]) == sorted(files["mnv_filter_listed"]) and \
        same("mnv_filter_whole", "mnv_filter_listed", files["mnv_filter_whole"])
    res["files_without_the_switch_unchanged"] = same("mnv_whole", "mnv_filter_whole", files["mnv_whole"]) and \
        same("mnv_listed", "mnv_filter_listed", files["mnv_listed"])
    res["new_files"] = sorted(set(files["mnv_filter_whole"]) - set(files["mnv_whole"]))
    for b in ("whole", "listed"):
        res["filter_minus_plain_%s_stage_s" % b] = round(res["mnv_filter_" + b]["stage_s"] - res["mnv_" + b]["stage_s"], 4)
    return res


def compare_depth(sh):
    """The MNV scan with --spikeScanMnvDepth 0.5,0.25, alone and beside the switch, whole and listed: the builds counted (S x R x T x
    (1 + F)), the files of the two builds compared, and a SUBSET of the passes as --spikeReps --spikePhase --spikeDepth runs of their own
    (SCALED), their cell lines held against the scan's depth sensitivity page."""
    import argparse
    from smcounter_amd.tools import spike_scan_lists as lists
    res = {"fractions": FRACS, "repetitions": REPEATS}
    for mode in DEPTH_MODES:
        runs = [_child("--one", mode, sh) for _ in range(REPEATS)]
        res[mode] = dict(runs[-1], **base._spread(runs, "wall_s"), **base._spread(runs, "stage_s"))
    files = {m: _files(sh["tmp"], m) for m in DEPTH_MODES}
    same = lambda a, b: sorted(files[a]) == sorted(files[b]) and all(files[a][f] == files[b][f] for f in files[a] if not f.endswith(".vcf"))
    res["files_equal_whole_and_listed"] = same("mnv_depth_whole", "mnv_depth_listed") and same("mnv_both_whole", "mnv_both_listed")
    tmp = sh["tmp"]
    names = lists.main(argparse.Namespace(runPath=None, bedTarget=sh["bed"], refGenome=sh["fa"], stride=sh["stride"], alt="transition", mnv=L,
                                          outPrefix=os.path.join(tmp, "dlists")))
    subset = names[::max(1, len(names) // SUBSET)][:SUBSET]
    total, per = 0.0, []
    for name in subset:
        runs = [_child("--pass", name, dict(sh, pass_depth=FRACS)) for _ in range(REPEATS)]
        per.append(base._spread(runs, "wall_s"))
        total += per[-1]["wall_s"]
    mine = {tuple(l.split("\t")[i] for i in (0, 5, 6)): l
            for l in open(os.path.join(tmp, "scan_mnv_depth_whole.spikeScan.mnv.depth.sensitivity.txt")).read().splitlines()[1:]}
    ok, compared = True, 0
    for name in subset:
        tag = os.path.basename(name).replace(".txt", "")
        for l in open(os.path.join(tmp, "own_%s.spikeAF.phase.sensitivity.txt" % tag)).read().splitlines()[1:]:
            f = l.split("\t")
            if f[6] != "full":
                ok &= mine[(f[0], f[5], f[6])] == l
                compared += 1
    res["passes"] = dict(subset=len(subset), subset_of=len(names), per_pass=per, subset_sum_s=round(total, 3),
                         all_passes_scaled_s=round(total * len(names) / len(subset), 3), lines_compared=compared,
                         scan_lines_equal_the_separate_runs=bool(ok),
                         note="a subset of the passes was timed; the figure for all passes is the subset's sum scaled by passes / subset")
    return res


def compare_passes(sh):
    """A subset of the passes as runs of their own (after compare_scan: their replicate pages are held against the scan's filter page)."""
    import argparse
    from smcounter_amd.tools import spike_scan_lists as lists
    import scan_filter_pages as pages
    tmp = sh["tmp"]
    names = lists.main(argparse.Namespace(runPath=None, bedTarget=sh["bed"], refGenome=sh["fa"], stride=sh["stride"], alt="transition", mnv=L,
                                          outPrefix=os.path.join(tmp, "lists")))
    subset = names[::max(1, len(names) // SUBSET)][:SUBSET]
    total, per = 0.0, []
    for name in subset:
        runs = [_child("--pass", name, sh) for _ in range(REPEATS)]
        per.append(base._spread(runs, "wall_s"))
        total += per[-1]["wall_s"]
    res = dict(subset=len(subset), subset_of=len(names), per_pass=per, subset_sum_s=round(total, 3),
               all_passes_scaled_s=round(total * len(names) / len(subset), 3),
               note="a subset of the passes was timed; the figure for all passes is the subset's sum scaled by passes / subset")
    page = os.path.join(tmp, "scan_mnv_filter_whole.spikeScan.mnv.filter.txt")
    if os.path.exists(page):
        mine = {tuple(l.split("\t")[:5]): l.split("\t") for l in open(page).read().splitlines()[1:]}
        same, compared = True, 0
        for name in subset:
            tag = os.path.basename(name).replace(".txt", "")
            member = {}
            for l in open(os.path.join(tmp, "own_%s.spikeAF.replicates.txt" % tag)).read().splitlines()[1:]:
                f = l.split("\t")
                member.setdefault(tuple(f[:5]), []).append((f[-2], f[-1]))
            for l in open(name).read().splitlines():
                c, p, ref, alt = l.split("\t")[:4]
                for t in TARGETS:
                    mem = [member[(c, "%d" % (int(p) + m), ref[m], alt[m], "%g" % t)] for m in range(L)]
                    joint = []
                    for reps in zip(*mem):
                        held = [n for n in pages.NAMES if any(n in x.split(";") for x, _ in reps)]
                        joint.append((";".join(held) or "PASS", "1" if all(int(x) == 1 for _, x in reps) else "0"))
                    same &= mine[(c, p, ref, alt, "%g" % t)] == pages.line([c, p, ref, alt, "%g" % t], joint)
                    compared += 1
        res.update(lines_compared=compared, scan_lines_equal_the_separate_runs=bool(same))
    return res


def compare_filter(sh):
    """One batch: smc_scan_filter_sets against smc_scan_filter plus the host's reduction, and the bytes each brings down."""
    import numpy as np
    from smcounter_amd import abi, devplanes, fasta, postfilter, spike, vc
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
    members = [k for s in sets for k in s.members]
    offsets = np.array([at[(mnvs[k].chrom, mnvs[k].pos)] for k in members], np.uint32)
    repeats = postfilter.load_repeat_regions(sh["bed"], sh["trf"], None)
    gate, always = spike.scan_filter_words([mnvs[k] for k in members], P.hpLen, ref, *repeats)
    set_off = np.arange(0, len(members) + 1, L, dtype=np.uint32)
    batch = np.tile(rows, COPIES)
    d_rows = DevBuf(eng, batch.nbytes + 256).upload(batch.view(np.uint8).reshape(-1))
    sync = lambda: eng.L.smc_device_sync(eng.ctx)

    def with_sets():
        return devplanes.scan_filter_sets(eng, d_rows, COPIES, nl, offsets, gate, always, set_off, members_of=[0])

    def with_members():
        words = devplanes.scan_filter(eng, d_rows, COPIES, nl, offsets, gate, always)
        return abi.scan_filter_joint_rule(words, set_off), words

    def median_ms(fn):
        fn(); sync()
        times = []
        for _ in range(25):
            t0 = time.perf_counter()
            fn(); sync()
            times.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "max_ms": round(max(times), 4)}
    joint, mem0 = with_sets()
    want, words = with_members()
    G, S = len(members), len(sets)
    out = {"copies": COPIES, "loci_per_copy": nl, "members": G, "sets": S,
           "equal": bool(np.array_equal(joint, want) and mem0[0].tobytes() == words[0].tobytes()),
           "scan_filter_sets": dict(median_ms(with_sets), bytes_down=4 * COPIES * S + 4 * G),
           "scan_filter_and_host_reduction": dict(median_ms(with_members), bytes_down=4 * COPIES * G)}
    d_rows.free()
    eng.close()
    return out


def compare_plain(sh, parent):
    """The default paths: no new switch, this tree against the parent's, both scans."""
    trees = [("parent", parent), ("this", ROOT)]
    res = {"rounds": PLAIN_ROUNDS}
    for mode in ("mnv_whole", "snv_whole"):
        runs = {who: [] for who, _ in trees}
        for i in range(PLAIN_ROUNDS):
            k = i % len(trees)
            for who, tree in trees[k:] + trees[:k]:
                runs[who].append(base._child("--one", mode, sh, tree))     # (spike_scan_mnv_perf's child: one command line for both trees)
        got = {who: dict(base._spread(runs[who], "stage_s"), **base._spread(runs[who], "wall_s")) for who in runs}
        lo, hi = got["parent"]["stage_min_s"], got["parent"]["stage_max_s"]
        got["this_median_within_parent_spread"] = bool(lo <= got["this"]["stage_s"] <= hi)
        d = [x - y for x, y in zip(got["this"]["stage_all_s"], got["parent"]["stage_all_s"])]
        got["this_minus_parent_paired_s"] = dict(median=round(statistics.median(d), 4), all=[round(x, 4) for x in d])
        res[mode] = got
    return res


def main():
    a = sys.argv[1:]
    if a and a[0] == "--one":
        return one(a[1], json.loads(a[2]))
    if a and a[0] == "--pass":
        return one_pass(a[1], json.loads(a[2]))
    parent = None
    if a and a[0] == "--parent":
        parent, a = os.path.abspath(a[1]), a[2:]
    out = a[0] if a else os.path.join(ROOT, "profiles", "spike_scan_mnv_axes_perf.json")
    names = a[1:] or ["scan", "passes", "filter", "depth"] + (["plain"] if parent else [])
    res = {}
    if os.path.exists(out):
        with open(out) as fh:
            res = json.load(fh)
    sh = _fixture()
    for n in names:
        res[n] = compare_scan(sh) if n == "scan" else compare_passes(sh) if n == "passes" else compare_filter(sh) if n == "filter" else \
            compare_depth(sh) if n == "depth" else compare_plain(sh, parent)
        print("%s done" % n, file=sys.stderr, flush=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
