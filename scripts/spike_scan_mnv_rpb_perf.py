"""Cost of --spikeScanMnvRpb (dev tool, GPU box) -> profiles/spike_scan_mnv_rpb_perf.json.

scripts/spike_scan_mnv_axes_perf.py's fixture and method - 128 loci at 20,000x, three targets, R = 32, S = 16, L = 2; one GPU; every
timed run a FRESH process behind a warm-up scan of two replicates, medians of REPEATS with min .. max and every run kept, the stage's own
clock beside the wall time; every child under a timeout of its own, and a child that fails ends the job.  Its helpers are imported, not
copied.  The reads-per-barcode targets are 4 and 2 (the file holds 10 reads per barcode).
  scan      the MNV scan with and without --spikeScanMnvRpb 4,2 under --spikeScanBuild whole and listed; the builds counted from the pass
            lines (S x R x T x (1 + Rr)); the files of the two builds compared byte for byte, and every file of the scan without the
            flag with the same file of the scan with it
  counts    ONE pass in one process, device synchronised around each way, the outputs asserted equal BEFORE either is timed: the joint
            counts by smc_scan_phase_rpb_counts - the read bits left in HBM, one call, the run's barcode-major order made once per
            decoded run and timed apart - against the existing host path on the same inputs: the bits downloaded, spike_rpb_records per
            member, spike_joint_records per set, the upload and smc_spike_phase_rpb_counts
  plain     --spikeScanMnv alone and --spikeScanRpb alone (the SNV scan at 4,2) on this tree and on a built checkout of the parent commit
            (--parent DIR), PLAIN_ROUNDS rounds of one fresh process per tree and scan, the order rotated from round to round; whether
            this tree's median lies within the parent's fastest .. slowest is stated per scan

usage: spike_scan_mnv_rpb_perf.py [--parent DIR] [out.json] [entry ...]      (children: --one <mode> <json>)"""
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
import spike_scan_mnv_perf as base  # noqa: E402  (the fixture, the command line's runner, the spreads)

TARGETS, L, REPEATS, PLAIN_ROUNDS = base.TARGETS, base.L, base.REPEATS, base.PLAIN_ROUNDS
RPBS = "4,2"
MNV = ["--spikeScanMnv=%d" % L]
MODES = {"mnv_whole": MNV, "mnv_listed": MNV + ["--spikeScanBuild=listed"], "mnv_rpb_whole": MNV + ["--spikeScanMnvRpb=" + RPBS],
         "mnv_rpb_listed": MNV + ["--spikeScanMnvRpb=" + RPBS, "--spikeScanBuild=listed"], "snv_rpb_whole": ["--spikeScanRpb=" + RPBS]}
CLOSING = re.compile(r"; --spikeScanMnvRpb: reads-per-barcode targets \S+: (\d+) cells per pass, (\d+) builds \(S x R x T x \(1 \+ Rr\)\), "
                     r"(\d+) select_copies_reads calls$", re.M)


def one(mode, shape):
    """(child) warm-up, then one timed scan -> a JSON line."""
    text = ",".join("%g" % t for t in TARGETS)
    run = base._cli(shape, ["--spikeScan=" + text, "--spikeScanStride=%d" % shape["stride"]] + MODES[mode])
    run("warm_" + mode, "--spikeScanReps=2")
    t, log = run("scan_" + mode, "--spikeScanReps=%d" % shape["reps"])
    closing = [l for l in log.splitlines() if l.startswith("--spikeScan:") and " stage " in l][-1]
    lines = re.findall(r"^--spikeScan pass \d+: (\d+) variants, (\d+) copies, (\d+) builds(?:, (\d+) of them whole)?, (\d+) verdicts", log, re.M)
    out = {"wall_s": round(t, 4), "stage_s": float(re.search(r"stage ([0-9.]+) s", closing).group(1)), "passes": len(lines),
           "copies": sum(int(l[1]) for l in lines), "builds": sum(int(l[2]) for l in lines)}
    m = CLOSING.search(log)
    if m:
        out.update(cells_per_pass=int(m.group(1)), builds_by_the_closing_line=int(m.group(2)), select_copies_reads_calls=int(m.group(3)))
    print(json.dumps(out))


def _child(what, arg, sh, tree=None):
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
    res = {"shape": dict(base.SHAPE), "targets": list(TARGETS), "mnv_letters": L, "rpb_targets": RPBS, "repetitions": REPEATS}
    modes = [m for m in MODES if m.startswith("mnv")]
    for mode in modes:
        runs = [_child("--one", mode, sh) for _ in range(REPEATS)]
        res[mode] = dict(runs[-1], **base._spread(runs, "wall_s"), **base._spread(runs, "stage_s"))
    files = {m: _files(sh["tmp"], m) for m in modes}
    same = lambda a, b, names: all(files[a][f] == files[b][f] for f in names if not f.endswith(".vcf"))      # (the .cut.vcf names its prefix)
    res["files_equal_whole_and_listed"] = sorted(files["mnv_rpb_whole"]) == sorted(files["mnv_rpb_listed"]) and \
        same("mnv_rpb_whole", "mnv_rpb_listed", files["mnv_rpb_whole"])
    res["files_without_the_flag_unchanged"] = same("mnv_whole", "mnv_rpb_whole", files["mnv_whole"]) and \
        same("mnv_listed", "mnv_rpb_listed", files["mnv_listed"])
    res["new_files"] = sorted(set(files["mnv_rpb_whole"]) - set(files["mnv_whole"]))
    n_r = len(RPBS.split(","))
    for b in ("whole", "listed"):
        with_flag, plain = res["mnv_rpb_" + b], res["mnv_" + b]
        res["builds_%s" % b] = dict(without=plain["builds"], with_flag=with_flag["builds"],
                                    with_flag_is_copies_x_1_plus_rr=bool(with_flag["builds"] == with_flag["copies"] * (1 + n_r)))
        res["flag_minus_plain_%s_stage_s" % b] = round(with_flag["stage_s"] - plain["stage_s"], 4)
        res["flag_over_plain_%s_stage" % b] = round(with_flag["stage_s"] / plain["stage_s"], 3)
    return res


def compare_counts(sh):
    """One pass of the fixture's MNV scan: the joint counts both ways on the same inputs, equal before either is timed."""
    import numpy as np
    from smcounter_amd import bamio, devplanes, dsaf, fasta
    from smcounter_amd.engine import Engine
    from smcounter_amd.params import VcParams
    from smcounter_amd.tools import spike_scan_lists as lists
    from smcounter_amd.tools import spike_variants as sv
    eng = Engine(0)
    ref = fasta.FastaFile(sh["fa"])
    P = VcParams(mtDepth=sh["mtDepth"], rpb=sh["rpb_param"])
    R, rpbs = sh["reps"], [float(x) for x in RPBS.split(",")]
    seeds = dsaf.rep_seeds(base.SEED, R)
    thr = [sv.threshold(t) for t in TARGETS]
    mnvs, leaders, _ = lists.scan_mnvs([(c, str(p)) for c, p in sh["loci"]], ref, L, "transition")
    members = lists.mnv_passes(mnvs, sh["stride"])[0][1]
    sets = mnvs.sets
    spans = devplanes._set_spans(mnvs, sets, sorted(range(len(sets)), key=lambda i: (sets[i].chrom, mnvs[sets[i].members[0]].pos)))
    chrom, lo, hi, span = next(spans)
    run = devplanes.AfRun(chrom, lo, hi, [], 0)
    rules = devplanes.philox_read_rules(sh["bam"], rpbs, [P] * len(rpbs), base.SEED, eng, flag="--spikeScanMnvRpb")
    sync = lambda: eng.L.smc_device_sync(eng.ctx)
    shared = {}
    try:
        nl = run.load(sh["bam"], ref, eng, P, 128_000_000, bamio.host_threads(), mism=True)
        taken = set(devplanes.sets_inside(mnvs, sets, span, lo, nl))
        group = [k for i in members if i in taken for k in sets[i].members]
        n_sets = len(group) // L
        var, ins = devplanes.af_run_variants([mnvs[k] for k in group], chrom, lo, ref)
        cov, _, _ = devplanes.allele_carriers_run(eng, run.up, run.A, lo, var, ins, counts=True)
        cover = np.asarray(cov)[:, :len(run.idents)] != 0
        t0 = time.perf_counter()
        shared = devplanes._scan_read_masks(eng, run, rules, seeds, "--spikeScanMnvRpb", order=True)
        sync()
        per_run_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        order_host = devplanes.run_barcode_major(run.A, shared["p_idents"], shared["first"])
        order_ms = (time.perf_counter() - t0) * 1e3
        rthr = [r.thr for r in rules]
        lead = [mnvs[group[s * L]].pos for s in range(n_sets)]
        rows = [list(range(s * L, (s + 1) * L)) for s in range(n_sets)]
        gids = [np.flatnonzero(cover[s * L:(s + 1) * L].all(axis=0)).astype(np.uint32) for s in range(n_sets)]
        singles = [[k] for k in range(len(group))]
        own = [np.flatnonzero(cover[k]).astype(np.uint32) for k in range(len(group))]
        covers = [run.idents[g] for g in own]
        psets = [sv.PhaseSet("", chrom, tuple(r)) for r in rows]

        def device(with_members):
            d_bits = devplanes.spike_read_bits_dev(eng, run.up, run.A, lo, var)
            try:
                return devplanes.scan_phase_rpb_counts(eng, shared["order"], d_bits, len(var), rows + (singles if with_members else []),
                                                       gids + (own if with_members else []),
                                                       lead + ([mnvs[group[k - k % L]].pos for k in range(len(group))] if with_members else []),
                                                       seeds, thr, rthr)
            finally:
                d_bits.free()

        stages = {}

        def host():
            t = [time.perf_counter()]
            bits = devplanes.spike_read_bits(eng, run.up, run.A, lo, var)
            t.append(time.perf_counter())
            records = [devplanes.spike_rpb_records(run.A, bits[k], own[k], shared["p_idents"], shared["first"]) for k in range(len(group))]
            t.append(time.perf_counter())
            joint = devplanes.spike_joint_records(psets, covers, records)
            t.append(time.perf_counter())
            out = devplanes.spike_phase_rpb_counts(eng, lead, [L] * n_sets, joint, seeds, thr, rthr)
            t.append(time.perf_counter())
            for name, a, b in zip(("bits_and_download", "spike_rpb_records", "spike_joint_records", "upload_and_counts"), t, t[1:]):
                stages.setdefault(name, []).append((b - a) * 1e3)
            return out, sum(len(j[2]) for j in joint)

        mine, (theirs, n_records) = device(False), host()
        assert np.array_equal(mine, theirs), "smc_scan_phase_rpb_counts and the host path disagree"
        assert np.array_equal(device(True)[:n_sets], mine)
        stages.clear()

        def median_ms(fn):
            fn(); sync()
            times = []
            for _ in range(15):
                t0 = time.perf_counter()
                fn(); sync()
                times.append((time.perf_counter() - t0) * 1e3)
            return {"median_ms": round(statistics.median(times), 3), "min_ms": round(min(times), 3), "max_ms": round(max(times), 3)}
        out = {"sets": n_sets, "members": len(group), "alignments": int(run.up.n_aln), "barcodes": int(run.A["n_bc"]), "replicates": R,
               "targets": len(thr), "read_thresholds": len(rthr), "joint_barcodes": int(sum(len(g) for g in gids)),
               "records_in_the_host_csr": int(n_records), "bit_bytes": int(len(var) * run.up.n_aln), "equal": True,
               "device_sets": median_ms(lambda: device(False)), "device_sets_and_members": median_ms(lambda: device(True)),
               "host_sets": median_ms(host)}
        out["host_stages_median_ms"] = {k: round(statistics.median(v), 3) for k, v in stages.items()}
        out["once_per_decoded_run"] = {"scan_read_masks_with_order_ms": round(per_run_ms, 3), "run_barcode_major_host_ms": round(order_ms, 3)}
        out["host_over_device"] = round(out["host_sets"]["median_ms"] / out["device_sets"]["median_ms"], 2)
        return out
    finally:
        for k in ("masks", "order"):
            if shared.get(k) is not None:
                shared[k].free()
        run.free()
        devplanes.close_rules(rules)
        eng.close()


def compare_plain(sh, parent):
    """The paths without the new flag: this tree against the parent's, --spikeScanMnv alone and --spikeScanRpb alone."""
    trees = [("parent", parent), ("this", ROOT)]
    res = {"rounds": PLAIN_ROUNDS}
    for mode in ("mnv_whole", "snv_rpb_whole"):
        runs = {who: [] for who, _ in trees}
        for i in range(PLAIN_ROUNDS):
            k = i % len(trees)
            for who, tree in trees[k:] + trees[:k]:
                runs[who].append(_child("--one", mode, sh, tree))
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
    parent = None
    if a and a[0] == "--parent":
        parent, a = os.path.abspath(a[1]), a[2:]
    out = a[0] if a else os.path.join(ROOT, "profiles", "spike_scan_mnv_rpb_perf.json")
    names = a[1:] or ["scan", "counts"] + (["plain"] if parent else [])
    res = {}
    if os.path.exists(out):
        with open(out) as fh:
            res = json.load(fh)
    sh = base._fixture()
    for n in names:
        res[n] = compare_scan(sh) if n == "scan" else compare_counts(sh) if n == "counts" else compare_plain(sh, parent)
        print("%s done" % n, file=sys.stderr, flush=True)
        with open(out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
