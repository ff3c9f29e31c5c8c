"""Cost of --spikeScanIndel (dev tool, GPU box).

On scripts/spike_scan_perf.py's input (a synthetic BAM, 128 loci x 2,000 barcodes x 10 reads by default), its three targets, R
replicates and stride S, wall time in process, after a warm-up run, medians of `REPEATS`:
(a) the run with --spikeScan --spikeScanIndel del1 beside the SNV scan on the same tree and the run without either; the stage's own
    clock, ms per copy built and called, and the verdicts the host decided, from the run log;
(b) for one batch - one pass of one target, B copies from one smc_spike_indels_reps call, device synchronised around each side -: the
    builds that leave their extras in HBM plus smc_scan_detect_keys, against the path they replace: the same builds with every
    locus's table made eagerly, a relocated record's texts through devplanes.copy_allele_key (which downloads the copy), and the
    id of the planted key looked up in the table.  The ids of both sides are compared;
(c) scripts/spike_scan_perf.py - the SNV scan - on this tree and on a checkout of the parent commit (`parent_tree`, built), each
    in fresh processes, alternating, `TREE_RUNS` times: the SNV scan's wall time and stage clock per run, to show whether it moved
    beyond its run-to-run spread.  Without `parent_tree` the part is left out and the result says so.

usage: spike_scan_indel_perf.py [out.json] [parent_tree] [n_loci] [n_umi] [rpb] [reps] [stride]   -> one JSON line"""
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import ds_af_restate  # noqa: E402
import ds_restate  # noqa: E402
import spike_scan_perf as snv  # noqa: E402  (the SNV scan's input, targets and seed)
from smcounter_amd import abi, bamio, cli, devplanes, fasta, synth  # noqa: E402
from smcounter_amd.engine import DevBuf, Engine  # noqa: E402
from smcounter_amd.tools import spike_scan_lists as lists  # noqa: E402
from smcounter_amd.tools import spike_variants as sv  # noqa: E402

TARGETS, SEED, REPEATS = snv.TARGETS, snv.SEED, snv.REPEATS
RULE = "del1"
COPIES = 8
TREE_RUNS = 2


def wall(tmp, bam, fa, bed, P, n_reps, stride):
    """(a)"""
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

    def figures(times, log):
        closing = [l for l in log.splitlines() if l.startswith("--spikeScan:") and " stage " in l][-1]
        per_pass = re.findall(r"^--spikeScan pass \d+: (\d+) variants, (\d+) copies, (\d+) builds, (\d+) verdicts decided by the host, "
                              r"([0-9.]+) s$", log, re.M)
        out = {"wall_s": round(statistics.median(times), 3), "wall_all_s": [round(x, 3) for x in times],
               "stage_s": float(re.search(r"stage ([0-9.]+) s", closing).group(1)), "passes": len(per_pass),
               "copies": sum(int(m[1]) for m in per_pass), "verdicts_decided_by_the_host": sum(int(m[3]) for m in per_pass),
               "verdicts": int(re.search(r"of (\d+) verdicts", closing).group(1)), "closing_line": closing}
        out["ms_per_copy"] = round(1e3 * out["stage_s"] / max(1, out["copies"]), 3)
        return out
    run("warm", "--spikeScan=" + text, "--spikeScanReps=2", "--spikeScanStride=%d" % stride, "--spikeScanIndel=" + RULE)
    run("warm", "--spikeScan=" + text, "--spikeScanReps=2", "--spikeScanStride=%d" % stride)
    indel, plain_scan, without, logs = [], [], [], {}
    for _ in range(REPEATS):
        t, logs["indel"] = run("indel", *(scan + ["--spikeScanIndel=" + RULE]))
        indel.append(t)
        t, logs["snv"] = run("snv", *scan)
        plain_scan.append(t)
        without.append(run("plain")[0])
    res = {"reps": n_reps, "stride": stride, "repetitions": REPEATS, "rule": RULE, "indel_scan": figures(indel, logs["indel"]),
           "snv_scan_same_tree": figures(plain_scan, logs["snv"]), "without_either_s": round(statistics.median(without), 3)}
    res["indel_over_snv_stage"] = round(res["indel_scan"]["stage_s"] / max(1e-9, res["snv_scan_same_tree"]["stage_s"]), 2)
    return res


def one_batch(eng, bam_path, fa_path, loci, P, stride):
    """(b)"""
    ref = fasta.FastaFile(fa_path)
    variants, _ = lists.scan_indels([(c, str(p)) for c, p in loci], ref, lists.parse_indel_rule(RULE))
    mine = [v for v in variants if v.pos % stride == 0]
    chrom = mine[0].chrom
    lo, hi = min(p for _, p in loci) - 1, max(p for _, p in loci)
    bam = bamio.NativeBam(bam_path)
    A = bam.alignments_run(chrom, lo, hi, 128_000_000, P, bamio.host_threads())
    nl = int(A["nl"])
    run = devplanes.AfRun(chrom, lo, hi, list(range(len(mine))), nl, bam=bam)
    run.A, run.run_ref = A, ref.fetch(chrom, lo, lo + nl).upper()
    run.idents, run.mism, run.up = bam.barcode_idents(A["n_bc"]), bam.run_mismatches(len(A["aln"])), devplanes.upload_run(eng, A, run.run_ref)
    spikes = devplanes.SpikeSet(mine, indels=True)
    svar, _ = spikes.chrom_variants(chrom, TARGETS[0])
    var, ins = devplanes.af_run_variants(mine, chrom, lo, ref)
    seeds = [SEED + j for j in range(COPIES)]
    made = devplanes.spike_indel_run_copies(eng, run.up, A, svar, spikes.ins[chrom], run.idents, seeds, [sv.threshold(TARGETS[0])] * COPIES,
                                            P.mismatchThr, run.mism[0], run.mism[1])
    sa, sb, sc = made["strides"]
    runs = [devplanes.RunOnDevice(devplanes._BufView(made["aln"], c * sa), devplanes._BufView(made["cig"], c * sc),
                                  devplanes._BufView(made["bq"], c * sb), run.up.loc, run.up.ref, run.up.n_aln, run.up.loc_host,
                                  pairs_used=int(made["totals"][c, 0])) for c in range(COPIES)]
    xcap = devplanes.build_xcap(nl)
    d_x, d_cnt = DevBuf(eng, 20 * xcap * COPIES + 256), DevBuf(eng, 8 * COPIES + 256)
    rows = np.zeros(COPIES * nl, abi.ROW_DTYPE)
    d_rows = DevBuf(eng, rows.nbytes + 256).upload(rows.view(np.uint8).reshape(-1))
    max_depth = eng.L.smc_build_max_depth()
    thr = 17
    sync = lambda: eng.L.smc_device_sync(eng.ctx)

    def kept(copy):
        return (devplanes._KeptRun(runs[c], A, None, A, bam.allele_key, bam.barcode_name, lambda n: run.idents, copy=runs[c] if copy else None)
                for c in range(COPIES))

    def on_device():
        extras = [devplanes.BuildExtras(devplanes._BufView(d_x, 20 * xcap * c), devplanes._BufView(d_cnt, 8 * c)) for c in range(COPIES)]
        d = devplanes._build_copies(eng, run, COPIES, kept(False), P, 32, "perf", ref, max_depth, "reference", 0, extras)
        try:
            return devplanes.scan_detect_keys(
                eng, d_rows, COPIES, nl, var, ins,
                dict(aln=made["aln"].data_ptr(), cig=made["cig"].data_ptr(), bq=made["bq"].data_ptr(), strides=(sa, sb, sc),
                     n_aln=run.up.n_aln, cap_pairs=made["caps"][0]),
                dict(x=d_x.data_ptr(), cnt=d_cnt.data_ptr(), x_stride=5 * xcap, cnt_stride=2, xcap=xcap), thr)[2], sum(e.n for e in extras)
        finally:
            d.free()

    def eager():
        d = devplanes._build_copies(eng, run, COPIES, kept(True), P, 32, "perf", ref, max_depth, "reference", 0)
        try:
            ids = np.zeros((COPIES, len(mine)), np.uint32)
            for c in range(COPIES):
                for g, v in enumerate(mine):
                    table = d.tables[c * nl + v.pos - 1 - lo]
                    ids[c, g] = table.index(v.key) if v.key in table else abi.SCAN_ID_NONE
            return ids
        finally:
            d.free()

    def median_ms(fn):
        fn(); sync()
        times = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            fn(); sync()
            times.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(times), 3)
    try:
        ids, n_extras = on_device()
        out = {"copies": COPIES, "loci_per_copy": nl, "listed": len(mine), "records_per_copy": int(run.up.n_aln), "extras_entries": int(n_extras),
               "keys_resolved": int((ids < abi.SCAN_ID_HOST).sum()), "ids_equal_the_eager_tables": bool(np.array_equal(ids, eager())),
               "builds_with_extras_in_hbm_and_scan_detect_keys_ms": median_ms(on_device),
               "builds_with_eager_tables_through_copy_allele_key_ms": median_ms(eager)}
        out["eager_over_device"] = round(out["builds_with_eager_tables_through_copy_allele_key_ms"] /
                                         max(1e-9, out["builds_with_extras_in_hbm_and_scan_detect_keys_ms"]), 2)
        return out
    finally:
        for b in (d_x, d_cnt, d_rows, made["aln"], made["bq"], made["cig"]):
            b.free()
        run.free()


def trees(parent, args):
    """(c)"""
    if not parent:
        return {"note": "no parent tree given: not measured"}
    out = {"this_tree": [], "parent_tree": [], "runs_each": TREE_RUNS}
    for _ in range(TREE_RUNS):
        for name, root in (("this_tree", ROOT), ("parent_tree", parent)):
            text = subprocess.check_output([sys.executable, os.path.join(root, "scripts", "spike_scan_perf.py")] + args, cwd=root,
                                           env=dict(os.environ, PYTHONPATH=root)).decode()
            w = json.loads(text.strip().splitlines()[-1])["wall"]
            out[name].append({"with_spikeScan_s": w["with_spikeScan_s"], "with_spikeScan_all_s": w["with_spikeScan_all_s"], "stage_s": w["stage_s"]})
    for name in ("this_tree", "parent_tree"):
        every = [x for r in out[name] for x in r["with_spikeScan_all_s"]]
        out[name + "_median_s"], out[name + "_min_max_s"] = round(statistics.median(every), 3), [min(every), max(every)]
    return out


def main():
    a = sys.argv[1:]
    out_path = a[0] if a else None
    parent = os.path.abspath(a[1]) if len(a) > 1 and a[1] not in ("", "-") else None
    n_loci, n_umi, rpb, n_reps, stride = (int(a[k]) if len(a) > k else d for k, d in ((2, 128), (3, 2000), (4, 10), (5, 32), (6, 16)))
    cfg = synth.SynthConfig("SPS", n_loci, n_umi, rpb, 20170502, alt_locus_frac=0.3, alt_af=0.1)
    tmp = tempfile.mkdtemp()
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, n_loci)
    bed = ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci)
    res = {"targets": list(TARGETS), "file": {"loci": n_loci, "barcodes_per_locus": n_umi, "reads_per_barcode": rpb, "records": len(A["aln"])}}
    eng = Engine(0)
    res["one_batch"] = one_batch(eng, bam, fa, loci, P, stride)
    eng.close()
    res["wall"] = wall(tmp, bam, fa, bed, P, n_reps, stride)
    res["snv_scan_on_both_trees"] = trees(parent, [str(x) for x in (n_loci, n_umi, rpb, n_reps, stride)])
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
