"""Cost of --dsAFReps (dev tool, GPU box).

On scripts/ds_af_perf.py's input (a synthetic BAM, `n_umi` barcodes x `rpb` reads per locus, four listed planted variants, three
targets), wall time in process of
(1) a run with --dsAF and --dsAFReps R,
(2) the same run without --dsAFReps,
(3) the baseline the flag replaces: the command line of (2) run R times with --dsSeed s_j, the sum of the R walls,
and, device synchronised around each loop, the time of one smc_af_rep_counts call over the file's sets and of one smc_af_rep_masks
call over the run that holds the listed variants; the replicate stage's time per (j, t) from the run's own clock.  The replicate
lines of (1) are compared with the detection lines of the runs of (3).

usage: ds_af_reps_perf.py [n_loci] [n_umi] [rpb] [reps] [out.json]   -> one JSON line (also written to out.json when given)"""
import contextlib
import io
import json
import os
import re
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402

import ds_af_restate  # noqa: E402
import ds_restate  # noqa: E402
from smcounter_amd import bamio, cli, devplanes, dsaf, fasta, synth  # noqa: E402
from smcounter_amd.engine import DevBuf, Engine  # noqa: E402
from smcounter_amd.tools import ds_allele_fraction as af  # noqa: E402

TARGETS = (0.05, 0.02, 0.01)
SEED = 1234567


def kernels(eng, bam, fa, variants, P, n_reps, loops=20):
    ref = fasta.FastaFile(fa)
    covers, carries = devplanes.ds_af_sets(bam, ref, variants, P, eng)
    res = af.titrate(covers, carries, list(TARGETS), SEED)
    idents, thr = dsaf.carrier_table(carries, [[row["thr"] for row in r["rows"]] for r in res])
    tab = devplanes.AfRepTable(eng, idents, thr, dsaf.rep_seeds(SEED, n_reps))
    lo, hi = min(v.pos for v in variants) - 1, max(v.pos for v in variants)
    b = bamio.NativeBam(bam)
    A = b.alignments_run(variants[0].chrom, lo, hi, 1 << 40, P, 0)
    run_idents = b.barcode_idents(A["n_bc"])
    b.close()
    n = len(run_idents)
    n_words = devplanes.mask_words(n)
    d_id = DevBuf(eng, 8 * n + 256).upload(run_idents)
    d_m = DevBuf(eng, 4 * n_reps * len(TARGETS) * n_words + 256)
    out = {"carriers": int(len(idents)), "covering_barcodes": int(sum(len(np.unique(c)) for c in covers)), "run_barcodes": n}
    tab.counts(covers, carries)                                                    # (warm-up)
    eng.L.smc_device_sync(eng.ctx)
    t0 = time.perf_counter()
    for _ in range(loops):
        tab.counts(covers, carries)                                                # (uploads the sets, returns after its copy back)
    out["counts_call_ms"] = round((time.perf_counter() - t0) * 1e3 / loops, 4)
    tab.masks(d_id.data_ptr(), n, d_m.data_ptr(), n_words)
    eng.L.smc_device_sync(eng.ctx)
    t0 = time.perf_counter()
    for _ in range(loops):
        tab.masks(d_id.data_ptr(), n, d_m.data_ptr(), n_words)
    eng.L.smc_device_sync(eng.ctx)
    out["masks_call_ms"] = round((time.perf_counter() - t0) * 1e3 / loops, 4)
    for x in (d_id, d_m):
        x.free()
    tab.free()
    return out


def wall(tmp, bam, fa, bed, vfile, P, n_reps, n_var):
    base = ["--bedTarget=%s" % bed, "--mtDepth=%d" % P.mtDepth, "--rpb=%g" % P.rpb, "--refGenome=%s" % fa, "--bamFile=%s" % bam,
            "--dsAF=" + ",".join("%g" % t for t in TARGETS), "--dsAFVariants=%s" % vfile]
    parser = cli.build_parser()

    def run(prefix, *extra):
        log = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(log):
            cli.main(parser.parse_args(base + ["--outPrefix=%s" % os.path.join(tmp, prefix)] + list(extra)))
        return round(time.perf_counter() - t0, 3), log.getvalue()
    run("warm", "--dsSeed=%d" % SEED)
    t_reps, log = run("reps", "--dsSeed=%d" % SEED, "--dsAFReps=%d" % n_reps)
    t_plain, _ = run("plain", "--dsSeed=%d" % SEED)
    stage = re.search(r"--dsAFReps: replicate stage ([0-9.]+) s \((.*)\)", log)
    res = {"reps": n_reps, "with_dsAFReps_s": t_reps, "without_dsAFReps_s": t_plain, "replicate_stage_s": float(stage.group(1)),
           "replicate_stage": stage.group(2), "replicate_stage_ms_per_replicate_and_target": round(1e3 * float(stage.group(1)) / (n_reps * len(TARGETS)), 3)}
    reps = [l.split("\t") for l in open(os.path.join(tmp, "reps.dsAF.replicates.txt")).read().splitlines()[1:]]
    total, same, compared = 0.0, True, 0
    for j, s in enumerate(dsaf.rep_seeds(SEED, n_reps)):
        t, _ = run("seed%d" % j, "--dsSeed=%d" % s)
        total += t
        det = [l.split("\t") for l in open(os.path.join(tmp, "seed%d.dsAF.detection.txt" % j)).read().splitlines()[1:]]
        for i in range(n_var):
            for k in range(len(TARGETS)):
                mine = reps[(i * len(TARGETS) + k) * n_reps + j]
                same &= mine[:5] + mine[7:] == det[i * (1 + len(TARGETS)) + 1 + k]
                compared += 1
    res.update(baseline_runs_sum_s=round(total, 3), baseline_over_with=round(total / t_reps, 2), lines_compared=compared,
               replicates_equal_the_separate_runs=bool(same))
    return res


def main():
    a = sys.argv[1:]
    n_loci = int(a[0]) if a else 128
    n_umi = int(a[1]) if len(a) > 1 else 2000
    rpb = int(a[2]) if len(a) > 2 else 10
    n_reps = int(a[3]) if len(a) > 3 else 32
    cfg = synth.SynthConfig("AFP", n_loci, n_umi, rpb, 20170502, alt_locus_frac=0.3, alt_af=0.1)
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, n_loci)
    bed = ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci)
    listed = ds_af_restate.planted(bam, fa, loci[n_loci // 2:n_loci // 2 + 24], min_frac=0.05, limit=4)
    vfile = ds_af_restate.write_variants(os.path.join(tmp, "v.txt"), listed)
    variants = af.parse_variants(vfile)
    res = {"targets": list(TARGETS), "file": {"loci": n_loci, "barcodes_per_locus": n_umi, "reads_per_barcode": rpb, "records": len(A["aln"]),
                                              "variants": ["%s:%d %s>%s" % (v.chrom, v.pos, v.ref, v.alt) for v in variants],
                                              "make_s": round(time.perf_counter() - t0, 1)}}
    eng = Engine(0)
    res["kernels"] = kernels(eng, bam, fa, variants, P, n_reps)
    eng.close()
    res["wall"] = wall(tmp, bam, fa, bed, vfile, P, n_reps, len(variants))
    line = json.dumps(res)
    print(line)
    if len(a) > 4:
        with open(a[4], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
