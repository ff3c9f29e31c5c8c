"""Cost of --dsAFDepth (dev tool, GPU box).

On scripts/ds_af_perf.py's input (a synthetic BAM, `n_umi` barcodes x `rpb` reads per locus, four listed planted variants) with three
targets, three fractions and R replicates, wall time in process of
(1) a run with --dsAF, --dsAFReps R and --dsAFDepth,
(2) the same run without --dsAFDepth,
(3) the workflow the flag replaces, per target and seed: tools/ds_allele_fraction.py --af t --seed s_j (a BAM), then a
    --dsMT f1,f2,f3 --dsSampler philox --dsSeed s_j run on it.  Timed for a SUBSET - every target with the first `subset` seeds - and
    scaled to T x R pairs,
and, device synchronised around each loop, the time of one smc_af_depth_counts call over the file's sets and of one
smc_af_depth_masks call over the run that holds the listed variants; the replicate stage's time per (j, t, f) from the run's own
clock (the stage of (1) minus the stage of (2), over R x T x F).  The cells of (1) are compared with the .dsMT<f> files of (3) for
seed s_0.

usage: ds_af_depth_perf.py [n_loci] [n_umi] [rpb] [reps] [out.json] [subset]   -> one JSON line (also written to out.json when given)"""
import argparse
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
FRACS = (0.5, 0.25, 0.1)
SEED = 1234567
SUFFIXES = (".smCounter.all.txt", ".smCounter.cut.txt", ".smCounter.cut.vcf")


def kernels(eng, bam, fa, variants, P, n_reps, loops=20):
    ref = fasta.FastaFile(fa)
    covers, carries = devplanes.ds_af_sets(bam, ref, variants, P, eng)
    res = af.titrate(covers, carries, list(TARGETS), SEED)
    idents, thr = dsaf.carrier_table(carries, [[row["thr"] for row in r["rows"]] for r in res])
    tab = devplanes.AfDepthTable(eng, idents, thr, dsaf.rep_seeds(SEED, n_reps), [devplanes.frac_threshold(f) for f in FRACS])
    lo, hi = min(v.pos for v in variants) - 1, max(v.pos for v in variants)
    b = bamio.NativeBam(bam)
    A = b.alignments_run(variants[0].chrom, lo, hi, 1 << 40, P, 0)
    run_idents = b.barcode_idents(A["n_bc"])
    b.close()
    n = len(run_idents)
    n_words = devplanes.mask_words(n)
    d_id = DevBuf(eng, 8 * n + 256).upload(run_idents)
    d_m = DevBuf(eng, 4 * n_reps * len(TARGETS) * len(FRACS) * n_words + 256)
    out = {"carriers": int(len(idents)), "covering_barcodes": int(sum(len(np.unique(c)) for c in covers)), "run_barcodes": n,
           "masks_per_call": n_reps * len(TARGETS) * len(FRACS)}
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


def wall(tmp, bam, fa, bed, vfile, P, n_reps, subset):
    common = ["--bedTarget=%s" % bed, "--mtDepth=%d" % P.mtDepth, "--rpb=%g" % P.rpb, "--refGenome=%s" % fa]
    dil = ["--dsAF=" + ",".join("%g" % t for t in TARGETS), "--dsAFVariants=%s" % vfile]
    depth = ",".join("%g" % f for f in FRACS)
    parser = cli.build_parser()

    def run(prefix, in_bam, *extra):
        log = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(log):
            cli.main(parser.parse_args(common + ["--bamFile=%s" % in_bam, "--outPrefix=%s" % os.path.join(tmp, prefix)] + list(extra)))
        return round(time.perf_counter() - t0, 3), log.getvalue()
    stage = lambda log: float(re.search(r"--dsAFReps: replicate stage ([0-9.]+) s", log).group(1))
    run("warm", bam, "--dsSeed=%d" % SEED, *dil)
    t_with, log_with = run("o", bam, "--dsSeed=%d" % SEED, "--dsAFReps=%d" % n_reps, "--dsAFDepth=" + depth, *dil)
    mine = {(t, f): [open(os.path.join(tmp, "o.dsAF%g.dsMT%g%s" % (t, f, s)), "rb").read() for s in SUFFIXES] for t in TARGETS for f in FRACS}
    t_without, log_without = run("plain", bam, "--dsSeed=%d" % SEED, "--dsAFReps=%d" % n_reps, *dil)
    cells = n_reps * len(TARGETS) * len(FRACS)
    res = {"reps": n_reps, "with_dsAFDepth_s": t_with, "without_dsAFDepth_s": t_without, "replicate_stage_with_s": stage(log_with),
           "replicate_stage_without_s": stage(log_without),
           "replicate_stage_ms_per_replicate_and_cell": round(1e3 * (stage(log_with) - stage(log_without)) / cells, 3)}
    # the workflow the flag replaces, for every target and the first `subset` seeds
    t_tool = t_run = 0.0
    same, compared = True, 0
    for j, s in enumerate(dsaf.rep_seeds(SEED, n_reps)[:subset]):
        for t in TARGETS:
            out = os.path.join(tmp, "af%g.s%d.bam" % (t, j))
            t0 = time.perf_counter()
            with contextlib.redirect_stdout(io.StringIO()):
                af.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=s, refGenome=fa))
                bamio.write_bai(out)
            t_tool += time.perf_counter() - t0
            prefix = "o.dsAF%g" % t if j == 0 else "w%d.dsAF%g" % (j, t)
            t_run += run(prefix, out, "--dsMT=" + depth, "--dsSampler=philox", "--dsSeed=%d" % s)[0]
            if j == 0:
                for f in FRACS:
                    same &= mine[(t, f)] == [open(os.path.join(tmp, "%s.dsMT%g%s" % (prefix, f, x)), "rb").read() for x in SUFFIXES]
                    compared += 1
    pairs = subset * len(TARGETS)
    scale = float(n_reps * len(TARGETS)) / pairs
    res.update(workflow_subset="every target x the first %d of %d seeds (%d of %d target-seed pairs)" % (subset, n_reps, pairs, n_reps * len(TARGETS)),
               workflow_tool_s=round(t_tool, 3), workflow_runs_s=round(t_run, 3), workflow_scaled_to_all_pairs_s=round((t_tool + t_run) * scale, 3),
               workflow_over_with=round((t_tool + t_run) * scale / t_with, 2), cells_compared=compared,
               cells_equal_the_workflow=bool(same))
    return res


def main():
    a = sys.argv[1:]
    n_loci = int(a[0]) if a else 128
    n_umi = int(a[1]) if len(a) > 1 else 2000
    rpb = int(a[2]) if len(a) > 2 else 10
    n_reps = int(a[3]) if len(a) > 3 else 32
    subset = int(a[5]) if len(a) > 5 else 2
    cfg = synth.SynthConfig("AFP", n_loci, n_umi, rpb, 20170502, alt_locus_frac=0.3, alt_af=0.1)
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, n_loci)
    bed = ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci)
    listed = ds_af_restate.planted(bam, fa, loci[n_loci // 2:n_loci // 2 + 24], min_frac=0.05, limit=4)
    vfile = ds_af_restate.write_variants(os.path.join(tmp, "v.txt"), listed)
    variants = af.parse_variants(vfile)
    res = {"targets": list(TARGETS), "fractions": list(FRACS),
           "file": {"loci": n_loci, "barcodes_per_locus": n_umi, "reads_per_barcode": rpb, "records": len(A["aln"]),
                    "variants": ["%s:%d %s>%s" % (v.chrom, v.pos, v.ref, v.alt) for v in variants], "make_s": round(time.perf_counter() - t0, 1)}}
    eng = Engine(0)
    res["kernels"] = kernels(eng, bam, fa, variants, P, n_reps)
    eng.close()
    res["wall"] = wall(tmp, bam, fa, bed, vfile, P, n_reps, subset)
    res["not_measured"] = "a file at the example run's depth, R in the hundreds, listed variants spread over many runs, kernel counters"
    line = json.dumps(res)
    print(line)
    if len(a) > 4:
        with open(a[4], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
