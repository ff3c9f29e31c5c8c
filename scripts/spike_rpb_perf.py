"""Cost of --spikeRpb (dev tool, GPU box).

On scripts/spike_depth_perf.py's input (a synthetic BAM, `n_umi` barcodes x `rpb` reads per locus, four listed SNVs, three targets), with
three reads-per-barcode targets in place of the barcode fractions, wall time in process, after a warm-up run, the median of `REPEATS`
alternating repetitions of
(a) a run with --spikeAF, --spikeReps R and --spikeRpb,
(b) the same run without --spikeRpb;
(c) the replicate stage of (a) and of (b) from the run's own clock; (d) device synchronised around it, one smc_spike_read_bits call
over the pre-pass's run and one smc_spike_rpb_counts call over all (variant, replicate, target, reads-per-barcode target), beside one
smc_spike_depth_counts call of the same shape, each with its uploads and the copy back; (e) the offline workflow the flag replaces, for
the (target, seed) pairs of `OFFLINE` - tools.spike_variants --af t --seed s, then the command line with --dsRpb r1,r2,..
--dsRpbSampler philox --dsSeed s on its output - timed once each and scaled to the T x R pairs of (a).  The cells' files of (a) are
compared with the workflow's for seed s_0.

usage: spike_rpb_perf.py [n_loci] [n_umi] [rpb] [reps] [out.json]   -> one JSON line (also written to out.json, default
profiles/spike_rpb_perf.json)"""
import argparse
import contextlib
import io
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ds_af_restate  # noqa: E402
import ds_restate  # noqa: E402
import spike_restate  # noqa: E402
from smcounter_amd import bamio, cli, devplanes, dsaf, fasta, synth  # noqa: E402
from smcounter_amd.engine import Engine  # noqa: E402
from smcounter_amd.tools import spike_variants as sv  # noqa: E402

TARGETS = (0.05, 0.02, 0.01)
RPBS = (5, 3, 1.5)
SEED = 1234567
REPEATS = 5
OFFLINE = ((0.05, 0), (0.01, 0), (0.02, 1))      # (target, replicate) pairs the offline workflow is timed on
SUFFIXES = (".smCounter.all.txt", ".smCounter.cut.txt", ".smCounter.cut.vcf")


def kernels(eng, bam, fa, variants, P, n_reps):
    """(d): the two entries over what the pre-pass keeps."""
    keep, rpb = {}, dict(targets=list(RPBS), params=[P] * (len(TARGETS) * len(RPBS)))
    fasta_file = fasta.FastaFile(fa)
    devplanes.spike_rules(bam, fasta_file, variants, list(TARGETS), [P] * len(TARGETS), SEED, eng, keep=keep, rpb=rpb)
    sync = lambda: eng.L.smc_device_sync(eng.ctx)
    pos, seeds, thr = [v.pos for v in variants], dsaf.rep_seeds(SEED, n_reps), [sv.threshold(t) for t in TARGETS]
    rthr = [r.thr for r in rpb["rules"][:len(RPBS)]]
    run = keep["runs"][0]
    var, _ = devplanes.af_run_variants([variants[k] for k in run.group], run.chrom, run.lo, fasta_file)

    def median_ms(fn):
        fn(); sync()                                              # (warm-up)
        times = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            fn(); sync()
            times.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(times), 4)
    out = {"covering_barcodes": int(sum(len(c) for c in keep["covers"])), "covering_records": int(sum(len(r[1]) for r in keep["records"])),
           "alignments_of_the_run": int(run.up.n_aln), "cells_counted": len(variants) * n_reps * len(TARGETS) * len(RPBS),
           "read_bits_call_ms": median_ms(lambda: devplanes.spike_read_bits(eng, run.up, run.A, run.lo, var)),
           "rpb_counts_call_ms": median_ms(lambda: devplanes.spike_rpb_counts(eng, pos, keep["covers"], keep["records"], seeds, thr, rthr)),
           "depth_counts_call_ms": median_ms(lambda: devplanes.spike_depth_counts(eng, pos, keep["covers"], keep["counters"], seeds, thr,
                                                                                  [1 << 32] * len(RPBS)))}
    devplanes.free_af_runs(keep["runs"])
    devplanes.close_rules(rpb["rules"])
    return out


def wall(tmp, bam, fa, bed, vfile, P, n_reps):
    base = ["--bedTarget=%s" % bed, "--mtDepth=%d" % P.mtDepth, "--rpb=%g" % P.rpb, "--refGenome=%s" % fa,
            "--spikeAF=" + ",".join("%g" % t for t in TARGETS), "--spikeVariants=%s" % vfile]
    text = ",".join("%g" % r for r in RPBS)
    parser = cli.build_parser()

    def run(prefix, *extra, src=bam, spike=True):
        log = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(log):
            cli.main(parser.parse_args((base if spike else base[:4]) + ["--bamFile=%s" % src, "--outPrefix=%s" % os.path.join(tmp, prefix)] + list(extra)))
        return time.perf_counter() - t0, log.getvalue()
    stage_of = lambda log: float(re.search(r"--spikeReps: replicate stage ([0-9.]+) s", log).group(1))
    run("warm", "--dsSeed=%d" % SEED, "--spikeReps=2", "--spikeRpb=%s" % text)
    with_, without, st_with, st_without = [], [], [], []
    for _ in range(REPEATS):
        t, log = run("cells", "--dsSeed=%d" % SEED, "--spikeReps=%d" % n_reps, "--spikeRpb=%s" % text)
        with_.append(t); st_with.append(stage_of(log))
        t, log = run("plain", "--dsSeed=%d" % SEED, "--spikeReps=%d" % n_reps)
        without.append(t); st_without.append(stage_of(log))
    t_with, t_without = statistics.median(with_), statistics.median(without)
    res = {"reps": n_reps, "repetitions": REPEATS, "with_spikeRpb_s": round(t_with, 3), "without_spikeRpb_s": round(t_without, 3),
           "with_spikeRpb_all_s": [round(x, 3) for x in with_], "without_spikeRpb_all_s": [round(x, 3) for x in without],
           "flag_costs_s": round(t_with - t_without, 3), "replicate_stage_with_s": statistics.median(st_with),
           "replicate_stage_without_s": statistics.median(st_without),
           "flag_ms_per_cell_and_replicate": round(1e3 * (t_with - t_without) / (n_reps * len(TARGETS) * len(RPBS)), 3)}
    # (e) the offline workflow on a stated subset of (target, seed) pairs, scaled to all T x R
    seeds = dsaf.rep_seeds(SEED, n_reps)
    total, same, compared = [], True, 0
    for t, j in OFFLINE:
        out = os.path.join(tmp, "off_%g_%d.bam" % (t, j))
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=seeds[j], refGenome=fa))
            if not os.path.exists(out + ".bai"):
                bamio.write_bai(out)
        t_tool = time.perf_counter() - t0
        prefix = "off.spikeAF%g.s%d" % (t, j)
        t_run, _ = run(prefix, "--dsRpb=%s" % text, "--dsRpbSampler=philox", "--dsSeed=%d" % seeds[j], src=out, spike=False)
        total.append(round(t_tool + t_run, 3))
        if j == 0:
            for r in RPBS:
                mine, theirs = os.path.join(tmp, "cells.spikeAF%g.dsRpb%g" % (t, r)), os.path.join(tmp, prefix + ".dsRpb%g" % r)
                for s in SUFFIXES:
                    same &= open(mine + s, "rb").read() == open(theirs + s, "rb").read().replace(theirs.encode(), mine.encode())
                    compared += 1
        os.remove(out)
    pairs = n_reps * len(TARGETS)
    res.update(offline_pairs=[list(p) for p in OFFLINE], offline_pair_s=total, offline_scaled_s=round(statistics.mean(total) * pairs, 1),
               offline_scaled_over_flag_cost=round(statistics.mean(total) * pairs / max(1e-9, t_with - t_without), 1),
               files_compared=compared, cells_equal_the_offline_workflow=bool(same))
    return res


def main():
    a = sys.argv[1:]
    n_loci = int(a[0]) if a else 128
    n_umi = int(a[1]) if len(a) > 1 else 2000
    rpb = int(a[2]) if len(a) > 2 else 10
    n_reps = int(a[3]) if len(a) > 3 else 32
    out_json = a[4] if len(a) > 4 else os.path.join(ROOT, "profiles", "spike_rpb_perf.json")
    cfg = synth.SynthConfig("SPP", n_loci, n_umi, rpb, 20170502, alt_locus_frac=0.3, alt_af=0.1)
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, n_loci)
    bed = ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci)
    variants = spike_restate.pick_positions(bam, fa, loci[n_loci // 2:n_loci // 2 + 24], 4)
    vfile = ds_af_restate.write_variants(os.path.join(tmp, "v.txt"), variants)
    res = {"targets": list(TARGETS), "rpb_targets": list(RPBS),
           "file": {"loci": n_loci, "barcodes_per_locus": n_umi, "reads_per_barcode": rpb, "records": len(A["aln"]),
                    "variants": ["%s:%d %s>%s" % (v.chrom, v.pos, v.ref, v.alt) for v in variants], "make_s": round(time.perf_counter() - t0, 1)}}
    eng = Engine(0)
    res["kernels"] = kernels(eng, bam, fa, sv.parse_variants(vfile, "v.txt"), P, n_reps)
    eng.close()
    res["wall"] = wall(tmp, bam, fa, bed, vfile, P, n_reps)
    line = json.dumps(res)
    print(line)
    with open(out_json, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
