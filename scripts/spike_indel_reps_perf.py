"""Cost of --spikeIndelReps (dev tool, GPU box).

On scripts/spike_reps_perf.py's shape (a synthetic BAM, `n_umi` barcodes x `rpb` reads per locus, four listed variants of which two
are an insertion and a deletion, three targets), wall time in process, after a warm-up run, the median of `REPEATS` alternating
repetitions of
(a) a run with --spikeAF and --spikeIndelReps R,
(b) the same run with --spikeIndels in its place,
and (c) the workflow the flag replaces: the command line of (b) run R times with --dsSeed s_j, the sum of the R walls (each run once);
(d) the replicate stage's parts from the run's own clock, and its time per replicate and target; (e) device synchronised around each,
one smc_spike_indels_reps call of B copies against B devplanes.spike_indel_run calls over the run that holds the listed variants, one
smc_spike_indel_touch call and one smc_spike_indel_counts call.  The replicate lines of (a) are compared with the detection lines of
the runs of (c).

usage: spike_indel_reps_perf.py [n_loci] [n_umi] [rpb] [reps] [out.json]   -> one JSON line (also written to out.json when given)"""
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
import spike_indel_restate  # noqa: E402
from smcounter_amd import bamio, cli, devplanes, dsaf, fasta, synth  # noqa: E402
from smcounter_amd.engine import Engine  # noqa: E402
from smcounter_amd.tools import spike_variants as sv  # noqa: E402

TARGETS = (0.05, 0.02, 0.01)
SEED = 1234567
REPEATS = 5


def kernels(eng, bam, fa, variants, P, n_reps, copies=16):
    """(e): the batched rewrite against single calls over the pre-pass's run, and the counts call."""
    keep = {}
    devplanes.spike_rules(bam, fasta.FastaFile(fa), variants, list(TARGETS), [P] * len(TARGETS), SEED, eng, keep=keep, indel_counters=True)
    run = keep["runs"][0]
    svar, _ = keep["spikes"].chrom_variants(run.chrom, TARGETS[0])
    caps = devplanes.spike_indel_caps(run.A, svar)
    ins = keep["spikes"].ins[run.chrom]
    seeds = dsaf.rep_seeds(SEED, copies)
    thr = sv.threshold(TARGETS[0])
    sync = lambda: eng.L.smc_device_sync(eng.ctx)

    def batched():
        made = devplanes.spike_indel_run_copies(eng, run.up, run.A, svar, ins, run.idents, seeds, [thr] * copies, P.mismatchThr, *run.mism)
        for k in ("aln", "bq", "cig"):
            made[k].free()

    def singles():
        for s in seeds:
            out = devplanes.spike_indel_run(eng, run.up, run.A, svar, ins, run.idents, s, P.mismatchThr, *run.mism, mism=False)[0]
            devplanes.free_spiked(out, run.up)

    def counts():
        devplanes.spike_indel_counts(eng, [v.pos for v in variants], keep["covers"], keep["counters"], dsaf.rep_seeds(SEED, n_reps),
                                     [sv.threshold(t) for t in TARGETS])

    def touch():
        devplanes.spike_indel_touch(eng, run.up, run.A, svar)

    def median_ms(fn):
        fn(); sync()                                              # (warm-up)
        times = []
        for _ in range(REPEATS):
            t0 = time.perf_counter()
            fn(); sync()
            times.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(times), 4)
    out = {"copies": copies, "run_alignments": int(run.up.n_aln), "run_pool_bytes": int(len(run.A["bq"])), "run_barcodes": int(run.A["n_bc"]),
           "covering_barcodes": int(sum(len(c) for c in keep["covers"])), "copy_capacity_pairs": int(caps[0]), "copy_capacity_cigar_words": int(caps[1])}
    # (both include their uploads of the variants, identities and NM arrays and the copy back of the statistics and totals; the single
    # calls take every variant at the same threshold, as the copies do; alternated)
    a, b = [], []
    for _ in range(3):
        a.append(median_ms(batched)); b.append(median_ms(singles))
    out.update(one_call_of_copies_ms=statistics.median(a), single_calls_ms=statistics.median(b), counts_call_ms=median_ms(counts), touch_call_ms=median_ms(touch))
    out["single_over_batched"] = round(out["single_calls_ms"] / out["one_call_of_copies_ms"], 2)
    devplanes.free_af_runs(keep["runs"])
    return out


def wall(tmp, bam, fa, bed, vfile, P, n_reps, n_var):
    base = ["--bedTarget=%s" % bed, "--mtDepth=%d" % P.mtDepth, "--rpb=%g" % P.rpb, "--refGenome=%s" % fa, "--bamFile=%s" % bam,
            "--spikeAF=" + ",".join("%g" % t for t in TARGETS), "--spikeVariants=%s" % vfile]
    parser = cli.build_parser()

    def run(prefix, *extra):
        log = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(log):
            cli.main(parser.parse_args(base + ["--outPrefix=%s" % os.path.join(tmp, prefix)] + list(extra)))
        return time.perf_counter() - t0, log.getvalue()
    run("warm", "--dsSeed=%d" % SEED, "--spikeIndelReps=2")
    with_, without, log = [], [], None
    for _ in range(REPEATS):
        t, log = run("reps", "--dsSeed=%d" % SEED, "--spikeIndelReps=%d" % n_reps)
        with_.append(t)
        without.append(run("plain", "--dsSeed=%d" % SEED, "--spikeIndels")[0])
    t_reps, t_plain = statistics.median(with_), statistics.median(without)
    stage = re.search(r"--spikeReps: replicate stage ([0-9.]+) s \((.*)\)", log)
    res = {"reps": n_reps, "repetitions": REPEATS, "with_spikeIndelReps_s": round(t_reps, 3), "with_spikeIndels_s": round(t_plain, 3),
           "with_spikeIndelReps_all_s": [round(x, 3) for x in with_], "with_spikeIndels_all_s": [round(x, 3) for x in without],
           "flag_costs_s": round(t_reps - t_plain, 3), "replicate_stage_s": float(stage.group(1)), "replicate_stage": stage.group(2),
           "replicate_stage_ms_per_replicate_and_target": round(1e3 * float(stage.group(1)) / (n_reps * len(TARGETS)), 3)}
    reps = [l.split("\t") for l in open(os.path.join(tmp, "reps.spikeAF.replicates.txt")).read().splitlines()[1:]]
    total, same, compared = 0.0, True, 0
    for j, s in enumerate(dsaf.rep_seeds(SEED, n_reps)):
        t, _ = run("seed%d" % j, "--dsSeed=%d" % s, "--spikeIndels")
        total += t
        det = [l.split("\t") for l in open(os.path.join(tmp, "seed%d.spikeAF.detection.txt" % j)).read().splitlines()[1:]]
        for i in range(n_var):
            for k in range(len(TARGETS)):
                mine = reps[(i * len(TARGETS) + k) * n_reps + j]
                same &= mine[:5] + mine[7:] == det[i * (1 + len(TARGETS)) + 1 + k]
                compared += 1
    res.update(separate_runs_sum_s=round(total, 3), separate_runs_over_flag_cost=round(total / max(1e-9, t_reps - t_plain), 2),
               lines_compared=compared, replicates_equal_the_separate_runs=bool(same))
    return res


def main():
    a = sys.argv[1:]
    n_loci = int(a[0]) if a else 128
    n_umi = int(a[1]) if len(a) > 1 else 2000
    rpb = int(a[2]) if len(a) > 2 else 10
    n_reps = int(a[3]) if len(a) > 3 else 32
    cfg = synth.SynthConfig("SIR", n_loci, n_umi, rpb, 20170502, alt_locus_frac=0.3, alt_af=0.1)
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, n_loci)
    bed = ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci)
    # (pick_variants gives an insertion of two letters, a deletion of three, an SNV and an insertion of one letter: the third indel by
    # position is made an SNV, so that two of the four are indels)
    variants, n_indels = [], 0
    for v in spike_indel_restate.pick_variants(bam, fa, loci[n_loci // 2:n_loci // 2 + 48], 4, gap=8):
        n_indels += len(v.ref) != len(v.alt)
        if len(v.ref) != len(v.alt) and n_indels > 2:
            v = spike_indel_restate.variant(v.chrom, v.pos, v.ref[0], "ACGT"[("ACGT".index(v.ref[0]) + 1) % 4])
        variants.append(v)
    vfile = ds_af_restate.write_variants(os.path.join(tmp, "v.txt"), variants)
    res = {"targets": list(TARGETS), "file": {"loci": n_loci, "barcodes_per_locus": n_umi, "reads_per_barcode": rpb, "records": len(A["aln"]),
                                              "variants": ["%s:%d %s>%s" % (v.chrom, v.pos, v.ref, v.alt) for v in variants],
                                              "make_s": round(time.perf_counter() - t0, 1)}}
    eng = Engine(0)
    res["kernels"] = kernels(eng, bam, fa, sv.parse_variants(vfile, "v.txt", indels=True), P, n_reps)
    eng.close()
    res["wall"] = wall(tmp, bam, fa, bed, vfile, P, n_reps, len(variants))
    line = json.dumps(res)
    print(line)
    if len(a) > 4:
        with open(a[4], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
