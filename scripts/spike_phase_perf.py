"""Cost of --spikePhase (dev tool, GPU box).

On scripts/spike_perf.py's input (a synthetic BAM, `n_umi` barcodes x `rpb` reads per locus, four listed SNVs, three targets) with two
of the four positions made one phase set (a PS= entry), wall time in process, after a warm-up, the median of `REPEATS` alternating
repetitions of
(a) device synchronised around it, one smc_spike_phase_counts call over all (set, replicate, target, fraction) beside one
    smc_spike_depth_counts call over all (variant, replicate, target, fraction), both with their uploads and the copy back;
(b) one smc_spike_alleles_reps call of 16 copies on the pre-pass's run with the set's `lead` filled, beside the same call with lead =
    0 everywhere (k_spike_rewrite makes one more load per record of a set);
(c) a run with --spikeAF and --spikePhase beside the same run without --spikePhase.

usage: spike_phase_perf.py [n_loci] [n_umi] [rpb] [reps] [out.json]   -> one JSON line (also written to out.json when given)"""
import contextlib
import io
import json
import os
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
from smcounter_amd import cli, devplanes, dsaf, fasta, synth  # noqa: E402
from smcounter_amd.engine import Engine  # noqa: E402
from smcounter_amd.tools import spike_variants as sv  # noqa: E402

TARGETS = (0.05, 0.02, 0.01)
FRACS = (0.5, 0.25, 0.1)
SEED = 1234567
REPEATS = 5
COPIES = 16


def _median_ms(fn, sync):
    fn(); sync()                                                  # (warm-up)
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn(); sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times)


def kernels(eng, bam, fa, variants, P, n_reps):
    keep, phase = {}, dict(sets=sv.phase_sets(variants))
    devplanes.spike_rules(bam, fasta.FastaFile(fa), variants, list(TARGETS), [P] * len(TARGETS), SEED, eng, keep=keep, phase=phase)
    sync = lambda: eng.L.smc_device_sync(eng.ctx)
    spikes = keep["spikes"]
    seeds, thr = dsaf.rep_seeds(SEED, n_reps), [sv.threshold(t) for t in TARGETS]
    dthr = [devplanes.frac_threshold(f) for f in FRACS]
    lead = [spikes.lead_pos[s.members[0]] for s in phase["sets"]]
    a, b = [], []
    for _ in range(3):                                            # (alternated)
        a.append(_median_ms(lambda: devplanes.spike_phase_counts(eng, lead, phase["joint"], seeds, thr, dthr), sync))
        b.append(_median_ms(lambda: devplanes.spike_depth_counts(eng, spikes.lead_pos, keep["covers"], keep["counters"], seeds, thr, dthr), sync))
    out = {"joint_barcodes": int(sum(len(ids) for ids, _ in phase["joint"])), "covering_barcodes": int(sum(len(c) for c in keep["covers"])),
           "phase_counts_call_ms": round(statistics.median(a), 4), "depth_counts_call_ms": round(statistics.median(b), 4)}
    run = keep["runs"][0]
    svar, _ = spikes.chrom_variants(run.chrom, TARGETS[0])
    flat = svar.copy()
    flat["lead"] = 0

    def copies(var):
        d_aln, d_bq, _, _ = devplanes.spike_run_copies(eng, run.up, run.A, var, run.idents, seeds[:COPIES] if n_reps >= COPIES else
                                                       dsaf.rep_seeds(SEED, COPIES), [thr[0]] * COPIES, P.mismatchThr, run.mism[0], run.mism[1])
        d_aln.free(); d_bq.free()
    a, b = [], []
    for _ in range(3):
        a.append(_median_ms(lambda: copies(svar), sync))
        b.append(_median_ms(lambda: copies(flat), sync))
    out.update(alignments=int(run.up.n_aln), pair_pool_bytes=int(len(run.A["bq"])), copies=COPIES,
               alleles_reps_with_lead_ms=round(statistics.median(a), 4), alleles_reps_lead_zero_ms=round(statistics.median(b), 4))
    devplanes.free_af_runs(keep["runs"])
    return out


def wall(tmp, bam, fa, bed, vfile, P):
    base = ["--bedTarget=%s" % bed, "--mtDepth=%d" % P.mtDepth, "--rpb=%g" % P.rpb, "--refGenome=%s" % fa, "--bamFile=%s" % bam,
            "--spikeAF=" + ",".join("%g" % t for t in TARGETS), "--spikeVariants=%s" % vfile, "--dsSeed=%d" % SEED]
    parser = cli.build_parser()

    def run(prefix, *extra):
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            cli.main(parser.parse_args(base + ["--outPrefix=%s" % os.path.join(tmp, prefix)] + list(extra)))
        return time.perf_counter() - t0
    run("warm", "--spikePhase")
    with_, without = [], []
    for _ in range(REPEATS):
        with_.append(run("phase", "--spikePhase"))
        without.append(run("plain"))
    return {"repetitions": REPEATS, "with_spikePhase_s": round(statistics.median(with_), 3), "without_spikePhase_s": round(statistics.median(without), 3),
            "with_spikePhase_all_s": [round(x, 3) for x in with_], "without_spikePhase_all_s": [round(x, 3) for x in without],
            "flag_costs_s": round(statistics.median(with_) - statistics.median(without), 3),
            "phase_page_written": os.path.exists(os.path.join(tmp, "phase.spikeAF.phase.txt"))}


def main():
    a = sys.argv[1:]
    n_loci = int(a[0]) if a else 128
    n_umi = int(a[1]) if len(a) > 1 else 2000
    rpb = int(a[2]) if len(a) > 2 else 10
    n_reps = int(a[3]) if len(a) > 3 else 32
    cfg = synth.SynthConfig("SPP", n_loci, n_umi, rpb, 20170502, alt_locus_frac=0.3, alt_af=0.1)
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, n_loci)
    bed = ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci)
    picked = spike_restate.pick_positions(bam, fa, loci[n_loci // 2:n_loci // 2 + 24], 4)
    vfile = os.path.join(tmp, "v.vcf")
    with open(vfile, "w") as fh:                                  # (the first two positions are one set, the others singletons)
        for k, v in enumerate(picked):
            fh.write("%s\t%d\t.\t%s\t%s\t.\t.\t%s\n" % (v.chrom, v.pos, v.ref, v.alt, "PS=hap" if k < 2 else "."))
    variants = sv.parse_variants(vfile, "v.vcf", phased=True)
    res = {"targets": list(TARGETS), "fractions": list(FRACS), "reps": n_reps,
           "file": {"loci": n_loci, "barcodes_per_locus": n_umi, "reads_per_barcode": rpb, "records": len(A["aln"]),
                    "variants": ["%s:%d %s>%s" % (v.chrom, v.pos, v.ref, v.alt) for v in variants],
                    "sets": [[variants[k].pos for k in s.members] for s in variants.sets], "make_s": round(time.perf_counter() - t0, 1)}}
    eng = Engine(0)
    res["kernels"] = kernels(eng, bam, fa, variants, P, n_reps)
    eng.close()
    res["wall"] = wall(tmp, bam, fa, bed, vfile, P)
    line = json.dumps(res)
    print(line)
    if len(a) > 4:
        with open(a[4], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
