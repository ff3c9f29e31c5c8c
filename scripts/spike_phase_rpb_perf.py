"""Cost of --spikePhaseRpb (dev tool, GPU box).

On scripts/spike_indel_reps_perf.py's input (a synthetic BAM, `n_umi` barcodes x `rpb` reads per locus, four listed variants of which
two are an insertion and a deletion, three targets) with its insertion and its first SNV made one phase set, the reads-per-barcode
targets 5 / 3 / 1.5, after a warm-up, medians of `REPEATS`:
(a) wall time in process of a run with --spikeAF, --spikeIndelReps R and --spikePhaseRpb on the list with PS=, alternating with the
    same run with --spikeIndelRpb on the list without PS=, and the replicate stage of both from the run's own clock;
(b) device synchronised around it, one smc_spike_phase_rpb_counts call over all (set, replicate, target, reads-per-barcode target)
    beside one smc_spike_indel_rpb_counts call over the set's members (the same draws: the leader's position).

usage: spike_phase_rpb_perf.py [n_loci] [n_umi] [rpb] [reps] [out.json]   -> one JSON line (also written to out.json, default
profiles/spike_phase_rpb_perf.json)"""
import contextlib
import io
import json
import os
import re
import statistics
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "tests"))

import ds_af_restate  # noqa: E402
import ds_restate  # noqa: E402
import spike_indel_phase_restate  # noqa: E402
import spike_indel_restate  # noqa: E402
from smcounter_amd import cli, devplanes, dsaf, fasta, synth  # noqa: E402
from smcounter_amd.engine import Engine  # noqa: E402
from smcounter_amd.tools import ds_allele_fraction as af  # noqa: E402
from smcounter_amd.tools import spike_variants as sv  # noqa: E402

TARGETS = (0.05, 0.02, 0.01)
RPBS = (5, 3, 1.5)
SEED = 1234567
REPEATS = 5


def median_ms(eng, fn):
    sync = lambda: eng.L.smc_device_sync(eng.ctx)
    fn(); sync()                                                  # (warm-up)
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn(); sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 4)


def kernels(eng, bam, fa, vfile, P, n_reps):
    """(b): the new entry over the set's (joint barcode, member) records beside smc_spike_indel_rpb_counts over its members."""
    variants = sv.parse_variants(vfile, "v.vcf", phased=True, indels=True)
    psets = sv.phase_sets(variants)
    keep, phase = {}, dict(sets=psets)
    rpb = dict(targets=list(RPBS), params=[P] * (len(TARGETS) * len(RPBS)), flag="--spikePhaseRpb")
    devplanes.spike_rules(bam, fasta.FastaFile(fa), variants, list(TARGETS), [P] * len(TARGETS), SEED, eng, keep=keep, rpb=rpb, indel_counters=True,
                          phase=phase)
    seeds, thr = dsaf.rep_seeds(SEED, n_reps), [sv.threshold(t) for t in TARGETS]
    rthr = [r.thr for r in rpb["rules"][:len(RPBS)]]
    lead = [keep["spikes"].lead_pos[s.members[0]] for s in psets]
    members = [k for s in psets for k in s.members]
    joint = phase["joint_records"]
    out = {"sets": len(psets), "members": len(members), "joint_barcodes": int(sum(len(j[0]) for j in joint)),
           "records_in_segments": int(sum(len(j[2]) for j in joint)),
           "covering_barcodes_of_the_members": int(sum(len(keep["covers"][k]) for k in members)),
           "covering_records_of_the_members": int(sum(len(keep["records"][k][1]) for k in members)),
           "cells_counted": len(psets) * n_reps * len(TARGETS) * len(RPBS),
           "phase_rpb_counts_call_ms": median_ms(eng, lambda: devplanes.spike_phase_rpb_counts(eng, lead, [len(s.members) for s in psets], joint,
                                                                                                seeds, thr, rthr)),
           "indel_rpb_counts_call_over_the_members_ms": median_ms(eng, lambda: devplanes.spike_rpb_counts(
               eng, [keep["spikes"].lead_pos[k] for k in members], [keep["covers"][k] for k in members], [keep["records"][k] for k in members],
               seeds, thr, rthr, four=True))}
    devplanes.free_af_runs(keep["runs"])
    devplanes.close_rules(rpb["rules"])
    return out


def wall(tmp, bam, fa, bed, with_sets, without_sets, P, n_reps):
    """(a)"""
    base = ["--bedTarget=%s" % bed, "--mtDepth=%d" % P.mtDepth, "--rpb=%g" % P.rpb, "--refGenome=%s" % fa, "--bamFile=%s" % bam,
            "--spikeAF=" + ",".join("%g" % t for t in TARGETS), "--dsSeed=%d" % SEED]
    text = ",".join("%g" % r for r in RPBS)
    parser = cli.build_parser()

    def run(prefix, *extra):
        log = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(log):
            cli.main(parser.parse_args(base + ["--outPrefix=%s" % os.path.join(tmp, prefix)] + list(extra)))
        return time.perf_counter() - t0, log.getvalue()
    stage_of = lambda log: float(re.search(r"--spikeReps: replicate stage ([0-9.]+) s", log).group(1))
    run("warm", "--spikeIndelReps=2", "--spikePhaseRpb=%s" % text, "--spikeVariants=%s" % with_sets)
    phased, plain, st_phased, st_plain = [], [], [], []
    for _ in range(REPEATS):
        t, log = run("phased", "--spikeIndelReps=%d" % n_reps, "--spikePhaseRpb=%s" % text, "--spikeVariants=%s" % with_sets)
        phased.append(t); st_phased.append(stage_of(log))
        t, log = run("plain", "--spikeIndelReps=%d" % n_reps, "--spikeIndelRpb=%s" % text, "--spikeVariants=%s" % without_sets)
        plain.append(t); st_plain.append(stage_of(log))
    t_phased, t_plain = statistics.median(phased), statistics.median(plain)
    return {"reps": n_reps, "repetitions": REPEATS, "with_spikePhaseRpb_s": round(t_phased, 3), "with_spikeIndelRpb_without_sets_s": round(t_plain, 3),
            "with_spikePhaseRpb_all_s": [round(x, 3) for x in phased], "with_spikeIndelRpb_without_sets_all_s": [round(x, 3) for x in plain],
            "the_set_costs_s": round(t_phased - t_plain, 3), "replicate_stage_with_spikePhaseRpb_s": statistics.median(st_phased),
            "replicate_stage_with_spikeIndelRpb_s": statistics.median(st_plain)}


def main():
    a = sys.argv[1:]
    n_loci = int(a[0]) if a else 128
    n_umi = int(a[1]) if len(a) > 1 else 2000
    rpb = int(a[2]) if len(a) > 2 else 10
    n_reps = int(a[3]) if len(a) > 3 else 32
    out_json = a[4] if len(a) > 4 else os.path.join(HERE, "profiles", "spike_phase_rpb_perf.json")
    cfg = synth.SynthConfig("SIR", n_loci, n_umi, rpb, 20170502, alt_locus_frac=0.3, alt_af=0.1)
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, n_loci)
    bed = ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci)
    # (spike_indel_reps_perf.py's list: an insertion of two letters, a deletion of three, an SNV, and the third indel made an SNV)
    variants, n_indels = [], 0
    for v in spike_indel_restate.pick_variants(bam, fa, loci[n_loci // 2:n_loci // 2 + 48], 4, gap=8):
        n_indels += len(v.ref) != len(v.alt)
        if len(v.ref) != len(v.alt) and n_indels > 2:
            v = spike_indel_restate.variant(v.chrom, v.pos, v.ref[0], "ACGT"[("ACGT".index(v.ref[0]) + 1) % 4])
        variants.append(v)
    # (the set: the insertion and the first SNV of the list)
    one = (next(k for k, v in enumerate(variants) if v.kind == af.INS), next(k for k, v in enumerate(variants) if v.kind == af.SNV))
    with_sets = spike_indel_phase_restate.write_listing(os.path.join(tmp, "v.vcf"), variants, [one])
    without_sets = spike_indel_phase_restate.write_listing(os.path.join(tmp, "w.vcf"), variants, [])
    res = {"targets": list(TARGETS), "rpb_targets": list(RPBS),
           "file": {"loci": n_loci, "barcodes_per_locus": n_umi, "reads_per_barcode": rpb, "records": len(A["aln"]),
                    "variants": ["%s:%d %s>%s" % (v.chrom, v.pos, v.ref, v.alt) for v in variants],
                    "set": ["%s:%d" % (variants[k].chrom, variants[k].pos) for k in sorted(one)], "make_s": round(time.perf_counter() - t0, 1)}}
    eng = Engine(0)
    res["kernels"] = kernels(eng, bam, fa, with_sets, P, n_reps)
    eng.close()
    res["wall"] = wall(tmp, bam, fa, bed, with_sets, without_sets, P, n_reps)
    line = json.dumps(res)
    print(line)
    with open(out_json, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
