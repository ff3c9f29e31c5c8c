"""Cost of --spikeIndelRpb (dev tool, GPU box).

On scripts/spike_indel_reps_perf.py's input (a synthetic BAM, `n_umi` barcodes x `rpb` reads per locus, four listed variants of which
two are an insertion and a deletion, three targets) with the reads-per-barcode targets 5 / 3 / 1.5, after a warm-up, medians of
`REPEATS`:
(a) wall time in process of a run with --spikeAF, --spikeIndelReps R and --spikeIndelRpb, alternating with the same run without
    --spikeIndelRpb, and the replicate stage of both from the run's own clock;
(b) device synchronised around it, one smc_spike_indel_rpb_counts call over all (variant, replicate, target, reads-per-barcode target)
    beside one smc_spike_rpb_counts call of the same shape on an SNV-only list (the same positions, every variant an SNV);
(c) one smc_spike_indel_read_bits call over the pre-pass's run beside one smc_spike_read_bits call on the SNV-only list;
(d) the 16-copy smc_spike_indels_reps call in a fresh process on this tree and, with `parent_root` (a checkout of the parent commit
    with its libraries built), in a fresh process on that tree: the path this change must not have moved.  The child is this file
    run as `spike_indel_rpb_perf.py --copies <root> <bam> <fasta> <variants>`; it uses nothing the parent lacks.

usage: spike_indel_rpb_perf.py [n_loci] [n_umi] [rpb] [reps] [out.json] [parent_root]   -> one JSON line (also written to out.json,
default profiles/spike_indel_rpb_perf.json)"""
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

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (--copies: the tree whose package and test helpers are imported - this one, or the parent's)
ROOT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == "--copies" else HERE
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ds_af_restate  # noqa: E402
import ds_restate  # noqa: E402
import spike_indel_restate  # noqa: E402
from smcounter_amd import cli, devplanes, dsaf, fasta, synth  # noqa: E402
from smcounter_amd.engine import Engine  # noqa: E402
from smcounter_amd.params import VcParams  # noqa: E402
from smcounter_amd.tools import spike_variants as sv  # noqa: E402

TARGETS = (0.05, 0.02, 0.01)
RPBS = (5, 3, 1.5)
SEED = 1234567
REPEATS = 5
COPIES = 16


def median_ms(eng, fn):
    sync = lambda: eng.L.smc_device_sync(eng.ctx)
    fn(); sync()                                                  # (warm-up)
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn(); sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(times), 4)


def copies_only(bam, fa, vfile, p_json):
    """(d), in a process of its own: one smc_spike_indels_reps call of COPIES copies over the pre-pass's run -> one JSON line."""
    P = VcParams(**json.loads(p_json))
    variants = sv.parse_variants(vfile, "v.txt", indels=True)
    eng = Engine(0)
    keep = {}
    devplanes.spike_rules(bam, fasta.FastaFile(fa), variants, list(TARGETS), [P] * len(TARGETS), SEED, eng, keep=keep, indel_counters=True)
    run = keep["runs"][0]
    svar, _ = keep["spikes"].chrom_variants(run.chrom, TARGETS[0])
    ins, seeds, thr = keep["spikes"].ins[run.chrom], dsaf.rep_seeds(SEED, COPIES), sv.threshold(TARGETS[0])

    def batched():
        made = devplanes.spike_indel_run_copies(eng, run.up, run.A, svar, ins, run.idents, seeds, [thr] * COPIES, P.mismatchThr, *run.mism)
        for k in ("aln", "bq", "cig"):
            made[k].free()
    got = [median_ms(eng, batched) for _ in range(3)]
    n_aln = int(run.up.n_aln)
    devplanes.free_af_runs(keep["runs"])
    eng.close()
    print(json.dumps({"copies": COPIES, "run_alignments": n_aln, "one_call_of_copies_ms": statistics.median(got), "medians_ms": got}))


def kernels(eng, bam, fa, variants, P, n_reps):
    """(b), (c): the two new entries over what the pre-pass keeps, beside the SNV entries on the same positions."""
    fasta_file = fasta.FastaFile(fa)
    out = {}
    snvs = [spike_indel_restate.variant(v.chrom, v.pos, v.ref[0], v.alt if len(v.ref) == len(v.alt) else "ACGT"[("ACGT".index(v.ref[0]) + 1) % 4])
            for v in variants]
    for tag, vs, four in (("indel", variants, True), ("snv", snvs, False)):
        keep, rpb = {}, dict(targets=list(RPBS), params=[P] * (len(TARGETS) * len(RPBS)))
        devplanes.spike_rules(bam, fasta_file, vs, list(TARGETS), [P] * len(TARGETS), SEED, eng, keep=keep, rpb=rpb, indel_counters=four)
        pos, seeds, thr = [v.pos for v in vs], dsaf.rep_seeds(SEED, n_reps), [sv.threshold(t) for t in TARGETS]
        rthr = [r.thr for r in rpb["rules"][:len(RPBS)]]
        run = keep["runs"][0]
        if four:
            svar, sorder = keep["spikes"].chrom_variants(run.chrom, TARGETS[0])
            var, ins = svar[[sorder.index(k) for k in run.group]], keep["spikes"].ins[run.chrom]
            bits = lambda: devplanes.spike_indel_read_bits(eng, run.up, run.A, run.lo, var, ins)
        else:
            var, _ = devplanes.af_run_variants([vs[k] for k in run.group], run.chrom, run.lo, fasta_file)
            bits = lambda: devplanes.spike_read_bits(eng, run.up, run.A, run.lo, var)
        out[tag] = {"covering_barcodes": int(sum(len(c) for c in keep["covers"])), "covering_records": int(sum(len(r[1]) for r in keep["records"])),
                    "alignments_of_the_run": int(run.up.n_aln), "cells_counted": len(vs) * n_reps * len(TARGETS) * len(RPBS),
                    "read_bits_call_ms": median_ms(eng, bits),
                    "rpb_counts_call_ms": median_ms(eng, lambda: devplanes.spike_rpb_counts(eng, pos, keep["covers"], keep["records"], seeds, thr,
                                                                                          rthr, four=four))}
        devplanes.free_af_runs(keep["runs"])
        devplanes.close_rules(rpb["rules"])
    return out


def wall(tmp, bam, fa, bed, vfile, P, n_reps):
    """(a)"""
    base = ["--bedTarget=%s" % bed, "--mtDepth=%d" % P.mtDepth, "--rpb=%g" % P.rpb, "--refGenome=%s" % fa, "--bamFile=%s" % bam,
            "--spikeAF=" + ",".join("%g" % t for t in TARGETS), "--spikeVariants=%s" % vfile, "--dsSeed=%d" % SEED]
    text = ",".join("%g" % r for r in RPBS)
    parser = cli.build_parser()

    def run(prefix, *extra):
        log = io.StringIO()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(log):
            cli.main(parser.parse_args(base + ["--outPrefix=%s" % os.path.join(tmp, prefix)] + list(extra)))
        return time.perf_counter() - t0, log.getvalue()
    stage_of = lambda log: float(re.search(r"--spikeReps: replicate stage ([0-9.]+) s", log).group(1))
    run("warm", "--spikeIndelReps=2", "--spikeIndelRpb=%s" % text)
    with_, without, st_with, st_without = [], [], [], []
    for _ in range(REPEATS):
        t, log = run("cells", "--spikeIndelReps=%d" % n_reps, "--spikeIndelRpb=%s" % text)
        with_.append(t); st_with.append(stage_of(log))
        t, log = run("plain", "--spikeIndelReps=%d" % n_reps)
        without.append(t); st_without.append(stage_of(log))
    t_with, t_without = statistics.median(with_), statistics.median(without)
    return {"reps": n_reps, "repetitions": REPEATS, "with_spikeIndelRpb_s": round(t_with, 3), "without_spikeIndelRpb_s": round(t_without, 3),
            "with_spikeIndelRpb_all_s": [round(x, 3) for x in with_], "without_spikeIndelRpb_all_s": [round(x, 3) for x in without],
            "flag_costs_s": round(t_with - t_without, 3), "replicate_stage_with_s": statistics.median(st_with),
            "replicate_stage_without_s": statistics.median(st_without),
            "flag_ms_per_cell_and_replicate": round(1e3 * (t_with - t_without) / (n_reps * len(TARGETS) * len(RPBS)), 3)}


def main():
    a = sys.argv[1:]
    if a and a[0] == "--copies":
        return copies_only(*a[2:6])
    n_loci = int(a[0]) if a else 128
    n_umi = int(a[1]) if len(a) > 1 else 2000
    rpb = int(a[2]) if len(a) > 2 else 10
    n_reps = int(a[3]) if len(a) > 3 else 32
    out_json = a[4] if len(a) > 4 else os.path.join(HERE, "profiles", "spike_indel_rpb_perf.json")
    parent_root = a[5] if len(a) > 5 else None
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
    vfile = ds_af_restate.write_variants(os.path.join(tmp, "v.txt"), variants)
    res = {"targets": list(TARGETS), "rpb_targets": list(RPBS),
           "file": {"loci": n_loci, "barcodes_per_locus": n_umi, "reads_per_barcode": rpb, "records": len(A["aln"]),
                    "variants": ["%s:%d %s>%s" % (v.chrom, v.pos, v.ref, v.alt) for v in variants], "make_s": round(time.perf_counter() - t0, 1)}}
    # (d) first, each in a fresh process, before this process opens the GPU
    import dataclasses
    p_json = json.dumps(dataclasses.asdict(P))
    res["copies_call"] = {}
    for tag, root in (("this_tree", HERE), ("parent", parent_root), ("this_tree_again", HERE)):
        if root is not None:
            line = subprocess.run([sys.executable, os.path.abspath(__file__), "--copies", root, bam, fa, vfile, p_json], check=True,
                                  stdout=subprocess.PIPE, timeout=300).stdout.decode().strip().splitlines()[-1]
            res["copies_call"][tag] = json.loads(line)
    eng = Engine(0)
    res["kernels"] = kernels(eng, bam, fa, sv.parse_variants(vfile, "v.txt", indels=True), P, n_reps)
    eng.close()
    res["wall"] = wall(tmp, bam, fa, bed, vfile, P, n_reps)
    line = json.dumps(res)
    print(line)
    with open(out_json, "w") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
