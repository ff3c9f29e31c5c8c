"""Cost of --spikeIndelPhase (dev tool, GPU box).

On scripts/spike_indel_reps_perf.py's input (a synthetic BAM, four listed variants of which two are indels, three targets) with two of
the four - the first indel and the first SNV by position - made one phase set, after a warm-up, medians of `REPEATS` alternating
repetitions, the device synchronised around each call:
(a) one smc_spike_indels_reps call of 16 copies over the pre-pass's run with `lead` all zero and with the set's `lead`;
(b) one smc_spike_indel_phase_counts call beside one smc_spike_phase_counts call on the same joint barcodes (three of the four columns);
(c) the run with --spikeIndelReps R, with and without --spikeIndelPhase (without it PS= is not read: the members draw on their own);
(d) the yardstick: the 16-copy call of (a) with `lead` all zero in a tree of the PARENT commit built elsewhere (`parent_root`), in the
    same session, a fresh child process per repetition, alternating with the same child over this tree.

usage: spike_indel_phase_perf.py [parent_root] [out.json] [n_loci] [n_umi] [rpb] [reps]  -> one JSON line (also written to out.json)
       spike_indel_phase_perf.py --child root bam fa variants mtDepth rpb               -> the child of (d): one line, milliseconds"""
import contextlib
import io
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TARGETS = (0.05, 0.02, 0.01)
SEED = 1234567
REPEATS = 5
COPIES = 16
CHILD_LIMIT = 300


def median_ms(fn, sync):
    fn(); sync()                                                  # (warm-up)
    times = []
    for _ in range(REPEATS):
        t0 = time.perf_counter()
        fn(); sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), times


def child(root, bam, fa, vfile, mt_depth, rpb):
    """(d) in a tree of its own: the pre-pass, then the 16-copy call with the records as that tree makes them for a file without sets."""
    sys.path.insert(0, root)
    from smcounter_amd import devplanes, dsaf, fasta
    from smcounter_amd.engine import Engine
    from smcounter_amd.params import VcParams
    from smcounter_amd.tools import spike_variants as sv
    P = VcParams(mtDepth=int(mt_depth), rpb=float(rpb))
    eng = Engine(0)
    keep = {}
    variants = sv.parse_variants(vfile, "v.txt", indels=True)
    devplanes.spike_rules(bam, fasta.FastaFile(fa), variants, list(TARGETS), [P] * len(TARGETS), SEED, eng, keep=keep, indel_counters=True)
    run = keep["runs"][0]
    svar, _ = keep["spikes"].chrom_variants(run.chrom, TARGETS[0])
    ins, seeds, thr = keep["spikes"].ins[run.chrom], dsaf.rep_seeds(SEED, COPIES), sv.threshold(TARGETS[0])

    def batched():
        made = devplanes.spike_indel_run_copies(eng, run.up, run.A, svar, ins, run.idents, seeds, [thr] * COPIES, P.mismatchThr, *run.mism)
        for k in ("aln", "bq", "cig"):
            made[k].free()
    med, times = median_ms(batched, lambda: eng.L.smc_device_sync(eng.ctx))
    devplanes.free_af_runs(keep["runs"])
    eng.close()
    print(json.dumps({"median_ms": round(med, 4), "all_ms": [round(x, 4) for x in times]}))


def yardstick(parent_root, bam, fa, vfile, P):
    """(d): REPEATS children over the parent's tree alternating with REPEATS over this one -> the medians of their medians."""
    def one(root):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", root, bam, fa, vfile, "%d" % P.mtDepth, "%g" % P.rpb]
        out = subprocess.run(cmd, capture_output=True, text=True, timeout=CHILD_LIMIT, cwd=root)
        if out.returncode != 0:
            raise RuntimeError("the child over %s ended with %d:\n%s" % (root, out.returncode, out.stderr[-2000:]))
        return json.loads(out.stdout.strip().splitlines()[-1])
    parent, mine = [], []
    for _ in range(REPEATS):
        parent.append(one(parent_root)); mine.append(one(ROOT))
    return {"parent_medians_ms": [x["median_ms"] for x in parent], "this_tree_medians_ms": [x["median_ms"] for x in mine],
            "parent_ms": round(statistics.median(x["median_ms"] for x in parent), 4),
            "this_tree_ms": round(statistics.median(x["median_ms"] for x in mine), 4),
            "parent_spread_ms": round(max(x["median_ms"] for x in parent) - min(x["median_ms"] for x in parent), 4),
            "recorded_for_the_parent_ms": 0.76}


def kernels(eng, bam, fa, variants, sets, P, n_reps):
    """(a) and (b) over the pre-pass's run and its joint barcodes."""
    import numpy as np
    from smcounter_amd import devplanes, dsaf, fasta
    from smcounter_amd.tools import spike_variants as sv
    keep, phase = {}, dict(sets=sets)
    devplanes.spike_rules(bam, fasta.FastaFile(fa), variants, list(TARGETS), [P] * len(TARGETS), SEED, eng, keep=keep, indel_counters=True, phase=phase)
    run = keep["runs"][0]
    with_lead, _ = keep["spikes"].chrom_variants(run.chrom, TARGETS[0])
    no_lead = with_lead.copy()
    no_lead["lead"] = 0
    ins, seeds, thr = keep["spikes"].ins[run.chrom], dsaf.rep_seeds(SEED, COPIES), sv.threshold(TARGETS[0])
    sync = lambda: eng.L.smc_device_sync(eng.ctx)

    def batched(svar):
        def fn():
            made = devplanes.spike_indel_run_copies(eng, run.up, run.A, svar, ins, run.idents, seeds, [thr] * COPIES, P.mismatchThr, *run.mism)
            for k in ("aln", "bq", "cig"):
                made[k].free()
        return fn
    joint4 = phase["joint"]
    joint3 = [(ids, np.ascontiguousarray(c[:, :, :3])) for ids, c in joint4]
    lead = [keep["spikes"].lead_pos[s.members[0]] for s in sets]
    rep_seeds, thrs = dsaf.rep_seeds(SEED, n_reps), [sv.threshold(t) for t in TARGETS]
    four = lambda: devplanes.spike_indel_phase_counts(eng, lead, joint4, rep_seeds, thrs, [1 << 32])
    three = lambda: devplanes.spike_phase_counts(eng, lead, joint3, rep_seeds, thrs, [1 << 32])
    a, b, c, d = [], [], [], []
    for _ in range(3):                                             # (alternated)
        a.append(median_ms(batched(no_lead), sync)[0]); b.append(median_ms(batched(with_lead), sync)[0])
        c.append(median_ms(four, sync)[0]); d.append(median_ms(three, sync)[0])
    out = {"copies": COPIES, "run_alignments": int(run.up.n_aln), "records_lead": with_lead["lead"].tolist(),
           "joint_barcodes": [int(len(ids)) for ids, _ in joint4], "members": [int(c4.shape[1]) for _, c4 in joint4],
           "copies_call_lead_all_zero_ms": round(statistics.median(a), 4), "copies_call_with_the_set_ms": round(statistics.median(b), 4),
           "indel_phase_counts_call_ms": round(statistics.median(c), 4), "phase_counts_call_ms": round(statistics.median(d), 4)}
    devplanes.free_af_runs(keep["runs"])
    return out


def wall(tmp, bam, fa, bed, vfile, P, n_reps):
    """(c): the run with and without the flag, alternating."""
    from smcounter_amd import cli
    base = ["--bedTarget=%s" % bed, "--mtDepth=%d" % P.mtDepth, "--rpb=%g" % P.rpb, "--refGenome=%s" % fa, "--bamFile=%s" % bam,
            "--spikeAF=" + ",".join("%g" % t for t in TARGETS), "--spikeVariants=%s" % vfile, "--dsSeed=%d" % SEED]
    parser = cli.build_parser()

    def run(prefix, *extra):
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(io.StringIO()):
            cli.main(parser.parse_args(base + ["--outPrefix=%s" % os.path.join(tmp, prefix)] + list(extra)))
        return time.perf_counter() - t0
    run("warm", "--spikeIndelReps=2", "--spikeIndelPhase")
    with_, without = [], []
    for _ in range(REPEATS):
        with_.append(run("phase", "--spikeIndelReps=%d" % n_reps, "--spikeIndelPhase"))
        without.append(run("plain", "--spikeIndelReps=%d" % n_reps))
    page = open(os.path.join(tmp, "phase.spikeAF.phase.replicates.txt")).read().splitlines()
    return {"reps": n_reps, "repetitions": REPEATS, "with_spikeIndelPhase_s": round(statistics.median(with_), 3),
            "without_s": round(statistics.median(without), 3), "with_spikeIndelPhase_all_s": [round(x, 3) for x in with_],
            "without_all_s": [round(x, 3) for x in without], "flag_costs_s": round(statistics.median(with_) - statistics.median(without), 3),
            "phase_replicate_lines": len(page) - 1}


def main():
    a = sys.argv[1:]
    parent_root = a[0] if a and a[0] not in ("", "-") else None
    n_loci, n_umi, rpb, n_reps = (int(a[k]) if len(a) > k else d for k, d in ((2, 128), (3, 2000), (4, 10), (5, 32)))
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import ds_af_restate
    import ds_restate
    import spike_indel_phase_restate as XR
    import spike_indel_restate
    from smcounter_amd import synth
    from smcounter_amd.engine import Engine
    from smcounter_amd.tools import spike_variants as sv
    cfg = synth.SynthConfig("SIR", n_loci, n_umi, rpb, 20170502, alt_locus_frac=0.3, alt_af=0.1)
    tmp = tempfile.mkdtemp()
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, n_loci)
    bed = ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci)
    # (scripts/spike_indel_reps_perf.py's four: the third indel by position made an SNV, so that two of the four are indels)
    variants, n_indels = [], 0
    for v in spike_indel_restate.pick_variants(bam, fa, loci[n_loci // 2:n_loci // 2 + 48], 4, gap=8):
        n_indels += len(v.ref) != len(v.alt)
        if len(v.ref) != len(v.alt) and n_indels > 2:
            v = spike_indel_restate.variant(v.chrom, v.pos, v.ref[0], "ACGT"[("ACGT".index(v.ref[0]) + 1) % 4])
        variants.append(v)
    members = (next(k for k, v in enumerate(variants) if len(v.ref) != len(v.alt)), next(k for k, v in enumerate(variants) if len(v.ref) == len(v.alt)))
    vfile = XR.write_listing(os.path.join(tmp, "v.vcf"), variants, [members])
    plain = ds_af_restate.write_variants(os.path.join(tmp, "plain.txt"), variants)
    res = {"targets": list(TARGETS), "file": {"loci": n_loci, "barcodes_per_locus": n_umi, "reads_per_barcode": rpb, "records": len(A["aln"]),
                                              "variants": ["%s:%d %s>%s" % (v.chrom, v.pos, v.ref, v.alt) for v in variants],
                                              "set": ["%s:%d" % (variants[k].chrom, variants[k].pos) for k in members]}}
    listed = sv.parse_variants(vfile, "v.vcf", phased=True, indels=True)
    eng = Engine(0)
    res["kernels"] = kernels(eng, bam, fa, listed, sv.phase_sets(listed), P, n_reps)
    eng.close()
    res["wall"] = wall(tmp, bam, fa, bed, vfile, P, n_reps)
    if parent_root:
        res["yardstick"] = yardstick(os.path.abspath(parent_root), bam, fa, plain, P)
    line = json.dumps(res)
    print(line)
    if len(a) > 1:
        with open(a[1], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        child(*sys.argv[2:8])
    else:
        main()
