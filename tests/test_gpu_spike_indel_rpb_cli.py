"""--spikeIndelRpb on the command line, with an SNV, an insertion and a deletion in the list: every file of the same run with
--spikeIndelReps alone stays byte for byte; the detection page's counts are the restatement's (tests/spike_indel_rpb_restate.py) and
its other columns the cells' own files; every replicate line is the detection line of a separate run with --dsSeed s_j; the sensitivity
table and the curve are what the replicate lines say; and THE SPECIFICATION - every cell's three files are the .dsRpb<r> files of a
--dsRpb r --dsRpbSampler philox run on the BAM tools.spike_variants --indels writes for its target.  One refusal of --dsRpbSampler
philox under the flag: a file without a barcode of two read names."""
import argparse
import os
import sys

import pytest

from conftest import ROOT
from smcounter_amd import bamio, cli, dsaf, spike
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import spike_depth_restate as DS  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import ds_rpb_restate  # noqa: E402
import spike_indel_restate as IR  # noqa: E402
import spike_indel_rpb_restate as RR  # noqa: E402
import test_gpu_spike_rpb_refusals as TR  # noqa: E402  (its tracking of tables and uploaded runs)
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line, the LOD tool's files)

pytestmark = pytest.mark.gpu
SEED = RR.SEED
SUFFIXES = TL.SUFFIXES


def _lines(path):
    return [l.split("\t") for l in open(path).read().splitlines()]


def _files(tmp_path, tag):
    return sorted(f for f in os.listdir(str(tmp_path)) if f.startswith(tag + "."))


def _cli_contract(tmp_path, bam, fa, loci, P, variants, targets, rpbs, n_reps, lod, capsys):
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = R.write_variants(str(tmp_path / "v.vcf"), variants, vcf=True)
    flags = ["--lod"] if lod else []
    T, Rr, V = len(targets), len(rpbs), len(variants)
    kw = dict(spikeAF=",".join("%g" % t for t in targets), spikeVariants=vfile, dsSeed=SEED)
    text = ",".join("%g" % r for r in rpbs)
    cells = [(t, r, P.mtDepth, ".spikeAF%g.dsRpb%g" % (t, r)) for t in targets for r in rpbs]
    assert {v.kind for v in variants} == {af.SNV, af.INS, af.DEL}
    # 1. every file of the run with --spikeIndelReps alone is unchanged (the LOD summary keeps its lines and gets one per cell, behind the targets')
    TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, spikeIndelReps=n_reps, **kw)
    names = _files(tmp_path, "o")
    old = {f: open(str(tmp_path / f), "rb").read() for f in names}
    assert {"o.spikeAF.detection.txt", "o.spikeAF.replicates.txt", "o.spikeAF.sensitivity.txt", "o.spikeAF.curve.txt"} <= set(names)
    capsys.readouterr()
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, spikeIndelReps=n_reps, spikeIndelRpb=text, **kw)
    log = capsys.readouterr().out
    added = sorted(set(_files(tmp_path, "o")) - set(names))
    assert added == sorted(["o" + c[3] + s for c in cells for s in SUFFIXES + (TL.LOD_SUFFIXES if lod else ())] +
                           ["o.spikeAF.rpb.%s.txt" % x for x in ("detection", "replicates", "sensitivity", "curve")])
    for f in names:
        now = open(str(tmp_path / f), "rb").read()
        if f == "o.lod.summary.txt":
            assert now.startswith(old[f]) and len(now.splitlines()) == len(old[f].splitlines()) + len(cells)
            assert [l.split(b"\t")[:2] for l in now.splitlines()[-len(cells):]] == [[os.path.basename(got + c[3]).encode(), b"%d" % c[2]] for c in cells]
        else:
            assert now == old[f], "%s changed with --spikeIndelRpb" % f
    mine = {c[3]: TL._read(got + c[3], SUFFIXES) for c in cells}
    if lod:
        for c in cells:
            assert TL._read(got + c[3], TL.LOD_SUFFIXES) == TL._tool_files(tmp_path, got + c[3] + SUFFIXES[0], "UMT", c[2]), c
    # (the run log: every cell's sampler, seed, probKeep, threshold and kept names)
    groups = RR.file_groups(bam)
    rthr = RR.read_thresholds(groups, rpbs)
    for t in targets:
        for r, q in zip(rpbs, rthr):
            head = "--spikeIndelRpb spiked allele fraction %g x target %g: sampler philox, seed %d, probKeep %.6g, threshold %d, " % (
                t, r, SEED, RR.rp.prob_keep(groups["counts"], float(r)), q)
            assert head in log, head
    # 2. the detection page: the cells' counts are the restatement's, its lines the cells' own files
    det = _lines(got + ".spikeAF.rpb.detection.txt")
    assert det[0] == list(spike.cell_detection_header(spike.RPB_AXIS)) + (["LOD"] if lod else []) and len(det) == 1 + V * T * Rr
    counts, recs, rthr2 = RR.restate_counts(bam, fa, variants, targets, rpbs, SEED, n_reps)
    assert rthr2 == rthr
    for i, v in enumerate(variants):
        for c, (t, r, d, suffix) in enumerate(cells):
            l = det[1 + i * T * Rr + c]
            assert l[:7] == [v.chrom, "%d" % v.pos, v.ref, v.alt, "%g" % t, "%g" % r, "%d" % d]
            assert l[7:12] == ["%d" % x for x in counts[i, 0, c // Rr, c % Rr]], (i, c)
            rows, cut = dsaf.read_output(got + suffix)
            n = dict(zip(RR.NAMES, (int(x) for x in l[7:12])))
            assert l[:5] + l[7:] == spike.detection_line(v, t, n, rows.get((v.chrom, "%d" % v.pos)), cut.get((v.chrom, "%d" % v.pos)),
                                                         float(l[19]) if lod else None).split("\t")
    assert (counts[:, 0, :, 0, 0] < counts[:, 0, :, -1, 0]).any() or (counts[:, 0, :, 0, 3] < counts[:, 0, :, -1, 3]).any()     # (the cells differ)
    # 3. every replicate line is the detection line of a separate run with --dsSeed s_j (both streams drawn with s_j)
    reps = _lines(got + ".spikeAF.rpb.replicates.txt")
    assert reps[0] == list(spike.cell_replicates_header(spike.RPB_AXIS)) and len(reps) == 1 + V * T * Rr * n_reps
    compared = 0
    for j, s in enumerate(PR.seeds(SEED, n_reps)):
        ref = TL._run_cli(tmp_path, "s%d" % j, bam, fa, bed, P, spikeIndelRpb=text, **dict(kw, dsSeed=s))
        one = _lines(ref + ".spikeAF.rpb.detection.txt")
        assert one[0] == list(spike.cell_detection_header(spike.RPB_AXIS)) and len(one) == 1 + V * T * Rr
        for i in range(V):
            for c in range(T * Rr):
                line = reps[1 + (i * T * Rr + c) * n_reps + j]
                assert line[7:9] == ["%d" % j, "%d" % s]
                assert line[:7] + line[9:] == one[1 + i * T * Rr + c], (i, c, j)
                assert line[9:14] == ["%d" % x for x in counts[i, j, c // Rr, c % Rr]]
                compared += 1
        if j == 0:
            assert [l[:19] for l in det[1:]] == one[1:]
    assert compared == V * T * Rr * n_reps
    # 4. the sensitivity table and the curve are what the replicate lines say
    sens = _lines(got + ".spikeAF.rpb.sensitivity.txt")
    assert sens[0] == list(spike.cell_sensitivity_header(spike.RPB_AXIS)) + (["LOD"] if lod else []) and "RPB" in sens[0] and "FRACTION" not in sens[0]
    want = DS.sensitivity_from(reps[1:], variants, [(c[0], c[1]) for c in cells], n_reps, dsaf.frac_text)
    assert len(sens) == 1 + V * T * Rr == 1 + len(want) and [l[:22] for l in sens[1:]] == want
    curve = _lines(got + ".spikeAF.rpb.curve.txt")
    assert curve[0] == list(spike.depth_curve_header(targets, lod, spike.RPB_AXIS)) and len(curve) == 1 + V * (1 + Rr)
    plain = _lines(got + ".spikeAF.replicates.txt")[1:]
    want = DS.curve_from(plain, [P.mtDepth] * T, reps[1:], variants, targets, rpbs, n_reps, dsaf.frac_text)
    assert [l[:8 + T] for l in curve[1:]] == want
    if lod:
        top = max(range(T), key=lambda t: targets[t])
        full_det = _lines(got + ".spikeAF.detection.txt")
        for i in range(V):
            for c in range(T * Rr):
                assert sens[1 + i * T * Rr + c][22] == det[1 + i * T * Rr + c][19]
            assert curve[1 + i * (1 + Rr)][8 + T] == full_det[1 + i * (1 + T) + 1 + top][17]
            for k in range(Rr):
                assert curve[1 + i * (1 + Rr) + 1 + k][8 + T] == det[1 + i * T * Rr + top * Rr + k][19]
    # 5. the specification: a cell is the .dsRpb<r> output of --dsRpb r --dsRpbSampler philox on the BAM the tool writes for t with --indels.  The
    # workflow writes under a prefix of its own; the .cut.vcf names its prefix in the sample column, so that one word is mapped
    checked = 0
    for t in targets:
        out = str(tmp_path / ("sp%g.bam" % t))
        sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=SEED, refGenome=fa, indels=True))
        if not os.path.exists(out + ".bai"):
            bamio.write_bai(out)
        ref = TL._run_cli(tmp_path, "w.spikeAF%g" % t, out, fa, bed, P, dsRpb=text, dsRpbSampler="philox", dsSeed=SEED)
        for r in rpbs:
            suffix = ".spikeAF%g.dsRpb%g" % (t, r)
            theirs = [x.replace((ref + ".dsRpb%g" % r).encode(), (got + suffix).encode()) for x in TL._read(ref + ".dsRpb%g" % r, SUFFIXES)]
            assert TL._read(got + suffix, SUFFIXES) == mine[suffix]                          # (nothing wrote over the cell's files)
            for a, b, s in zip(mine[suffix], theirs, SUFFIXES):
                assert a == b, "cell %s: %s differs from the two-step workflow's" % (suffix, s)
            checked += 1
    assert checked == T * Rr


def test_cli_cells_equal_the_two_step_workflow_on_the_synthetic_bam(tmp_path, capsys):
    bam, fa, loci, P, variants = RR.synth_case(str(tmp_path))
    _cli_contract(tmp_path, bam, fa, loci, P, variants, (0.2, 0.05), (1.5, 3), 4, False, capsys)


def test_cli_cells_equal_the_two_step_workflow_on_bam_cigars_with_lod(tmp_path, capsys):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    _cli_contract(tmp_path, bam, fa, loci, P, IR.pick_variants(bam, fa, loci, 4, gap=8), (0.3, 0.1), (1.5, 3), 4, True, capsys)


tracked = TR.tracked


def test_a_file_without_a_multi_name_barcode_is_refused_under_the_flag(tmp_path, tracked):
    """--dsRpbSampler philox's refusal, named after this flag: before any file, the table closed and every run freed, and the same
    command works afterwards in the same process."""
    bam, fa, loci, P = ds_restate.make_case(str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    variants = IR.pick_variants(bam, fa, loci, 4, gap=8)
    assert {v.kind for v in variants} == {af.SNV, af.INS, af.DEL}
    vfile = R.write_variants(str(tmp_path / "v.txt"), variants)

    def run(tag, bam_file, **kw):
        prefix = str(tmp_path / tag)
        cli.main(dict(outPrefix=prefix, bamFile=bam_file, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, hpLen=P.hpLen, refGenome=fa, spikeAF="0.3",
                      spikeVariants=vfile, spikeIndelRpb="1.5,3", dsSeed=SEED, **kw))
        return prefix
    one = ds_rpb_restate.write_one_name_per_barcode(bam, str(tmp_path / "one.bam"))
    with pytest.raises(SystemExit, match=r"--spikeIndelRpb 1\.5: .*one\.bam has no barcode with more than one read name"):
        run("bad", one)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("bad.")]
    TR._released(tracked)
    good = run("good", bam, spikeIndelReps=2)
    assert os.path.exists(good + ".spikeAF0.3.dsRpb1.5.smCounter.all.txt") and os.path.exists(good + ".spikeAF.rpb.replicates.txt")
    TR._released(tracked)
