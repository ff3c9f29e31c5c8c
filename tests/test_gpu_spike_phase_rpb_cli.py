"""--spikePhaseRpb on the command line, on the synthetic case (two sets and an unphased variant) and on bam_cigars (with --lod): THE
SPECIFICATION - every cell's three files are the .dsRpb<r> files of a --dsRpb r --dsRpbSampler philox run on the BAM
tools.spike_variants --phased --indels writes for its target; every file of the same run with --spikeIndelPhase --spikeIndelReps alone
stays byte for byte; the detection page's counts are those of a --spikeIndelRpb run drawn with the leaders' positions (the restatement's);
the rpb phase page's counts are the restatement's (tests/spike_phase_rpb_restate.py) and CALLED_ALL the cells' own .cut.txt; every
replicate line is the page line of a separate run with --dsSeed s_j; the sensitivity page is what the replicate lines say.  A list
without sets gives the --spikeIndelRpb run byte for byte.  One refusal of --dsRpbSampler philox under the flag."""
import argparse
import os
import sys

import pytest

from conftest import ROOT
from smcounter_amd import bamio, cli, dsaf, spike
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import ds_rpb_restate  # noqa: E402
import spike_indel_restate as IR  # noqa: E402
import spike_phase_restate as PH  # noqa: E402
import spike_phase_rpb_restate as ZR  # noqa: E402
import test_gpu_spike_indel_phase_cli as PC  # noqa: E402  (its runs of the command line in child processes, its masked trees)
import test_gpu_spike_rpb_refusals as TR  # noqa: E402  (its tracking of tables and uploaded runs)

pytestmark = pytest.mark.gpu
XR, PR = ZR.XR, ZR.PR
SEED = ZR.SEED
SUFFIXES, LOD_SUFFIXES = PC.SUFFIXES, PC.LOD_SUFFIXES
REPS, RPBS = 4, (1.5, 3)
BAM_CIGARS_SETS = ((0, 1), (2, 3))                    # (of the six variants picked: an insertion + a deletion, a deletion + an insertion)
_start, _finish, _read, _lines, _tree = PC._start, PC._finish, PC._read, PC._lines, PC._tree


def _inputs(name, tmp):
    """-> (bam, fasta, loci, params, variants, the sets' members, targets, whether the run takes --lod)."""
    if name == "synth":
        bam, fa, loci, P, variants, sets = ZR.synth_case(tmp)
        return bam, fa, loci, P, variants, sets, (0.2, 0.05), False
    bam, fa, loci, P = ds_restate.load_fixture(name, tmp)
    variants = IR.pick_variants(bam, fa, loci, 6, gap=8)                                # (two chromosomes: a set lies on one)
    assert all(len({variants[k].chrom for k in m}) == 1 for m in BAM_CIGARS_SETS)
    return bam, fa, loci, P, variants, list(BAM_CIGARS_SETS), (0.3, 0.1), True


@pytest.fixture(scope="module", params=("synth", "bam_cigars"))
def runs(request, tmp_path_factory):
    """The run under test and every run it is compared with, started together (seven processes) and made once per input."""
    tmp = tmp_path_factory.mktemp("phase_rpb_cli_" + request.param)
    bam, fa, loci, P, variants, sets, targets, lod = _inputs(request.param, str(tmp))
    assert {v.kind for v in variants} == {af.SNV, af.INS, af.DEL}
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    vfile = ZR.write_listing(str(tmp / "v.vcf"), variants, sets)
    text = ",".join("%g" % r for r in RPBS)
    kw = dict(spikeAF=",".join("%g" % t for t in targets), spikeVariants=vfile)
    flags = ["--lod"] if lod else []
    started = [_start(tmp, "o", bam, fa, bed, P, flags=flags, spikePhaseRpb=text, spikeIndelReps=REPS, dsSeed=SEED, **kw),
               _start(tmp, "b", bam, fa, bed, P, flags=flags + ["--spikeIndelPhase"], spikeIndelReps=REPS, dsSeed=SEED, **kw)]
    for j, s in enumerate(PR.seeds(SEED, REPS)):
        if j:                                                                            # (replicate 0 has the seed of the run itself)
            started.append(_start(tmp, "s%d" % j, bam, fa, bed, P, spikePhaseRpb=text, dsSeed=s, **kw))
    for t in targets:
        out = str(tmp / ("tool%g.bam" % t))
        sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=SEED, refGenome=fa, phased=True, indels=True))
        bamio.write_bai(out)
        started.append(_start(tmp, "w.spikeAF%g" % t, out, fa, bed, P, dsRpb=text, dsRpbSampler="philox", dsSeed=SEED))
    assert len(started) <= 16
    done = _finish(started)
    groups = XR.file_groups(bam)
    recs = XR.records(bam, fa, variants, groups)
    return dict(tmp=tmp, bam=bam, fa=fa, P=P, variants=variants, sets=sets, targets=targets, lod=lod, got=done[0], base=done[1],
                seeded=dict(zip(range(1, REPS), done[2:2 + REPS - 1])), tool=dict(zip(targets, done[2 + REPS - 1:])),
                recs=recs, rthr=XR.read_thresholds(groups, RPBS))


def _cells(runs):
    return [(t, r, runs["P"].mtDepth, ".spikeAF%g.dsRpb%g" % (t, r)) for t in runs["targets"] for r in RPBS]


def test_every_cell_equals_the_two_step_workflow_on_the_tools_bam(runs):
    got = runs["got"]
    moved = 0
    for t in runs["targets"]:
        ref = runs["tool"][t]
        for r in RPBS:
            cell, theirs = "%s.spikeAF%g.dsRpb%g" % (got, t, r), "%s.dsRpb%g" % (ref, r)
            mine = _read(cell, SUFFIXES)
            for a, b, s in zip(mine, [x.replace(theirs.encode(), cell.encode()) for x in _read(theirs, SUFFIXES)], SUFFIXES):
                assert a == b, "cell %g x %g: %s differs from the two-step workflow's" % (t, r, s)
            moved += mine[0] != _read(got, SUFFIXES)[0]
    assert moved == len(runs["targets"]) * len(RPBS)


def test_the_files_of_the_run_without_the_flag_stay_and_the_new_ones_are_those_listed(runs):
    mine, base = _tree(runs["tmp"], "o"), _tree(runs["tmp"], "b")
    cells, lod = _cells(runs), runs["lod"]
    assert {".spikeAF.phase.txt", ".spikeAF.phase.replicates.txt", ".spikeAF.phase.sensitivity.txt", ".spikeAF.detection.txt",
            ".spikeAF.replicates.txt"} <= set(base)
    assert sorted(set(mine) - set(base)) == sorted(
        [c[3] + s for c in cells for s in SUFFIXES + (LOD_SUFFIXES if lod else ())] +
        [".spikeAF.rpb.%s.txt" % x for x in ("detection", "replicates", "sensitivity", "curve", "phase", "phase.replicates", "phase.sensitivity")])
    for f in sorted(base):
        if f == ".lod.summary.txt":
            assert mine[f].startswith(base[f]) and len(mine[f].splitlines()) == len(base[f].splitlines()) + len(cells)
        else:
            assert mine[f] == base[f], "%s changed with --spikePhaseRpb" % f


def test_the_detection_page_is_drawn_with_the_leaders_positions(runs):
    got, variants, targets = runs["got"], runs["variants"], list(runs["targets"])
    T, Rr, V = len(targets), len(RPBS), len(variants)
    lead = PH.lead_positions(variants, runs["sets"])
    assert lead != [v.pos for v in variants]
    counts = XR.counts_from(runs["recs"], lead, [PR.threshold(t) for t in targets], runs["rthr"], PR.seeds(SEED, REPS))
    det = _lines(got + ".spikeAF.rpb.detection.txt")
    assert det[0] == list(spike.cell_detection_header(spike.RPB_AXIS)) + (["LOD"] if runs["lod"] else []) and len(det) == 1 + V * T * Rr
    for i, v in enumerate(variants):
        for c, (t, r, d, suffix) in enumerate(_cells(runs)):
            l = det[1 + i * T * Rr + c]
            assert l[:7] == [v.chrom, "%d" % v.pos, v.ref, v.alt, "%g" % t, "%g" % r, "%d" % d]
            assert l[7:12] == ["%d" % x for x in counts[i, 0, c // Rr, c % Rr]], (i, c)
    reps = _lines(got + ".spikeAF.rpb.replicates.txt")
    assert len(reps) == 1 + V * T * Rr * REPS
    for i in range(V):
        for c in range(T * Rr):
            for j in range(REPS):
                assert reps[1 + (i * T * Rr + c) * REPS + j][9:14] == ["%d" % x for x in counts[i, j, c // Rr, c % Rr]]


def _want_line(name, members, cell, prefix, c):
    _, cut = dsaf.read_output(prefix)
    key = lambda v: (v.chrom, "%d" % v.pos)
    called = int(all(key(v) in cut and cut[key(v)][0] == v.ref and v.alt in cut[key(v)][1] for v in members))
    return [name, members[0].chrom, ",".join("%d" % v.pos for v in members), ",".join(v.ref for v in members), ",".join(v.alt for v in members),
            "%g" % cell[0], "%g" % cell[1], "%d" % cell[2]] + ["%d" % x for x in c] + \
           [dsaf.frac_text(int(c[3]) / int(c[0]) if int(c[0]) else 0.0), "%d" % called]


def test_the_rpb_phase_pages_are_the_restatement_and_the_cells_own_cut(runs):
    got, targets, variants, sets = runs["got"], list(runs["targets"]), runs["variants"], runs["sets"]
    cells = _cells(runs)
    C, G = len(cells), len(sets)
    lead = [min(variants[k].pos for k in m) for m in sets]
    counts = ZR.counts_from(ZR.set_rows(runs["recs"], sets), lead, [PR.threshold(t) for t in targets], runs["rthr"], PR.seeds(SEED, REPS))
    page = _lines(got + ".spikeAF.rpb.phase.txt")
    assert page[0] == list(spike.phase_header(spike.RPB_AXIS)) and "RPB" in page[0] and "FRACTION" not in page[0] and len(page) == 1 + G * C
    names = ["hap" + ("%d" % g if g else "") for g in range(G)]
    for g, m in enumerate(sets):
        members = [variants[k] for k in m]
        for c, cell in enumerate(cells):
            assert page[1 + g * C + c] == _want_line(names[g], members, cell, got + cell[3], counts[g, 0, c // len(RPBS), c % len(RPBS)]), (g, c)
    assert any(0 < int(l[PH.P_S]) < int(l[PH.P_N]) for l in page[1:])
    # the full-depth phase page holds the unthinned numbers: thinning takes joint barcodes away
    full = _lines(got + ".spikeAF.phase.txt")
    assert any(int(page[1 + g * C][PH.P_N]) < int(full[1 + g * (1 + len(targets))][PH.P_N]) for g in range(G))
    # the replicate lines: the rpb phase page of a separate run with --dsSeed s_j; replicate 0 the run's own page
    reps = _lines(got + ".spikeAF.rpb.phase.replicates.txt")
    assert reps[0] == list(spike.phase_replicates_header(spike.RPB_AXIS)) and len(reps) == 1 + G * C * REPS
    for j, seed_j in enumerate(PR.seeds(SEED, REPS)):
        single = page if j == 0 else _lines(runs["seeded"][j] + ".spikeAF.rpb.phase.txt")
        for k in range(G * C):
            line = reps[1 + k * REPS + j]
            assert line[8:10] == ["%d" % j, "%d" % seed_j] and line[:8] + line[10:] == single[1 + k], (k, j)
            assert line[10:14] == ["%d" % x for x in counts[k // C, j, (k % C) // len(RPBS), k % len(RPBS)]]
    assert len({tuple(reps[1 + j][10:14]) for j in range(REPS)}) > 1                      # (the replicates differ)
    # the sensitivity page: what the replicate lines say
    sens = _lines(got + ".spikeAF.rpb.phase.sensitivity.txt")
    assert sens[0] == list(spike.phase_sensitivity_header(spike.RPB_AXIS)) and len(sens) == 1 + G * C
    for k in range(G * C):
        per = reps[1 + k * REPS:1 + (k + 1) * REPS]
        called = sum(int(l[PH.R_CALLED]) for l in per)
        lo, hi = PR.wilson(called, REPS)
        afs = [int(l[PH.R_V1]) / int(l[PH.R_N]) if int(l[PH.R_N]) else 0.0 for l in per]
        assert sens[1 + k] == per[0][:8] + ["%d" % REPS, "%d" % called, dsaf.frac_text(called / REPS), dsaf.frac_text(lo), dsaf.frac_text(hi),
                                            dsaf.frac_text(sum(afs) / REPS), dsaf.frac_text(min(afs)), dsaf.frac_text(max(afs))]


def test_the_run_log_names_the_flag_per_cell_and_per_set(tmp_path, capsys):
    bam, fa, loci, P, variants, sets, targets, _ = _inputs("bam_cigars", str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = ZR.write_listing(str(tmp_path / "v.vcf"), variants, sets)
    capsys.readouterr()
    cli.main(dict(outPrefix=str(tmp_path / "o"), bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, hpLen=P.hpLen, refGenome=fa, spikeAF="0.3",
                  spikeVariants=vfile, spikePhaseRpb="1.5,3", dsSeed=SEED))
    log = capsys.readouterr().out
    groups = XR.file_groups(bam)
    for r, q in zip(RPBS, XR.read_thresholds(groups, RPBS)):
        assert "--spikePhaseRpb spiked allele fraction 0.3 x target %g: sampler philox, seed %d, probKeep %.6g, threshold %d, " % (
            r, SEED, XR.rp.prob_keep(groups["counts"], float(r)), q) in log
        for name in ("hap", "hap1"):
            assert "--spikePhaseRpb 0.3 x target %g: set %s (2 members) N_ALL " % (r, name) in log
    assert "--spikeIndelRpb" not in log


def test_a_list_without_sets_gives_the_files_of_spike_indel_rpb(tmp_path):
    bam, fa, loci, P, variants, _, _, _ = _inputs("bam_cigars", str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = ZR.write_listing(str(tmp_path / "v.vcf"), variants, [])
    kw = dict(spikeAF="0.3,0.1", spikeVariants=vfile, dsSeed=SEED, spikeIndelReps=2)
    _finish([_start(tmp_path, "a", bam, fa, bed, P, flags=["--lod"], spikePhaseRpb="1.5,3", **kw),
             _start(tmp_path, "b", bam, fa, bed, P, flags=["--lod"], spikeIndelRpb="1.5,3", **kw)])
    mine, theirs = _tree(tmp_path, "a"), _tree(tmp_path, "b")
    assert sorted(mine) == sorted(theirs) and ".spikeAF.rpb.detection.txt" in mine and ".spikeAF.rpb.replicates.txt" in mine
    assert not [f for f in mine if "phase" in f]
    for f in sorted(mine):
        assert mine[f] == theirs[f], f


tracked = TR.tracked


def test_a_file_without_a_multi_name_barcode_is_refused_under_the_flag(tmp_path, tracked):
    """--dsRpbSampler philox's refusal, named after this flag: before any file, the table closed and every run freed, and the same
    command works afterwards in the same process."""
    bam, fa, loci, P = ds_restate.make_case(str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    variants = IR.pick_variants(bam, fa, loci, 4, gap=8)
    assert {v.kind for v in variants} == {af.SNV, af.INS, af.DEL} and len({v.chrom for v in variants[:2]}) == 1
    vfile = ZR.write_listing(str(tmp_path / "v.vcf"), variants, [(0, 1)])

    def run(tag, bam_file, **kw):
        prefix = str(tmp_path / tag)
        cli.main(dict(outPrefix=prefix, bamFile=bam_file, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, hpLen=P.hpLen, refGenome=fa, spikeAF="0.3",
                      spikeVariants=vfile, spikePhaseRpb="1.5,3", dsSeed=SEED, **kw))
        return prefix
    one = ds_rpb_restate.write_one_name_per_barcode(bam, str(tmp_path / "one.bam"))
    with pytest.raises(SystemExit, match=r"--spikePhaseRpb 1\.5: .*one\.bam has no barcode with more than one read name"):
        run("bad", one)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("bad.")]
    TR._released(tracked)
    good = run("good", bam, spikeIndelReps=2)
    assert os.path.exists(good + ".spikeAF0.3.dsRpb1.5.smCounter.all.txt") and os.path.exists(good + ".spikeAF.rpb.phase.replicates.txt")
    TR._released(tracked)
