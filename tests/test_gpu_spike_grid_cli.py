"""--spikeGrid on the command line: every file of the run without the three flags stays byte for byte; the detection page's counts are
the restatement's (tests/spike_grid_restate.py) and its other columns the cells' own files; every replicate line is the detection
line of a separate run with --dsSeed s_j; the sensitivity and budget pages are what the replicate lines and the restated kept names
say; THE SPECIFICATION - every cell's three files are the .dsMT<f>.dsRpb<r> files of a --dsGrid run with both philox samplers on the
BAM tools.spike_variants writes for its target; and cell (t, 1, r) is the --spikeRpb run's cell (t, r)."""
import argparse
import os
import sys

import pytest

from conftest import ROOT
from smcounter_amd import bamio, dsaf, spike
from smcounter_amd.py2compat import py2_round
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_grid_restate as GR  # noqa: E402
import ds_restate  # noqa: E402
import spike_depth_restate as DS  # noqa: E402
import spike_grid_restate as G  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402
import spike_rpb_restate as RR  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line, the LOD tool's files)

pytestmark = pytest.mark.gpu
SEED = RR.SEED
SUFFIXES = TL.SUFFIXES


def _lines(path):
    return [l.split("\t") for l in open(path).read().splitlines()]


def _files(tmp_path, tag):
    return sorted(f for f in os.listdir(str(tmp_path)) if f.startswith(tag + "."))


def _cli_contract(tmp_path, bam, fa, loci, P, variants, targets, fracs, rpbs, n_reps, lod, capsys):
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = R.write_variants(str(tmp_path / "v.vcf"), variants, vcf=True)
    flags = ["--lod"] if lod else []
    T, F, Rr, V = len(targets), len(fracs), len(rpbs), len(variants)
    C = T * F * Rr
    seeds = PR.seeds(SEED, n_reps)
    groups = RR.file_groups(bam)
    # (on the CPU first: every (seed, fraction) used keeps a barcode of two or more names - the run would refuse otherwise, rightly)
    assert G.keeps_a_multi_name_barcode(groups, fracs, seeds)
    kw = dict(spikeAF=",".join("%g" % t for t in targets), spikeVariants=vfile, dsSeed=SEED)
    axes = dict(spikeDepth=",".join("%g" % f for f in fracs), spikeRpb=",".join("%g" % r for r in rpbs))
    depth_of = lambda f: max(1, int(py2_round(f * P.mtDepth)))
    cells = [(t, f, r, depth_of(f), ".spikeAF%g.dsMT%g.dsRpb%g" % (t, f, r)) for t in targets for f in fracs for r in rpbs]
    # 1. every file of a run without the three flags is unchanged (the LOD summary gets one line per cell, behind the targets')
    TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, spikeReps=n_reps, **kw)
    names = _files(tmp_path, "o")
    old = {f: open(str(tmp_path / f), "rb").read() for f in names}
    capsys.readouterr()
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags + ["--spikeGrid"], spikeReps=n_reps, **dict(kw, **axes))
    log = capsys.readouterr().out
    added = sorted(set(_files(tmp_path, "o")) - set(names))
    # (no depth-only and no reads-only cell, no .depth. / .rpb. page: the grid's files alone)
    assert added == sorted(["o" + c[4] + s for c in cells for s in SUFFIXES + (TL.LOD_SUFFIXES if lod else ())] +
                           ["o.spikeAF.grid.%s.txt" % x for x in ("detection", "replicates", "sensitivity", "budget")])
    for f in names:
        now = open(str(tmp_path / f), "rb").read()
        if f == "o.lod.summary.txt":
            assert now.startswith(old[f]) and len(now.splitlines()) == len(old[f].splitlines()) + C
            assert [l.split(b"\t")[:2] for l in now.splitlines()[-C:]] == [[os.path.basename(got + c[4]).encode(), b"%d" % c[3]] for c in cells]
        else:
            assert now == old[f], "%s changed with --spikeGrid" % f
    mine = {c[4]: TL._read(got + c[4], SUFFIXES) for c in cells}
    if lod:
        for c in cells:
            assert TL._read(got + c[4], TL.LOD_SUFFIXES) == TL._tool_files(tmp_path, got + c[4] + SUFFIXES[0], "UMT", c[3]), c
    # (the run log: every cell's sampler, seed, probKeep, both thresholds and kept names)
    counts, recs, rd_thr, prob = G.restate_counts(bam, fa, variants, targets, fracs, rpbs, SEED, n_reps)
    qnames = ds_restate.placed_qnames(bam)
    pairs = [(f, r) for f in fracs for r in rpbs]
    kept0 = [len(k) for k in GR.restate(qnames, pairs, SEED)["kept"]]
    for t in targets:
        for q, (f, r) in enumerate(pairs):
            line = "--spikeGrid spiked allele fraction %g x fraction %g x target %g: sampler philox, seed %d, probKeep %.6g, barcode threshold %d, " \
                   "read threshold %d, %d of " % (t, f, r, SEED, prob[0, q // Rr, q % Rr], G.frac_threshold(f), int(rd_thr[0, q // Rr, q % Rr]), kept0[q])
            assert line in log, line
    # 2. the detection page: the cells' counts are the restatement's, its lines the cells' own files
    det = _lines(got + ".spikeAF.grid.detection.txt")
    assert det[0] == list(spike.cell_detection_header(spike.GRID_AXIS)) + (["LOD"] if lod else []) and len(det) == 1 + V * C
    assert det[0][:8] == ["CHROM", "POS", "REF", "ALT", "TARGET", "FRACTION", "RPB", "MTDEPTH"]
    flat = counts.reshape(V, n_reps, T * F * Rr, 5)
    for i, v in enumerate(variants):
        for c, (t, f, r, d, suffix) in enumerate(cells):
            l = det[1 + i * C + c]
            assert l[:8] == [v.chrom, "%d" % v.pos, v.ref, v.alt, "%g" % t, "%g" % f, "%g" % r, "%d" % d]
            assert l[8:13] == ["%d" % x for x in flat[i, 0, c]], (i, c)
            rows, cut = dsaf.read_output(got + suffix)
            n = dict(zip(RR.NAMES, (int(x) for x in l[8:13])))
            assert l[:5] + l[8:] == spike.detection_line(v, t, n, rows.get((v.chrom, "%d" % v.pos)), cut.get((v.chrom, "%d" % v.pos)),
                                                         float(l[20]) if lod else None).split("\t")
    assert len({flat[:, 0, c].tobytes() for c in range(C)}) > T                              # (the cells differ within a target)
    # 3. every replicate line is the detection line of a separate run with --dsSeed s_j (all three streams drawn with s_j)
    reps = _lines(got + ".spikeAF.grid.replicates.txt")
    assert reps[0] == list(spike.cell_replicates_header(spike.GRID_AXIS)) and len(reps) == 1 + V * C * n_reps
    assert reps[0][7:10] == ["MTDEPTH", "REP", "SEED"]
    compared = 0
    for j, s in enumerate(seeds):
        ref = TL._run_cli(tmp_path, "s%d" % j, bam, fa, bed, P, flags=["--spikeGrid"], **dict(kw, dsSeed=s, **axes))
        one = _lines(ref + ".spikeAF.grid.detection.txt")
        assert len(one) == 1 + V * C
        for i in range(V):
            for c in range(C):
                line = reps[1 + (i * C + c) * n_reps + j]
                assert line[8:10] == ["%d" % j, "%d" % s]
                assert line[:8] + line[10:] == one[1 + i * C + c], (i, c, j)
                assert line[10:15] == ["%d" % x for x in flat[i, j, c]]
                compared += 1
        if j == 0:
            assert [l[:20] for l in det[1:]] == one[1:]
    assert compared == V * C * n_reps
    assert (rd_thr[1:, 1:] != rd_thr[0, 1:]).any()                                           # (a replicate's thresholds are its own below f = 1)
    # 4. the sensitivity page is what the replicate lines say (the one-axis restatement's columns with RPB taken out and put back)
    sens = _lines(got + ".spikeAF.grid.sensitivity.txt")
    assert sens[0] == list(spike.cell_sensitivity_header(spike.GRID_AXIS)) + (["LOD"] if lod else []) and sens[0][-1 - bool(lod)] == "N_MEAN"
    want = DS.sensitivity_from([l[:6] + l[7:] for l in reps[1:]], variants, [(c[0], c[1]) for c in cells], n_reps, dsaf.frac_text)
    assert len(sens) == 1 + V * C == 1 + len(want)
    for l, w, c in zip(sens[1:], want, cells * V):
        assert l[:6] + l[7:23] == w and l[6] == "%g" % c[2]
    if lod:
        assert [l[23] for l in sens[1:]] == [l[20] for l in det[1:]]
    # ... and the budget page what they and the restated kept names say
    budget = _lines(got + ".spikeAF.grid.budget.txt")
    assert budget[0] == list(spike.BUDGET_HEADER) and len(budget) == 1 + V * C
    n_names = groups["counts"]["names"]
    costs = [k / n_names for k in kept0]
    order = G.cost_order(costs)
    at = 1
    for i, v in enumerate(variants):
        for k, t in enumerate(targets):
            rates = []
            for q in order:
                c = k * F * Rr + q
                per = reps[1 + (i * C + c) * n_reps:1 + (i * C + c + 1) * n_reps]
                called = sum(int(l[-1]) for l in per)
                lo, hi = PR.wilson(called, n_reps)
                rates.append(called / n_reps)
                assert budget[at][:16] == [v.chrom, "%d" % v.pos, v.ref, v.alt, "%g" % t, "%g" % pairs[q][0], "%g" % pairs[q][1], "%d" % cells[c][3],
                                           "%d" % kept0[q], dsaf.frac_text(costs[q]), dsaf.frac_text(sum(int(l[10]) for l in per) / n_reps),
                                           "%d" % n_reps, "%d" % called, dsaf.frac_text(called / n_reps), dsaf.frac_text(lo), dsaf.frac_text(hi)], (i, k, q)
                at += 1
            assert [l[16] for l in budget[at - F * Rr:at]] == ["%d" % x for x in G.cheapest95(rates)]
    assert at == len(budget) and costs[order[0]] < costs[order[-1]] == max(costs)
    # 5. the specification: a cell is the .dsMT<f>.dsRpb<r> output of the --dsGrid run with both philox samplers on the BAM the tool
    # writes for t, at the target's mtDepth.  The .cut.vcf names its prefix in the sample column, so that one word is mapped
    checked = 0
    for t in targets:
        out = str(tmp_path / ("sp%g.bam" % t))
        sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=SEED, refGenome=fa))
        if not os.path.exists(out + ".bai"):
            bamio.write_bai(out)
        ref = TL._run_cli(tmp_path, "w.spikeAF%g" % t, out, fa, bed, P, flags=["--dsGrid"], dsMT=axes["spikeDepth"], dsRpb=axes["spikeRpb"],
                          dsSampler="philox", dsRpbSampler="philox", dsSeed=SEED)
        for f, r in pairs:
            theirs_at, suffix = ref + ".dsMT%g.dsRpb%g" % (f, r), ".spikeAF%g.dsMT%g.dsRpb%g" % (t, f, r)
            theirs = [x.replace(theirs_at.encode(), (got + suffix).encode()) for x in TL._read(theirs_at, SUFFIXES)]
            assert TL._read(got + suffix, SUFFIXES) == mine[suffix]                          # (nothing wrote over the cell's files)
            for a, b, s in zip(mine[suffix], theirs, SUFFIXES):
                assert a == b, "cell %s: %s differs from the two-step workflow's" % (suffix, s)
            checked += 1
    assert checked == C
    # 6. f = 1 gives the reads-only column: cell (t, 1, r) is the --spikeRpb run's cell (t, r)
    if 1.0 in fracs:
        alone = TL._run_cli(tmp_path, "r", bam, fa, bed, P, spikeRpb=axes["spikeRpb"], **kw)
        same = 0
        for t in targets:
            for r in rpbs:
                theirs_at, suffix = alone + ".spikeAF%g.dsRpb%g" % (t, r), ".spikeAF%g.dsMT1.dsRpb%g" % (t, r)
                assert [x.replace(theirs_at.encode(), (got + suffix).encode()) for x in TL._read(theirs_at, SUFFIXES)] == mine[suffix], suffix
                same += 1
        assert same == T * Rr


def test_cli_cells_equal_the_two_step_workflow_on_the_synthetic_bam(tmp_path, capsys):
    bam, fa, loci, P, _ = R.synth_bam(str(tmp_path), RR.SYNTH_CFG)
    _cli_contract(tmp_path, bam, fa, loci, P, RR.pick_mixed(bam, fa, loci, 3), (0.2, 0.05), (1, 0.5), (1.5, 3), 4, False, capsys)


def test_cli_cells_equal_the_two_step_workflow_on_bam_cigars_with_lod(tmp_path, capsys):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    _cli_contract(tmp_path, bam, fa, loci, P, SR.pick_positions(bam, fa, loci, 3), (0.3, 0.1), (1, 0.5), (1.5, 3), 4, True, capsys)


def test_replicates_in_several_batches_are_the_replicates_in_one(tmp_path, capsys, monkeypatch):
    """A batch's copies are selected at all F x Rr pairs by one smc_select_alignments_reads_copies call over the masks of its
    consecutive seeds.  With room for three copies the four replicates go in batches of three and one - the second batch's masks
    start behind the first's - and every page and every cell's files are what the one-batch run writes."""
    from smcounter_amd import devplanes
    bam, fa, loci, P, _ = R.synth_bam(str(tmp_path), RR.SYNTH_CFG)
    variants = RR.pick_mixed(bam, fa, loci, 2)
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = R.write_variants(str(tmp_path / "v.vcf"), variants, vcf=True)
    kw = dict(spikeAF="0.2,0.05", spikeVariants=vfile, dsSeed=SEED, spikeDepth="1,0.5", spikeRpb="1.5,3", spikeReps=4)
    sizes, select = [], devplanes.select_copies_reads

    def spy(eng, runs, A, lo, d_masks, n_words, copy_stride_words, n_masks):
        sizes.append((len(runs), n_masks, copy_stride_words == n_masks * n_words))
        return select(eng, runs, A, lo, d_masks, n_words, copy_stride_words, n_masks)
    monkeypatch.setattr(devplanes, "select_copies_reads", spy)
    one = TL._run_cli(tmp_path, "one", bam, fa, bed, P, flags=["--spikeGrid"], **kw)
    assert sizes and {s for s in sizes} == {(4, 4, True)}                                    # (every call: 4 copies x 4 pairs)
    del sizes[:]
    monkeypatch.setattr(devplanes, "SPIKE_MAX_COPIES", 3)
    two = TL._run_cli(tmp_path, "two", bam, fa, bed, P, flags=["--spikeGrid"], **kw)
    assert {s for s in sizes} == {(3, 4, True), (1, 4, True)}
    capsys.readouterr()
    names = [f[len("one"):] for f in _files(tmp_path, "one")]
    assert names == [f[len("two"):] for f in _files(tmp_path, "two")] and ".spikeAF.grid.budget.txt" in names
    for n in names:
        a, b = open(one + n, "rb").read(), open(two + n, "rb").read()
        assert a == b.replace(two.encode(), one.encode()), n
