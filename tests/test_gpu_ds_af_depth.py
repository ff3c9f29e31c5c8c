"""--dsAFDepth on the GPU: smc_af_depth_masks / smc_af_depth_counts against the restatement (tests/ds_af_depth_restate.py), bit for
bit; f = 1 against smc_af_rep_masks and smc_af_rep_counts; the device depth draw against devplanes.philox_keep_host; the command line's cells against the
two-step workflow they replace (tools.ds_allele_fraction, then --dsMT --dsSampler philox on its BAM), against separate runs with
--dsSeed s_j, and its tables against what the test computes from the replicate lines."""
import argparse
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, bamio, devplanes, dsaf
from smcounter_amd.engine import DevBuf
from smcounter_amd.py2compat import py2_round
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_depth_restate as DR  # noqa: E402
import ds_af_reps_restate as RR  # noqa: E402
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import test_ds_af_depth as TD  # noqa: E402  (check_bounds and its fixed inputs)
import test_gpu_ds_af_reps as TR  # noqa: E402  (its helpers: fixtures, the tool's sets, the deep synthetic run)
import test_gpu_lod as TL  # noqa: E402  (a run of the command line)

pytestmark = pytest.mark.gpu
SEED = 7
REPS = 3
TARGETS = (0.02, 0.2, 0.9)              # (0.9 lies above every fraction met: k = 1, a threshold of exactly 2^32)
FRACS = (0.3, 1.0, 0.05)                # (1.0: a depth threshold of exactly 2^32 - the masks of smc_af_rep_masks)
SUFFIXES = TR.SUFFIXES


def _table(eng, covers, carries, targets, fracs, seeds):
    thr = RR.thresholds(covers, carries, targets)
    idents, table = dsaf.carrier_table(carries, thr)
    return devplanes.AfDepthTable(eng, idents, table, seeds, [devplanes.frac_threshold(f) for f in fracs]), idents, table


def _device(eng, run_idents, covers, carries, targets, fracs, seed, n_reps, draws=False):
    """The two calls over one run's identities -> (masks uint32 [R, T, F, n_words], counts uint32 [V, R, T, F, 2], the table's
    identities, the depth draws, smc_af_rep_masks' masks [R, T, n_words] and smc_af_rep_counts' counts [V, R, T, 2] of the same
    table)."""
    tab, idents, _ = _table(eng, covers, carries, targets, fracs, dsaf.rep_seeds(seed, n_reps))
    n, cells = len(run_idents), len(targets) * len(fracs)
    n_words = devplanes.mask_words(n)
    d_id = DevBuf(eng, 8 * max(1, n) + 256).upload(np.ascontiguousarray(run_idents, np.uint64) if n else np.zeros(1, np.uint64))
    d_m = DevBuf(eng, 4 * n_reps * cells * n_words + 256)
    d_m.upload(np.full(n_reps * cells * n_words, 0xA5A5A5A5, np.uint32))          # (every word must be written)
    d_p = DevBuf(eng, 4 * n_reps * len(targets) * n_words + 256)
    d_u = DevBuf(eng, 4 * n_reps * max(1, n) + 256) if draws else None
    try:
        tab.masks(d_id.data_ptr(), n, d_m.data_ptr(), n_words, d_u.data_ptr() if draws else None)
        masks = d_m.download(np.uint32, n_reps * cells * n_words).reshape(n_reps, len(targets), len(fracs), n_words)
        u = d_u.download(np.uint32, n_reps * n).reshape(n_reps, n) if draws else None
        plain_tab = devplanes.AfRepTable(eng, tab.idents, tab.thr, tab.seeds)
        try:
            plain_tab.masks(d_id.data_ptr(), n, d_p.data_ptr(), n_words)
            plain = d_p.download(np.uint32, n_reps * len(targets) * n_words).reshape(n_reps, len(targets), n_words)
            plain_counts = plain_tab.counts(covers, carries)
        finally:
            plain_tab.free()
        counts = tab.counts(covers, carries)
    finally:
        for b in (d_id, d_m, d_p, d_u):
            if b is not None:
                b.free()
        tab.free()
    return masks, counts, idents, u, plain, plain_counts


def _check(eng, run_idents, covers, carries, targets=TARGETS, fracs=FRACS, seed=SEED, n_reps=REPS):
    """masks and counts == the restatement, bit for bit; the f = 1 masks and counts == smc_af_rep_masks' and smc_af_rep_counts' ->
    (mask words compared, counters compared, carriers of the table)."""
    keep, want = DR.restate(run_idents, covers, carries, targets, fracs, seed, n_reps)
    masks, counts, idents, _, plain, plain_counts = _device(eng, run_idents, covers, carries, targets, fracs, seed, n_reps)
    n_words = devplanes.mask_words(len(run_idents))
    assert masks.shape == (n_reps, len(targets), len(fracs), n_words)
    assert np.array_equal(masks, RR.pack(keep, n_words))
    assert counts.shape == want.shape == (len(covers), n_reps, len(targets), len(fracs), 2) and np.array_equal(counts, want)
    ones = [k for k, f in enumerate(fracs) if f >= 1.0]
    for k in ones:
        assert np.array_equal(masks[:, :, k], plain)
        assert plain_counts.shape == (len(covers), n_reps, len(targets), 2) and np.array_equal(counts[:, :, :, k], plain_counts)
    assert ones or fracs != FRACS
    return masks.size, counts.size, len(idents)


def _check_all_tables(eng, run_idents, covers, carries):
    """The fixture's own table, then a table of one carrier and of zero carriers over the same run."""
    words, counters, n_car = _check(eng, run_idents, covers, carries)
    with_carriers = [v for v in range(len(carries)) if len(carries[v])]
    if with_carriers:
        v = with_carriers[0]
        one = [np.asarray(c)[:1] if k == v else np.asarray(c)[:0] for k, c in enumerate(carries)]
        assert _check(eng, run_idents, covers, one)[2] == 1
    assert _check(eng, run_idents, covers, [np.asarray(c)[:0] for c in carries])[2] == 0
    return words, counters, n_car


@pytest.mark.parametrize("name", TR.FIXTURES)
def test_masks_and_counts_equal_the_restatement_on_the_fixtures(engine0, tmp_path, name):
    bam_path, fa, loci, P = TR._fixture(name, str(tmp_path))
    bam = bamio.NativeBam(bam_path)
    runs = carriers = 0
    try:
        for chrom, lo, hi in ds_restate.stretches(loci):
            here = [(chrom, p) for p in range(lo + 1, hi + 1)]
            variants = R.pick_variants(bam_path, fa, here)
            covers, carries = TR._sets(bam_path, fa, variants)
            A = bam.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
            run_idents = bam.barcode_idents(A["n_bc"])
            words, counters, n_car = _check_all_tables(engine0, run_idents, covers, carries)
            assert words == REPS * len(TARGETS) * len(FRACS) * devplanes.mask_words(int(A["n_bc"]))
            assert counters == len(variants) * REPS * len(TARGETS) * len(FRACS) * 2
            runs += 1
            carriers += n_car
    finally:
        bam.close()
    assert runs == len(ds_restate.stretches(loci)) and runs >= 1
    if name != "bam_overcap":
        assert carriers > 0


def test_masks_and_counts_equal_the_restatement_on_a_deep_synthetic_run(engine0, tmp_path):
    bam_path, fa, here, P = TR._deep(tmp_path)
    variants = R.planted(bam_path, fa, here, limit=3) + R.pick_variants(bam_path, fa, here)
    seen = set()
    variants = [v for v in variants if not ((v.chrom, v.pos) in seen or seen.add((v.chrom, v.pos)))]      # (one variant per position)
    covers, carries = TR._sets(bam_path, fa, variants)
    bam = bamio.NativeBam(bam_path)
    try:
        A = bam.alignments_run(here[0][0], here[0][1] - 1, here[-1][1], ds_restate.BIG, P, 2)
        run_idents = bam.barcode_idents(A["n_bc"])
    finally:
        bam.close()
    assert int(A["n_bc"]) > 64 and devplanes.mask_words(int(A["n_bc"])) >= 3                    # (masks span several words)
    words, counters, n_car = _check_all_tables(engine0, run_idents, covers, carries)
    assert n_car > 1 and counters == len(variants) * REPS * len(TARGETS) * len(FRACS) * 2
    # 32 cells in one launch, the most a call takes
    _check(engine0, run_idents, covers, carries, targets=(0.01, 0.02, 0.05, 0.2), fracs=(0.02, 0.05, 0.1, 0.2, 0.3, 0.5, 0.75, 1.0), n_reps=2)


def test_device_counts_hold_the_binomial_widths(engine0, tmp_path):
    """The bounds of tests/test_ds_af_depth.py - each variant listed alone, and all together - same input and seed, on
    smc_af_depth_counts' numbers."""
    covers, carries, _ = TD._synth(tmp_path)

    def counts_of(cov, car):
        tab, _, _ = _table(engine0, cov, car, TD.TARGETS, TD.FRACS, [TD.SEED])
        try:
            return tab.counts(cov, car)
        finally:
            tab.free()
    assert TD.check_bounds(counts_of, covers, carries) >= 12
    assert TD.check_joint_bounds(counts_of, covers, carries) >= 12                 # (all variants listed together, as a run lists them)


def test_device_depth_draw_equals_philox_keep_host(engine0):
    rng = np.random.RandomState(20240607)
    ids = np.unique(rng.randint(0, 1 << 62, 4200).astype(np.uint64) * np.uint64(3) + np.uint64(1))[:4096]
    assert len(ids) == 4096
    run = ids[rng.permutation(len(ids))]
    seeds, fracs = [7, (1 << 32) + 5, RR.M64], (0.5, 0.013, 1.0)
    tab = devplanes.AfDepthTable(engine0, ids[:0], np.zeros((0, 1), np.uint64), np.array(seeds, np.uint64), [devplanes.frac_threshold(f) for f in fracs])
    n_words = devplanes.mask_words(len(run))
    d_id = DevBuf(engine0, 8 * len(run) + 256).upload(run)
    d_m, d_u = DevBuf(engine0, 4 * 9 * n_words + 256), DevBuf(engine0, 4 * 3 * len(run) + 256)
    try:
        tab.masks(d_id.data_ptr(), len(run), d_m.data_ptr(), n_words, d_u.data_ptr())
        u = d_u.download(np.uint32, 3 * len(run)).reshape(3, len(run))
        m = d_m.download(np.uint32, 9 * n_words).reshape(3, 1, 3, n_words)
    finally:
        for b in (d_id, d_m, d_u):
            b.free()
        tab.free()
    L = _lib.load()
    compared = 0
    for j, s in enumerate(seeds):
        assert np.array_equal(u[j].astype(np.uint64), DR.depth_draw(run, s))
        for k, f in enumerate(fracs):
            want = devplanes.philox_keep_host(L, run, f, s)
            assert np.array_equal(m[j, 0, k], RR.pack(want, n_words))
            assert np.array_equal(u[j].astype(np.uint64) < np.uint64(devplanes.frac_threshold(f)), want)
            compared += len(want)
    assert compared == 9 * 4096 and len({u[j].tobytes() for j in range(3)}) == 3


def test_refusals_of_the_two_calls(engine0):
    ids = np.array([5, 9, 9, 12], np.uint64)
    thr = np.full((4, 1), 1 << 31, np.uint64)
    d = DevBuf(engine0, 4096)
    half = [1 << 31]
    for bad_ids, bad_thr, depth, msg in ((ids, thr, half, "not strictly ascending"),
                                         (ids[[0, 1, 3]], np.full((3, 1), (1 << 32) + 1, np.uint64), half, r"above 2\^32"),
                                         (ids[[0, 1, 3]], thr[:3], [(1 << 32) + 1], r"depth threshold 0 is above 2\^32"),
                                         (ids[[0, 1, 3]], np.full((3, 3), 1, np.uint64), [1 << 31] * 11, "at most 32 cells"),
                                         (ids[[0, 1, 3]], np.full((3, 33), 1, np.uint64), half, "at most 32")):
        tab = devplanes.AfDepthTable(engine0, bad_ids, bad_thr, np.array([1, 2], np.uint64), depth)
        try:
            with pytest.raises(_lib.SmcError, match=msg):
                tab.masks(d.data_ptr(), 4, d.data_ptr(), devplanes.mask_words(4))
            with pytest.raises(_lib.SmcError, match=msg):
                tab.counts([ids[:1]], [ids[:1]])
        finally:
            tab.free()
    tab = devplanes.AfDepthTable(engine0, ids[[0, 1, 3]], thr[:3], np.arange(1001, dtype=np.uint64), half)
    try:
        with pytest.raises(_lib.SmcError, match="at most 1000"):
            tab.masks(d.data_ptr(), 4, d.data_ptr(), devplanes.mask_words(4))
    finally:
        tab.free()
    tab = devplanes.AfDepthTable(engine0, ids[[0, 1, 3]], thr[:3], np.array([1, 2], np.uint64), half)
    try:
        with pytest.raises(_lib.SmcError, match="words per mask"):
            tab.masks(d.data_ptr(), 100, d.data_ptr(), 2)
        with pytest.raises(_lib.SmcError, match="too many mask words"):
            tab.masks(d.data_ptr(), 64, d.data_ptr(), 1 << 31)
    finally:
        tab.free()
        d.free()


def _files(tmp_path, tag):
    return sorted(f for f in os.listdir(str(tmp_path)) if f.startswith(tag + "."))


def _strip(line):
    """A depth line without FRACTION and MTDEPTH: the plain format."""
    return line[:5] + line[7:]


def _cli_contract(tmp_path, bam, fa, loci, P, variants, targets, fracs, n_reps, lod):
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = R.write_variants(str(tmp_path / "v.vcf"), variants, vcf=True)
    flags = ["--lod"] if lod else []
    T, F, V = len(targets), len(fracs), len(variants)
    kw = dict(dsAF=",".join("%g" % t for t in targets), dsAFVariants=vfile, dsSeed=SEED)
    depth = ",".join("%g" % f for f in fracs)
    cells = [(t, f, max(1, int(py2_round(f * P.mtDepth))), ".dsAF%g.dsMT%g" % (t, f)) for t in targets for f in fracs]
    # 1. every file of a run without the flag is unchanged (the LOD summary keeps its lines and gets one per cell)
    TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, dsAFReps=n_reps, **kw)
    names = _files(tmp_path, "o")
    old = {f: open(str(tmp_path / f), "rb").read() for f in names}
    assert {"o.dsAF.detection.txt", "o.dsAF.replicates.txt", "o.dsAF.sensitivity.txt"} <= set(names)
    assert len(names) == (3 + 2 * bool(lod)) * (1 + T) + 3 + bool(lod)
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, dsAFReps=n_reps, dsAFDepth=depth, **kw)
    added = sorted(set(_files(tmp_path, "o")) - set(names))
    want_added = ["o" + c[3] + s for c in cells for s in SUFFIXES + (TL.LOD_SUFFIXES if lod else ())] + \
                 ["o.dsAF.depth.%s.txt" % x for x in ("detection", "replicates", "sensitivity", "curve")]
    assert added == sorted(want_added)
    same = 0
    for f in names:
        now = open(str(tmp_path / f), "rb").read()
        if f == "o.lod.summary.txt":
            assert now.startswith(old[f]) and len(now.splitlines()) == len(old[f].splitlines()) + len(cells)
            assert [l.split(b"\t")[:2] for l in now.splitlines()[-len(cells):]] == [[os.path.basename(got + c[3]).encode(), b"%d" % c[2]] for c in cells]
        else:
            assert now == old[f], "%s changed with --dsAFDepth" % f
        same += 1
    assert same == len(names)
    mine = {c[3]: TL._read(got + c[3], SUFFIXES) for c in cells}
    if lod:
        for c in cells:
            assert TL._read(got + c[3], TL.LOD_SUFFIXES) == TL._tool_files(tmp_path, got + c[3] + SUFFIXES[0], "UMT", c[2]), c
    # 2. the detection page: the cells' counts are the restatement's, its lines the cells' own files
    det = TR._lines(got + ".dsAF.depth.detection.txt")
    assert det[0] == list(dsaf.DEPTH_DETECTION_HEADER) + (["LOD"] if lod else []) and len(det) == 1 + V * T * F
    covers, carries = TR._sets(bam, fa, variants)
    _, counts = DR.restate(np.zeros(0, np.uint64), covers, carries, targets, fracs, SEED, n_reps)
    plain_det = TR._lines(got + ".dsAF.detection.txt")
    for i, v in enumerate(variants):
        for c, (t, f, d, suffix) in enumerate(cells):
            l = det[1 + i * T * F + c]
            assert l[:7] == [v.chrom, "%d" % v.pos, v.ref, v.alt, "%g" % t, "%g" % f, "%d" % d]
            assert l[7:9] == ["%d" % x for x in counts[i, 0, c // F, c % F]]
            assert l[10] == plain_det[1 + i * (1 + T) + 1 + c // F][8]                       # (K: the target's)
            rows, cut = dsaf.read_output(got + suffix)
            assert _strip(l) == dsaf.detection_line(v, t, int(l[7]), int(l[8]), float(l[10]), rows.get((v.chrom, "%d" % v.pos)),
                                                    cut.get((v.chrom, "%d" % v.pos)), float(l[17]) if lod else None).split("\t")
    # 3. every replicate line is the detection line of a separate run with --dsSeed s_j
    reps = TR._lines(got + ".dsAF.depth.replicates.txt")
    assert reps[0] == list(dsaf.DEPTH_REPLICATES_HEADER) and len(reps) == 1 + V * T * F * n_reps
    compared = 0
    for j, s in enumerate(RR.seeds(SEED, n_reps)):
        ref = TL._run_cli(tmp_path, "s%d" % j, bam, fa, bed, P, dsAFDepth=depth, **dict(kw, dsSeed=s))
        one = TR._lines(ref + ".dsAF.depth.detection.txt")
        assert one[0] == list(dsaf.DEPTH_DETECTION_HEADER) and len(one) == 1 + V * T * F
        for i in range(V):
            for c in range(T * F):
                line = reps[1 + (i * T * F + c) * n_reps + j]
                assert line[7:9] == ["%d" % j, "%d" % s]
                assert line[:7] + line[9:] == one[1 + i * T * F + c], (i, c, j)
                assert line[9:11] == ["%d" % x for x in counts[i, j, c // F, c % F]]
                compared += 1
        if j == 0:
            assert [l[:17] for l in det[1:]] == one[1:]
    assert compared == V * T * F * n_reps
    # 4. the sensitivity table and the curve are what the replicate lines say
    sens = TR._lines(got + ".dsAF.depth.sensitivity.txt")
    assert sens[0] == list(dsaf.DEPTH_SENSITIVITY_HEADER) + (["LOD"] if lod else [])
    flat = [l[:5] + l[7:] for l in reps[1:]]                                               # (REP SEED behind TARGET: the plain replicate line)
    want = TR._sensitivity_from(flat, variants, [c[0] for c in cells], n_reps)
    assert len(sens) == 1 + V * T * F == 1 + len(want)
    for i in range(V):
        for c, (t, f, d, _) in enumerate(cells):
            k = i * T * F + c
            per = reps[1 + k * n_reps:1 + (k + 1) * n_reps]
            n_mean = dsaf.frac_text(sum(int(l[9]) for l in per) / float(n_reps))
            assert sens[1 + k][:20] == want[k][:5] + ["%g" % f, "%d" % d] + want[k][5:] + [n_mean]
            if lod:
                assert sens[1 + k][20] == det[1 + k][17]
    curve = TR._lines(got + ".dsAF.depth.curve.txt")
    order = sorted(range(T), key=lambda t: targets[t])
    assert curve[0] == list(dsaf.CURVE_HEADER) + ["RATE@%g" % targets[t] for t in order] + ["T95"] + (["LOD"] if lod else [])
    assert len(curve) == 1 + V * (1 + F)
    plain = TR._lines(got + ".dsAF.replicates.txt")[1:]
    top = max(range(T), key=lambda t: targets[t])
    full_lod = TR._lines(got + ".dsAF.detection.txt") if lod else None
    for i, v in enumerate(variants):
        for k, f in enumerate([None] + list(fracs)):
            if f is None:
                per = [plain[(i * T + t) * n_reps:(i * T + t + 1) * n_reps] for t in range(T)]
                ns, called, depth_text = [[int(l[7]) for l in p] for p in per], [[int(l[16]) for l in p] for p in per], "%d" % P.mtDepth
            else:
                at = [1 + (i * T * F + t * F + k - 1) * n_reps for t in range(T)]
                per = [reps[a:a + n_reps] for a in at]
                ns, called, depth_text = [[int(l[9]) for l in p] for p in per], [[int(l[18]) for l in p] for p in per], "%d" % cells[k - 1][2]
            rates = [sum(c) / float(n_reps) for c in called]
            best = DR.t95(targets, rates)
            line = curve[1 + i * (1 + F) + k]
            assert line[:7] == [v.chrom, "%d" % v.pos, v.ref, v.alt, "full" if f is None else "%g" % f, depth_text,
                                dsaf.frac_text(sum(sum(n) / float(n_reps) for n in ns) / T)]
            assert line[7:8 + T] == [dsaf.frac_text(rates[t]) for t in order] + ["NA" if best is None else "%g" % best]
            if lod:
                assert line[8 + T] == (full_lod[1 + i * (1 + T) + 1 + top][15] if f is None else det[1 + i * T * F + top * F + k - 1][17])
    # 5. the specification: a cell is the .dsMT<f> output of --dsMT f --dsSampler philox on the BAM the tool writes for t.  The workflow
    # writes under a prefix of its own; the .cut.vcf names its prefix in the sample column, so that one word is mapped before comparing
    checked = 0
    for t in targets:
        out = str(tmp_path / ("af%g.bam" % t))
        af.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=SEED, refGenome=fa))
        bamio.write_bai(out)
        ref = TL._run_cli(tmp_path, "w.dsAF%g" % t, out, fa, bed, P, dsMT=depth, dsSampler="philox", dsSeed=SEED)
        for f in fracs:
            suffix = ".dsAF%g.dsMT%g" % (t, f)
            theirs = [x.replace((ref + ".dsMT%g" % f).encode(), (got + suffix).encode()) for x in TL._read(ref + ".dsMT%g" % f, SUFFIXES)]
            assert TL._read(got + suffix, SUFFIXES) == mine[suffix]                          # (nothing wrote over the cell's files)
            for a, b, s in zip(mine[suffix], theirs, SUFFIXES):
                assert a == b, "cell %s: %s differs from the two-step workflow's" % (suffix, s)
            checked += 1
    assert checked == T * F
    return det, curve


def test_cli_cells_equal_the_two_step_workflow_on_the_case_fixture(tmp_path):
    bam, fa, loci, P = ds_restate.make_case(str(tmp_path))
    variants = R.pick_variants(bam, fa, loci)
    assert variants
    _cli_contract(tmp_path, bam, fa, loci, P, variants, (0.05, 0.2), (0.5, 0.25), 4, lod=False)


def test_cli_cells_equal_the_two_step_workflow_on_bam_cigars_with_lod(tmp_path):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    variants = R.pick_variants(bam, fa, loci)
    assert {"SNV", "INS", "DEL"} <= {"SNV" if len(v.key) == 1 else v.key[:3] for v in variants}
    _cli_contract(tmp_path, bam, fa, loci, P, variants, (0.2, 0.05), (0.5, 1.0), 4, lod=True)
