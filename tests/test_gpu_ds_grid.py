"""--dsGrid on the GPU: the composed philox rule over the file-wide table (smc_read_groups_counts_frac / _masks_grid / _kept_grid)
against the host restatement (tests/ds_grid_restate.py), and the command line's cells against the workflows they stand for - the
reference's three steps (tools.ds_mt, tools.ds_reads_within_mt, smCounter), or a philox --dsRpb run on a BAM of the philox barcodes."""
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import bamio, cli, devplanes
from smcounter_amd.py2compat import py2_round

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_grid_restate as gr  # noqa: E402
import ds_restate  # noqa: E402
import ds_rpb_philox_restate as rp  # noqa: E402
import ds_rpb_restate  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURES = ("case", "bam_cigars", "bam_overcap", "bam_deep")
FRACS = (0.1, 0.5, 1.0)
SEED = 1234567


def _fixture(name, tmp):
    return ds_restate.make_case(tmp) if name == "case" else ds_restate.load_fixture(name, tmp)


def _check_counts(eng, path, qn, chunk):
    """counts_frac of the table built from the file pass in chunks of `chunk` records == the restated counters per fraction."""
    g = gr.restate(qn, [(f, 2.0) for f in FRACS], SEED)
    groups = devplanes.ReadGroups(eng)
    try:
        bam = bamio.NativeBam(path)
        for first, keys in bam.name_keys(chunk, 4):
            groups.add(keys, first)
        bam.close()
        groups.finish()
        assert groups.status() == 0
        got = groups.counts_frac(SEED, [gr.frac_threshold(f) for f in FRACS])
        assert got == [g["fcounts"][f] for f in FRACS], (got, g["fcounts"])
        assert groups.counts_frac(SEED, []) == []
    finally:
        groups.close()
    return g


@pytest.mark.parametrize("name", FIXTURES)
def test_counts_frac_equals_the_restatement_on_the_fixtures(engine0, tmp_path, name):
    path = _fixture(name, str(tmp_path))[0]
    qn = ds_restate.placed_qnames(path)
    for chunk in (1 << 20, 7):
        g = _check_counts(engine0, path, qn, chunk)
    c = g["counts"]
    assert g["fcounts"][1.0] == dict(names=c["names"], barcodes=c["barcodes"], one=c["one"], multi=c["multi"],
                                     multi_names=c["multi_names"], first_names=c["barcodes"])


def test_counts_frac_equals_the_restatement_on_a_million_records(engine0, tmp_path):
    path = str(tmp_path / "names.bam")
    qn = rp.write_names_bam(path, 1_050_000)
    g1 = _check_counts(engine0, path, qn, 1 << 22)
    g2 = _check_counts(engine0, path, qn, 100_003)
    assert g1["fcounts"] == g2["fcounts"]
    assert 0 < g1["fcounts"][0.1]["barcodes"] < g1["fcounts"][0.5]["barcodes"] < g1["counts"]["barcodes"]


def _unpack(words, n_ids, n_masks):
    w = words.reshape(n_masks, -1)
    return [np.unpackbits(w[t].view(np.uint8), bitorder="little")[:n_ids].astype(bool) for t in range(n_masks)]


@pytest.mark.parametrize("name", FIXTURES)
def test_run_masks_and_kept_counts_are_the_restated_cells(engine0, tmp_path, name):
    bam_path, _, loci, P = _fixture(name, str(tmp_path))
    cells = [(f, r) for f in (0.5, 1.0) for r in (1.5, 2.0, 4.0)]
    g = gr.restate(ds_restate.placed_qnames(bam_path), cells, SEED)
    targets = devplanes.philox_read_rules(bam_path, (2.0,), [P], SEED, engine0, chunk=13)
    try:
        rules = devplanes.philox_grid_rules(bam_path, cells, [P] * len(cells), SEED, targets[0].groups)
        assert [(r.frac, r.target) for r in rules] == cells and all(r.groups is targets[0].groups and r.grid for r in rules)
        assert [r.prob_keep for r in rules] == g["probs"] and [r.thr for r in rules] == g["thr"]
        assert [r.bc_thr for r in rules] == g["bc_thr"] and [r.n_names for r in rules] == [g["fcounts"][f]["names"] for f, _ in cells]
        assert [r.n_kept for r in rules] == [len(k) for k in g["kept"]]
        assert [r.sampler for r in rules] == ["philox"] * len(cells) and rules[0].flag == "--dsGrid"
        bam = bamio.NativeBam(bam_path)
        for chrom, lo, hi in ds_restate.stretches(loci):
            A = bam.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
            idents, shared = bam.pair_idents(A["n_pair"])
            assert not shared
            buf, n_words, index = devplanes._run_read_masks(engine0, rules[0].groups, rules, idents, chrom, lo, A["nl"])
            m = _unpack(buf.download(np.uint32, n_words * len(rules)), len(idents), len(rules))
            buf.free()
            names = [bam.pair_name(k) for k in range(int(A["n_pair"]))]
            for rule, kept in zip(rules, g["kept"]):
                assert np.array_equal(m[index[id(rule)]], np.array([q in kept for q in names], bool)), rule.label
        bam.close()
        assert rules[0].groups.status() == 0
    finally:
        devplanes.close_rules(targets)


def _run_cli(tmp, tag, bam, fa, bed, P, grid=False, **kw):
    """The command line with these options (--dsGrid, a flag without a value, when `grid`) -> the output prefix."""
    prefix = str(tmp / tag)
    opts = dict(outPrefix=prefix, bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, hpLen=P.hpLen, minBQ=P.minBQ,
                minMQ=P.minMQ, mismatchThr=P.mismatchThr, mtDrop=P.mtDrop, maxMT=P.maxMT, primerDist=P.primerDist, refGenome=fa, **kw)
    argv = ["--%s=%s" % (k, v) for k, v in opts.items()] + (["--dsGrid"] if grid else [])
    cli.main(cli.build_parser().parse_args(argv))
    return prefix


def _files(prefix):
    return [open(prefix + s, "rb").read() for s in (".smCounter.all.txt", ".smCounter.cut.txt", ".smCounter.cut.vcf")]


def _assert_same(x_files, y_files, what):
    for x, y, suffix in zip(x_files, y_files, ("all.txt", "cut.txt", "cut.vcf")):
        if x != y:
            lx, ly = x.splitlines(), y.splitlines()
            k = next((i for i, (u, v) in enumerate(zip(lx, ly)) if u != v), min(len(lx), len(ly)))
            raise AssertionError("%s: %s differs (%d vs %d lines) at line %d:\n%r\n%r" % (what, suffix, len(lx), len(ly), k,
                                                                                        lx[k] if k < len(lx) else None, ly[k] if k < len(ly) else None))


CASES = [(n, None) for n in FIXTURES] + [("bam_deep", 40)]
GRID_F, GRID_R = (0.5, 0.25), (2.0, 4.0)


def _depth(f, P):
    return max(1, int(py2_round(f * P.mtDepth)))


@pytest.mark.parametrize("name,max_mt", CASES)
def test_cli_reference_cells_equal_the_three_step_workflow(tmp_path, name, max_mt):
    """Every cell's files byte for byte against smCounter at --mtDepth d_f --rpb r on write_rpb_bam(write_ds_bam(bam, f), r); the
    full-depth, fraction and target files byte-identical to the same run without --dsGrid.  Each reference run writes under the
    prefix of the file it is compared with (the VCF header names it), after that file has been read."""
    bam_path, fa, loci, P = _fixture(name, str(tmp_path))
    if max_mt:
        P = dataclasses.replace(P, maxMT=max_mt)
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    kw = dict(dsMT="0.5,0.25", dsRpb="2,4", dsSeed=SEED)
    alone = _run_cli(tmp_path, "o", bam_path, fa, bed, P, **kw)
    others = ["", ".dsMT0.5", ".dsMT0.25", ".dsRpb2", ".dsRpb4"]
    before = {s: _files(alone + s) for s in others}
    got = _run_cli(tmp_path, "o", bam_path, fa, bed, P, grid=True, **kw)
    for s in others:
        _assert_same(_files(got + s), before[s], "%s %s without and with --dsGrid" % (name, s or "full depth"))
    cells = {(f, r): _files("%s.dsMT%g.dsRpb%g" % (got, f, r)) for f in GRID_F for r in GRID_R}
    for f in GRID_F:
        ds_bam = ds_restate.write_ds_bam(bam_path, str(tmp_path / ("ds%g.bam" % f)), f, SEED)
        for r in GRID_R:
            rpb_bam = ds_rpb_restate.write_rpb_bam(ds_bam, str(tmp_path / ("ds%g_rpb%g.bam" % (f, r))), r, SEED)
            want = _run_cli(tmp_path, "o.dsMT%g.dsRpb%g" % (f, r), rpb_bam, fa, bed, dataclasses.replace(P, mtDepth=_depth(f, P), rpb=r))
            _assert_same(cells[(f, r)], _files(want), "%s f=%g r=%g" % (name, f, r))


@pytest.mark.parametrize("name,max_mt", CASES)
def test_cli_philox_cells_equal_philox_targets_on_the_kept_barcodes(tmp_path, name, max_mt):
    """Every cell's files against --dsRpb r --dsRpbSampler philox --dsRpbMtDepth d_f on write_kept_bam of the restated philox barcode
    set at f; the same cells with runs cut small (--batchReads 20)."""
    bam_path, fa, loci, P = _fixture(name, str(tmp_path))
    if max_mt:
        P = dataclasses.replace(P, maxMT=max_mt)
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    g = gr.restate(ds_restate.placed_qnames(bam_path), [(f, r) for f in GRID_F for r in GRID_R], SEED)
    kw = dict(dsMT="0.5,0.25", dsRpb="2,4", dsSampler="philox", dsRpbSampler="philox", dsSeed=SEED)
    got = _run_cli(tmp_path, "o", bam_path, fa, bed, P, grid=True, **kw)
    mine = {(f, r): _files("%s.dsMT%g.dsRpb%g" % (got, f, r)) for f in GRID_F for r in GRID_R}
    cut = _run_cli(tmp_path, "c", bam_path, fa, bed, P, grid=True, batchReads=20, **kw)
    cut_files = {(f, r): _files("%s.dsMT%g.dsRpb%g" % (cut, f, r)) for f in GRID_F for r in GRID_R}
    for f in GRID_F:
        kb = ds_restate.write_kept_bam(bam_path, str(tmp_path / ("kept%g.bam" % f)), gr.kept_barcodes(g, f))
        d = _depth(f, P)
        for tag, files in (("o", mine), ("c", cut_files)):
            want = _run_cli(tmp_path, "%s.dsMT%g" % (tag, f), kb, fa, bed, P, dsRpb="2,4", dsRpbSampler="philox",
                            dsRpbMtDepth="%d,%d" % (d, d), dsSeed=SEED)
            for r in GRID_R:
                _assert_same(files[(f, r)], _files("%s.dsRpb%g" % (want, r)), "%s f=%g r=%g (%s)" % (name, f, r, tag))


def test_cli_philox_cell_without_a_multi_name_barcode_is_refused_and_frees_the_table(tmp_path, monkeypatch):
    """A file whose one barcode of several names is dropped by the --dsMT philox draw at 0.5: the cell (0.5, 2) is refused before any
    file is written, and the targets' file-wide table in HBM is freed."""
    import bam_fixture
    from smcounter_amd.tools import ds_reads_within_mt as rw
    case = bam_fixture.make_case(str(tmp_path))
    qn = ds_restate.placed_qnames(case["bam"])
    per_bc, order = rw.group_reads(qn)
    drawn = gr.bc_draws(rp.fnv64(order), SEED)
    multi = next(bc for bc, u in zip(order, drawn.tolist()) if len(per_bc[bc]) > 1 and u >= gr.frac_threshold(0.5))
    bam = gr.one_multi_barcode_bam(case["bam"], str(tmp_path / "onemulti.bam"), multi)
    seen = []
    grid_rules = devplanes.philox_grid_rules

    def spy(path, cells, params_list, seed, groups):
        seen.append(groups)
        return grid_rules(path, cells, params_list, seed, groups)
    monkeypatch.setattr(devplanes, "philox_grid_rules", spy)
    argv = ["--outPrefix=%s" % (tmp_path / "o"), "--bamFile=%s" % bam, "--bedTarget=%s" % case["bed"], "--mtDepth=12", "--rpb=3.0",
            "--hpLen=8", "--refGenome=%s" % case["fasta"], "--dsMT=1,0.5", "--dsRpb=2", "--dsSampler=philox", "--dsRpbSampler=philox",
            "--dsSeed=%d" % SEED, "--dsGrid"]
    with pytest.raises(SystemExit, match=r"--dsGrid fraction 0\.5 x target 2: no barcode kept at 0\.5 in .*onemulti\.bam has more "
                                         r"than one read name"):
        cli.main(cli.build_parser().parse_args(argv))
    assert len(seen) == 1 and seen[0]._h is None                     # (the table: freed)
    assert not [f for f in os.listdir(str(tmp_path)) if ".smCounter." in f]
