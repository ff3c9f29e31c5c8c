"""--dsGrid without a GPU: the reference cells' kept names against the three-step workflow (tools.ds_mt, then
tools.ds_reads_within_mt on its BAM), the philox cells' restatement (tests/ds_grid_restate.py) against a philox --dsRpb restatement on
the kept barcodes' names, the barcode identities the composed draw rests on, and the flags and their refusals."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, bamio, cli, devplanes
from smcounter_amd.tools import ds_reads_within_mt as rw
from smcounter_amd.tools.ds_mt import barcode_of

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_grid_restate as gr  # noqa: E402
import ds_restate  # noqa: E402
import ds_rpb_philox_restate as rp  # noqa: E402
import ds_rpb_restate  # noqa: E402

FIXTURES = ("case", "bam_cigars", "bam_overcap", "bam_deep")
FRACS = (0.3, 0.5, 1.0)
TARGETS = (2.0, 4.0)
SEED = 1234567


def _fixture(name, tmp):
    return ds_restate.make_case(tmp) if name == "case" else ds_restate.load_fixture(name, tmp)


def _reference_cells(path, P, fracs, targets):
    cells = [(f, r) for f in fracs for r in targets]
    frac_rules = devplanes.reference_rules(path, fracs, [P] * len(fracs), SEED)
    grouped = devplanes.group_placed_reads(path)
    rules = devplanes.reference_grid_rules(path, cells, [P] * len(cells), SEED, {r.frac: r.kept for r in frac_rules}, grouped)
    return cells, rules, grouped


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_cells_are_the_three_step_workflows(name, tmp_path):
    path, _, _, P = _fixture(name, str(tmp_path))
    cells, rules, _ = _reference_cells(path, P, FRACS, TARGETS)
    assert [(r.frac, r.target) for r in rules] == cells
    assert all(r.grid and r.level == "read" and r.sampler == "reference" and r.flag == "--dsGrid" for r in rules)
    for f in FRACS:
        qn = ds_restate.placed_qnames(ds_restate.write_ds_bam(path, str(tmp_path / ("ds%g.bam" % f)), f, SEED))
        for r in TARGETS:
            rule = rules[cells.index((f, r))]
            kept, prob = rw.select_reads(qn, r, SEED)
            assert rule.kept == kept, (f, r)
            assert rule.prob_keep == prob                                          # (bit for bit)
            assert rule.n_names == len(dict.fromkeys(qn))
            assert rule.label == "fraction %g x target %g" % (f, r)
            if rule.kept_idents is not None:
                assert np.array_equal(rule.kept_idents, np.sort(devplanes.fnv64_array(sorted(kept))))
    # (the cells differ from fraction to fraction: the second script's stream runs over another set of barcodes)
    assert rules[cells.index((0.3, 2.0))].kept != rules[cells.index((1.0, 2.0))].kept


@pytest.mark.parametrize("name", FIXTURES)
def test_fraction_one_cells_are_the_targets(name, tmp_path):
    path, _, _, P = _fixture(name, str(tmp_path))
    cells, rules, grouped = _reference_cells(path, P, (1.0,), TARGETS)
    alone = devplanes.reference_read_rules(path, TARGETS, [P] * len(TARGETS), SEED)
    again = devplanes.reference_read_rules(path, TARGETS, [P] * len(TARGETS), SEED, grouped=grouped)
    for c, a, b in zip(rules, alone, again):
        assert c.kept == a.kept == b.kept and c.prob_keep == a.prob_keep == b.prob_keep and c.n_names == a.n_names


@pytest.mark.parametrize("name", FIXTURES)
def test_name_keys_barcode_identities_are_the_decoders(name, tmp_path):
    """The composed draw takes a name's barcode identity from the file pass (smc_bam_name_keys); --dsSampler philox draws over the
    decoder's (smc_bam_barcode_idents).  They must be one hash of one text."""
    path, _, loci, P = _fixture(name, str(tmp_path))
    bam = bamio.NativeBam(path)
    keys = np.concatenate([k.copy() for _, k in bam.name_keys(1 << 20, 2)])
    qn = ds_restate.placed_qnames(path)
    of_text = dict(zip((barcode_of(q) for q in qn), keys[:, 1].tolist()))
    seen = 0
    for chrom, lo, hi in ds_restate.stretches(loci):
        A = bam.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
        idents = bam.barcode_idents(A["n_bc"])
        for g in range(int(A["n_bc"])):
            assert of_text[bam.barcode_name(g)] == int(idents[g])
            seen += 1
    bam.close()
    assert seen


@pytest.mark.parametrize("name", FIXTURES)
def test_philox_cell_is_a_philox_target_on_the_kept_barcodes(name, tmp_path):
    path = _fixture(name, str(tmp_path))[0]
    qn = ds_restate.placed_qnames(path)
    cells = [(f, r) for f in (0.1, 0.5, 1.0) for r in (1.5, 2.0, 4.0)]
    g = gr.restate(qn, cells, SEED)
    L = _lib.load(with_torch=False)
    bc_ident = rp.fnv64(g["barcode"])
    for f in (0.1, 0.5, 1.0):
        # the numpy barcode draw is the library's --dsMT rule
        assert np.array_equal(g["bc_keep"][f], devplanes.philox_keep_host(L, bc_ident, f, SEED)), f
    for (f, r), kept, p in zip(cells, g["kept"], g["probs"]):
        keep = gr.kept_barcodes(g, f)
        sub = [q for q in qn if barcode_of(q) in keep]
        if not sub:
            continue
        want = rp.restate(sub, (r,), SEED)
        assert want["counts"]["names"] == g["fcounts"][f]["names"]
        assert kept == want["kept"][0] and p == want["probs"][0], (f, r)
    assert any(0 < len(k) < len(g["names"]) for k in g["kept"])


def test_frac_threshold_is_the_select_rule():
    assert devplanes.frac_threshold(1.0) == 1 << 32 and devplanes.frac_threshold(0.5) == 1 << 31
    assert devplanes.frac_threshold(0.1) == int(np.floor(0.1 * 4294967296.0)) == gr.frac_threshold(0.1)


BASE = ["--outPrefix", "o/x", "--bamFile", "a.bam", "--bedTarget", "t.bed", "--mtDepth", "3612", "--rpb", "8.6"]


def test_flags_parse_and_name_the_outputs():
    p = cli.build_parser()
    assert p.parse_args(BASE).dsGrid is False and cli.ds_grid_cells(p.parse_args(BASE + ["--dsMT", "0.5", "--dsRpb", "2"])) == []
    a = p.parse_args(BASE + ["--dsMT", "0.5,0.25", "--dsRpb", "2,4", "--dsGrid"])
    assert a.dsGrid is True
    assert cli.ds_grid_cells(a) == [(0.5, 2.0, 1806, "o/x.dsMT0.5.dsRpb2"), (0.5, 4.0, 1806, "o/x.dsMT0.5.dsRpb4"),
                                    (0.25, 2.0, 903, "o/x.dsMT0.25.dsRpb2"), (0.25, 4.0, 903, "o/x.dsMT0.25.dsRpb4")]
    a = p.parse_args(BASE + ["--dsMT", "1,0.1", "--dsMtDepth", "7,5", "--dsRpb", "3", "--dsRpbMtDepth", "9", "--dsGrid"])
    assert cli.ds_grid_cells(a) == [(1.0, 3.0, 7, "o/x.dsMT1.dsRpb3"), (0.1, 3.0, 5, "o/x.dsMT0.1.dsRpb3")]
    a = p.parse_args(BASE + ["--dsMT", "0.5", "--dsRpb", "2", "--dsGrid", "--dsSampler", "philox", "--dsRpbSampler", "philox"])
    assert cli.ds_rpb_targets(a) == [(2.0, 3612, "o/x.dsRpb2")] and len(cli.ds_grid_cells(a)) == 1
    help_text = " ".join(p.format_help().split())
    assert "--dsGrid" in help_text and "dsMT<f>.dsRpb<r>" in help_text
    assert "philox is not available here" in help_text and "no cross product" in help_text


@pytest.mark.parametrize("extra,msg", [
    (["--dsRpb", "2"], "needs both --dsMT and --dsRpb"),
    (["--dsMT", "0.5"], "needs both --dsMT and --dsRpb"),
    ([], "needs both --dsMT and --dsRpb"),
    (["--dsMT", "0.5", "--dsRpb", "2", "--dsSampler", "philox"], "--dsSampler philox and --dsRpbSampler reference"),
    (["--dsMT", "0.5", "--dsRpb", "2", "--dsRpbSampler", "philox"], "--dsSampler reference and --dsRpbSampler philox"),
    (["--dsMT", "0.5", "--dsRpb", "2", "--dsSampler", "philox", "--dsRpbSampler", "reference"], "--dsSampler philox and --dsRpbSampler"),
    (["--dsMT", "0.1,0.2,0.3,0.4,0.5,0.6", "--dsRpb", "1,2,3,4,5,6"], "36 cells, at most 32"),
])
def test_refusals_of_the_flags(extra, msg):
    with pytest.raises(SystemExit, match=msg):
        cli.ds_grid_cells(cli.build_parser().parse_args(BASE + extra + ["--dsGrid"]))


def test_thirty_two_cells_are_taken():
    a = cli.build_parser().parse_args(BASE + ["--dsMT", "0.2,0.4,0.6,0.8", "--dsRpb", "1,2,3,4,5,6,7,8", "--dsGrid"])
    cells = cli.ds_grid_cells(a)
    assert len(cells) == 32 == cli.GRID_MAX_CELLS and cells[-1] == (0.8, 8.0, 2890, "o/x.dsMT0.8.dsRpb8")


class _NoMultiTable(object):
    """A table whose barcodes kept at every fraction are all of one read name."""

    def counts_frac(self, seed, bc_thr):
        return [dict(names=3, barcodes=3, one=3, multi=0, multi_names=0, first_names=3) for _ in bc_thr]

    def kept_grid(self, seed, bc_thr, rd_thr):
        raise AssertionError("no cell is drawn when one is refused")


def test_philox_cell_without_a_multi_name_barcode_is_refused():
    with pytest.raises(ValueError, match=r"--dsGrid fraction 0\.5 x target 4: no barcode kept at 0\.5 in x\.bam has more than one"):
        devplanes.philox_grid_rules("x.bam", [(0.5, 4.0)], [None], SEED, _NoMultiTable())


def test_philox_without_dsgrid_stays_refused():
    p = cli.build_parser()
    for rs in ([], ["--dsRpbSampler", "philox"]):
        with pytest.raises(SystemExit, match="--dsSampler philox is not available"):
            cli.ds_rpb_targets(p.parse_args(BASE + ["--dsMT", "0.5", "--dsRpb", "2", "--dsSampler", "philox"] + rs))


def _cli_args(tmp, **kw):
    import bam_fixture
    case = bam_fixture.make_case(str(tmp))
    d = dict(outPrefix=str(tmp / "o"), bamFile=case["bam"], bedTarget=case["bed"], mtDepth=12, rpb=3.0, hpLen=8,
             refGenome=case["fasta"], dsMT="0.5", dsRpb="2", dsGrid=True)
    d.update(kw)
    return d


def _ns(d):
    """The command line of a dict (cli.main(dict) passes every item as --key=value; --dsGrid is a flag without a value)."""
    argv = [("--%s" % k) if k == "dsGrid" else "--%s=%s" % (k, v) for k, v in d.items() if k != "dsGrid" or v]
    return cli.build_parser().parse_args(argv)


def _no_outputs(tmp):
    return not [f for f in os.listdir(str(tmp)) if ".smCounter." in f]


@pytest.mark.parametrize("kw,msg", [
    (dict(dsRpb=""), "needs both --dsMT and --dsRpb"),
    (dict(dsMT=""), "needs both --dsMT and --dsRpb"),
    (dict(dsSampler="philox"), "--dsSampler philox and --dsRpbSampler reference"),
    (dict(dsRpbSampler="philox"), "--dsSampler reference and --dsRpbSampler philox"),
    (dict(dsMT="0.1,0.2,0.3,0.4,0.5,0.6,0.7,0.8,0.9", dsRpb="2,3,4,5"), "36 cells, at most 32"),
])
def test_refusals_end_the_command_line_before_any_file(tmp_path, kw, msg):
    with pytest.raises(SystemExit, match=msg):
        cli.main(_ns(_cli_args(tmp_path, **kw)))
    assert _no_outputs(tmp_path)


def test_cell_without_a_multi_name_barcode_is_refused(tmp_path):
    from smcounter_amd.tools import ds_mt
    d = _cli_args(tmp_path)
    qn = ds_restate.placed_qnames(d["bamFile"])
    per_bc, order = rw.group_reads(qn)
    # a barcode of several names that ds.mt.py drops at 0.5: the only one left with several names
    multi = next(bc for bc in order if len(per_bc[bc]) > 1 and bc not in ds_mt.select_barcodes(qn, 0.5, SEED))
    d["bamFile"] = gr.one_multi_barcode_bam(d["bamFile"], str(tmp_path / "onemulti.bam"), multi)
    assert multi not in ds_mt.select_barcodes(ds_restate.placed_qnames(d["bamFile"]), 0.5, SEED)
    d["dsMT"] = "1,0.5"
    with pytest.raises(SystemExit, match=r"--dsGrid fraction 0\.5 x target 2: no barcode kept at 0\.5 in .*onemulti\.bam has more "
                                         r"than one read name"):
        cli.main(_ns(d))
    assert _no_outputs(tmp_path)


def test_abi_entries_are_bound():
    L = _lib.load(with_torch=False)
    assert L.smc_abi_version() == 11
    for s in ("smc_read_groups_counts_frac", "smc_read_groups_masks_grid", "smc_read_groups_kept_grid"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
