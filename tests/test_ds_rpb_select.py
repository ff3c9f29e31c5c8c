"""--dsRpb without a GPU: what in-run read down-sampling within barcodes means, pinned to the reference workflow
(tools.ds_reads_within_mt, then a decode of the BAM it wrote); the reference's kept read names; the decoder's read-name identities;
the command-line flags and refusals."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import bamio, cli, devplanes
from smcounter_amd.tools import ds_reads_within_mt

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import ds_rpb_restate  # noqa: E402

FIXTURES = ("case", "bam_cigars", "bam_overcap", "bam_deep")
TARGETS = {"case": (1.5, 2.0, 9.0), "bam_cigars": (1.5, 2.5), "bam_overcap": (1.5, 2.5), "bam_deep": (2.0, 4.0)}
SEED = 1234567


def _fixture(name, tmp):
    return ds_restate.make_case(tmp) if name == "case" else ds_restate.load_fixture(name, tmp)


@pytest.mark.parametrize("name", FIXTURES)
def test_host_restatement_equals_the_decode_of_the_down_sampled_bam(name, tmp_path):
    bam_path, _, loci, P = _fixture(name, str(tmp_path))
    qn = ds_restate.placed_qnames(bam_path)
    full = bamio.NativeBam(bam_path)
    n_runs = 0
    for r in TARGETS[name]:
        kept, prob = ds_reads_within_mt.select_reads(qn, r, SEED)
        ds_path = ds_rpb_restate.write_rpb_bam(bam_path, str(tmp_path / ("rpb%g.bam" % r)), r, SEED)
        ds = bamio.NativeBam(ds_path)
        for chrom, lo, hi in ds_restate.stretches(loci):
            A = full.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
            idents, shared = full.pair_idents(A["n_pair"])
            assert not shared and len(idents) == A["n_pair"]
            mask = ds_rpb_restate.pair_mask(full, A["n_pair"], kept)
            sel = ds_rpb_restate.select(A, mask, lo)
            B = ds.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
            ds_rpb_restate.assert_same_run(sel, A, B)
            for f in ("bc_gid", "pair_gid"):          # (renumbered by first kept appearance: the decoder's ids themselves)
                assert np.array_equal(sel["aln"][f], B["aln"][f]), f
            if prob >= 1.0:
                assert sel["kept"] == len(A["aln"]) and np.array_equal(sel["loc"], A["loc"])
            elif 0 < sel["kept"] < len(A["aln"]):
                n_runs += 1
        ds.close()
    full.close()
    assert n_runs >= 1          # (runs where the drop took some alignments and left some)


def test_decoder_pair_identities_name_the_reads(tmp_path):
    bam_path, _, loci, P = _fixture("bam_cigars", str(tmp_path))
    bam = bamio.NativeBam(bam_path)
    c, lo, hi = ds_restate.stretches(loci)[0]
    A = bam.alignments_run(c, lo, hi, ds_restate.BIG, P, 2)
    idents, shared = bam.pair_idents(A["n_pair"])
    names = [bam.pair_name(g) for g in range(A["n_pair"])]
    assert not shared and np.array_equal(idents, devplanes.fnv64_array(names))
    # every alignment's full name is its read-name id's name
    qn = [q for q in ds_restate.placed_qnames(bam_path)]
    assert len(set(names)) == len(names) and set(names) <= set(qn)
    assert bam.pair_name(-1) == "" and bam.pair_name(A["n_pair"]) == ""
    bam.close()
    # a read id shared by two names (they differ in the last field only) is reported
    shared_bam = ds_rpb_restate.write_shared_read_ids(ds_restate.make_case(str(tmp_path))[0], str(tmp_path / "shared.bam"))
    _, _, loci, P = ds_restate.make_case(str(tmp_path))
    bam = bamio.NativeBam(shared_bam)
    c, lo, hi = ds_restate.stretches(loci)[0]
    A = bam.alignments_run(c, lo, hi, ds_restate.BIG, P, 2)
    _, shared = bam.pair_idents(A["n_pair"])
    assert shared
    bam.close()


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_read_rules_are_select_reads(name, tmp_path):
    bam_path, _, _, P = _fixture(name, str(tmp_path))
    qn = ds_restate.placed_qnames(bam_path)
    assert bamio.placed_qnames(bam_path) == qn
    targets = TARGETS[name] + (50.0,)                   # (50: probKeep >= 1 on every fixture - every read kept)
    rules = devplanes.reference_read_rules(bam_path, targets, [P] * len(targets), 99)
    n_names = len(set(qn))
    for r, rule in zip(targets, rules):
        kept, prob = ds_reads_within_mt.select_reads(qn, r, 99)
        assert rule.kept == kept and rule.prob_keep == prob and rule.target == r and rule.level == "read"
        assert rule.n_names == n_names and rule.flag == "--dsRpb"
        assert rule.kept_idents is not None and np.array_equal(rule.kept_idents, np.sort(devplanes.fnv64_array(sorted(kept))))
    assert rules[-1].prob_keep >= 1.0 and rules[-1].kept == set(qn)


def test_no_multi_read_barcode_is_refused(tmp_path):
    src = ds_restate.make_case(str(tmp_path))[0]
    one = ds_rpb_restate.write_one_name_per_barcode(src, str(tmp_path / "one.bam"))
    with pytest.raises(ZeroDivisionError):                   # (the reference's behaviour)
        ds_reads_within_mt.select_reads(ds_restate.placed_qnames(one), 2.0, SEED)
    with pytest.raises(ValueError, match=r"--dsRpb 2: .*one\.bam has no barcode with more than one read name"):
        devplanes.reference_read_rules(one, [2.0], [None], SEED)


def test_flags_parse_and_name_the_outputs():
    p = cli.build_parser()
    base = ["--outPrefix", "o/x", "--bamFile", "a.bam", "--bedTarget", "t.bed", "--mtDepth", "3612", "--rpb", "8.6"]
    a = p.parse_args(base)
    assert a.dsRpb is None and a.dsRpbMtDepth is None and cli.ds_rpb_targets(a) == []
    a = p.parse_args(base + ["--dsRpb", "2,4.5,8"])
    assert cli.ds_rpb_targets(a) == [(2.0, 3612, "o/x.dsRpb2"), (4.5, 3612, "o/x.dsRpb4.5"), (8.0, 3612, "o/x.dsRpb8")]
    a = p.parse_args(base + ["--dsRpb", "2,0.5", "--dsRpbMtDepth", "100,7", "--dsMT", "0.5"])
    assert cli.ds_rpb_targets(a) == [(2.0, 100, "o/x.dsRpb2"), (0.5, 7, "o/x.dsRpb0.5")]
    assert cli.ds_fractions(a) == [(0.5, 1806, "o/x.dsMT0.5")]          # (--dsMT unchanged beside it)
    for bad, msg in ((["--dsRpb", "0"], "> 0"), (["--dsRpb", "-1"], "> 0"), (["--dsRpb", "a"], "targets > 0 expected"),
                     (["--dsRpb", "2,nan"], "> 0"), (["--dsRpb", ","], "> 0"),
                     (["--dsRpb", "2", "--dsRpbMtDepth", "1,2"], "2 depths for 1 --dsRpb targets"),
                     (["--dsRpb", "2", "--dsRpbMtDepth", "x"], "integers expected"),
                     (["--dsRpb", "2", "--dsSampler", "philox"], "philox is not available")):
        with pytest.raises(SystemExit, match=msg):
            cli.ds_rpb_targets(p.parse_args(base + bad))
    help_text = " ".join(p.format_help().split())
    assert "--dsRpb" in help_text and "--dsRpbMtDepth" in help_text and "philox is not available here" in help_text


def _cli_args(tmp, **kw):
    import bam_fixture
    case = bam_fixture.make_case(str(tmp))
    d = dict(outPrefix=str(tmp / "o"), bamFile=case["bam"], bedTarget=case["bed"], mtDepth=12, rpb=3.0, hpLen=8,
             refGenome=case["fasta"], dsRpb="2")
    d.update(kw)
    return d


def test_philox_with_dsrpb_is_refused(tmp_path):
    with pytest.raises(SystemExit, match="--dsSampler philox is not available"):
        cli.main(_cli_args(tmp_path, dsMT="0.5", dsSampler="philox"))


@pytest.mark.parametrize("kw", [{}, {"dsMT": "0.5"}])
def test_more_than_one_rank_is_refused(tmp_path, monkeypatch, kw):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--dsRpb runs in one process only"):
        cli.main(_cli_args(tmp_path, **kw))


@pytest.mark.parametrize("env", [("SMC_PLANES", "host"), ("SMC_BAM_DECODER", "python")])
def test_host_built_planes_are_refused(tmp_path, monkeypatch, env):
    monkeypatch.setenv(*env)
    with pytest.raises(SystemExit, match=r"--dsRpb needs the device builder: .*chrQ:281"):
        cli.main(_cli_args(tmp_path))
    assert not os.path.exists(str(tmp_path / "o.smCounter.all.txt"))


def test_file_without_a_multi_read_barcode_is_refused(tmp_path):
    d = _cli_args(tmp_path)
    d["bamFile"] = ds_rpb_restate.write_one_name_per_barcode(d["bamFile"], str(tmp_path / "one.bam"))
    with pytest.raises(SystemExit, match=r"--dsRpb 2: .*one\.bam has no barcode with more than one read name"):
        cli.main(d)
    assert not os.path.exists(str(tmp_path / "o.smCounter.all.txt"))
