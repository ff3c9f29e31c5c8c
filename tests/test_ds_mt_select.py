"""--dsMT without a GPU: what in-run molecule down-sampling means, pinned to the reference workflow (tools.ds_mt, then a decode of
the BAM it wrote); the reference's kept set; the philox rule; the command-line flags."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import bamio, cli, devplanes
from smcounter_amd.tools import ds_mt

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402

FIXTURES = ("case", "bam_cigars", "bam_overcap", "bam_deep")


def _fixture(name, tmp):
    return ds_restate.make_case(tmp) if name == "case" else ds_restate.load_fixture(name, tmp)


@pytest.mark.parametrize("name", FIXTURES)
def test_host_restatement_equals_the_decode_of_the_down_sampled_bam(name, tmp_path):
    bam_path, _, loci, P = _fixture(name, str(tmp_path))
    qn = ds_restate.placed_qnames(bam_path)
    full = bamio.NativeBam(bam_path)
    n_runs = 0
    for pct in (0.3, 0.5, 1.0):
        kept = ds_mt.select_barcodes(qn, pct, 1234567)
        ds_path = ds_restate.write_ds_bam(bam_path, str(tmp_path / ("ds%g.bam" % pct)), pct, 1234567)
        ds = bamio.NativeBam(ds_path)
        for chrom, lo, hi in ds_restate.stretches(loci):
            A = full.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
            mask = ds_restate.mask_of(full, A["n_bc"], kept)
            sel = ds_restate.select(A, mask, lo)
            B = ds.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
            ds_restate.assert_same_run(sel, A, B)
            if pct == 1.0:
                assert sel["kept"] == len(A["aln"]) and np.array_equal(sel["loc"], A["loc"])
            elif 0 < sel["kept"] < len(A["aln"]):
                n_runs += 1
        ds.close()
    full.close()
    assert n_runs >= 2          # (runs where the drop took some alignments and left some)


@pytest.mark.parametrize("name", ("case", "bam_overcap"))
def test_reference_kept_set_is_ds_mt_s(name, tmp_path):
    bam_path, _, _, P = _fixture(name, str(tmp_path))
    qn = ds_restate.placed_qnames(bam_path)
    order = bamio.placed_barcodes(bam_path)
    assert order == list(dict.fromkeys(ds_mt.barcode_of(q) for q in qn))
    fr = (0.25, 0.5, 0.9)
    rules = devplanes.reference_rules(bam_path, fr, [P] * 3, 99)
    for f, r in zip(fr, rules):
        assert r.kept == ds_mt.select_barcodes(qn, f, 99)
        assert r.kept_idents is not None and len(r.kept_idents) == len(r.kept)
    # the identities the per-run mask is made from are the decoder's (smc_bam_barcode_idents)
    bam = bamio.NativeBam(bam_path)
    c, lo, hi = _fixture_run(bam_path, name, str(tmp_path))
    A = bam.alignments_run(c, lo, hi, ds_restate.BIG, P, 1)
    names = [bam.barcode_name(g) for g in range(A["n_bc"])]
    assert np.array_equal(devplanes.fnv64_array(names), bam.barcode_idents(A["n_bc"]))
    assert [devplanes._fnv64(t) for t in names[:5]] == devplanes.fnv64_array(names[:5]).tolist()
    bam.close()


def _fixture_run(bam_path, name, tmp):
    _, _, loci, _ = _fixture(name, tmp)
    return ds_restate.stretches(loci)[0]


def test_philox_rule_is_deterministic_and_nested():
    from smcounter_amd import _lib
    L = _lib.load()
    ids = devplanes.fnv64_array(["UMI%05d" % k for k in range(3000)])
    a = devplanes.philox_keep_host(L, ids, 0.5, 7)
    assert np.array_equal(a, devplanes.philox_keep_host(L, ids, 0.5, 7))
    q = devplanes.philox_keep_host(L, ids, 0.25, 7)
    assert not (q & ~a).any() and devplanes.philox_keep_host(L, ids, 1.0, 7).all()
    assert abs(a.mean() - 0.5) < 0.05 and abs(q.mean() - 0.25) < 0.05
    assert not np.array_equal(a, devplanes.philox_keep_host(L, ids, 0.5, 8))
    # (word 0 of Philox4x32-10 with the domain tag in counter word 2: not the stream smc_philox_marks draws from)
    import ctypes
    out = (ctypes.c_uint32 * 4)()
    L.smc_philox4x32_10_host((ctypes.c_uint32 * 4)(1, 2, devplanes.DS_DOMAIN, 0), (ctypes.c_uint32 * 2)(3, 4), out)
    other = (ctypes.c_uint32 * 4)()
    L.smc_philox4x32_10_host((ctypes.c_uint32 * 4)(1, 2, 0, 0), (ctypes.c_uint32 * 2)(3, 4), other)
    assert list(out) != list(other)


def test_flags_parse_and_name_the_outputs():
    p = cli.build_parser()
    base = ["--outPrefix", "o/x", "--bamFile", "a.bam", "--bedTarget", "t.bed", "--mtDepth", "3612", "--rpb", "8.6"]
    a = p.parse_args(base)
    assert a.dsMT is None and a.dsSampler == "reference" and a.dsSeed == 1234567 and cli.ds_fractions(a) == []
    a = p.parse_args(base + ["--dsMT", "0.5,0.25,0.125"])
    assert cli.ds_fractions(a) == [(0.5, 1806, "o/x.dsMT0.5"), (0.25, 903, "o/x.dsMT0.25"), (0.125, 452, "o/x.dsMT0.125")]
    a = p.parse_args(base[:7] + ["3", "--rpb", "1", "--dsMT", "0.1,1", "--dsMtDepth", "7,9", "--dsSampler", "philox", "--dsSeed", "5"])
    assert cli.ds_fractions(a) == [(0.1, 7, "o/x.dsMT0.1"), (1.0, 9, "o/x.dsMT1")] and a.dsSampler == "philox" and a.dsSeed == 5
    a = p.parse_args(base[:7] + ["3", "--rpb", "1", "--dsMT", "0.1"])
    assert cli.ds_fractions(a) == [(0.1, 1, "o/x.dsMT0.1")]                 # max(1, round(0.3))
    for bad in (["--dsMT", "0"], ["--dsMT", "1.5"], ["--dsMT", "a"], ["--dsMT", "0.5", "--dsMtDepth", "1,2"]):
        with pytest.raises(SystemExit):
            cli.ds_fractions(p.parse_args(base + bad))
    help_text = " ".join(p.format_help().split())
    assert "--dsMT" in help_text and "NOT the reference's sample" in help_text


def _cli_args(tmp, **kw):
    import bam_fixture
    case = bam_fixture.make_case(str(tmp))
    d = dict(outPrefix=str(tmp / "o"), bamFile=case["bam"], bedTarget=case["bed"], mtDepth=12, rpb=3.0, hpLen=8,
             refGenome=case["fasta"], dsMT="0.5")
    d.update(kw)
    return d


def test_more_than_one_rank_is_refused(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one process only"):
        cli.main(_cli_args(tmp_path))


@pytest.mark.parametrize("env", [("SMC_PLANES", "host"), ("SMC_BAM_DECODER", "python")])
def test_host_built_planes_are_refused(tmp_path, monkeypatch, env):
    monkeypatch.setenv(*env)
    with pytest.raises(SystemExit, match=r"--dsMT needs the device builder: .*chrQ:281"):
        cli.main(_cli_args(tmp_path))
    assert not os.path.exists(str(tmp_path / "o.smCounter.all.txt"))
