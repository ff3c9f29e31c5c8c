"""--dsRpbSampler philox without a GPU: the rule restated (tests/ds_rpb_philox_restate.py) against the reference's grouping and
probKeep, its consequences (first names kept, nested sets), the native file pass that feeds the device table, and the flags."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, bamio, cli, devplanes
from smcounter_amd.tools import ds_reads_within_mt as rw
from smcounter_amd.tools.ds_mt import barcode_of

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import ds_rpb_philox_restate as rp  # noqa: E402

FIXTURES = ("case", "bam_cigars", "bam_overcap", "bam_deep")
TARGETS = (0.5, 1.0, 1.5, 2.0, 4.0, 9.0, 50.0)
SEED = 1234567


def _fixture(name, tmp):
    return ds_restate.make_case(tmp) if name == "case" else ds_restate.load_fixture(name, tmp)


@pytest.mark.parametrize("name", FIXTURES)
def test_restated_grouping_and_prob_keep_are_the_references(name, tmp_path):
    qn = ds_restate.placed_qnames(_fixture(name, str(tmp_path))[0])
    per_bc, order = rw.group_reads(qn)
    g = rp.group(qn)
    assert g["names"] == [q for q in dict.fromkeys(qn)]
    assert g["counts"]["names"] == sum(len(v) for v in per_bc.values()) and g["counts"]["barcodes"] == len(order)
    # the first names are the reference's: the first of every barcode's list
    assert {n for n, f in zip(g["names"], g["first"]) if f} == {v[0] for v in per_bc.values()}
    for r in TARGETS:
        assert rp.prob_keep(g["counts"], r) == rw.prob_keep(per_bc, r)          # (bit for bit: the same double expression)


def _lib_loaded():
    return _lib.load(with_torch=False)


def test_numpy_philox_is_the_librarys():
    L = _lib_loaded()
    import ctypes
    idents = rp.fnv64(["a:b:c", "x", "SAMPLE:ACGTACGTAC:17", ""]).tolist() + [0, 2 ** 64 - 1]
    for seed in (0, 1234567, 2 ** 40 + 3):
        got = rp.draws(np.array(idents, np.uint64), seed)
        for v, u in zip(idents, got.tolist()):
            out = (ctypes.c_uint32 * 4)()
            L.smc_philox4x32_10_host((ctypes.c_uint32 * 4)(v & 0xFFFFFFFF, v >> 32, 0x64735250, 0),
                                     (ctypes.c_uint32 * 2)(seed & 0xFFFFFFFF, seed >> 32), out)
            assert out[0] == u
    assert devplanes.RPB_DOMAIN == rp.DOMAIN != devplanes.DS_DOMAIN


@pytest.mark.parametrize("name", FIXTURES)
def test_first_names_kept_and_sets_nested(name, tmp_path):
    qn = ds_restate.placed_qnames(_fixture(name, str(tmp_path))[0])
    g = rp.restate(qn, TARGETS, SEED)
    names = set(g["names"])
    firsts = {n for n, f in zip(g["names"], g["first"]) if f}
    for k in range(len(TARGETS)):
        assert firsts <= g["kept"][k] <= names
        assert g["thr"][k] == devplanes.read_threshold(g["probs"][k])
        if k:
            assert g["kept"][k - 1] <= g["kept"][k]                               # nested across targets
        if g["probs"][k] >= 1.0:
            assert g["thr"][k] == 1 << 32 and g["kept"][k] == names
        if g["probs"][k] <= 0.0:                                                  # (r <= 1)
            assert g["thr"][k] == 0 and g["kept"][k] == firsts
    assert g["probs"][-1] >= 1.0 and g["probs"][0] < 0.0 and any(0 < p < 1.0 for p in g["probs"])


def test_threshold_clamps():
    assert devplanes.read_threshold(-0.5) == 0 and devplanes.read_threshold(0.0) == 0
    assert devplanes.read_threshold(0.5) == 1 << 31 and devplanes.read_threshold(1.0) == 1 << 32
    assert devplanes.read_threshold(7.0) == 1 << 32 and devplanes.read_threshold(float("nan")) == 0
    assert devplanes.read_threshold(2.0 ** -33) == 0 and devplanes.read_threshold(2.0 ** -32) == 1


def _pass(path, chunk):
    bam = bamio.NativeBam(path)
    parts = [(f, k.copy()) for f, k in bam.name_keys(chunk, 3)]
    bam.close()
    return parts


@pytest.mark.parametrize("name", FIXTURES)
def test_native_file_pass_equals_the_host_hashes(name, tmp_path):
    path = _fixture(name, str(tmp_path))[0]
    qn = ds_restate.placed_qnames(path)
    bcs = [barcode_of(q) for q in qn]
    want = np.stack([devplanes.fnv64_array(qn), devplanes.fnv64_array(bcs),
                     devplanes.check32_array(qn).astype(np.uint64) | devplanes.check32_array(bcs).astype(np.uint64) << np.uint64(32)], 1)
    for chunk in (1, 7, len(qn), 1 << 22):
        parts = _pass(path, chunk)
        assert all(len(k) <= chunk for _, k in parts)
        assert [f for f, _ in parts] == [chunk * i for i in range(len(parts))]       # each chunk's first ordinal
        got = np.concatenate([k for _, k in parts])
        assert np.array_equal(got, want), chunk
    # the check words are a second hash, not the identity's low bits
    assert not np.array_equal(want[:, 2] & np.uint64(0xFFFFFFFF), want[:, 0] & np.uint64(0xFFFFFFFF))


def test_native_file_pass_after_a_run_and_on_a_large_file(tmp_path):
    path = _fixture("bam_cigars", str(tmp_path))[0]
    _, _, loci, P = _fixture("bam_cigars", str(tmp_path))
    qn = ds_restate.placed_qnames(path)
    bam = bamio.NativeBam(path)
    c, lo, hi = ds_restate.stretches(loci)[0]
    bam.alignments_run(c, lo, hi, ds_restate.BIG, P, 2)                      # (a run first: the pass starts from the file's start)
    got = np.concatenate([k.copy() for _, k in bam.name_keys(100, 2)])
    assert np.array_equal(got[:, 0], devplanes.fnv64_array(qn))
    got = np.concatenate([k.copy() for _, k in bam.name_keys(1 << 20, 2)])  # (and again)
    assert np.array_equal(got[:, 0], devplanes.fnv64_array(qn))
    bam.close()
    big = str(tmp_path / "names.bam")
    names = rp.write_names_bam(big, 150000)
    parts = _pass(big, 65536 + 17)
    assert [len(k) for _, k in parts] == [65553, 65553, 150000 - 2 * 65553]
    got = np.concatenate([k for _, k in parts])
    assert np.array_equal(got[:, 0], devplanes.fnv64_array(names))
    assert np.array_equal(got[:, 1], devplanes.fnv64_array([barcode_of(q) for q in names]))


def test_name_without_a_barcode_field_is_an_error(tmp_path):
    import struct
    header = b"BAM\1" + struct.pack("<ii", 0, 1) + struct.pack("<i", 2) + b"c\0" + struct.pack("<i", 1000)
    nb = b"nocolon\0"
    body = struct.pack("<iiBBHHHiiii", 0, 5, len(nb), 60, 4680, 0, 0, 0, -1, -1, 0) + nb
    path = str(tmp_path / "bad.bam")
    bamio.write_raw(path, header, [struct.pack("<i", len(body)) + body])
    with pytest.raises(bamio.BamError, match="no barcode field"):
        _pass(path, 10)


BASE = ["--outPrefix", "o/x", "--bamFile", "a.bam", "--bedTarget", "t.bed", "--mtDepth", "3612", "--rpb", "8.6"]


def test_flags():
    p = cli.build_parser()
    a = p.parse_args(BASE + ["--dsRpb", "2,4", "--dsRpbSampler", "philox"])
    assert a.dsRpbSampler == "philox" and cli.ds_rpb_targets(a) == [(2.0, 3612, "o/x.dsRpb2"), (4.0, 3612, "o/x.dsRpb4")]
    a = p.parse_args(BASE + ["--dsRpb", "2", "--dsRpbSampler", "reference"])
    assert cli.ds_rpb_targets(a) == [(2.0, 3612, "o/x.dsRpb2")]
    assert p.parse_args(BASE).dsRpbSampler is None and p.parse_args(BASE + ["--dsRpb", "2"]).dsRpbSampler is None
    for extra in (["--dsRpbSampler", "philox"], ["--dsRpbSampler", "reference"], ["--dsRpbSampler", "philox", "--dsMT", "0.5"]):
        with pytest.raises(SystemExit, match="--dsRpbSampler .*needs --dsRpb"):
            cli.ds_rpb_targets(p.parse_args(BASE + extra))
    with pytest.raises(SystemExit):
        p.parse_args(BASE + ["--dsRpb", "2", "--dsRpbSampler", "other"])
    # --dsSampler (the barcode sampler of --dsMT) stays refused with --dsRpb, whichever read sampler
    for rs in ([], ["--dsRpbSampler", "philox"]):
        with pytest.raises(SystemExit, match="--dsSampler philox is not available"):
            cli.ds_rpb_targets(p.parse_args(BASE + ["--dsRpb", "2", "--dsSampler", "philox"] + rs))
    help_text = " ".join(p.format_help().split())
    assert "philox is not available here" in help_text and "--dsRpbSampler" in help_text


def test_dsrpbsampler_without_dsrpb_ends_the_command_line(tmp_path):
    import bam_fixture
    case = bam_fixture.make_case(str(tmp_path))
    with pytest.raises(SystemExit, match="needs --dsRpb"):
        cli.main(dict(outPrefix=str(tmp_path / "o"), bamFile=case["bam"], bedTarget=case["bed"], mtDepth=12, rpb=3.0, hpLen=8,
                      refGenome=case["fasta"], dsRpbSampler="philox"))
    assert not os.path.exists(str(tmp_path / "o.smCounter.all.txt"))


@pytest.mark.parametrize("env", [("SMC_PLANES", "host"), ("SMC_BAM_DECODER", "python"), ("WORLD_SIZE", "2")])
def test_philox_sampler_keeps_the_refusals(tmp_path, monkeypatch, env):
    import bam_fixture
    case = bam_fixture.make_case(str(tmp_path))
    monkeypatch.setenv(*env)
    with pytest.raises(SystemExit, match="--dsRpb (needs the device builder|runs in one process only)"):
        cli.main(dict(outPrefix=str(tmp_path / "o"), bamFile=case["bam"], bedTarget=case["bed"], mtDepth=12, rpb=3.0, hpLen=8,
                      refGenome=case["fasta"], dsRpb="2", dsRpbSampler="philox"))


def test_abi_11_binds_the_table():
    L = _lib_loaded()
    assert L.smc_abi_version() == 11
    for s in ("smc_read_groups_create", "smc_read_groups_add", "smc_read_groups_finish", "smc_read_groups_masks", "smc_read_groups_kept",
              "smc_read_groups_status", "smc_read_groups_destroy", "smc_select_alignments_keyed", "smc_select_alignments"):
        assert s in _lib.SYMBOLS and hasattr(L, s)
