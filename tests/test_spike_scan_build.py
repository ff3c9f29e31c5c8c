"""--spikeScanBuild without a GPU: the entry's declaration and binding, the flag's refusals before any file, its default, the slot and
dense-index arithmetic of the host wrapper, the run log's pass line."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, cli, devplanes, spike

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402


def test_the_header_declares_the_entry_and_the_abi_stays_11():
    h = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"\bint smc_build_listed\(smc_ctx\* ctx, const smc_params\* params, const smc_listed_copy\* d_copies,", h)
    assert re.search(r"#define SMC_ABI_VERSION 11\b", h)
    assert re.search(r"#define SMC_LISTED_UNFLAGGED 64u", h) and devplanes.BUILD_ST_UNFLAGGED == 64
    assert (devplanes.LISTED_MAX_LOCI, devplanes.LISTED_MAX_COPIES) == tuple(
        int(re.search(r"#define %s (\d+)" % n, h).group(1)) for n in ("SMC_LISTED_MAX_LOCI", "SMC_LISTED_MAX_COPIES"))
    assert devplanes.LISTED_COPY_DTYPE.itemsize == 48 and "typedef struct smc_listed_copy {       /* 48 bytes */" in h
    assert "k_build_listed.inc" in open(os.path.join(ROOT, "smcounter_amd", "csrc", "smcounter_hip.hip")).read()


def test_lib_binds_the_entry():
    L = _lib.load()
    assert L.smc_abi_version() == 11
    assert "smc_build_listed" in _lib.SYMBOLS and hasattr(L, "smc_build_listed") and len(L.smc_build_listed.argtypes) == 23


def _argv(tmp, **kw):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp))
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    d = dict(outPrefix=str(tmp / "o"), bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, refGenome=fa)
    d.update(kw)
    return ["--%s=%s" % (k, v) for k, v in d.items() if v is not None]


@pytest.mark.parametrize("kw,msg", [
    (dict(spikeScanBuild="listed"), "--spikeScanBuild belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScanBuild="whole"), "--spikeScanBuild belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScan="0.3", spikeScanReps="4", spikeScanBuild="sparse"), "--spikeScanBuild: whole or listed expected, got 'sparse'"),
    (dict(spikeScan="0.3", spikeScanBuild="listed"), "it needs --spikeScanReps"),
    (dict(spikeScan="0.3", spikeScanReps="4", spikeScanBuild="listed", spikeAF="0.3"), "--spikeScan cannot be combined with --spikeAF"),
])
def test_refusals_before_any_file(tmp_path, kw, msg):
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(cli.build_parser().parse_args(_argv(tmp_path, **kw)))
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_the_default_is_whole(tmp_path):
    ns = dict(spikeScan="0.3", spikeScanReps="4")
    base = dict(targets=[0.3], reps=4, stride=256, alt="transition")
    plan = spike.scan(cli.build_parser().parse_args(_argv(tmp_path, spikeScan="0.3", spikeScanReps="4")))   # (a command line without the flag)
    assert plan == base and spike.scan_build(plan) == "whole"
    assert spike.scan(argparse.Namespace(spikeScanBuild="whole", **ns)) == base                     # (no key without `listed`)
    plan = spike.scan(argparse.Namespace(spikeScanBuild="listed", spikeScanFilter=True, spikeScanDepth="0.5", **ns))
    assert plan == dict(base, fracs=[0.5], filter=True, build="listed") and spike.scan_build(plan) == "listed"
    assert spike.scan(argparse.Namespace(spikeScanBuild=None)) is None
    assert "--spikeScanBuild" in cli.build_parser().format_help()


def test_listed_layout_on_a_hand_made_loc_array():
    loc = np.zeros(6, abi.DEV_LOCUS_DTYPE)
    loc["n"] = [5, 0, 64, 65, 7, 1]
    lay = devplanes.listed_layout(loc, [0, 2, 3, 5], 3)
    assert lay["caps"].tolist() == [8, 64, 68, 4] and lay["caps"].dtype == np.uint32
    assert lay["stride"] == 144 and lay["n_slots"] == 3 * 144 and lay["n_ustart"] == 3 * (144 + 4) + 1
    assert [lay["slot"](0, g) for g in range(4)] == [0, 8, 72, 140] and lay["slot"](2, 1) == 2 * 144 + 8
    # (a locus's umi_start stretch is its slots and one closing entry: locus g of a copy starts g entries behind its slots)
    assert [lay["ustart"](0, g) for g in range(4)] == [0, 9, 74, 143] and lay["ustart"](1, 0) == 148 and lay["ustart"](2, 3) == 2 * 148 + 143
    assert [lay["index"](c, g) for c in range(3) for g in range(4)] == list(range(12))
    # every locus's stretch ends before the next one's begins, the last copy's within n_ustart
    ends = [lay["ustart"](c, g) + int(lay["caps"][g]) + 1 for c in range(3) for g in range(4)]
    starts = [lay["ustart"](c, g) for c in range(3) for g in range(4)]
    assert all(e <= s for e, s in zip(ends, starts[1:])) and ends[-1] <= lay["n_ustart"]
    empty = devplanes.listed_layout(loc, [1], 2)
    assert empty["caps"].tolist() == [0] and empty["stride"] == 0 and empty["n_ustart"] == 3
    for bad in ([2, 2], [3, 2], [6], [-1]):
        with pytest.raises(ValueError, match="do not ascend within the run's 6 loci"):
            devplanes.listed_layout(loc, bad, 1)


def test_copy_room_counts_listed_slots():
    class Up(object):
        n_aln = 1000
    run = argparse.Namespace(up=Up(), A=dict(n_slots=devplanes.AF_REP_BATCH_SLOTS // 6 - 128, bq=np.zeros(2 * 150000, np.uint8)), nl=128)
    assert devplanes._copy_room(run, None, False)[0] == 6                                          # whole-run slots: six copies
    assert devplanes._copy_room(run, None, False, listed_slots=8 * 20000 + 9)[0] == min(devplanes.SPIKE_MAX_COPIES, devplanes.AF_REP_BATCH_SLOTS // 160009)


def test_the_pass_line_is_parsed_with_and_without_the_new_field():
    old = "--spikeScan pass 3: 4 variants, 12 copies, 36 builds, 5 verdicts decided by the host, 0.125 s"
    new = "--spikeScan pass 3: 4 variants, 12 copies, 36 builds, 2 of them whole, 5 verdicts decided by the host, 0.125 s"
    want = dict(k=3, variants=4, copies=12, builds=36, whole=None, host=5, seconds=0.125)
    assert spike.scan_pass_line(old) == want and spike.scan_pass_line(new + "\n") == dict(want, whole=2)
    assert spike.scan_pass_line("--spikeScan: 32 loci x 2 targets") is None


def test_a_run_known_to_be_declined_keeps_whole_run_slots():
    """listed_takes: what spike_scan asks before it sizes a batch by listed slots - not a run with an unflagged alignment (every copy
    would be declined and the batch built whole), and no more loci than one call lists."""
    import types
    from smcounter_amd import devplanes
    run = types.SimpleNamespace(A=dict(status=0))
    assert devplanes.listed_takes(run, 1) and devplanes.listed_takes(run, devplanes.LISTED_MAX_LOCI)
    assert not devplanes.listed_takes(run, 0) and not devplanes.listed_takes(run, devplanes.LISTED_MAX_LOCI + 1)
    assert not devplanes.listed_takes(types.SimpleNamespace(A=dict(status=1)), 1)
    assert (devplanes.LISTED_SHARED_ORDER, devplanes.LISTED_DENSE_LOCUS, devplanes.LISTED_XMAX) == (1, 2, 58)
    h = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert "#define SMC_LISTED_SHARED_ORDER 1" in h and "#define SMC_LISTED_DENSE_LOCUS 2" in h
