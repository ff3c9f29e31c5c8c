"""--spikeScanMnvFilter and --spikeScanMnvDepth without a GPU: the flags' parsing and every refusal before any file is written, spike.scan()'s dict, the joint
FILTER rule in numpy (abi.scan_filter_joint_rule) on hand-made member words, the page writers on hand-made entries with the lines
checked literally, the entry's declaration and binding, and the refusals that stay (the existing MNV refusals fire first)."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, cli, devplanes, dsaf, spike
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import scan_filter_pages as pages  # noqa: E402
import test_spike_scan_mnv as TM  # noqa: E402  (its arguments of a run and its hand-made MNVs)

HOST, SHIFT = abi.SCAN_FLT_HOST, abi.SCAN_FLT_MEMBER_SHIFT
LSM, HP, REPT = (dict((n, b) for b, n in abi.SCAN_FILTER_NAMES)[n] for n in ("LSM", "HP", "RepT"))
SWITCH = "spikeScanMnvFilter"


# ---- the command line
@pytest.mark.parametrize("kw,msg", [
    (dict(spikeScanMnv=None), "--spikeScanMnvFilter belongs to --spikeScanMnv: it needs --spikeScanMnv"),
    (dict(spikeScanMnv=None, spikeScanFilter=True), "--spikeScanMnvFilter belongs to --spikeScanMnv: it needs --spikeScanMnv"),
    (dict(spikeScan=None, spikeScanReps=None, spikeScanStride=None, spikeScanMnv=None),
     "--spikeScanMnvFilter belongs to --spikeScan: it needs --spikeScan"),
    # beside the other axes the MNV scan's own refusals fire first, with the messages they have
    (dict(spikeScanDepth="0.5"), "--spikeScanMnv cannot be combined with --spikeScanDepth: the depth axis of an MNV scan is not built"),
    (dict(spikeScanRpb="2"), "--spikeScanMnv cannot be combined with --spikeScanRpb: the reads-per-barcode axis of an MNV scan is not built"),
    (dict(spikeScanFilter=True), "--spikeScanMnv cannot be combined with --spikeScanFilter: the filter axis of an MNV scan is not built"),
    (dict(spikeScanIndel="del1"), "--spikeScanMnv cannot be combined with --spikeScanIndel"),
    # everything --spikeScanMnv refuses
    (dict(spikeScanMnv="9"), "--spikeScanMnv: an integer in 2 .. 8 expected"),
    (dict(spikeScanMnv="3", spikeScanStride="2"), "the smallest stride allowed is 3"),
    (dict(spikeScanReps=None), "it needs --spikeScanReps"),
    (dict(spikeReps="4"), "--spikeScan cannot be combined with --spikeReps"),
    (dict(dsMT="0.5"), "--spikeScan cannot be combined with --dsMT"),
    (dict(spikeScanBuild="some"), "--spikeScanBuild: whole or listed expected"),
])
def test_cli_refusals_before_any_file(tmp_path, kw, msg):
    args = TM._args(tmp_path, **kw)
    switches = ["--" + SWITCH] + (["--spikeScanFilter"] if args.pop("spikeScanFilter", False) else [])
    args = cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in args.items()] + switches)
    assert getattr(args, SWITCH) is True
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(args)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_more_processes_are_refused_and_the_switch_is_read(tmp_path, monkeypatch):
    ns = argparse.Namespace(spikeScan="0.7,0.3", spikeScanReps="32", spikeScanMnv="3", spikeScanStride=3, spikeScanBuild="listed")
    today = dict(targets=[0.7, 0.3], reps=32, stride=3, alt="transition", mnv=3, build="listed")
    assert spike.scan(ns) == today                                       # without the switch: the dict of today
    ns.spikeScanMnvFilter = False
    assert spike.scan(ns) == today
    ns.spikeScanMnvFilter = True
    assert spike.scan(ns) == dict(today, mnv_filter=True)
    assert spike.scan(argparse.Namespace(spikeScan="0.5", spikeScanReps="8", spikeScanMnv="2", spikeScanStride="4", spikeScanAlt="complement",
                                         spikeScanMnvFilter=True)) == dict(targets=[0.5], reps=8, stride=4, alt="complement", mnv=2, mnv_filter=True)
    assert cli.build_parser().get_default("spikeScanMnvFilter") is False
    assert "--spikeScanMnvFilter" in cli.build_parser().format_help()
    monkeypatch.setenv("WORLD_SIZE", "2")
    args = cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in TM._args(tmp_path).items()] + ["--" + SWITCH])
    with pytest.raises(SystemExit, match="--spikeScan runs in one process only"):
        cli.main(args)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_the_stage_keeps_its_refusals_and_takes_mnv_axes():
    call = lambda **kw: devplanes.spike_scan("x.bam", None, sv.PhasedVariants(), [], [0.5], None, 1, 2, None, 5, None, **kw)
    for kw in (dict(flt=True), dict(depth=dict(fracs=[0.5])), dict(rpb=dict(targets=[2])), dict(indel=True)):
        with pytest.raises(ValueError, match="not built"):
            call(mnv=2, **kw)
        with pytest.raises(ValueError, match="not built"):
            call(mnv=2, mnv_axes=dict(flt=True), **kw)
    with pytest.raises(ValueError, match="need --spikeScanMnv"):
        call(mnv_axes=dict(flt=True))
    with pytest.raises(ValueError, match="not built"):
        call(mnv=2, mnv_axes=dict(rpb=dict(targets=[2])))
    with pytest.raises(ValueError, match="need --spikeScanMnv"):
        call(mnv_axes=dict(depth=dict(fracs=[0.5])))


DEPTH = "spikeScanMnvDepth"


@pytest.mark.parametrize("kw,msg", [
    (dict(spikeScanMnv=None), "--spikeScanMnvDepth belongs to --spikeScanMnv: it needs --spikeScanMnv"),
    (dict(spikeScan=None, spikeScanReps=None, spikeScanStride=None, spikeScanMnv=None),
     "--spikeScanMnvDepth belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScanMnvDepth="half"), "--spikeScanMnvDepth: comma-separated fractions in (0, 1] expected, got 'half'"),
    (dict(spikeScanMnvDepth="0.5;0.25"), "--spikeScanMnvDepth: comma-separated fractions in (0, 1] expected"),
    (dict(spikeScanMnvDepth="0.5,0"), "--spikeScanMnvDepth: every fraction must lie in (0, 1]"),
    (dict(spikeScanMnvDepth="1.5"), "--spikeScanMnvDepth: every fraction must lie in (0, 1]"),
    (dict(spikeScanMnvDepth="-0.5"), "--spikeScanMnvDepth: every fraction must lie in (0, 1]"),
    (dict(spikeScanMnvDepth=","), "--spikeScanMnvDepth: every fraction must lie in (0, 1]"),
    (dict(spikeScanMnvDepth="0.5,0.50"), "--spikeScanMnvDepth: a fraction is listed twice"),
    (dict(spikeScanMnvDepth=",".join("%g" % (x / 20.0) for x in range(1, 18))), "--spikeScanMnvDepth: 2 targets x 17 fractions = 34 cells, at most 32"),
    (dict(spikeScanDepth="0.5"), "--spikeScanMnv cannot be combined with --spikeScanDepth: the depth axis of an MNV scan is not built"),
    (dict(spikeScanRpb="2"), "--spikeScanMnv cannot be combined with --spikeScanRpb: the reads-per-barcode axis of an MNV scan is not built"),
    (dict(spikeScanFilter=True), "--spikeScanMnv cannot be combined with --spikeScanFilter: the filter axis of an MNV scan is not built"),
    (dict(spikeScanIndel="del1"), "--spikeScanMnv cannot be combined with --spikeScanIndel"),
    (dict(spikeScanMnv="9"), "--spikeScanMnv: an integer in 2 .. 8 expected"),
    (dict(spikeScanReps=None), "it needs --spikeScanReps"),
    (dict(dsMT="0.5"), "--spikeScan cannot be combined with --dsMT"),
])
@pytest.mark.parametrize("beside", (False, True))
def test_depth_refusals_before_any_file(tmp_path, kw, msg, beside):
    """The depth flag alone and beside the switch."""
    args = TM._args(tmp_path, **dict(dict(spikeScanMnvDepth="0.5,0.25"), **kw))
    switches = (["--" + SWITCH] if beside else []) + (["--spikeScanFilter"] if args.pop("spikeScanFilter", False) else [])
    args = cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in args.items()] + switches)
    if beside and " belongs to " in msg:         # (beside the switch the first of the two flags is named)
        msg = msg.replace(DEPTH, SWITCH)
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(args)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_the_depth_flag_is_read():
    ns = argparse.Namespace(spikeScan="0.7,0.3", spikeScanReps="32", spikeScanMnv="3", spikeScanStride=3)
    today = dict(targets=[0.7, 0.3], reps=32, stride=3, alt="transition", mnv=3)
    assert spike.scan(ns) == today
    ns.spikeScanMnvDepth = "0.5, 0.25,1"
    assert spike.scan(ns) == dict(today, mnv_fracs=[0.5, 0.25, 1.0])
    ns.spikeScanMnvFilter = True
    assert spike.scan(ns) == dict(today, mnv_fracs=[0.5, 0.25, 1.0], mnv_filter=True)
    ns.spikeScanMnvDepth = ",".join("%g" % (x / 20.0) for x in range(1, 17))      # 2 x 16 = 32 cells: allowed
    assert len(spike.scan(ns)["mnv_fracs"]) == 16
    assert cli.build_parser().get_default(DEPTH) is None and "--spikeScanMnvDepth" in cli.build_parser().format_help()
    # --spikeScanDepth keeps its own messages
    with pytest.raises(SystemExit, match=re.escape("--spikeScanDepth: a fraction is listed twice")):
        spike.scan(argparse.Namespace(spikeScan="0.5", spikeScanReps="8", spikeScanDepth="0.5,0.5"))


def test_depth_page_writers_from_hand_made_entries(tmp_path):
    leaders = [("chrA", 3), ("chrA", 7), ("chrB", 4)]
    mnvs = TM._mnvs(leaders, 2)
    loci = [("chrA", 3, 0), ("chrA", 5, None), ("chrA", 7, 1), ("chrB", 4, 2)]
    targets, fracs, R, mt_depth = [0.7, 0.3], [0.5, 0.25], 4, 240
    # called replicates: set 0 everywhere at 0.7 and at full depth and 0.5 at 0.3 (F95 0.25 / 0.5); set 1 at full depth only (F95 1);
    # set 2 never in all replicates (F95 NA)
    n_called = {(0, 0, None): 4, (0, 0, 0): 4, (0, 0, 1): 4, (0, 1, None): 4, (0, 1, 0): 4, (0, 1, 1): 3,
                (1, 0, None): 4, (1, 0, 0): 3, (1, 0, 1): 0, (1, 1, None): 4, (1, 1, 0): 1, (1, 1, 1): 0,
                (2, 0, None): 3, (2, 0, 0): 4, (2, 0, 1): 4, (2, 1, None): 0, (2, 1, 0): 0, (2, 1, 1): 0}
    n_all = {None: 100, 0: 50, 1: 24}
    per = lambda i, t, f: [(dict(N_ALL=n_all[f] + i + j, V0_ALL=0, S_ALL=5 + j, V1_ALL=5 + j), int(j < n_called[(i, t, f)])) for j in range(R)]
    full = {(i, t): per(i, t, None) for i in range(3) for t in range(2)}
    cells = {(i, t, f): per(i, t, f) for i in range(3) for t in range(2) for f in range(2)}
    prefix = str(tmp_path / "o")
    spike.write_scan_mnv_depth(prefix, loci, mnvs, mnvs.sets, targets, fracs, mt_depth, full, cells)
    mts = [120, 60]
    assert [spike.scan_depth_mt(mt_depth, f) for f in fracs] == mts
    sens = open(prefix + ".spikeScan.mnv.depth.sensitivity.txt").read().splitlines()
    assert sens[0].split("\t") == list(spike.phase_sensitivity_header())
    assert sens[1:] == [spike.phase_sensitivity_line(mnvs.sets[i], mnvs, targets[t], fracs[f], mts[f], cells[(i, t, f)])
                        for i in range(3) for t in range(2) for f in range(2)]
    assert sens[1].split("\t")[:11] == ["chrA:3", "chrA", "3,4", "A,A", "G,G", "0.7", "0.5", "120", "4", "4", "1.0"]
    curve = open(prefix + ".spikeScan.mnv.depth.curve.txt").read().splitlines()
    assert curve[0] == "CHROM\tPOS\tREF\tALT\tDEPTH\tMTDEPTH\tN_MEAN\tRATE@0.3\tRATE@0.7\tT95"
    # (N_MEAN: the mean N_ALL of the cell over replicates and targets - 100 + i + 1.5 at full depth)
    assert curve[1:] == ["chrA\t3\tAA\tGG\tfull\t240\t101.5\t1.0\t1.0\t0.3", "chrA\t3\tAA\tGG\t0.5\t120\t51.5\t1.0\t1.0\t0.3",
                         "chrA\t3\tAA\tGG\t0.25\t60\t25.5\t0.75\t1.0\t0.7",
                         "chrA\t7\tAA\tGG\tfull\t240\t102.5\t1.0\t1.0\t0.3", "chrA\t7\tAA\tGG\t0.5\t120\t52.5\t0.25\t0.75\tNA",
                         "chrA\t7\tAA\tGG\t0.25\t60\t26.5\t0.0\t0.0\tNA",
                         "chrB\t4\tAA\tGG\tfull\t240\t103.5\t0.0\t0.75\tNA", "chrB\t4\tAA\tGG\t0.5\t120\t53.5\t0.0\t1.0\t0.7",
                         "chrB\t4\tAA\tGG\t0.25\t60\t27.5\t0.0\t1.0\t0.7"]
    need = open(prefix + ".spikeScan.mnv.depth.need.txt").read().splitlines()
    assert need == ["CHROM\tPOS\tREF\tALT\tTARGET\tN_ALL\tF95\tMTDEPTH95\tN95",
                    "chrA\t3\tAA\tGG\t0.7\t100\t0.25\t60\t25.5", "chrA\t3\tAA\tGG\t0.3\t100\t0.5\t120\t51.5",
                    "chrA\t7\tAA\tGG\t0.7\t101\t1\t240\t102.5", "chrA\t7\tAA\tGG\t0.3\t101\t1\t240\t102.5",
                    # (set 2 at 0.7: both fractions reach 0.95 but full depth does not - NA, as F95's rule has it)
                    "chrB\t4\tAA\tGG\t0.7\t102\tNA\tNA\tNA", "chrB\t4\tAA\tGG\t0.3\t102\tNA\tNA\tNA"]
    # F95 NA writes 2, and so does a skipped locus
    assert open(prefix + ".spikeScan0.7.mnv.f95.bedgraph").read().splitlines() == \
        ["chrA\t2\t3\t0.25", "chrA\t4\t5\t2", "chrA\t6\t7\t1", "chrB\t3\t4\t2"]
    assert open(prefix + ".spikeScan0.3.mnv.f95.bedgraph").read().splitlines() == \
        ["chrA\t2\t3\t0.5", "chrA\t4\t5\t2", "chrA\t6\t7\t1", "chrB\t3\t4\t2"]
    assert open(prefix + ".spikeScan0.3.dsMT0.25.mnv.rate.bedgraph").read().splitlines() == \
        ["chrA\t2\t3\t0.75", "chrA\t6\t7\t0.0", "chrB\t3\t4\t0.0"]
    # T95 NA writes 1, and so does a skipped locus
    assert open(prefix + ".spikeScan.dsMT0.5.mnv.t95.bedgraph").read().splitlines() == \
        ["chrA\t2\t3\t0.3", "chrA\t4\t5\t1", "chrA\t6\t7\t1", "chrB\t3\t4\t0.7"]
    assert sorted(os.listdir(str(tmp_path))) == sorted(
        ["o.spikeScan.mnv.depth.sensitivity.txt", "o.spikeScan.mnv.depth.curve.txt", "o.spikeScan.mnv.depth.need.txt",
         "o.spikeScan.dsMT0.5.mnv.t95.bedgraph", "o.spikeScan.dsMT0.25.mnv.t95.bedgraph", "o.spikeScan0.7.mnv.f95.bedgraph",
         "o.spikeScan0.3.mnv.f95.bedgraph"] + ["o.spikeScan%g.dsMT%g.mnv.rate.bedgraph" % (t, f) for t in targets for f in fracs])
    # the cells' filter page of both flags
    called = np.zeros((3, 2, 2, R), bool)
    words = np.zeros((3, 2, 2, R), np.uint32)
    called[0], words[0, :, 1] = True, REPT | (2 << SHIFT)
    spike.write_scan_filter_cells(prefix, [spike.scan_mnv_variant(ps, mnvs) for ps in mnvs.sets], targets, fracs, mts, called, words, mnv=True)
    page = open(prefix + ".spikeScan.mnv.depth.filter.txt").read().splitlines()
    assert page[0].split("\t") == ["CHROM", "POS", "REF", "ALT", "TARGET", "FRACTION", "MTDEPTH", "REPS", "CALLED_ALL", "PASS_ALL", "RATE_PASS",
                                   "LO95", "HI95"] + list(pages.NAMES)
    assert len(page) == 1 + 3 * 2 * 2
    assert page[1].split("\t")[:11] == ["chrA", "3", "AA", "GG", "0.7", "0.5", "120", "4", "4", "4", "1.0"]
    assert page[2].split("\t")[:11] == ["chrA", "3", "AA", "GG", "0.7", "0.25", "60", "4", "4", "0", "0.0"]
    assert page[2].split("\t")[13 + pages.NAMES.index("RepT")] == "4" and page[5].split("\t")[7:10] == ["4", "0", "0"]


# ---- the joint rule
def test_the_joint_filter_rule_in_numpy():
    m = np.array([[0, LSM, 0, 0, HP | REPT, HOST, 0, 0, LSM | HOST, 0, 0, 0, 0, REPT, 0, 0, 0],
                  [0] * 17], np.uint32)
    off = [0, 1, 2, 4, 7, 9, 17]                  # sets of 1, 1, 2, 3, 2 and 8 members
    words = abi.scan_filter_joint_rule(m, off)
    assert words.dtype == np.uint32 and words.shape == (2, 6)
    assert words[0].tolist() == [
        0,                                        # one member, PASS
        LSM | (1 << SHIFT),                       # one member, not PASS
        0,                                        # two members, both PASS
        HP | REPT | HOST | (1 << SHIFT),          # a HOST member (no name bit: it is not counted as not PASS) beside a member with names
        LSM | HOST | (0x2 << SHIFT),              # the HOST member is the one with the name
        REPT | (0x10 << SHIFT)]                   # eight members, one of them not PASS: member 4
    assert words[1].tolist() == [0] * 6
    # garbage above the names and below bit 31 never shows
    assert abi.scan_filter_joint_rule([[0x7FFFC000]], [0, 1]).tolist() == [[0]]
    full = np.full((1, 8), abi.SCAN_FLT_NAMES_MASK | HOST, np.uint32)
    assert abi.scan_filter_joint_rule(full, [0, 8]).tolist() == [[abi.SCAN_FLT_NAMES_MASK | HOST | (0xFF << SHIFT)]]
    assert abi.scan_filter_joint_rule(np.zeros((3, 0), np.uint32), [0]).shape == (3, 0)
    assert abi.SCAN_FLT_NAMES_MASK < (1 << SHIFT) and SHIFT + abi.SPIKE_PHASE_MAX_MEMBERS <= 31


# ---- the pages
def test_page_writers_from_hand_made_entries(tmp_path):
    leaders = [("chrA", 3), ("chrA", 7), ("chrB", 4), ("chrB", 6)]
    mnvs = TM._mnvs(leaders, 2)
    loci = [("chrA", 3, 0), ("chrA", 5, None), ("chrA", 7, 1), ("chrB", 4, 2), ("chrB", 5, None), ("chrB", 6, 3)]
    targets, R = [0.7, 0.3], 4
    # set 0: never called; set 1: called everywhere, RepT on member 0 in every replicate: PASS nowhere; set 2: called 3 / 2 times, one
    # replicate LSM on both members; set 3: called and PASS in every replicate at 0.7 (a T95_PASS), 3 of 4 at 0.3
    called = np.zeros((4, 2, R), bool)
    words = np.zeros((4, 2, R), np.uint32)
    called[1], words[1] = True, REPT | (1 << SHIFT)
    called[2, 0, :3], called[2, 1, :2] = True, True
    words[2, :, 0] = LSM | (3 << SHIFT)
    words[2, 0, 3] = HP                           # (not called there: must not count)
    called[3, 0], called[3, 1, :3] = True, True
    prefix = str(tmp_path / "o")
    spike.write_scan_mnv_filter(prefix, loci, mnvs, mnvs.sets, targets, [90, 91, 92, 93], called, words)
    page = open(prefix + ".spikeScan.mnv.filter.txt").read().splitlines()
    assert page[0].split("\t") == ["CHROM", "POS", "REF", "ALT", "TARGET", "REPS", "CALLED_ALL", "PASS_ALL", "RATE_PASS", "LO95", "HI95"] + \
        list(pages.NAMES)
    z = ["0"] * 14
    tally = lambda **kw: "\t".join(str(kw.get(n, 0)) for n in pages.NAMES)
    w = lambda k: "\t".join(dsaf.frac_text(x) for x in (k / 4.0,) + tuple(dsaf.wilson(k, 4)))
    assert page[1:] == [
        "chrA\t3\tAA\tGG\t0.7\t4\t0\t0\t" + w(0) + "\t" + "\t".join(z),
        "chrA\t3\tAA\tGG\t0.3\t4\t0\t0\t" + w(0) + "\t" + "\t".join(z),
        "chrA\t7\tAA\tGG\t0.7\t4\t4\t0\t" + w(0) + "\t" + tally(RepT=4),
        "chrA\t7\tAA\tGG\t0.3\t4\t4\t0\t" + w(0) + "\t" + tally(RepT=4),
        "chrB\t4\tAA\tGG\t0.7\t4\t3\t2\t" + w(2) + "\t" + tally(LSM=1),
        "chrB\t4\tAA\tGG\t0.3\t4\t2\t1\t" + w(1) + "\t" + tally(LSM=1),
        "chrB\t6\tAA\tGG\t0.7\t4\t4\t4\t" + w(4) + "\t" + "\t".join(z),
        "chrB\t6\tAA\tGG\t0.3\t4\t3\t3\t" + w(3) + "\t" + "\t".join(z)]
    assert w(4) == "1.0\t0.510109\t1.0" and w(0) == "0.0\t0.0\t0.489891" and w(2) == "0.5\t0.150039\t0.849961"
    curve = open(prefix + ".spikeScan.mnv.filter.curve.txt").read().splitlines()
    assert curve == ["CHROM\tPOS\tREF\tALT\tN_ALL\tRATE_PASS@0.3\tRATE_PASS@0.7\tT95_PASS",
                     "chrA\t3\tAA\tGG\t90\t0.0\t0.0\tNA",
                     "chrA\t7\tAA\tGG\t91\t0.0\t0.0\tNA",
                     "chrB\t4\tAA\tGG\t92\t0.25\t0.5\tNA",
                     "chrB\t6\tAA\tGG\t93\t0.75\t1.0\t0.7"]
    assert open(prefix + ".spikeScan0.7.mnv.passrate.bedgraph").read().splitlines() == \
        ["chrA\t2\t3\t0.0", "chrA\t6\t7\t0.0", "chrB\t3\t4\t0.5", "chrB\t5\t6\t1.0"]
    assert open(prefix + ".spikeScan0.3.mnv.passrate.bedgraph").read().splitlines() == \
        ["chrA\t2\t3\t0.0", "chrA\t6\t7\t0.0", "chrB\t3\t4\t0.25", "chrB\t5\t6\t0.75"]
    # T95_PASS NA writes 1, and so does a skipped locus
    assert open(prefix + ".spikeScan.mnv.t95pass.bedgraph").read().splitlines() == \
        ["chrA\t2\t3\t1", "chrA\t4\t5\t1", "chrA\t6\t7\t1", "chrB\t3\t4\t1", "chrB\t4\t5\t1", "chrB\t5\t6\t0.7"]
    assert sorted(os.listdir(str(tmp_path))) == sorted(["o.spikeScan.mnv.filter.txt", "o.spikeScan.mnv.filter.curve.txt",
                                                        "o.spikeScan0.7.mnv.passrate.bedgraph", "o.spikeScan0.3.mnv.passrate.bedgraph",
                                                        "o.spikeScan.mnv.t95pass.bedgraph"])
    # the page restated the way the GPU test restates it from replicate pages: (FILTER column, CALLED column) per replicate
    text = lambda wd: ";".join(n for b, n in abi.SCAN_FILTER_NAMES if int(wd) & b) or "PASS"
    for n, line in enumerate(page[1:]):
        i, t = divmod(n, 2)
        assert line.split("\t") == pages.line(line.split("\t")[:5], [(text(words[i, t, j]), "%d" % called[i, t, j]) for j in range(R)])


def test_the_snv_filter_pages_keep_their_names_and_headers(tmp_path):
    """write_scan_filter serves both scans: without `mnv` its files are --spikeScanFilter's."""
    v = [TM.af.Variant("chrA", 3, "A", "G", "G", TM.af.SNV)]
    spike.write_scan_filter(str(tmp_path / "o"), [("chrA", 3, 0), ("chrA", 4, None)], v, [0.5], [77], np.ones((1, 1, 2), bool),
                            np.array([[[0, LSM]]], np.uint32))
    assert sorted(os.listdir(str(tmp_path))) == ["o.spikeScan.filter.curve.txt", "o.spikeScan.filter.txt", "o.spikeScan.t95pass.bedgraph",
                                                 "o.spikeScan0.5.passrate.bedgraph"]
    page = open(str(tmp_path / "o.spikeScan.filter.txt")).read().splitlines()
    assert page[0].split("\t") == list(pages.HEADER) and page[1].split("\t")[:8] == ["chrA", "3", "A", "G", "0.5", "2", "2", "1"]
    assert open(str(tmp_path / "o.spikeScan.filter.curve.txt")).read().splitlines()[0] == "CHROM\tPOS\tREF\tALT\tN\tRATE_PASS@0.5\tT95_PASS"
    assert open(str(tmp_path / "o.spikeScan.t95pass.bedgraph")).read().splitlines() == ["chrA\t2\t3\t1", "chrA\t3\t4\t1"]


# ---- the entry
def test_the_entry_is_declared_and_bound_and_the_abi_number_stays():
    text = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"^int smc_scan_filter_sets\(", text, re.M) and re.search(r"^int smc_scan_filter\(", text, re.M)
    assert re.search(r"^#define SMC_ABI_VERSION 11$", text, re.M) and re.search(r"^#define SMC_SCAN_FLT_MEMBER_SHIFT 16$", text, re.M)
    assert "smc_scan_filter_sets" in _lib.SYMBOLS
    host = open(os.path.join(ROOT, "smcounter_amd", "csrc", "host_abi.inc")).read()
    assert re.search(r"^int smc_scan_filter_sets\(", host, re.M)
    L = _lib.load()
    assert L.smc_abi_version() == 11 and hasattr(L, "smc_scan_filter_sets")
    assert len(L.smc_scan_filter_sets.argtypes) == 17
    assert callable(devplanes.scan_filter_sets)
