"""--spikeScanMnvRpb without a GPU: the flag's parsing and every refusal before any file is written, spike.scan()'s dict, the stage's
refusals (the key is "reads"; "rpb" stays refused), and the page writers on hand-made entries with the lines checked literally."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import abi, cli, devplanes, spike
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import scan_filter_pages as pages  # noqa: E402
import test_spike_scan_mnv as TM  # noqa: E402  (its arguments of a run and its hand-made MNVs)

FLAG = "spikeScanMnvRpb"
SHIFT = abi.SCAN_FLT_MEMBER_SHIFT
REPT = dict((n, b) for b, n in abi.SCAN_FILTER_NAMES)["RepT"]


@pytest.mark.parametrize("kw,msg", [
    (dict(spikeScanMnv=None), "--spikeScanMnvRpb belongs to --spikeScanMnv: it needs --spikeScanMnv"),
    (dict(spikeScan=None, spikeScanReps=None, spikeScanStride=None, spikeScanMnv=None),
     "--spikeScanMnvRpb belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScanMnvDepth="0.5"), "--spikeScanMnvRpb cannot be combined with --spikeScanMnvDepth in one run: the grid of targets x barcode "
                                    "fractions x reads-per-barcode targets is not built"),
    (dict(spikeScanMnvRpb="two"), "--spikeScanMnvRpb: comma-separated reads-per-barcode targets > 0 expected, got 'two'"),
    (dict(spikeScanMnvRpb="2;1.5"), "--spikeScanMnvRpb: comma-separated reads-per-barcode targets > 0 expected"),
    (dict(spikeScanMnvRpb="2,0"), "--spikeScanMnvRpb: every target must be a number > 0"),
    (dict(spikeScanMnvRpb="-1"), "--spikeScanMnvRpb: every target must be a number > 0"),
    (dict(spikeScanMnvRpb=","), "--spikeScanMnvRpb: every target must be a number > 0"),
    (dict(spikeScanMnvRpb="inf"), "--spikeScanMnvRpb: every target must be a number > 0"),
    (dict(spikeScanMnvRpb="2,2.0"), "--spikeScanMnvRpb: a target is listed twice"),
    (dict(spikeScanMnvRpb=",".join("%g" % (1 + x / 10.0) for x in range(17))),
     "--spikeScanMnvRpb: 2 targets x 17 reads-per-barcode targets = 34 cells, at most 32"),
    # everything --spikeScanMnv refuses, with today's messages - the flag beside --spikeScanRpb among them
    (dict(spikeScanRpb="2"), "--spikeScanMnv cannot be combined with --spikeScanRpb: the reads-per-barcode axis of an MNV scan is not built"),
    (dict(spikeScanDepth="0.5"), "--spikeScanMnv cannot be combined with --spikeScanDepth: the depth axis of an MNV scan is not built"),
    (dict(spikeScanFilter=True), "--spikeScanMnv cannot be combined with --spikeScanFilter: the filter axis of an MNV scan is not built"),
    (dict(spikeScanIndel="del1"), "--spikeScanMnv cannot be combined with --spikeScanIndel"),
    (dict(spikeScanMnv="9"), "--spikeScanMnv: an integer in 2 .. 8 expected"),
    (dict(spikeScanMnv="3", spikeScanStride="2"), "the smallest stride allowed is 3"),
    (dict(spikeScanReps=None), "it needs --spikeScanReps"),
    (dict(spikeReps="4"), "--spikeScan cannot be combined with --spikeReps"),
    (dict(spikePhaseRpb="2"), "--spikeScan cannot be combined with --spikePhaseRpb"),
    (dict(dsMT="0.5"), "--spikeScan cannot be combined with --dsMT"),
    (dict(dsRpb="2"), "--spikeScan cannot be combined with --dsRpb"),
    (dict(spikeScanBuild="some"), "--spikeScanBuild: whole or listed expected"),
])
@pytest.mark.parametrize("beside", (False, True))
def test_refusals_before_any_file(tmp_path, kw, msg, beside):
    """The flag alone and beside --spikeScanMnvFilter, through spike.scan and through cli.main."""
    args = TM._args(tmp_path, **dict(dict(spikeScanMnvRpb="2,1.5"), **kw))
    switches = (["--spikeScanMnvFilter"] if beside else []) + (["--spikeScanFilter"] if args.pop("spikeScanFilter", False) else [])
    args = cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in args.items()] + switches)
    if beside and " belongs to " in msg:         # (beside the switch the first of the two flags is named)
        msg = msg.replace(FLAG, "spikeScanMnvFilter")
    with pytest.raises(SystemExit, match=re.escape(msg)):
        spike.scan(args)
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(args)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_the_flag_is_read_and_more_processes_are_refused(tmp_path, monkeypatch):
    ns = argparse.Namespace(spikeScan="0.7,0.3", spikeScanReps="32", spikeScanMnv="3", spikeScanStride=3)
    today = dict(targets=[0.7, 0.3], reps=32, stride=3, alt="transition", mnv=3)
    assert spike.scan(ns) == today
    ns.spikeScanMnvRpb = "4, 2,1.5"
    assert spike.scan(ns) == dict(today, mnv_rpbs=[4.0, 2.0, 1.5])
    ns.spikeScanMnvFilter, ns.spikeScanBuild = True, "listed"
    assert spike.scan(ns) == dict(today, mnv_rpbs=[4.0, 2.0, 1.5], mnv_filter=True, build="listed")
    ns.spikeScanMnvRpb = ",".join("%g" % (1 + x / 10.0) for x in range(16))          # 2 x 16 = 32 cells: allowed
    assert len(spike.scan(ns)["mnv_rpbs"]) == 16
    parser = cli.build_parser()
    assert parser.get_default(FLAG) is None and "--spikeScanMnvRpb" in parser.format_help()
    assert "smc_scan_phase_rpb_counts" in re.sub(r"\s+", " ", parser.format_help())
    # --spikeScanRpb keeps its own messages
    with pytest.raises(SystemExit, match=re.escape("--spikeScanRpb: a target is listed twice")):
        spike.scan(argparse.Namespace(spikeScan="0.5", spikeScanReps="8", spikeScanRpb="2,2"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    args = parser.parse_args(["--%s=%s" % (k, v) for k, v in TM._args(tmp_path, spikeScanMnvRpb="2").items()])
    with pytest.raises(SystemExit, match="--spikeScan runs in one process only"):
        cli.main(args)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_the_stage_takes_reads_and_keeps_its_refusals():
    call = lambda **kw: devplanes.spike_scan("x.bam", None, sv.PhasedVariants(), [], [0.5], None, 1, 2, None, 5, None, **kw)
    reads = dict(targets=[2.0], params=[None], thresholds=[5])
    with pytest.raises(ValueError, match="need --spikeScanMnv"):
        call(mnv_axes=dict(reads=reads))
    with pytest.raises(ValueError, match=re.escape("--spikeScanMnvRpb: the grid of barcode fractions x reads-per-barcode targets is not built")):
        call(mnv=2, mnv_axes=dict(reads=reads, depth=dict(fracs=[0.5])))
    with pytest.raises(ValueError, match=re.escape("--spikeScanMnv: the reads-per-barcode axis of an MNV scan is not built")):
        call(mnv=2, mnv_axes=dict(rpb=reads))
    with pytest.raises(ValueError, match="not built"):
        call(mnv=2, mnv_axes=dict(reads=reads, rpb=reads))
    for kw in (dict(flt=True), dict(depth=dict(fracs=[0.5])), dict(rpb=reads), dict(indel=True)):
        with pytest.raises(ValueError, match="not built"):
            call(mnv=2, mnv_axes=dict(reads=reads), **kw)


def test_page_writers_from_hand_made_entries(tmp_path):
    leaders = [("chrA", 3), ("chrA", 7), ("chrB", 4)]
    mnvs = TM._mnvs(leaders, 2)
    loci = [("chrA", 3, 0), ("chrA", 5, None), ("chrA", 7, 1), ("chrB", 4, 2)]
    targets, rpbs, R, mt_depth, run_rpb = [0.7, 0.3], [2.0, 1.5], 4, 240, 2.9
    # called replicates (None: full depth; 0: r = 2; 1: r = 1.5).  Set 0: everywhere at 0.7 (R95 1.5); at 0.3 full and r = 2 (R95 2).
    # Set 1: at full depth only (R95 full).  Set 2: at 0.7 both cells pass and full depth does not (NA); at 0.3 never (NA).
    n_called = {(0, 0, None): 4, (0, 0, 0): 4, (0, 0, 1): 4, (0, 1, None): 4, (0, 1, 0): 4, (0, 1, 1): 3,
                (1, 0, None): 4, (1, 0, 0): 3, (1, 0, 1): 0, (1, 1, None): 4, (1, 1, 0): 1, (1, 1, 1): 0,
                (2, 0, None): 3, (2, 0, 0): 4, (2, 0, 1): 4, (2, 1, None): 0, (2, 1, 0): 0, (2, 1, 1): 0}
    n_all = {None: 100, 0: 80, 1: 60}
    per = lambda i, t, r: [(dict(N_ALL=n_all[r] + i + j, V0_ALL=0, S_ALL=5 + j, V1_ALL=5 + j), int(j < n_called[(i, t, r)])) for j in range(R)]
    full = {(i, t): per(i, t, None) for i in range(3) for t in range(2)}
    cells = {(i, t, r): per(i, t, r) for i in range(3) for t in range(2) for r in range(2)}
    prefix = str(tmp_path / "o")
    spike.write_scan_mnv_rpb(prefix, loci, mnvs, mnvs.sets, targets, rpbs, mt_depth, run_rpb, full, cells)
    sens = open(prefix + ".spikeScan.mnv.rpb.sensitivity.txt").read().splitlines()
    head = list(spike.phase_sensitivity_header(spike.RPB_AXIS))
    assert sens[0].split("\t") == head and head[5:8] == ["TARGET", "RPB", "MTDEPTH"] and "LOD" not in head
    # every cell is called at the scan's mtDepth
    assert sens[1:] == [spike.phase_sensitivity_line(mnvs.sets[i], mnvs, targets[t], rpbs[r], mt_depth, cells[(i, t, r)])
                        for i in range(3) for t in range(2) for r in range(2)]
    assert sens[1].split("\t")[:11] == ["chrA:3", "chrA", "3,4", "A,A", "G,G", "0.7", "2", "240", "4", "4", "1.0"]
    assert sens[2].split("\t")[:11] == ["chrA:3", "chrA", "3,4", "A,A", "G,G", "0.7", "1.5", "240", "4", "4", "1.0"]
    curve = open(prefix + ".spikeScan.mnv.rpb.curve.txt").read().splitlines()
    assert curve[0].split("\t") == list(spike.depth_curve_header(targets, False, spike.RPB_AXIS))
    assert curve[0] == "CHROM\tPOS\tREF\tALT\tRPB\tMTDEPTH\tN_MEAN\tRATE@0.3\tRATE@0.7\tT95"
    # (N_MEAN: the mean N_ALL' of the cell over replicates and targets - 100 + i + 1.5 at full depth)
    assert curve[1:] == ["chrA\t3\tAA\tGG\tfull\t240\t101.5\t1.0\t1.0\t0.3", "chrA\t3\tAA\tGG\t2\t240\t81.5\t1.0\t1.0\t0.3",
                         "chrA\t3\tAA\tGG\t1.5\t240\t61.5\t0.75\t1.0\t0.7",
                         "chrA\t7\tAA\tGG\tfull\t240\t102.5\t1.0\t1.0\t0.3", "chrA\t7\tAA\tGG\t2\t240\t82.5\t0.25\t0.75\tNA",
                         "chrA\t7\tAA\tGG\t1.5\t240\t62.5\t0.0\t0.0\tNA",
                         "chrB\t4\tAA\tGG\tfull\t240\t103.5\t0.0\t0.75\tNA", "chrB\t4\tAA\tGG\t2\t240\t83.5\t0.0\t1.0\t0.7",
                         "chrB\t4\tAA\tGG\t1.5\t240\t63.5\t0.0\t1.0\t0.7"]
    # R95: the smallest of (1.5, 2, full) whose rate is at least 0.95 together with every larger entry's; N95 the mean N_ALL' there
    need = open(prefix + ".spikeScan.mnv.rpb.need.txt").read().splitlines()
    assert need == ["CHROM\tPOS\tREF\tALT\tTARGET\tN_ALL\tR95\tN95",
                    "chrA\t3\tAA\tGG\t0.7\t100\t1.5\t61.5", "chrA\t3\tAA\tGG\t0.3\t100\t2\t81.5",
                    "chrA\t7\tAA\tGG\t0.7\t101\tfull\t102.5", "chrA\t7\tAA\tGG\t0.3\t101\tfull\t102.5",
                    "chrB\t4\tAA\tGG\t0.7\t102\tNA\tNA", "chrB\t4\tAA\tGG\t0.3\t102\tNA\tNA"]
    # the fill values of .spikeScan<t>.r95.bedgraph: `full` as the run's --rpb, NA and a skipped locus twice the largest of --rpb and the targets
    assert open(prefix + ".spikeScan0.7.mnv.r95.bedgraph").read().splitlines() == \
        ["chrA\t2\t3\t1.5", "chrA\t4\t5\t5.8", "chrA\t6\t7\t2.9", "chrB\t3\t4\t5.8"]
    assert open(prefix + ".spikeScan0.3.mnv.r95.bedgraph").read().splitlines() == \
        ["chrA\t2\t3\t2", "chrA\t4\t5\t5.8", "chrA\t6\t7\t2.9", "chrB\t3\t4\t5.8"]
    assert open(prefix + ".spikeScan0.3.dsRpb1.5.mnv.rate.bedgraph").read().splitlines() == \
        ["chrA\t2\t3\t0.75", "chrA\t6\t7\t0.0", "chrB\t3\t4\t0.0"]
    # T95 NA writes 1, and so does a skipped locus
    assert open(prefix + ".spikeScan.dsRpb2.mnv.t95.bedgraph").read().splitlines() == \
        ["chrA\t2\t3\t0.3", "chrA\t4\t5\t1", "chrA\t6\t7\t1", "chrB\t3\t4\t0.7"]
    assert sorted(os.listdir(str(tmp_path))) == sorted(
        ["o.spikeScan.mnv.rpb.sensitivity.txt", "o.spikeScan.mnv.rpb.curve.txt", "o.spikeScan.mnv.rpb.need.txt",
         "o.spikeScan.dsRpb2.mnv.t95.bedgraph", "o.spikeScan.dsRpb1.5.mnv.t95.bedgraph", "o.spikeScan0.7.mnv.r95.bedgraph",
         "o.spikeScan0.3.mnv.r95.bedgraph"] + ["o.spikeScan%g.dsRpb%g.mnv.rate.bedgraph" % (t, r) for t in targets for r in rpbs])
    # the cells' filter page beside the switch
    called = np.zeros((3, 2, 2, R), bool)
    words = np.zeros((3, 2, 2, R), np.uint32)
    called[0], words[0, :, 1] = True, REPT | (2 << SHIFT)
    spike.write_scan_filter_cells(prefix, [spike.scan_mnv_variant(ps, mnvs) for ps in mnvs.sets], targets, rpbs, [mt_depth] * 2, called, words,
                                  spike.RPB_AXIS, mnv=True)
    page = open(prefix + ".spikeScan.mnv.rpb.filter.txt").read().splitlines()
    assert page[0].split("\t") == ["CHROM", "POS", "REF", "ALT", "TARGET", "RPB", "MTDEPTH", "REPS", "CALLED_ALL", "PASS_ALL", "RATE_PASS",
                                   "LO95", "HI95"] + list(pages.NAMES)
    assert len(page) == 1 + 3 * 2 * 2
    assert page[1].split("\t")[:11] == ["chrA", "3", "AA", "GG", "0.7", "2", "240", "4", "4", "4", "1.0"]
    assert page[2].split("\t")[:11] == ["chrA", "3", "AA", "GG", "0.7", "1.5", "240", "4", "4", "0", "0.0"]
    assert page[2].split("\t")[13 + pages.NAMES.index("RepT")] == "4" and page[5].split("\t")[7:10] == ["4", "0", "0"]


def test_the_snv_scans_read_axis_keeps_its_names_and_headers(tmp_path):
    """write_scan_rpb serves both scans: without `mnv` its files are --spikeScanRpb's."""
    v = [TM.af.Variant("chrA", 3, "A", "G", "G", TM.af.SNV)]
    e = lambda n: [spike.scan_entry(v[0], dict(N=n, V0=0, S=3, READS=9, V1=3), True) for _ in range(2)]
    spike.write_scan_rpb(str(tmp_path / "o"), [("chrA", 3, 0), ("chrA", 4, None)], v, [0.5], [2.0], 240, 3.0, {(0, 0): e(50)}, {(0, 0, 0): e(40)})
    assert sorted(os.listdir(str(tmp_path))) == ["o.spikeScan.dsRpb2.t95.bedgraph", "o.spikeScan.rpb.curve.txt", "o.spikeScan.rpb.need.txt",
                                                 "o.spikeScan.rpb.sensitivity.txt", "o.spikeScan0.5.dsRpb2.rate.bedgraph", "o.spikeScan0.5.r95.bedgraph"]
    assert open(str(tmp_path / "o.spikeScan.rpb.sensitivity.txt")).read().splitlines()[0].split("\t") == list(spike.SCAN_RPB_SENSITIVITY_HEADER)
    assert open(str(tmp_path / "o.spikeScan.rpb.need.txt")).read().splitlines() == ["CHROM\tPOS\tREF\tALT\tTARGET\tN\tR95\tN95",
                                                                                  "chrA\t3\tA\tG\t0.5\t50\t2\t40.0"]
    assert open(str(tmp_path / "o.spikeScan0.5.r95.bedgraph")).read().splitlines() == ["chrA\t2\t3\t2", "chrA\t3\t4\t6"]
