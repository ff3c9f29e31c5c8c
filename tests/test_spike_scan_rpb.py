"""--spikeScanRpb without a GPU: every refusal before any file, the scans' messages unchanged without it, the page writers on hand-made
entries - the R95 rule, the skipped loci in the bedgraphs, the headers."""
import os
import re
import sys

import pytest

from conftest import ROOT
from smcounter_amd import cli, dsaf, spike
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402


def _args(tmp, **kw):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp))
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    d = dict(outPrefix=str(tmp / "o"), bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, refGenome=fa, spikeScan="0.3,0.7",
             spikeScanReps="4", spikeScanRpb="1.5,3")
    d.update(kw)
    return {k: v for k, v in d.items() if v is not None}


@pytest.mark.parametrize("kw,msg", [
    (dict(spikeScan=None, spikeScanReps=None), "--spikeScanRpb belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScanReps=None), "it needs --spikeScanReps"),
    (dict(spikeScanDepth="0.5"), "--spikeScanRpb cannot be combined with --spikeScanDepth in one run: the grid of targets x barcode "
                                 "fractions x reads-per-barcode targets is not built"),
    (dict(spikeScanIndel="del2", spikeScanDepth="0.5"), "--spikeScanRpb cannot be combined with --spikeScanDepth"),
    (dict(spikeScanRpb="1.5,x"), "--spikeScanRpb: comma-separated reads-per-barcode targets > 0 expected, got '1.5,x'"),
    (dict(spikeScanRpb="two"), "--spikeScanRpb: comma-separated reads-per-barcode targets > 0 expected, got 'two'"),
    (dict(spikeScanRpb="1.5,0"), "--spikeScanRpb: every target must be a number > 0, got '1.5,0'"),
    (dict(spikeScanRpb="-2"), "--spikeScanRpb: every target must be a number > 0, got '-2'"),
    (dict(spikeScanRpb="inf"), "--spikeScanRpb: every target must be a number > 0, got 'inf'"),
    (dict(spikeScanRpb=","), "--spikeScanRpb: every target must be a number > 0, got ','"),
    (dict(spikeScanRpb="1.5,1.50"), "--spikeScanRpb: a target is listed twice"),
    (dict(spikeScanRpb=",".join("%g" % (1 + 0.5 * k) for k in range(17))),
     "--spikeScanRpb: 2 targets x 17 reads-per-barcode targets = 34 cells, at most 32"),
    # everything --spikeScan and --spikeScanIndel refuse, with their texts
    (dict(spikeRpb="2"), "--spikeScan cannot be combined with --spikeRpb"),
    (dict(spikeIndelRpb="2"), "--spikeScan cannot be combined with --spikeIndelRpb"),
    (dict(dsRpb="2"), "--spikeScan cannot be combined with --dsRpb"),
    (dict(spikeScan="0.1,0.10"), "--spikeScan: a target is listed twice"),
    (dict(spikeScanReps="1"), "--spikeScanReps: an integer in 2 .. 1000 expected, got 1"),
    (dict(spikeScanStride="0"), "--spikeScanStride: an integer >= 1 expected, got 0"),
    (dict(spikeScanIndel="del2", spikeScanAlt="transition"), "--spikeScanIndel cannot be combined with --spikeScanAlt"),
    (dict(spikeScanIndel="del2", spikeScanStride="3"), "--spikeScanStride"),
    (dict(spikeScanIndel="sub2"), "--spikeScanIndel"),
])
def test_cli_refusals_before_any_file(tmp_path, kw, msg):
    assert spike.MAX_CELLS == 32
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(_args(tmp_path, **kw))
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_the_scans_messages_do_not_change_without_the_flag(tmp_path):
    for kw, msg in ((dict(spikeScanReps=None), "--spikeScan measures a detection rate over replicates: it needs --spikeScanReps"),
                    (dict(spikeScan=None), "--spikeScanReps belongs to --spikeScan: it needs --spikeScan"),
                    (dict(spikeScan="0.5,1"), "--spikeScan: every target allele fraction must lie in (0, 1)"),
                    (dict(spikeScan=None, spikeScanReps=None, spikeScanIndel="del2"), "--spikeScanIndel belongs to --spikeScan: it needs --spikeScan"),
                    (dict(spikeScanIndel="del2", spikeScanAlt="transition"), "--spikeScanIndel cannot be combined with --spikeScanAlt"),
                    (dict(spikeScan=None, spikeScanReps=None, spikeScanDepth="0.5"), "--spikeScanDepth belongs to --spikeScan: it needs --spikeScan"),
                    (dict(spikeScanDepth="0.5,0"), "--spikeScanDepth: every fraction must lie in (0, 1], got '0.5,0'"),
                    (dict(spikeScanDepth="0.5,0.50"), "--spikeScanDepth: a fraction is listed twice")):
        with pytest.raises(SystemExit) as e:
            cli.main(_args(tmp_path, spikeScanRpb=None, **kw))
        assert str(e.value).startswith(msg)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_the_flag_is_parsed_into_the_scans_dict():
    import argparse
    ns = argparse.Namespace(spikeScan="0.3,0.7", spikeScanReps="4", spikeScanRpb="1.5, 3,20")
    got = spike.scan(ns)
    assert got["rpbs"] == [1.5, 3.0, 20.0] and got["targets"] == [0.3, 0.7] and got["reps"] == 4 and "fracs" not in got
    assert "rpbs" not in spike.scan(argparse.Namespace(spikeScan="0.3,0.7", spikeScanReps="4"))
    assert spike.scan(argparse.Namespace(spikeScan="0.3", spikeScanReps="4", spikeScanIndel="del2", spikeScanRpb="2"))["rpbs"] == [2.0]
    assert "--spikeScanRpb" in cli.build_parser().format_help()


# ---- the writers on hand-made entries
V = [af.Variant("chrA", 101, "A", "G", "G", af.SNV), af.Variant("chrA", 103, "C", "T", "T", af.SNV), af.Variant("chrB", 7, "G", "A", "A", af.SNV)]
LOCI = [("chrA", 101, 0), ("chrA", 102, None), ("chrA", 103, 1), ("chrB", 7, 2)]        # (chrA:102: skipped for its letter)
TARGETS, RPBS, R = [0.1, 0.02], [4, 2], 100                                              # (the r are listed in descending order)
MT, RUN_RPB = 1000, 6.5


def _per(v, n, called):
    """R replicates of which the first `called` are called; N covering barcodes."""
    return [spike.scan_entry(v, dict(N=n, V0=1, S=3 + (j % 2), READS=9, V1=4 + (j % 3)), j < called) for j in range(R)]


def _entries(full_called, cell_called):
    """full_called[i][t], cell_called[i][t][r]: the called replicates."""
    full = {(i, t): _per(V[i], 200 + i, full_called[i][t]) for i in range(3) for t in range(2)}
    cells = {(i, t, r): _per(V[i], 190 + i - 10 * r, cell_called[i][t][r]) for i in range(3) for t in range(2) for r in range(2)}
    return full, cells


# variant 0: monotone - target 0.1 passes down to r = 2, target 0.02 only at full depth
# variant 1: NOT monotone at target 0.1 (0.96 at r = 2 but 0.9 at r = 4: R95 = full); target 0.02 fails at full depth (NA) though r = 4 passes
# variant 2: passes at r = 4, not at r = 2; target 0.02 fails everywhere
FULL = [[100, 95], [99, 94], [100, 0]]
CELLS = [[[100, 97], [94, 50]], [[90, 96], [99, 10]], [[95, 94], [0, 0]]]
R95 = [["2", "full"], ["full", "NA"], ["4", "NA"]]


def _write(tmp_path):
    full, cells = _entries(FULL, CELLS)
    prefix = str(tmp_path / "w")
    spike.write_scan_rpb(prefix, LOCI, V, TARGETS, RPBS, MT, RUN_RPB, full, cells)
    return prefix, full, cells


def test_the_headers():
    assert spike.SCAN_RPB_SENSITIVITY_HEADER == ("CHROM", "POS", "REF", "ALT", "TARGET", "RPB", "MTDEPTH", "REPS", "CALLED", "RATE",
                                                 "LO95", "HI95", "AF_MEAN", "AF_MIN", "AF_MAX", "S_MIN", "S_MAX", "V_MIN", "V_MAX", "N_MEAN")
    assert spike.SCAN_RPB_NEED_HEADER == ("CHROM", "POS", "REF", "ALT", "TARGET", "N", "R95", "N95")
    assert spike.depth_curve_header(TARGETS, False, spike.RPB_AXIS) == ("CHROM", "POS", "REF", "ALT", "RPB", "MTDEPTH", "N_MEAN", "RATE@0.02",
                                                                        "RATE@0.1", "T95")


def test_the_pages_are_the_rpb_pages_lines(tmp_path):
    prefix, full, cells = _write(tmp_path)
    sens = open(prefix + ".spikeScan.rpb.sensitivity.txt").read().splitlines()
    assert sens[0].split("\t") == list(spike.SCAN_RPB_SENSITIVITY_HEADER) and len(sens) == 1 + 3 * 2 * 2
    head = spike.cell_sensitivity_header(spike.RPB_AXIS)
    drop = [head.index(c) for c in ("PI_MEAN", "PI_MIN")]
    n = 1
    for i, v in enumerate(V):
        for t, target in enumerate(TARGETS):
            for r, rpb in enumerate(RPBS):
                # (the line --spikeRpb's page has for the cell: every cell at the run's mtDepth)
                want = spike.depth_sensitivity_line(v, target, rpb, MT, cells[(i, t, r)]).split("\t")
                assert sens[n].split("\t") == [x for k, x in enumerate(want) if k not in drop]
                assert sens[n].split("\t")[5:7] == ["%g" % rpb, "%d" % MT]
                assert sens[n].split("\t")[-1] == dsaf.frac_text(float(190 + i - 10 * r))              # (N_MEAN stays)
                n += 1
    curve = open(prefix + ".spikeScan.rpb.curve.txt").read().splitlines()
    assert curve[0].split("\t") == list(spike.depth_curve_header(TARGETS, False, spike.RPB_AXIS)) and len(curve) == 1 + 3 * 3
    n = 1
    for i, v in enumerate(V):
        assert curve[n] == spike.depth_curve_line(v, None, [MT, MT], TARGETS, [full[(i, 0)], full[(i, 1)]])
        assert curve[n].split("\t")[4:6] == ["full", "%d" % MT]
        for r, rpb in enumerate(RPBS):
            assert curve[n + 1 + r] == spike.depth_curve_line(v, rpb, [MT] * 2, TARGETS, [cells[(i, 0, r)], cells[(i, 1, r)]])
        n += 3
    assert "LOD" not in "\n".join(sens) and "LOD" not in "\n".join(curve)


def test_the_r95_rule_and_the_need_page(tmp_path):
    assert spike.r95([2, 4], [0.97, 1.0], 1.0) == 0                             # monotone: the smallest target
    assert spike.r95([4, 2], [1.0, 0.97], 1.0) == 1                             # (the order of the list does not matter)
    assert spike.r95([2, 4], [0.96, 0.9], 0.99) == dsaf.FULL                    # 0.96 at 2 but 0.9 at 4: only full depth
    assert spike.r95([2, 4], [0.5, 0.94], 0.95) == dsaf.FULL                    # only full depth passes (at least 0.95)
    assert spike.r95([2, 4], [0.99, 0.99], 0.94) is None                        # full depth fails
    assert spike.r95([2, 4], [0.5, 0.95], 0.95) == 1
    prefix, _, _ = _write(tmp_path)
    need = [l.split("\t") for l in open(prefix + ".spikeScan.rpb.need.txt").read().splitlines()]
    assert need[0] == list(spike.SCAN_RPB_NEED_HEADER) and len(need) == 1 + 3 * 2
    n = 1
    for i, v in enumerate(V):
        for t, target in enumerate(TARGETS):
            want, row = R95[i][t], need[n]
            assert row[:6] == [v.chrom, "%d" % v.pos, v.ref, v.alt, "%g" % target, "%d" % (200 + i)]
            if want == "NA":
                assert row[6:] == ["NA", "NA"]
            elif want == "full":
                assert row[6:] == ["full", dsaf.frac_text(float(200 + i))]
            else:
                assert row[6:] == [want, dsaf.frac_text(float(190 + i - 10 * RPBS.index(int(want))))]
            n += 1


def test_the_bedgraphs_and_their_skipped_loci(tmp_path):
    prefix, _, _ = _write(tmp_path)
    sens = [l.split("\t") for l in open(prefix + ".spikeScan.rpb.sensitivity.txt").read().splitlines()][1:]
    curve = [l.split("\t") for l in open(prefix + ".spikeScan.rpb.curve.txt").read().splitlines()]
    need = [l.split("\t") for l in open(prefix + ".spikeScan.rpb.need.txt").read().splitlines()][1:]
    i_rate, i_t95 = spike.SCAN_RPB_SENSITIVITY_HEADER.index("RATE"), curve[0].index("T95")
    for t in TARGETS:
        for r in RPBS:
            lines = open("%s.spikeScan%g.dsRpb%g.rate.bedgraph" % (prefix, t, r)).read().splitlines()
            mine = [x for x in sens if x[4] == "%g" % t and x[5] == "%g" % r]
            assert lines == ["%s\t%d\t%d\t%s" % (x[0], int(x[1]) - 1, int(x[1]), x[i_rate]) for x in mine] and len(lines) == 3   # (no skipped locus)
    for r in RPBS:
        t95 = {(x[0], int(x[1])): x[i_t95] for x in curve[1:] if x[4] == "%g" % r}
        lines = open("%s.spikeScan.dsRpb%g.t95.bedgraph" % (prefix, r)).read().splitlines()
        assert lines == ["%s\t%d\t%d\t%s" % (c, p - 1, p, "1" if t95.get((c, p), "NA") == "NA" else t95[(c, p)]) for c, p, _ in LOCI]
        assert lines[1] == "chrA\t101\t102\t1"                                     # (the skipped locus)
    assert "NA" in [x[i_t95] for x in curve[1:]]
    # R95 as a number: `full` is the run's --rpb, NA and a skipped locus twice the larger of --rpb and the largest r - above the axis
    for t, target in enumerate(TARGETS):
        lines = open("%s.spikeScan%g.r95.bedgraph" % (prefix, target)).read().splitlines()
        page = {(x[0], int(x[1])): x[6] for x in need if x[4] == "%g" % target}
        assert [page[(c, p)] for c, p, i in LOCI if i is not None] == [R95[i][t] for i in range(3)]
        text = lambda w: "13" if w in (None, "NA") else "6.5" if w == "full" else w
        assert lines == ["%s\t%d\t%d\t%s" % (c, p - 1, p, text(page.get((c, p)))) for c, p, _ in LOCI]
    assert open(prefix + ".spikeScan0.02.r95.bedgraph").read().splitlines()[:3] == ["chrA\t100\t101\t6.5", "chrA\t101\t102\t13", "chrA\t102\t103\t13"]
    # (a listed r above --rpb lifts the mark above the axis)
    full, cells = _entries(FULL, CELLS)
    spike.write_scan_rpb(str(tmp_path / "hi"), LOCI, V, TARGETS, RPBS, MT, 1.0, full, cells)
    assert open(str(tmp_path / "hi") + ".spikeScan0.02.r95.bedgraph").read().splitlines()[:2] == ["chrA\t100\t101\t1", "chrA\t101\t102\t8"]
    names = sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("w."))
    assert len(names) == 3 + 4 + 2 + 2
