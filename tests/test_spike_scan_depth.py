"""--spikeScanDepth without a GPU: every refusal before any file, the scan's messages unchanged beside it, the page writers on hand-made
entries - the F95 rule, the skipped loci in the bedgraphs, the headers."""
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
             spikeScanReps="4", spikeScanDepth="0.5,0.25")
    d.update(kw)
    return {k: v for k, v in d.items() if v is not None}


@pytest.mark.parametrize("kw,msg", [
    (dict(spikeScan=None, spikeScanReps=None), "--spikeScanDepth belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScanReps=None), "it needs --spikeScanReps"),
    (dict(spikeScanDepth="0.5,x"), "--spikeScanDepth: comma-separated fractions in (0, 1] expected, got '0.5,x'"),
    (dict(spikeScanDepth="half"), "--spikeScanDepth: comma-separated fractions in (0, 1] expected, got 'half'"),
    (dict(spikeScanDepth="0.5,0"), "--spikeScanDepth: every fraction must lie in (0, 1], got '0.5,0'"),
    (dict(spikeScanDepth="1.5"), "--spikeScanDepth: every fraction must lie in (0, 1], got '1.5'"),
    (dict(spikeScanDepth="-0.5"), "--spikeScanDepth: every fraction must lie in (0, 1], got '-0.5'"),
    (dict(spikeScanDepth=","), "--spikeScanDepth: every fraction must lie in (0, 1], got ','"),
    (dict(spikeScanDepth="0.5,0.50"), "--spikeScanDepth: a fraction is listed twice"),
    (dict(spikeScanDepth=",".join("%g" % (0.05 * k) for k in range(1, 18))), "--spikeScanDepth: 2 targets x 17 fractions = 34 cells, at most 32"),
    # everything --spikeScan and --spikeScanIndel refuse, with their texts
    (dict(spikeDepth="0.5"), "--spikeScan cannot be combined with --spikeDepth"),
    (dict(spikeIndelDepth="0.5"), "--spikeScan cannot be combined with --spikeIndelDepth"),
    (dict(dsMT="0.5"), "--spikeScan cannot be combined with --dsMT"),
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
                    (dict(spikeScan="0.5,1"), "--spikeScan: every target allele fraction must lie in (0, 1)")):
        with pytest.raises(SystemExit) as e:
            cli.main(_args(tmp_path, spikeScanDepth=None, **kw))
        assert str(e.value).startswith(msg)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_the_flag_is_parsed_into_the_scans_dict():
    import argparse
    ns = argparse.Namespace(spikeScan="0.3,0.7", spikeScanReps="4", spikeScanDepth="0.5, 0.25,1")
    got = spike.scan(ns)
    assert got["fracs"] == [0.5, 0.25, 1.0] and got["targets"] == [0.3, 0.7] and got["reps"] == 4
    assert "fracs" not in spike.scan(argparse.Namespace(spikeScan="0.3,0.7", spikeScanReps="4"))
    assert "--spikeScanDepth" in cli.build_parser().format_help()
    assert spike.scan_depth_mt(1000, 0.25) == 250 and spike.scan_depth_mt(3, 0.1) == 1 and spike.scan_depth_mt(5, 0.5) == 3      # (py2 round)


# ---- the writers on hand-made entries
V = [af.Variant("chrA", 101, "A", "G", "G", af.SNV), af.Variant("chrA", 103, "C", "T", "T", af.SNV), af.Variant("chrB", 7, "G", "A", "A", af.SNV)]
LOCI = [("chrA", 101, 0), ("chrA", 102, None), ("chrA", 103, 1), ("chrB", 7, 2)]        # (chrA:102: skipped for its letter)
TARGETS, FRACS, R = [0.1, 0.02], [0.5, 0.25], 100


def _per(v, n, called):
    """R replicates of which the first `called` are called; N covering barcodes."""
    return [spike.scan_entry(v, dict(N=n, V0=1, S=3 + (j % 2), READS=9, V1=4 + (j % 3)), j < called) for j in range(R)]


def _entries(full_called, cell_called):
    """full_called[i][t], cell_called[i][t][f]: the called replicates."""
    full = {(i, t): _per(V[i], 200 + i, full_called[i][t]) for i in range(3) for t in range(2)}
    cells = {(i, t, f): _per(V[i], (200 + i) // (2 << f), cell_called[i][t][f]) for i in range(3) for t in range(2) for f in range(2)}
    return full, cells


# variant 0: monotone - target 0.1 passes down to 0.25, target 0.02 only at full depth
# variant 1: NOT monotone at target 0.1 (0.96 at 0.25 but 0.9 at 0.5: F95 = 1); target 0.02 fails at full depth (NA) though 0.5 passes
# variant 2: passes at 0.5, not at 0.25; target 0.02 fails everywhere
FULL = [[100, 95], [99, 94], [100, 0]]
CELLS = [[[100, 97], [94, 50]], [[90, 96], [99, 10]], [[95, 94], [0, 0]]]
F95 = [["0.25", "1"], ["1", "NA"], ["0.5", "NA"]]


def _write(tmp_path, mt_depth=1000):
    full, cells = _entries(FULL, CELLS)
    prefix = str(tmp_path / "w")
    spike.write_scan_depth(prefix, LOCI, V, TARGETS, FRACS, mt_depth, full, cells)
    return prefix, full, cells


def test_the_headers():
    assert spike.SCAN_DEPTH_SENSITIVITY_HEADER == ("CHROM", "POS", "REF", "ALT", "TARGET", "FRACTION", "MTDEPTH", "REPS", "CALLED", "RATE",
                                                   "LO95", "HI95", "AF_MEAN", "AF_MIN", "AF_MAX", "S_MIN", "S_MAX", "V_MIN", "V_MAX", "N_MEAN")
    assert spike.SCAN_NEED_HEADER == ("CHROM", "POS", "REF", "ALT", "TARGET", "N", "F95", "MTDEPTH95", "N95")
    assert spike.depth_curve_header(TARGETS) == ("CHROM", "POS", "REF", "ALT", "DEPTH", "MTDEPTH", "N_MEAN", "RATE@0.02", "RATE@0.1", "T95")


def test_the_pages_are_the_depth_pages_lines(tmp_path):
    prefix, full, cells = _write(tmp_path)
    sens = open(prefix + ".spikeScan.depth.sensitivity.txt").read().splitlines()
    assert sens[0].split("\t") == list(spike.SCAN_DEPTH_SENSITIVITY_HEADER) and len(sens) == 1 + 3 * 2 * 2
    drop = [spike.DEPTH_SENSITIVITY_HEADER.index(c) for c in ("PI_MEAN", "PI_MIN")]
    n = 1
    for i, v in enumerate(V):
        for t, target in enumerate(TARGETS):
            for f, frac in enumerate(FRACS):
                want = spike.depth_sensitivity_line(v, target, frac, [500, 250][f], cells[(i, t, f)]).split("\t")
                assert sens[n].split("\t") == [x for k, x in enumerate(want) if k not in drop]
                assert sens[n].split("\t")[-1] == dsaf.frac_text(float((200 + i) // (2 << f)))            # (N_MEAN stays)
                n += 1
    curve = open(prefix + ".spikeScan.depth.curve.txt").read().splitlines()
    assert curve[0].split("\t") == list(spike.depth_curve_header(TARGETS)) and len(curve) == 1 + 3 * 3
    n = 1
    for i, v in enumerate(V):
        assert curve[n] == spike.depth_curve_line(v, None, [1000, 1000], TARGETS, [full[(i, 0)], full[(i, 1)]])
        assert curve[n].split("\t")[4:6] == ["full", "1000"]
        for f, frac in enumerate(FRACS):
            assert curve[n + 1 + f] == spike.depth_curve_line(v, frac, [[500, 250][f]] * 2, TARGETS, [cells[(i, 0, f)], cells[(i, 1, f)]])
        n += 3
    with_lod = open(prefix + ".spikeScan.depth.sensitivity.txt").read()
    assert "LOD" not in with_lod and "LOD" not in "\n".join(curve)


def test_the_f95_rule_and_the_need_page(tmp_path):
    assert spike.f95([0.5, 0.25, 1.0], [1.0, 0.97, 1.0]) == 1                   # monotone: the smallest depth
    assert spike.f95([0.5, 0.25, 1.0], [0.9, 0.96, 0.99]) == 2                  # 0.96 at 0.25 but 0.9 at 0.5: full depth
    assert spike.f95([0.5, 0.25, 1.0], [0.99, 0.99, 0.94]) is None              # full depth fails
    assert spike.f95([0.5, 1.0], [0.95, 0.95]) == 0                             # (at least 0.95)
    prefix, _, _ = _write(tmp_path)
    need = [l.split("\t") for l in open(prefix + ".spikeScan.depth.need.txt").read().splitlines()]
    assert need[0] == list(spike.SCAN_NEED_HEADER) and len(need) == 1 + 3 * 2
    n = 1
    for i, v in enumerate(V):
        for t, target in enumerate(TARGETS):
            want = F95[i][t]
            row = need[n]
            assert row[:6] == [v.chrom, "%d" % v.pos, v.ref, v.alt, "%g" % target, "%d" % (200 + i)]
            if want == "NA":
                assert row[6:] == ["NA", "NA", "NA"]
            else:
                d = float(want)
                n95 = float(200 + i) if d == 1.0 else float((200 + i) // (2 << FRACS.index(d)))
                assert row[6:] == [want, "%d" % max(1, int(round(d * 1000))), dsaf.frac_text(n95)]
            n += 1
    # fraction 1 listed: it is the axis's 1, full depth is not added a second time
    full, cells = _entries(FULL, CELLS)
    spike.write_scan_depth(str(tmp_path / "one"), LOCI, V, TARGETS, [1.0, 0.25], 1000, full, cells)
    need = [l.split("\t") for l in open(str(tmp_path / "one") + ".spikeScan.depth.need.txt").read().splitlines()]
    assert need[1][6:8] == ["0.25", "250"] and need[3][6:8] == ["NA", "NA"]     # (variant 1 at 0.1: 0.9 at the listed 1)


def test_the_bedgraphs_and_their_skipped_loci(tmp_path):
    prefix, _, _ = _write(tmp_path)
    sens = [l.split("\t") for l in open(prefix + ".spikeScan.depth.sensitivity.txt").read().splitlines()][1:]
    curve = [l.split("\t") for l in open(prefix + ".spikeScan.depth.curve.txt").read().splitlines()]
    i_rate, i_t95 = spike.SCAN_DEPTH_SENSITIVITY_HEADER.index("RATE"), curve[0].index("T95")
    for t in TARGETS:
        for f in FRACS:
            lines = open("%s.spikeScan%g.dsMT%g.rate.bedgraph" % (prefix, t, f)).read().splitlines()
            mine = [x for x in sens if x[4] == "%g" % t and x[5] == "%g" % f]
            assert lines == ["%s\t%d\t%d\t%s" % (x[0], int(x[1]) - 1, int(x[1]), x[i_rate]) for x in mine] and len(lines) == 3   # (no skipped locus)
    for f in FRACS:
        t95 = {(x[0], int(x[1])): x[i_t95] for x in curve[1:] if x[4] == "%g" % f}
        lines = open("%s.spikeScan.dsMT%g.t95.bedgraph" % (prefix, f)).read().splitlines()
        assert lines == ["%s\t%d\t%d\t%s" % (c, p - 1, p, "1" if t95.get((c, p), "NA") == "NA" else t95[(c, p)]) for c, p, _ in LOCI]
        assert lines[1] == "chrA\t101\t102\t1"                                     # (the skipped locus)
    assert "NA" in [x[i_t95] for x in curve[1:]]
    for t, target in enumerate(TARGETS):
        lines = open("%s.spikeScan%g.f95.bedgraph" % (prefix, target)).read().splitlines()
        want = [F95[0][t], None, F95[1][t], F95[2][t]]
        assert lines == ["%s\t%d\t%d\t%s" % (c, p - 1, p, "2" if w in (None, "NA") else w) for (c, p, _), w in zip(LOCI, want)]
    assert open(prefix + ".spikeScan0.02.f95.bedgraph").read().splitlines()[1:3] == ["chrA\t101\t102\t2", "chrA\t102\t103\t2"]
    names = sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("w."))
    assert len(names) == 3 + 4 + 2 + 2
