"""--spikeReps without a GPU: the flag's parsing and refusals, the two ABI entries' declarations, the three files' lines on hand-made
entries, Wilson against hand values, and the claim the counts call rests on - V1 follows from (reads, alt0, single) alone."""
import argparse
import os
import re
import sys

import pytest

from conftest import ROOT
from smcounter_amd import _lib, cli, dsaf, spike

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402

V = R.V("chr1", 100, "A", "G", "G")
NS = lambda **kw: argparse.Namespace(**kw)
TARGETS = [(0.01, 100, "o.spikeAF0.01")]


def test_flag_is_parsed():
    ns = cli.build_parser().parse_args("--outPrefix o --bamFile b --bedTarget t --mtDepth 3 --rpb 2 --spikeReps 16".split())
    assert ns.spikeReps == 16 and spike.reps(ns, TARGETS) == 16
    assert spike.reps(NS(), TARGETS) is None and spike.reps(NS(spikeReps=None), []) is None
    assert spike.reps(NS(spikeReps="5"), TARGETS) == 5 and spike.reps(NS(spikeReps=2), TARGETS) == 2 and spike.reps(NS(spikeReps=1000), TARGETS) == 1000


@pytest.mark.parametrize("value, tg, msg", ((4, [], "it needs --spikeAF"), (1, TARGETS, r"must lie in 2 \.\. 1000, got 1"),
                                            (1001, TARGETS, r"must lie in 2 \.\. 1000, got 1001"), (-3, TARGETS, "must lie in"),
                                            ("x", TARGETS, r"an integer in 2 \.\. 1000 expected, got 'x'"),
                                            (2.5, TARGETS, r"an integer in 2 \.\. 1000 expected"), ("2.5", TARGETS, "an integer in")))
def test_refusals(value, tg, msg):
    with pytest.raises(SystemExit, match=msg):
        spike.reps(NS(spikeReps=value), tg)


def test_refused_before_any_file_is_written(tmp_path):
    """The command line itself: --spikeReps without --spikeAF, and what --spikeAF refuses, end the run before it opens anything (the
    BAM named here does not exist)."""
    base = dict(outPrefix=str(tmp_path / "o"), bamFile=str(tmp_path / "none.bam"), bedTarget=str(tmp_path / "none.bed"), mtDepth=10, rpb=2.0,
                refGenome=str(tmp_path / "none.fa"))
    for more, msg in ((dict(spikeReps=4), "it needs --spikeAF"), (dict(spikeReps=1, spikeAF="0.1", spikeVariants="v"), "must lie in"),
                      (dict(spikeReps=4, spikeAF="0.1"), "it needs --spikeVariants"),
                      (dict(spikeReps=4, spikeAF="0.1", spikeVariants="v", dsMT="0.5"), "cannot be combined")):
        with pytest.raises(SystemExit, match=msg):
            cli.main(dict(base, **more))
    assert os.listdir(str(tmp_path)) == []
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args("--outPrefix o --bamFile b --bedTarget t --mtDepth 3 --rpb 2 --spikeReps 2.5".split())


def test_the_two_entries_are_declared():
    text = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"#define SMC_ABI_VERSION 11\b", text)
    assert re.search(r"\bint smc_spike_alleles_reps\(smc_ctx\* ctx,", text) and re.search(r"\bint smc_spike_rep_counts\(smc_ctx\* ctx,", text)
    assert "#define SMC_SPIKE_MAX_COPIES" in text
    assert "smc_spike_alleles_reps" in _lib.SYMBOLS and "smc_spike_rep_counts" in _lib.SYMBOLS


ROW = ["chr1", "100", "A", "G"] + ["x"] * (len(dsaf.HEADER_ALL) - 4)


def _row(pi):
    r = list(ROW)
    r[dsaf._COL["PI"]] = pi
    return r


def _entry(s, v1, pi=None, called=False, n=200, v0=1):
    return (dict(N=n, V0=v0, S=s, READS=3 * s, V1=v1), None if pi is None else _row(pi), ("A", ["G"]) if called else None)


def test_replicate_line_is_the_detection_line_with_two_fields():
    r, row, cut = _entry(7, 8, "12.5", True)
    det = spike.detection_line(V, 0.05, r, row, cut).split("\t")
    rep = spike.replicate_line(V, 0.05, 3, (1 << 64) - 1, r, row, cut).split("\t")
    assert rep[:5] + rep[7:] == det and rep[5:7] == ["3", "18446744073709551615"]
    assert tuple(spike.REPLICATES_HEADER) == spike.DETECTION_HEADER[:5] + ("REP", "SEED") + spike.DETECTION_HEADER[5:]
    assert len(rep) == len(spike.REPLICATES_HEADER) and rep[PR.S] == "7" and rep[PR.V1] == "8" and rep[PR.CALLED] == "1" and rep[PR.N] == "200"
    none = spike.replicate_line(V, 0.05, 0, 1, r, None, None).split("\t")
    assert none[PR.PI] == "" and none[PR.CALLED] == "0"


def test_sensitivity_lines():
    assert spike.SENSITIVITY_HEADER == ("CHROM", "POS", "REF", "ALT", "TARGET", "REPS", "CALLED", "RATE", "LO95", "HI95", "AF_MEAN", "AF_MIN",
                                        "AF_MAX", "S_MIN", "S_MAX", "V_MIN", "V_MAX", "PI_MEAN", "PI_MIN")
    every = [_entry(4, 5, "20.0", True), _entry(6, 7, "30.0", True), _entry(5, 5, "25.0", True), _entry(9, 10, "45.0", True)]
    f = spike.sensitivity_line(V, 0.02, every).split("\t")
    lo, _ = PR.wilson(4, 4)
    assert f == ["chr1", "100", "A", "G", "0.02", "4", "4", "1.0", dsaf.frac_text(lo), "1.0", dsaf.frac_text(27 / 800.0), "0.025", "0.05",
                 "4", "9", "5", "10", "30.0", "20.0"]
    nobody = [_entry(0, 1, "0.5"), _entry(1, 1, "1.5")]
    f = spike.sensitivity_line(V, 0.02, nobody, lod=0.0123).split("\t")
    assert f[5:10] == ["2", "0", "0.0", "0.0", dsaf.frac_text(PR.wilson(0, 2)[1])] and f[13:17] == ["0", "1", "1", "1"] and f[19] == "0.0123"
    # a replicate without a row counts PI as 0
    f = spike.sensitivity_line(V, 0.02, [_entry(3, 4, "10.0", True), _entry(2, 2)]).split("\t")
    assert f[6] == "1" and f[17:19] == ["5.0", "0.0"]
    # the helper computes the same from replicate lines
    for per in (every, nobody):
        lines = [spike.replicate_line(V, 0.02, j, j, *e).split("\t") for j, e in enumerate(per)]
        assert PR.sensitivity_from(lines, [V], [0.02], len(per), dsaf.frac_text) == [spike.sensitivity_line(V, 0.02, per).split("\t")]


def test_curve_lines_and_the_monotone_rule():
    yes, no = _entry(5, 6, "30.0", True), _entry(1, 1, "1.0")
    targets = [0.05, 0.01, 0.02]                    # (the order given; the columns ascend)
    assert spike.curve_header(targets) == ("CHROM", "POS", "REF", "ALT", "N", "RATE@0.01", "RATE@0.02", "RATE@0.05", "T95")
    assert spike.curve_header(targets, True)[-1] == "LOD"
    f = spike.curve_line(V, 200, targets, [[yes] * 4, [no] * 4, [yes] * 4]).split("\t")
    assert f == ["chr1", "100", "A", "G", "200", "0.0", "1.0", "1.0", "0.02"]
    # a dip above disqualifies what lies below it: 0.01 found, 0.02 missed, 0.05 found -> T95 0.05
    f = spike.curve_line(V, 200, targets, [[yes] * 4, [yes] * 4, [no] * 4], lod=0.031).split("\t")
    assert f[5:] == ["1.0", "0.0", "1.0", "0.05", "0.031"]
    f = spike.curve_line(V, 200, targets, [[yes, no, no, no], [yes] * 4, [yes] * 4]).split("\t")
    assert f[5:] == ["1.0", "1.0", "0.25", "NA"]
    per = [[yes] * 4, [yes] * 4, [no] * 4]
    lines = [spike.replicate_line(V, t, j, j, *e).split("\t") for t, p in zip(targets, per) for j, e in enumerate(p)]
    assert PR.curve_from(lines, [V], targets, 4, dsaf.frac_text) == [spike.curve_line(V, 200, targets, per).split("\t")]


def test_wilson_against_hand_values():
    # (p + z^2 / 2n -+ z sqrt(p (1 - p) / n + z^2 / 4 n^2)) / (1 + z^2 / n), z = 1.959964: worked by hand (at 0 of n the upper end is z^2 / (n + z^2) = 3.841459 / 19.841459)
    for (k, n), (lo, hi) in (((8, 16), (0.279996, 0.720004)), ((0, 16), (0.0, 0.193608)), ((16, 16), (0.806392, 1.0)), ((1, 4), (0.045587, 0.699358))):
        got = dsaf.wilson(k, n)
        assert abs(got[0] - lo) < 1e-6 and abs(got[1] - hi) < 1e-6, (k, n, got)
        mine = PR.wilson(k, n)
        assert abs(mine[0] - got[0]) < 1e-12 and abs(mine[1] - got[1]) < 1e-12


def test_v1_needs_no_spiked_copy(tmp_path):
    """(S, READS, V1) restated from (reads, alt0, single) and the draws alone equal spike_restate.restate - which walks every read of
    the pileup and rewrites its key - on the hand-made BAM, for several seeds and targets, 0 and 1 among them."""
    bam, fa, loci, P, variants = SR.make_case(str(tmp_path))
    targets, n_reps = (0.0, 0.3, 0.6, 1.0), 4
    want = PR.restate(bam, fa, variants, targets, 20240607, n_reps, P.mismatchThr)
    counters = PR.host_counters(bam, fa, variants)
    compared = moved = 0
    for j, s in enumerate(PR.seeds(20240607, n_reps)):
        for t, target in enumerate(targets):
            for i, v in enumerate(variants):
                names, cnt = counters[i]
                st = want[j][t][1][i]
                got = PR.counts_rule(cnt, SR.draw(names, s, v.pos), PR.threshold(target))
                assert got == (st["S"], st["READS"], st["V1"]), (s, target, v.pos)
                assert st["N"] == len(names)
                moved += st["V1"] != st["V0"]
                compared += 1
                if target == 0.0:
                    assert got == (0, 0, st["V0"])
                if target == 1.0:
                    assert got == (len(names), int(cnt[:, 2].sum()), int((2 * cnt[:, 2].astype(int) > cnt[:, 0]).sum()))
    assert compared == n_reps * len(targets) * len(variants) and moved > 0
    # not every read of a covering barcode is one the rewrite can touch, here
    assert any(bool((c[:, 2] < c[:, 0]).any()) for _, c in counters)
