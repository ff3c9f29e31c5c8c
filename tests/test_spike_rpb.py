"""--spikeRpb without a GPU: the flag's parsing and refusals, the cells' prefixes and mtDepths, the cell's rule, the pages' headers and
lines, the two ABI entries' declarations, and the restatement's own properties (tests/spike_rpb_restate.py) - at
the full read threshold it is the --spikeDepth restatement word for word, the kept sets are nested in r, threshold 0 keeps first names
only - and the condition on the GPU tests' synthetic input: thinning bites there."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, cli, devplanes, dsaf, spike

sys.path.insert(0, os.path.join(ROOT, "tests"))
import spike_depth_restate as DS  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402
import spike_rpb_restate as RR  # noqa: E402

SEED = RR.SEED
ONE = 1 << 32
TARGETS = (0.05, 0.3, 0.7)


def test_the_entries_are_declared():
    text = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"#define SMC_ABI_VERSION 11\b", text)
    assert re.search(r"\bint smc_spike_read_bits\(smc_ctx\* ctx, const smc_dev_aln\* d_aln,", text)
    assert re.search(r"\bint smc_spike_rpb_counts\(smc_ctx\* ctx, const uint64_t\* d_cov_ident,", text)
    assert "smc_spike_read_bits" in _lib.SYMBOLS and "smc_spike_rpb_counts" in _lib.SYMBOLS
    L = _lib.load()
    assert len(L.smc_spike_read_bits.argtypes) == 15 and len(L.smc_spike_rpb_counts.argtypes) == 19
    hip = open(os.path.join(ROOT, "smcounter_amd", "csrc", "smcounter_hip.hip")).read()
    assert hip.index('#include "k_spike_cells.inc"') < hip.index('#include "k_spike_rpb.inc"') < hip.index('#include "host_abi.inc"')
    kernels = open(os.path.join(ROOT, "smcounter_amd", "csrc", "k_spike_rpb.inc")).read()
    assert "rg_draw(" in kernels and "af_shows(" in kernels and "asm" not in kernels     # (the shared draw and key rule; no inline assembly)
    assert (devplanes.SPB_COVERS, devplanes.SPB_ALT, devplanes.SPB_SINGLE) == (RR.COVERS, RR.ALT, RR.SINGLE)
    assert RR.rp.DOMAIN == devplanes.RPB_DOMAIN and SR.SPIKE_DOMAIN == devplanes.SPIKE_DOMAIN


@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """The GPU tests' synthetic input, its covering records and its read thresholds (computed once, only read)."""
    bam, fa, P, variants = RR.synth_inputs(str(tmp_path_factory.mktemp("rpb")))
    groups = RR.file_groups(bam)
    return variants, RR.records(bam, fa, variants, groups), RR.read_thresholds(groups, RR.RPB_TARGETS)


def _tie(recs, positions, reps=3):
    seeds, thr = PR.seeds(SEED, reps), [PR.threshold(t) for t in TARGETS]
    counters = [RR.barcode_counters(rows) for rows in recs]
    mine = RR.counts_from(recs, positions, thr, [ONE], seeds)
    theirs = DS.counts_from(counters, positions, thr, [ONE], seeds)
    assert mine.shape == theirs.shape == (len(recs), reps, len(thr), 1, 5) and mine.dtype == theirs.dtype == np.uint32
    assert np.array_equal(mine, theirs) and mine[:, :, :, :, 2].any()
    return mine.size


def test_full_read_threshold_is_the_depth_restatement_at_fraction_one(synth, tmp_path):
    variants, recs, _ = synth
    assert _tie(recs, [v.pos for v in variants]) == len(variants) * 3 * 3 * 5
    bam, fa, loci, P, given = SR.make_case(str(tmp_path))          # (records inside deletions, with indels behind the base, soft clips)
    recs = RR.records(bam, fa, given)
    assert any(not r.single for rows in recs for r in rows) and any(r.alt for rows in recs for r in rows)
    assert _tie(recs, [v.pos for v in given]) == len(given) * 3 * 3 * 5
    # the host counters the --spikeReps restatement builds are the sums of the records' bits
    for (names, cnt), rows in zip(PR.host_counters(bam, fa, given), recs):
        mine = RR.barcode_counters(rows)
        assert list(names) == mine[0] and np.array_equal(cnt, mine[1])


def test_kept_sets_are_nested_and_threshold_zero_keeps_first_names(synth):
    variants, recs, rthr = synth
    assert 0 < rthr[0] < rthr[1] < rthr[2] == ONE
    for rows, v in zip(recs, variants):
        full = RR.barcode_counters(rows)[1].astype(np.int64)
        last = None
        for q in [0] + rthr:
            texts, cnt = RR.kept_counters(rows, q, SEED)
            assert (cnt <= full).all() and (last is None or (last <= cnt).all())
            last = cnt
        assert np.array_equal(last, full)
        texts, zero = RR.kept_counters(rows, 0, SEED)
        firsts = np.array([sum(r.first for r in rows if r.barcode == b) for b in texts])
        assert np.array_equal(zero[:, 0], firsts) and 0 < (firsts > 0).sum() < len(texts)


def test_thinning_bites_on_the_gpu_tests_input(synth):
    """A condition on the inputs, checked on the restatement alone: at the smallest reads-per-barcode target a listed variant loses
    covering barcodes, a barcode that is still there changes its majority, and a cell's READS falls below the full-depth one."""
    variants, recs, rthr = synth
    fewer = flipped = 0
    for rows in recs:
        _, full = RR.kept_counters(rows, ONE, SEED)
        _, thin = RR.kept_counters(rows, rthr[0], SEED)
        there = thin[:, 0] > 0
        fewer += int((~there).sum()) > 0
        for col in (1, 2):                                                                # (car0, car1)
            flipped += int((((2 * full[:, col] > full[:, 0]) != (2 * thin[:, col] > thin[:, 0])) & there).sum())
    assert fewer >= 1 and flipped >= 1
    counts = RR.counts_from(recs, [v.pos for v in variants], [PR.threshold(0.7)], [rthr[0], ONE], [SEED])
    assert (counts[:, 0, 0, 0, 0] < counts[:, 0, 0, 1, 0]).any()                          # N' < N
    assert (counts[:, 0, 0, 0, 3] < counts[:, 0, 0, 1, 3]).any()                          # READS' < READS


# ---- the command line
NS = lambda **kw: argparse.Namespace(**kw)
CLI_TARGETS = [(0.01, 100, "o.spikeAF0.01"), (0.05, 25, "o.spikeAF0.05")]


def test_flag_is_parsed_into_cells():
    ns = cli.build_parser().parse_args("--outPrefix o --bamFile b --bedTarget t --mtDepth 3 --rpb 2 --spikeRpb 1.5,3".split())
    assert ns.spikeRpb == "1.5,3"
    rs, cells = spike.rpb_cells(ns, CLI_TARGETS)
    assert rs == [1.5, 3.0]
    # targets outer, reads-per-barcode targets inner; a cell is called at its target's mtDepth
    assert cells == [(0, 0.01, 1.5, 100, "o.spikeAF0.01.dsRpb1.5"), (0, 0.01, 3.0, 100, "o.spikeAF0.01.dsRpb3"),
                     (1, 0.05, 1.5, 25, "o.spikeAF0.05.dsRpb1.5"), (1, 0.05, 3.0, 25, "o.spikeAF0.05.dsRpb3")]
    assert spike.rpb_cells(NS(), CLI_TARGETS) == (None, []) and spike.rpb_cells(NS(spikeRpb=None), []) == (None, [])


@pytest.mark.parametrize("more, tg, msg", (
    (dict(spikeRpb="2"), [], "it needs --spikeAF"), (dict(spikeRpb="a,b"), CLI_TARGETS, "comma-separated reads-per-barcode targets"),
    (dict(spikeRpb="2;3"), CLI_TARGETS, "comma-separated reads-per-barcode targets"), (dict(spikeRpb="0"), CLI_TARGETS, "must be a number > 0"),
    (dict(spikeRpb="2,-1"), CLI_TARGETS, "must be a number > 0"), (dict(spikeRpb=","), CLI_TARGETS, "must be a number > 0"),
    (dict(spikeRpb="nan"), CLI_TARGETS, "must be a number > 0"), (dict(spikeRpb="2,2.0"), CLI_TARGETS, "listed twice"),
    (dict(spikeRpb=",".join("%g" % (1 + 0.1 * k) for k in range(17))), CLI_TARGETS, "2 targets x 17 reads-per-barcode targets = 34 cells, at most 32"),
    (dict(spikeRpb="2", spikeDepth="0.5"), CLI_TARGETS, "--spikeDepth in one run .the combination is not built"),
    (dict(spikeRpb="2", spikePhase=True), CLI_TARGETS, "--spikePhase in one run .the combination is not built"),
    (dict(spikeRpb="2", spikeIndels=True), CLI_TARGETS, "--spikeIndels in one run .the combination is not built"),
    (dict(spikeRpb="2", spikeIndelReps=3), CLI_TARGETS, "--spikeIndelReps in one run .the combination is not built"),
    (dict(spikeRpb="2", spikeIndelDepth="0.5"), CLI_TARGETS, "--spikeIndelDepth in one run .the combination is not built"),
    (dict(spikeRpb="2", spikeIndelPhase=True), CLI_TARGETS, "--spikeIndelPhase in one run .the combination is not built")))
def test_refusals(more, tg, msg):
    with pytest.raises(SystemExit, match=msg):
        spike.rpb_cells(NS(**more), tg)


def test_refused_before_any_file_is_written(tmp_path):
    """The command line itself ends the run before it opens anything (the BAM named here does not exist)."""
    base = dict(outPrefix=str(tmp_path / "o"), bamFile=str(tmp_path / "none.bam"), bedTarget=str(tmp_path / "none.bed"), mtDepth=10, rpb=2.0,
                refGenome=str(tmp_path / "none.fa"))
    sp = dict(spikeAF="0.1", spikeVariants="v")
    for more, msg in ((dict(spikeRpb="2"), "it needs --spikeAF"), (dict(sp, spikeRpb="x"), "comma-separated reads-per-barcode targets"),
                      (dict(sp, spikeRpb="2,0"), "must be a number > 0"), (dict(sp, spikeRpb="2,2"), "listed twice"),
                      (dict(sp, spikeRpb=",".join("%g" % (1 + 0.1 * k) for k in range(33))), "at most 32"),
                      (dict(sp, spikeRpb="2", spikeDepth="0.5"), "--spikeRpb cannot be combined with --spikeDepth"),
                      (dict(sp, spikeRpb="2", spikePhase=""), "--spikeRpb cannot be combined with --spikePhase"),
                      (dict(sp, spikeRpb="2", spikeIndels=""), "--spikeRpb cannot be combined with --spikeIndels"),
                      (dict(sp, spikeRpb="2", spikeIndelReps=3), "--spikeRpb cannot be combined with --spikeIndelReps in one run"),
                      (dict(sp, spikeRpb="2", spikeIndelDepth="0.5"), "--spikeRpb cannot be combined with --spikeIndelDepth in one run"),
                      (dict(sp, spikeRpb="2", spikeIndelPhase=""), "--spikeRpb cannot be combined with --spikeIndelPhase in one run"),
                      (dict(spikeAF="0.1", spikeRpb="2"), "it needs --spikeVariants"),
                      (dict(sp, spikeRpb="2", spikeAF="0.1,0.10"), "listed twice"),
                      # today's refusal of a spike-in beside a down-sampling flag, word for word
                      (dict(sp, dsRpb="2"), r"--spikeAF cannot be combined with --dsRpb in one run \(spike-ins on a down-sampled file are not built\)"),
                      (dict(sp, spikeRpb="2", dsRpb="2"), r"--spikeAF cannot be combined with --dsRpb in one run \(spike-ins on a down-sampled file are not built\)")):
        given = dict(base, **more)
        ns = cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in given.items() if v != ""] + ["--" + k for k, v in given.items() if v == ""])
        with pytest.raises(SystemExit, match=msg):
            cli.main(ns)
    assert os.listdir(str(tmp_path)) == []


def test_the_rule_of_a_cell():
    rule = devplanes.DsRule(1.0, None, seed=7, level="read", target=1.5, prob_keep=0.25, groups=object(), thr=1 << 30, af=0.05, spike=object())
    assert rule.spike_rpb_cell and not rule.spike_cell and rule.flag == "--spikeRpb"
    assert rule.label == "spiked allele fraction 0.05 x target 1.5" and rule.sampler == "philox"
    plain = devplanes.DsRule(1.0, None, level="read", target=1.5)
    assert not plain.spike_rpb_cell and plain.flag == "--dsRpb" and plain.label == "target 1.5"
    depth = devplanes.DsRule(0.5, None, af=0.05, spike=object(), bc_thr=1 << 31)
    assert not depth.spike_rpb_cell and depth.flag == "--spikeDepth"


V = SR.V("chr1", 100, "A", "G", "G")
ROW = ["chr1", "100", "A", "G"] + ["x"] * (len(dsaf.HEADER_ALL) - 4)


def test_the_pages_are_the_depth_pages_with_another_axis(tmp_path):
    assert spike.cell_detection_header(spike.RPB_AXIS) == ("CHROM", "POS", "REF", "ALT", "TARGET", "RPB", "MTDEPTH", "N", "V0", "S", "READS", "V1",
                                                           "AF", "UMT", "VMT", "VMF", "PI", "FILTER", "CALLED")
    assert spike.cell_detection_header() == spike.DEPTH_DETECTION_HEADER and spike.cell_replicates_header() == spike.DEPTH_REPLICATES_HEADER
    assert spike.cell_sensitivity_header() == spike.DEPTH_SENSITIVITY_HEADER
    swap = lambda h: tuple("RPB" if x == "FRACTION" else x for x in h)
    assert spike.cell_replicates_header(spike.RPB_AXIS) == swap(spike.DEPTH_REPLICATES_HEADER)
    assert spike.cell_sensitivity_header(spike.RPB_AXIS) == swap(spike.DEPTH_SENSITIVITY_HEADER)
    assert spike.depth_curve_header([0.05, 0.01], True, spike.RPB_AXIS) == ("CHROM", "POS", "REF", "ALT", "RPB", "MTDEPTH", "N_MEAN", "RATE@0.01",
                                                                            "RATE@0.05", "T95", "LOD")
    assert spike.depth_curve_header([0.05, 0.01], True) == spike.depth_curve_header([0.05, 0.01], True, spike.DEPTH_AXIS)
    # a cell's line: the depth page's line function, the reads-per-barcode target in the axis column
    r = dict(N=100, V0=1, S=7, READS=21, V1=8)
    line = spike.depth_detection_line(V, 0.05, 1.5, 903, r, None, None).split("\t")
    assert line[:7] == ["chr1", "100", "A", "G", "0.05", "1.5", "903"] and line[7:13] == ["100", "1", "7", "21", "8", "0.08"]
    # the detection page on hand-made cells
    prefix = str(tmp_path / "o")
    cells = [(t, target, rr, 100, "%s.spikeAF%g.dsRpb%g" % (prefix, target, rr), None) for t, target in enumerate((0.05, 0.01)) for rr in (1.5, 3.0)]
    for c in cells:
        with open(c[4] + ".smCounter.all.txt", "w") as fh:
            fh.write("\t".join(dsaf.HEADER_ALL) + "\n" + "\t".join(ROW) + "\n")
        with open(c[4] + ".smCounter.cut.txt", "w") as fh:
            fh.write("CHROM\tPOS\tREF\tALT\n")
    counts = [[dict(N=10 + c, V0=0, S=c, READS=2 * c, V1=c) for c in range(4)]]
    spike.write_depth_detection(prefix, [V], cells, counts, None, spike.RPB_AXIS)
    assert sorted(f for f in os.listdir(str(tmp_path)) if ".rpb." in f or ".depth." in f) == ["o.spikeAF.rpb.detection.txt"]
    det = [l.split("\t") for l in open(prefix + ".spikeAF.rpb.detection.txt").read().splitlines()]
    assert det[0] == list(spike.cell_detection_header(spike.RPB_AXIS)) and len(det) == 5
    assert [l[4:7] for l in det[1:]] == [["0.05", "1.5", "100"], ["0.05", "3", "100"], ["0.01", "1.5", "100"], ["0.01", "3", "100"]]
    assert det[2][7:12] == ["11", "0", "1", "2", "1"]


def _row(pi):
    r = list(ROW)
    r[dsaf._COL["PI"]] = pi
    return r


def _entry(s, v1, pi=None, called=False, n=100, v0=1):
    return (dict(N=n, V0=v0, S=s, READS=3 * s, V1=v1), None if pi is None else _row(pi), ("A", ["G"]) if called else None)


def test_replicate_pages_on_hand_made_rows(tmp_path):
    """The three replicate pages with the reads-per-barcode axis: the depth pages' writers and line functions, another infix and column."""
    prefix = str(tmp_path / "o")
    v2 = SR.V("chr1", 200, "C", "T", "T")
    targets, rpbs = [0.05, 0.01], [1.5, 3.0]
    cells = [(t, target, rr, 100, "%s.spikeAF%g.dsRpb%g" % (prefix, target, rr), None) for t, target in enumerate(targets) for rr in rpbs]
    yes, no = _entry(5, 6, "30.0", True), _entry(1, 1, "1.0", n=80)
    entries = {(i, c): [yes if (c + j) % 2 else no for j in range(2)] for i in range(2) for c in range(4)}
    full_entries = {(i, t): [yes, yes] for i in range(2) for t in range(2)}
    spike.write_depth_replicates(prefix, [V, v2], cells, [7, 8], entries, spike.RPB_AXIS)
    reps = [l.split("\t") for l in open(prefix + ".spikeAF.rpb.replicates.txt").read().splitlines()]
    assert reps[0] == list(spike.cell_replicates_header(spike.RPB_AXIS)) and len(reps) == 1 + 2 * 4 * 2
    assert reps[1] == spike.depth_replicate_line(V, 0.05, 1.5, 100, 0, 7, *entries[(0, 0)][0]).split("\t")
    assert [l[5] for l in reps[1:9:2]] == ["1.5", "3", "1.5", "3"] and [l[DS.REP] for l in reps[1:5]] == ["0", "1", "0", "1"]
    spike.write_depth_sensitivity(prefix, [V, v2], cells, entries, None, spike.RPB_AXIS)
    sens = [l.split("\t") for l in open(prefix + ".spikeAF.rpb.sensitivity.txt").read().splitlines()]
    assert sens[0] == list(spike.cell_sensitivity_header(spike.RPB_AXIS))
    assert sens[1:] == DS.sensitivity_from(reps[1:], [V, v2], [(c[1], c[2]) for c in cells], 2, dsaf.frac_text)
    assert sens[1] == spike.depth_sensitivity_line(V, 0.05, 1.5, 100, entries[(0, 0)]).split("\t")
    spike.write_depth_curve(prefix, [V, v2], targets, rpbs, [(200, None), (200, None)], cells, full_entries, entries, None, spike.RPB_AXIS)
    curve = [l.split("\t") for l in open(prefix + ".spikeAF.rpb.curve.txt").read().splitlines()]
    assert curve[0] == list(spike.depth_curve_header(targets, False, spike.RPB_AXIS)) and len(curve) == 1 + 2 * 3
    assert [l[4] for l in curve[1:4]] == ["full", "1.5", "3"] and [l[5] for l in curve[1:4]] == ["200", "100", "100"]
    full_lines = [spike.replicate_line(v, t, j, j, *e).split("\t") for i, v in enumerate([V, v2]) for k, t in enumerate(targets)
                  for j, e in enumerate(full_entries[(i, k)])]
    assert curve[1:] == DS.curve_from(full_lines, [200, 200], reps[1:], [V, v2], targets, rpbs, 2, dsaf.frac_text)
    assert sorted(os.listdir(str(tmp_path))) == ["o.spikeAF.rpb.curve.txt", "o.spikeAF.rpb.replicates.txt", "o.spikeAF.rpb.sensitivity.txt"]
