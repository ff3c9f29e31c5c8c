"""--spikeGrid without a GPU: the switch's parsing and refusals (nothing written), today's refusal of the two axis flags without
it, the cells' order, names and mtDepths, the pages' headers and lines on hand-made rows, the budget page's order and CHEAPEST95,
the restatement's own properties, and the two ABI entries' declarations."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, cli, devplanes, dsaf, spike

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import spike_grid_restate as G  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_rpb_restate as RR  # noqa: E402
import test_gpu_spike_rpb as TR  # noqa: E402  (its made-up records)

V = R.V("chr1", 100, "A", "G", "G")
NS = lambda **kw: argparse.Namespace(**kw)
TARGETS = [(0.01, 100, "o.spikeAF0.01"), (0.05, 25, "o.spikeAF0.05")]
ONE = 1 << 32


def test_the_entries_are_declared():
    text = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"#define SMC_ABI_VERSION 11\b", text)
    assert re.search(r"\bint smc_spike_grid_counts\(smc_ctx\* ctx, const uint64_t\* d_cov_ident,", text)
    assert re.search(r"\bint smc_read_groups_counts_frac_seeds\(smc_read_groups\* g, const uint64_t\* seeds, int32_t n_seeds,", text)
    assert {"smc_spike_grid_counts", "smc_read_groups_counts_frac_seeds"} <= set(_lib.SYMBOLS)
    L = _lib.load()
    assert L.smc_abi_version() == 11
    assert len(L.smc_spike_grid_counts.argtypes) == 22 and len(L.smc_read_groups_counts_frac_seeds.argtypes) == 6
    assert spike.MAX_CELLS == cli.GRID_MAX_CELLS == 32


def test_switch_is_parsed_into_cells():
    ns = cli.build_parser().parse_args("--outPrefix o --bamFile b --bedTarget t --mtDepth 3 --rpb 2 --spikeGrid --spikeDepth 1,0.5 "
                                       "--spikeRpb 1.5,3".split())
    assert ns.spikeGrid is True
    assert cli.build_parser().parse_args("--outPrefix o --bamFile b --bedTarget t --mtDepth 3 --rpb 2".split()).spikeGrid is False
    fracs, rpbs, cells = spike.grid_cells(ns, TARGETS)
    assert fracs == [1.0, 0.5] and rpbs == [1.5, 3.0]
    # targets outer, then fractions, then r; depth_cells' mtDepth of (t, f): 12.5 rounds away from zero
    assert cells == [(0, 0.01, (1.0, 1.5), 100, "o.spikeAF0.01.dsMT1.dsRpb1.5"), (0, 0.01, (1.0, 3.0), 100, "o.spikeAF0.01.dsMT1.dsRpb3"),
                     (0, 0.01, (0.5, 1.5), 50, "o.spikeAF0.01.dsMT0.5.dsRpb1.5"), (0, 0.01, (0.5, 3.0), 50, "o.spikeAF0.01.dsMT0.5.dsRpb3"),
                     (1, 0.05, (1.0, 1.5), 25, "o.spikeAF0.05.dsMT1.dsRpb1.5"), (1, 0.05, (1.0, 3.0), 25, "o.spikeAF0.05.dsMT1.dsRpb3"),
                     (1, 0.05, (0.5, 1.5), 13, "o.spikeAF0.05.dsMT0.5.dsRpb1.5"), (1, 0.05, (0.5, 3.0), 13, "o.spikeAF0.05.dsMT0.5.dsRpb3")]
    assert spike.grid_cells(NS(), TARGETS) == (None, None, []) and spike.grid_cells(NS(spikeGrid=False, spikeDepth="1", spikeRpb="2"), TARGETS)[2] == []


GRID = dict(spikeGrid=True, spikeDepth="1,0.5", spikeRpb="1.5,3")


@pytest.mark.parametrize("more, tg, msg", (
    (dict(), [], "it needs --spikeAF"),
    (dict(spikeDepth=None), TARGETS, r"needs both --spikeDepth and --spikeRpb \(--spikeDepth is missing\)"),
    (dict(spikeRpb=""), TARGETS, r"needs both --spikeDepth and --spikeRpb \(--spikeRpb is missing\)"),
    (dict(spikePhase=True), TARGETS, "cannot be combined with --spikePhase in one run"),
    (dict(spikeIndels=True), TARGETS, "cannot be combined with --spikeIndels "),
    (dict(spikeIndelReps=4), TARGETS, "cannot be combined with --spikeIndelReps"),
    (dict(spikeIndelDepth="0.5"), TARGETS, "cannot be combined with --spikeIndelDepth"),
    (dict(spikeIndelRpb="2"), TARGETS, "cannot be combined with --spikeIndelRpb"),
    (dict(spikeIndelPhase=True), TARGETS, "cannot be combined with --spikeIndelPhase"),
    (dict(spikePhaseRpb="2"), TARGETS, "cannot be combined with --spikePhaseRpb"),
    (dict(spikeScan="0.1"), TARGETS, r"cannot be combined with --spikeScan in one run \(the combination is not built\)"),
    (dict(spikeScanDepth="0.5"), TARGETS, "cannot be combined with --spikeScanDepth"),
    (dict(spikeScanRpb="2"), TARGETS, "cannot be combined with --spikeScanRpb"),
    (dict(spikeDepth="0.5,2"), TARGETS, r"--spikeDepth: every fraction must lie in \(0, 1\]"),
    (dict(spikeDepth="0.5,0.50"), TARGETS, "--spikeDepth: a fraction is listed twice"),
    (dict(spikeRpb="0"), TARGETS, "--spikeRpb: every target must be a number > 0"),
    (dict(spikeRpb="2,2.0"), TARGETS, "--spikeRpb: a target is listed twice"),
    (dict(spikeRpb="x"), TARGETS, "--spikeRpb: comma-separated reads-per-barcode targets"),
    (dict(spikeDepth="1,0.5,0.25", spikeRpb="1.5,2,3,4,5,6"), TARGETS, "2 targets x 3 fractions x 6 reads-per-barcode targets = 36 cells, at most 32"),
    (dict(spikeDepth=",".join("%g" % (0.01 * k) for k in range(1, 18))), TARGETS, "--spikeDepth: 2 targets x 17 fractions = 34 cells, at most 32")))
def test_refusals(more, tg, msg):
    with pytest.raises(SystemExit, match=msg):
        spike.grid_cells(NS(**dict(GRID, **more)), tg)


def test_thirty_two_cells_are_taken():
    _, _, cells = spike.grid_cells(NS(spikeGrid=True, spikeDepth="1,0.5,0.25,0.125", spikeRpb="1.5,2,3,4"), TARGETS)
    assert len(cells) == 32 and len({c[4] for c in cells}) == 32


def test_refused_before_any_file_is_written(tmp_path):
    """The command line itself ends the run before it opens anything (the BAM named here does not exist) - and without the switch the
    two axis flags stay refused with today's message."""
    base = dict(outPrefix=str(tmp_path / "o"), bamFile=str(tmp_path / "none.bam"), bedTarget=str(tmp_path / "none.bed"), mtDepth=10, rpb=2.0,
                refGenome=str(tmp_path / "none.fa"))
    sp = dict(spikeAF="0.1", spikeVariants="v")
    axes = dict(spikeDepth="1,0.5", spikeRpb="1.5,3")
    for more, msg in ((dict(axes, spikeGrid=True), "it needs --spikeAF"), (dict(sp, spikeGrid=True, spikeDepth="0.5"), "--spikeRpb is missing"),
                      (dict(sp, spikeGrid=True, spikeRpb="2"), "--spikeDepth is missing"), (dict(sp, spikeGrid=True), "is missing"),
                      (dict(sp, **axes, spikeGrid=True, spikePhase=True), "cannot be combined with --spikePhase"),
                      (dict(sp, **axes, spikeGrid=True, spikeIndels=True), "cannot be combined with --spikeIndels"),
                      (dict(sp, **axes, spikeGrid=True, spikeReps=1), "must lie in 2 .. 1000"),
                      (dict(sp, spikeGrid=True, spikeDepth="1,0.5,0.25", spikeRpb="1,2,3,4,5,6,7,8,9,10,11"), "= 33 cells, at most 32"),
                      (dict(sp, **axes, spikeGrid=True, dsMT="0.5"), "cannot be combined with --dsMT"),
                      (dict(spikeAF="0.1", spikeGrid=True, **axes), "it needs --spikeVariants"),
                      (dict(sp, **axes), r"--spikeRpb cannot be combined with --spikeDepth in one run \(the combination is not built\)")):
        argv = [x for k, v in dict(base, **more).items() for x in (["--" + k] if v is True else ["--%s=%s" % (k, v)])]
        with pytest.raises(SystemExit, match=msg):
            cli.main(cli.build_parser().parse_args(argv))
    assert os.listdir(str(tmp_path)) == []


def test_rule_labels_and_flags():
    P = object()
    groups, spikes = object(), argparse.Namespace(rpb_flag="--spikeGrid", indels=False)
    rule = devplanes.DsRule(0.5, P, kept=None, seed=7, level="read", target=3.0, prob_keep=0.25, n_names=10, groups=groups, thr=1 << 30,
                            grid=True, bc_thr=1 << 31, af=0.05, spike=spikes)
    assert rule.spike_rpb_cell and rule.flag == "--spikeGrid" and rule.sampler == "philox"
    assert rule.label == "spiked allele fraction 0.05 x fraction 0.5 x target 3"
    plain = devplanes.DsRule(1.0, P, kept=None, seed=7, level="read", target=3.0, groups=groups, thr=5, af=0.05,
                             spike=argparse.Namespace(rpb_flag=None, indels=False))
    assert plain.flag == "--spikeRpb" and plain.label == "spiked allele fraction 0.05 x target 3"       # (unchanged without the switch)


def _row(pi, alt="G"):
    f = [""] * 40
    f[0:4] = ["chr1", "100", "A", alt]
    return f


def _per(called, n, n_cov=50):
    """Replicates as the pages take them: `called` of `n` carry a cut that calls V."""
    return [(dict(N=n_cov + j, V0=1, S=3 + j, READS=9, V1=4), None, ("A", {"G"}) if j < called else None) for j in range(n)]


def test_page_headers_and_lines():
    assert spike.GRID_AXIS == ("grid", ("FRACTION", "RPB"))
    det = spike.cell_detection_header(spike.GRID_AXIS)
    assert det == ("CHROM", "POS", "REF", "ALT", "TARGET", "FRACTION", "RPB", "MTDEPTH", "N", "V0", "S", "READS", "V1", "AF", "UMT", "VMT", "VMF",
                   "PI", "FILTER", "CALLED")
    rep = spike.cell_replicates_header(spike.GRID_AXIS)
    assert rep[:10] == det[:8] + ("REP", "SEED") and rep[10:] == det[8:]
    sens = spike.cell_sensitivity_header(spike.GRID_AXIS)
    assert sens[:8] == det[:8] and sens[8:11] == ("REPS", "CALLED", "RATE") and sens[-1] == "N_MEAN"
    # the one-column axes are what they were
    assert spike.cell_detection_header() == spike.DETECTION_HEADER[:5] + ("FRACTION", "MTDEPTH") + spike.DETECTION_HEADER[5:]
    assert spike.cell_replicates_header(spike.RPB_AXIS)[5:9] == ("RPB", "MTDEPTH", "REP", "SEED")
    r = dict(N=40, V0=1, S=5, READS=11, V1=6)
    one = spike.depth_detection_line(V, 0.05, 0.5, 13, r, None, None).split("\t")
    two = spike.depth_detection_line(V, 0.05, (0.5, 3.0), 13, r, None, None).split("\t")
    assert len(two) == len(det) and two[:8] == ["chr1", "100", "A", "G", "0.05", "0.5", "3", "13"] and two[8:13] == ["40", "1", "5", "11", "6"]
    assert two[:6] == one[:6] and two[7:] == one[6:]
    rl = spike.depth_replicate_line(V, 0.05, (0.5, 3.0), 13, 2, 99, r, None, None).split("\t")
    assert len(rl) == len(rep) and rl[8:10] == ["2", "99"] and rl[:8] == two[:8] and rl[10:] == two[8:]
    assert spike.depth_replicate_line(V, 0.05, 0.5, 13, 2, 99, r, None, None).split("\t")[5:9] == ["0.5", "13", "2", "99"]
    sl = spike.depth_sensitivity_line(V, 0.05, (1.0, 1.5), 25, _per(3, 4)).split("\t")
    assert len(sl) == len(sens) and sl[:11] == ["chr1", "100", "A", "G", "0.05", "1", "1.5", "25", "4", "3", dsaf.frac_text(0.75)]
    assert sl[-1] == dsaf.frac_text((50 + 51 + 52 + 53) / 4.0)


def test_budget_order_and_cheapest95(tmp_path):
    assert spike.BUDGET_HEADER == ("CHROM", "POS", "REF", "ALT", "TARGET", "FRACTION", "RPB", "MTDEPTH", "KEPT_NAMES", "COST", "N_MEAN", "REPS",
                                   "CALLED", "RATE", "LO95", "HI95", "CHEAPEST95")
    cells = [((1.0, 3.0), 100, 800), ((1.0, 1.5), 100, 400), ((0.5, 3.0), 50, 400), ((0.5, 1.5), 50, 200)]
    per = [_per(20, 20), _per(19, 20), _per(20, 20), _per(10, 20)]
    lines = [l.split("\t") for l in spike.budget_lines(V, 0.05, cells, 1000, per)]
    # by cost ascending; the tie at 0.4 keeps the listed order; the first line at 0.95 or more is marked, and only that one
    assert [(l[5], l[6]) for l in lines] == [("0.5", "1.5"), ("1", "1.5"), ("0.5", "3"), ("1", "3")]
    assert [l[8] for l in lines] == ["200", "400", "400", "800"] and [l[9] for l in lines] == [dsaf.frac_text(x) for x in (0.2, 0.4, 0.4, 0.8)]
    assert [l[13] for l in lines] == [dsaf.frac_text(x) for x in (0.5, 0.95, 1.0, 1.0)] and [l[16] for l in lines] == ["0", "1", "0", "0"]
    assert [l[7] for l in lines] == ["50", "100", "50", "100"] and [l[11] for l in lines] == ["20"] * 4 and [l[12] for l in lines] == ["10", "19", "20", "20"]
    lo, hi = dsaf.wilson(19, 20)
    assert lines[1][14:16] == [dsaf.frac_text(lo), dsaf.frac_text(hi)] and lines[0][10] == dsaf.frac_text(sum(50 + j for j in range(20)) / 20.0)
    assert G.cost_order([0.8, 0.4, 0.4, 0.2]) == spike.budget_order([0.8, 0.4, 0.4, 0.2]) == [3, 1, 2, 0]
    assert G.cheapest95([0.5, 0.95, 1.0, 1.0]) == [0, 1, 0, 0]
    # no cell reaches 0.95: no line is marked
    none = [l.split("\t") for l in spike.budget_lines(V, 0.05, cells, 1000, [_per(18, 20)] * 4)]
    assert [l[16] for l in none] == ["0"] * 4 and G.cheapest95([0.9] * 4) == [0] * 4
    # the page: per variant and target its own block, each sorted and marked on its own
    W = R.V("chr1", 200, "A", "G", "G")
    page = [(k, t, fr, d, "p", None, kept) for k, t in ((0, 0.01), (1, 0.05)) for fr, d, kept in cells]
    entries = {(i, c): per[c % 4] if (i, c // 4) != (1, 1) else _per(0, 20) for i in range(2) for c in range(8)}
    spike.write_budget(str(tmp_path / "o"), [V, W], page, 1000, entries)
    text = open(str(tmp_path / "o.spikeAF.grid.budget.txt")).read().split("\n")
    assert text[0].split("\t") == list(spike.BUDGET_HEADER) and text[-1] == "" and len(text) == 2 + 16
    body = [l.split("\t") for l in text[1:-1]]
    assert [(l[1], l[4]) for l in body] == [("100", "0.01")] * 4 + [("100", "0.05")] * 4 + [("200", "0.01")] * 4 + [("200", "0.05")] * 4
    assert [l[16] for l in body] == ["0", "1", "0", "0"] * 3 + ["0"] * 4
    assert all([l[9] for l in body[b:b + 4]] == [dsaf.frac_text(x) for x in (0.2, 0.4, 0.4, 0.8)] for b in (0, 4, 8, 12))


def test_restatement_reduces_to_the_one_axis_restatements():
    """With one fraction of 1 and equal thresholds the restated counts are spike_rpb_restate's; a barcode threshold of 0 keeps nobody;
    the per-seed thresholds are probKeep over the barcodes kept under that seed."""
    recs = TR._made([40, 0, 9], seed=2)
    pos, seeds = [5, 6, 7], PR.seeds(11, 3)
    thr, rthr = [PR.threshold(t) for t in (0.2, 0.7)], [0, PR.threshold(0.4), ONE]
    rd = np.tile(np.array(rthr, np.uint64), (3, 2, 1))
    got = G.counts_from(recs, pos, thr, [ONE, 0], rd, seeds)
    assert got.shape == (3, 3, 2, 2, 3, 5) and np.array_equal(got[:, :, :, 0], RR.counts_from(recs, pos, thr, rthr, seeds))
    assert not got[:, :, :, 1].any()
    half = G.counts_from(recs, pos, thr, [ONE, ONE // 2], rd, seeds)
    assert (half[:, :, :, 1, :, 0] <= half[:, :, :, 0, :, 0]).all() and half[0, :, :, 1, :, 0].sum() < half[0, :, :, 0, :, 0].sum()
    names = ["q:B%dACGT:%d" % (b, i) for b in range(60) for i in range(1 + b % 4)]
    groups = G.rp.group(names)
    fracs, rpbs = (1.0, 0.5), (1.5, 3.0)
    assert G.keeps_a_multi_name_barcode(groups, fracs, seeds)
    t, p = G.read_thresholds(groups, fracs, rpbs, seeds)
    c = groups["counts"]
    full = [G.rp.prob_keep(c, r) for r in rpbs]
    assert (p[:, 0] == np.array(full)).all() and len({p[j, 1].tobytes() for j in range(3)}) > 1          # (f = 1: the file's; f < 1: the seed's own)
    assert [int(x) for x in t[0, 0]] == [G.rp.threshold(x) for x in full]
    k = G.seed_counters(groups, fracs, seeds)
    assert (k[:, 0] == [c["barcodes"], c["one"], c["multi"], c["multi_names"]]).all() and (k[:, 1, 0] < c["barcodes"]).all()
    assert devplanes.grid_prob_keep(dict(one=3, multi=2, multi_names=7), 2.0) == 1.0 * (2.0 - 1.0) * 5 / 5
    assert devplanes.grid_prob_keep((3, 2, 2), 2.0) is None


class _FakeGroups(object):
    """counts_frac_seeds from a table of (barcodes, one, multi, multi_names) per (seed, fraction threshold)."""

    def __init__(self, table):
        self.table, self.calls = table, 0

    def counts_frac_seeds(self, seeds, bc_thr):
        self.calls += 1
        return np.array([[self.table[(int(s), int(t))] for t in bc_thr] for s in seeds], np.uint64)


def test_thresholds_of_every_replicate_and_the_refusal_that_names_replicate_seed_and_fraction():
    half = devplanes.frac_threshold(0.5)
    seeds = PR.seeds(PR.M64 - 1, 4)                                                           # (the seeds wrap: 2^64 - 2, 2^64 - 1, 0, 1)
    table = {(s, ONE): (10, 4, 6, 20) for s in seeds}
    table.update({(seeds[0], half): (5, 2, 3, 9), (seeds[1], half): (6, 3, 3, 8), (seeds[2], half): (4, 1, 3, 12), (seeds[3], half): (5, 3, 2, 5)})
    groups = _FakeGroups(table)
    thr, prob = devplanes.grid_read_thresholds(groups, seeds, (1.0, 0.5), (1.5, 3.0))
    assert groups.calls == 1 and thr.shape == prob.shape == (4, 2, 2) and thr.dtype == np.uint64           # (ONE launch for all R x F)
    for j, s in enumerate(seeds):
        for k, t in enumerate((ONE, half)):
            _, one, multi, names = table[(s, t)]
            for q, r in enumerate((1.5, 3.0)):
                p = 1.0 * (r - 1.0) * (one + multi) / (names - multi)
                assert prob[j, k, q] == p and int(thr[j, k, q]) == devplanes.read_threshold(p)
    assert (thr[:, 0] == thr[0, 0]).all() and len({thr[j, 1].tobytes() for j in range(4)}) == 4
    # replicate 2 keeps at 0.5 only barcodes of one name (multi_names == multi, here 0 == 0): the refusal names it, its seed and f
    table[(seeds[2], half)] = (3, 3, 0, 0)
    with pytest.raises(ValueError, match=r"^--spikeGrid: replicate 2 \(seed 0\), fraction 0\.5: no barcode kept there has more than one read name, "
                                         r"so ds\.reads\.withinMT\.py's probKeep \(:58\) is not defined \(it divides by zero\)$"):
        devplanes.grid_read_thresholds(_FakeGroups(table), seeds, (1.0, 0.5), (1.5, 3.0))
    # ... and the first one in replicate order when several fail; one replicate alone is the run's own seed
    table[(seeds[1], half)] = (2, 2, 0, 0)
    with pytest.raises(ValueError, match=r"replicate 1 \(seed %d\), fraction 0\.5" % (PR.M64)):
        devplanes.grid_read_thresholds(_FakeGroups(table), seeds, (1.0, 0.5), (1.5, 3.0))
    with pytest.raises(ValueError, match=r"^--spikeGrid: replicate 0 \(seed 0\), fraction 0\.5"):
        devplanes.grid_read_thresholds(_FakeGroups(table), seeds[2:3], (1.0, 0.5), (3.0,))
    assert devplanes.grid_read_thresholds(_FakeGroups(table), seeds[:1], (1.0, 0.5), (3.0,))[0].shape == (1, 2, 1)
