"""--spikeDepth without a GPU: the flag's parsing and refusals, the cells' prefixes and mtDepths, the restatement's own properties
(nested sets, f = 1, the depth draw, deviation bounds on the synthetic BAM), the four pages' lines on hand-made rows, and the ABI
entry's declaration."""
import argparse
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, cli, devplanes, dsaf, spike

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import spike_depth_restate as DS  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402

SEED = 20240607
V = R.V("chr1", 100, "A", "G", "G")
NS = lambda **kw: argparse.Namespace(**kw)
TARGETS = [(0.01, 100, "o.spikeAF0.01"), (0.05, 25, "o.spikeAF0.05")]


def test_flag_is_parsed_into_cells():
    ns = cli.build_parser().parse_args("--outPrefix o --bamFile b --bedTarget t --mtDepth 3 --rpb 2 --spikeDepth 0.5,0.1".split())
    assert ns.spikeDepth == "0.5,0.1"
    fr, cells = spike.depth_cells(ns, TARGETS)
    assert fr == [0.5, 0.1]
    # targets outer, fractions inner; max(1, py2_round(f x mtDepth of the target)): 12.5 rounds AWAY from zero as Python 2 does, 2.5 too
    assert cells == [(0, 0.01, 0.5, 50, "o.spikeAF0.01.dsMT0.5"), (0, 0.01, 0.1, 10, "o.spikeAF0.01.dsMT0.1"),
                     (1, 0.05, 0.5, 13, "o.spikeAF0.05.dsMT0.5"), (1, 0.05, 0.1, 3, "o.spikeAF0.05.dsMT0.1")]
    assert spike.depth_cells(NS(), TARGETS) == (None, []) and spike.depth_cells(NS(spikeDepth=None), []) == (None, [])
    assert spike.depth_cells(NS(spikeDepth="1"), TARGETS[:1])[1] == [(0, 0.01, 1.0, 100, "o.spikeAF0.01.dsMT1")]
    assert spike.depth_cells(NS(spikeDepth="0.001"), TARGETS[1:])[1][0][3] == 1                    # (never below 1)
    assert spike.depth_cells(NS(spikeDepth="0.5"), [(0.2, 5, "p")])[1][0][3] == 3                   # (2.5 -> 3, not the even 2)


@pytest.mark.parametrize("value, tg, msg", (("0.5", [], "it needs --spikeAF"), ("a,b", TARGETS, "comma-separated fractions"),
                                            ("0.5;0.1", TARGETS, "comma-separated fractions"), ("0", TARGETS, r"must lie in \(0, 1\]"),
                                            ("0.5,1.5", TARGETS, r"must lie in \(0, 1\]"), ("-0.1", TARGETS, "must lie in"),
                                            (",", TARGETS, "must lie in"), ("nan", TARGETS, "must lie in"),
                                            ("0.5,0.50", TARGETS, "listed twice"),
                                            (",".join("%g" % (0.01 * k) for k in range(1, 18)), TARGETS, "2 targets x 17 fractions = 34 cells, at most 32")))
def test_refusals(value, tg, msg):
    with pytest.raises(SystemExit, match=msg):
        spike.depth_cells(NS(spikeDepth=value), tg)


def test_refused_before_any_file_is_written(tmp_path):
    """The command line itself ends the run before it opens anything (the BAM named here does not exist)."""
    base = dict(outPrefix=str(tmp_path / "o"), bamFile=str(tmp_path / "none.bam"), bedTarget=str(tmp_path / "none.bed"), mtDepth=10, rpb=2.0,
                refGenome=str(tmp_path / "none.fa"))
    sp = dict(spikeAF="0.1", spikeVariants="v")
    for more, msg in ((dict(spikeDepth="0.5"), "it needs --spikeAF"), (dict(sp, spikeDepth="x"), "comma-separated fractions"),
                      (dict(sp, spikeDepth="0.5,2"), "must lie in"), (dict(sp, spikeDepth="0.5,0.5"), "listed twice"),
                      (dict(sp, spikeDepth=",".join("%g" % (0.01 * k) for k in range(1, 34))), "at most 32"),
                      (dict(spikeAF="0.1", spikeDepth="0.5"), "it needs --spikeVariants"),
                      (dict(sp, spikeDepth="0.5", dsMT="0.5"), "cannot be combined with --dsMT"),
                      (dict(sp, spikeDepth="0.5", spikeAF="0.1,0.10"), "listed twice")):
        with pytest.raises(SystemExit, match=msg):
            cli.main(dict(base, **more))
    assert os.listdir(str(tmp_path)) == []


def test_the_entry_is_declared():
    text = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"#define SMC_ABI_VERSION 11\b", text)
    assert re.search(r"\bint smc_spike_depth_counts\(smc_ctx\* ctx, const uint64_t\* d_cov_ident,", text)
    assert "smc_spike_depth_counts" in _lib.SYMBOLS
    assert "L.smc_abi_version() != 11" in open(os.path.join(ROOT, "smcounter_amd", "_lib.py")).read()
    assert spike.MAX_CELLS == cli.GRID_MAX_CELLS == 32


def _synth(tmp_path):
    bam, fa, loci, P, _ = R.synth_bam(str(tmp_path))
    return bam, fa, P, SR.pick_positions(bam, fa, loci[20:44], 4)


def test_sets_are_nested_and_f1_is_the_spike_in(tmp_path):
    bam, fa, P, variants = _synth(tmp_path)
    targets, fracs, reps = (0.02, 0.1, 0.4), (0.1, 0.25, 0.5, 1.0), 3
    counts, counters = DS.restate_counts(bam, fa, variants, targets, fracs, SEED, reps)
    assert counts.shape == (len(variants), reps, 3, 4, 5)
    compared = 0
    for i, ((names, cnt), v) in enumerate(zip(counters, variants)):
        c64 = cnt.astype(np.int64)
        for j, s in enumerate(PR.seeds(SEED, reps)):
            keep = [DS.depth_keep(names, f, s) for f in fracs]
            u = SR.draw(names, s, v.pos)
            hit = [u < np.uint64(PR.threshold(t)) for t in targets]
            for f in range(1, 4):
                assert not (keep[f - 1] & ~keep[f]).any()                               # the kept sets are nested in f
            assert keep[3].all()
            for t in range(3):
                for f in range(4):
                    n2, v02, s2, reads2, v12 = (int(x) for x in counts[i, j, t, f])
                    assert n2 == int(keep[f].sum()) and s2 == int((keep[f] & hit[t]).sum())
                    if t:
                        assert not (hit[t - 1] & ~hit[t]).any() and s2 >= int(counts[i, j, t - 1, f, 2])    # S' nested in t
                    if f:
                        assert s2 >= int(counts[i, j, t, f - 1, 2]) and n2 >= int(counts[i, j, t, f - 1, 0])    # ... and in f
                    assert v02 <= n2 and s2 <= n2 and v12 <= n2
                    compared += 1
                # f = 1: spike_reps_restate.counts_rule's numbers, the cover's size and the carriers
                assert [int(x) for x in counts[i, j, t, 3, 2:]] == list(PR.counts_rule(cnt, u, PR.threshold(targets[t])))
                assert int(counts[i, j, t, 3, 0]) == len(names) and int(counts[i, j, t, 3, 1]) == int((2 * c64[:, 1] > c64[:, 0]).sum())
    assert compared == len(variants) * reps * 12
    assert len({counts[:, j].tobytes() for j in range(reps)}) == reps                  # (the replicates draw differently)


def test_cells_records_are_the_spike_ins_records_of_the_kept_barcodes(tmp_path):
    """The restatement's second way: spike_restate.restate's records filtered by the kept barcodes give the cell's S' that the counts
    rule gives, on the hand-made BAM whose read names carry the barcode."""
    bam, fa, loci, P, variants = SR.make_case(str(tmp_path))
    barcode_of = lambda key: key[0].split(":")[2]
    t, fracs = 0.5, (0.3, 0.7, 1.0)
    counts, counters = DS.restate_counts(bam, fa, variants, (t,), fracs, SEED, 1)
    assert all(set(names) <= {"%s%02d" % (s, b) for s in ("FIRST", "LAST", "INDEL", "INSB", "DELB", "CLIP", "ALT", "THIRD", "NONM", "FLIP", "FAR")
                              for b in range(SR.N_BC)} for names, _ in counters)
    sizes = []
    for f, frac in enumerate(fracs):
        recs, s2 = DS.cell_records(bam, fa, variants, t, frac, SEED, P.mismatchThr, barcode_of)
        assert s2 == [int(counts[i, 0, 0, f, 2]) for i in range(len(variants))]
        sizes.append(len(recs))
    full, _ = SR.restate(bam, fa, variants, t, SEED, P.mismatchThr)
    assert sizes[0] < sizes[1] < sizes[2] == len(full)


def test_restated_depth_draw_is_the_dsmt_philox_rule():
    L = _lib.load()
    texts = ["ACGTACGTAC%d" % k for k in range(300)]
    ids = PR.idents(texts)
    assert np.array_equal(ids, devplanes.fnv64_array(texts))
    for seed in (7, (1 << 32) + 5, PR.M64):
        for f in (0.001, 0.3, 0.5, 1.0):
            assert np.array_equal(DS.depth_keep(texts, f, seed), devplanes.philox_keep_host(L, ids, f, seed))
    for f in (1e-9, 0.1, 0.25, 1.0 / 3, 0.999999, 1.0):
        assert DS.frac_thr(f) == devplanes.frac_threshold(f)
    assert SR.SPIKE_DOMAIN == devplanes.SPIKE_DOMAIN != devplanes.DS_DOMAIN


# (the bounds are conditions of the draws, four standard deviations of a binomial: N' ~ Bin(N, f), S' ~ Bin(N, f t) - the two streams
# are independent.  Seed, targets and fractions at which the restatement holds them on the synthetic BAM.)
BOUND_TARGETS, BOUND_FRACS = (0.1, 0.3), (0.25, 0.5)


def check_bounds(counts, n_of):
    """counts [V, 1, T, F, 5] against |N' - f N| <= 4 sqrt(N f (1 - f)) and |S' - f t N| <= 4 sqrt(N f t (1 - f t)) -> cells checked."""
    checked = 0
    for i, n in enumerate(n_of):
        for t, target in enumerate(BOUND_TARGETS):
            for f, frac in enumerate(BOUND_FRACS):
                n2, s2 = int(counts[i, 0, t, f, 0]), int(counts[i, 0, t, f, 2])
                assert abs(n2 - frac * n) <= 4 * math.sqrt(n * frac * (1 - frac)), (i, t, f, n2, n)
                assert abs(s2 - frac * target * n) <= 4 * math.sqrt(n * frac * target * (1 - frac * target)), (i, t, f, s2, n)
                checked += 1
    return checked


def test_deviation_bounds_on_the_synthetic_bam(tmp_path):
    bam, fa, P, variants = _synth(tmp_path)
    counts, counters = DS.restate_counts(bam, fa, variants, BOUND_TARGETS, BOUND_FRACS, SEED, 1)
    n_of = [len(names) for names, _ in counters]
    assert min(n_of) >= 50
    assert check_bounds(counts, n_of) == len(variants) * 4


ROW = ["chr1", "100", "A", "G"] + ["x"] * (len(dsaf.HEADER_ALL) - 4)


def _row(pi):
    r = list(ROW)
    r[dsaf._COL["PI"]] = pi
    return r


def _entry(s, v1, pi=None, called=False, n=100, v0=1):
    return (dict(N=n, V0=v0, S=s, READS=3 * s, V1=v1), None if pi is None else _row(pi), ("A", ["G"]) if called else None)


def test_detection_and_replicate_lines():
    assert spike.DEPTH_DETECTION_HEADER == ("CHROM", "POS", "REF", "ALT", "TARGET", "FRACTION", "MTDEPTH", "N", "V0", "S", "READS", "V1", "AF",
                                            "UMT", "VMT", "VMF", "PI", "FILTER", "CALLED")
    assert spike.DEPTH_REPLICATES_HEADER == spike.DEPTH_DETECTION_HEADER[:7] + ("REP", "SEED") + spike.DEPTH_DETECTION_HEADER[7:]
    r, row, cut = _entry(7, 8, "12.5", True)
    plain = spike.detection_line(V, 0.05, r, row, cut).split("\t")
    det = spike.depth_detection_line(V, 0.05, 0.25, 903, r, row, cut).split("\t")
    assert det[:5] + det[7:] == plain and det[5:7] == ["0.25", "903"] and len(det) == len(spike.DEPTH_DETECTION_HEADER)
    assert det[7:13] == ["100", "1", "7", "21", "8", "0.08"]
    assert spike.depth_detection_line(V, 0.05, 0.25, 903, r, row, cut, lod=0.0125).split("\t")[-1] == "0.0125"
    zero = spike.depth_detection_line(V, 0.05, 0.25, 903, dict(N=0, V0=0, S=0, READS=0, V1=0), None, None).split("\t")
    assert zero[7:13] == ["0", "0", "0", "0", "0", dsaf.frac_text(0.0)] and zero[-1] == "0"          # AF 0 when N is 0
    rep = spike.depth_replicate_line(V, 0.05, 0.25, 903, 3, (1 << 64) - 1, r, row, cut).split("\t")
    assert rep[:7] + rep[9:] == det and rep[7:9] == ["3", "18446744073709551615"] and len(rep) == len(spike.DEPTH_REPLICATES_HEADER)
    assert (rep[DS.N], rep[DS.V0], rep[DS.S], rep[DS.READS], rep[DS.V1], rep[DS.PI], rep[DS.CALLED]) == ("100", "1", "7", "21", "8", "12.5", "1")
    assert (rep[DS.FRACTION], rep[DS.MTDEPTH], rep[DS.REP], rep[DS.SEED]) == ("0.25", "903", "3", "18446744073709551615")


def test_sensitivity_lines():
    assert spike.DEPTH_SENSITIVITY_HEADER == spike.SENSITIVITY_HEADER[:5] + ("FRACTION", "MTDEPTH") + spike.SENSITIVITY_HEADER[5:] + ("N_MEAN",)
    per = [_entry(4, 5, "20.0", True, n=90), _entry(6, 7, "30.0", True, n=110), _entry(5, 5, "25.0", False, n=100), _entry(9, 10, "45.0", True, n=104)]
    plain = spike.sensitivity_line(V, 0.02, per).split("\t")
    f = spike.depth_sensitivity_line(V, 0.02, 0.5, 1806, per).split("\t")
    assert f[:5] + f[7:-1] == plain and f[5:7] == ["0.5", "1806"] and f[-1] == dsaf.frac_text(101.0)
    assert spike.depth_sensitivity_line(V, 0.02, 0.5, 1806, per, lod=0.5).split("\t")[-2:] == [dsaf.frac_text(101.0), "0.5"]
    lines = [spike.depth_replicate_line(V, 0.02, 0.5, 1806, j, j, *e).split("\t") for j, e in enumerate(per)]
    assert DS.sensitivity_from(lines, [V], [(0.02, 0.5)], 4, dsaf.frac_text) == [f]


def test_curve_lines():
    yes, no = _entry(5, 6, "30.0", True), _entry(1, 1, "1.0")
    half = _entry(2, 3, "30.0", True, n=50)
    targets, fracs = [0.05, 0.01], [0.5]
    assert spike.depth_curve_header(targets) == ("CHROM", "POS", "REF", "ALT", "DEPTH", "MTDEPTH", "N_MEAN", "RATE@0.01", "RATE@0.05", "T95")
    assert spike.depth_curve_header(targets, True)[-1] == "LOD"
    full = spike.depth_curve_line(V, None, [200, 200], targets, [[yes] * 4, [yes, yes, yes, no]]).split("\t")
    assert full == ["chr1", "100", "A", "G", "full", "200", "100.0", "0.75", "1.0", "0.05"]
    cell = spike.depth_curve_line(V, 0.5, [100, 80], targets, [[half] * 4, [no] * 4], lod=0.04).split("\t")
    assert cell == ["chr1", "100", "A", "G", "0.5", "100,80", "75.0", "0.0", "1.0", "0.05", "0.04"]
    none = spike.depth_curve_line(V, 0.5, [100, 100], targets, [[no] * 4, [yes] * 4]).split("\t")
    assert none[7:] == ["1.0", "0.0", "NA"]
    # the helper computes the same from replicate lines
    full_per, cell_per = [[yes] * 4, [yes, yes, yes, no]], [[half] * 4, [no] * 4]
    full_lines = [spike.replicate_line(V, t, j, j, *e).split("\t") for t, p in zip(targets, full_per) for j, e in enumerate(p)]
    cell_lines = [spike.depth_replicate_line(V, t, 0.5, d, j, j, *e).split("\t") for t, d, p in zip(targets, (100, 80), cell_per) for j, e in enumerate(p)]
    assert DS.curve_from(full_lines, [200, 200], cell_lines, [V], targets, fracs, 4, dsaf.frac_text) == [full, cell[:-1]]


def test_files_on_hand_made_rows(tmp_path):
    """The four writers: headers, the order of the lines (variants, then targets outer and fractions inner; the curve `full` first),
    the LOD columns."""
    prefix = str(tmp_path / "o")
    v2 = R.V("chr1", 200, "C", "T", "T")
    targets, fracs = [0.05, 0.01], [0.5, 0.25]
    cells = [(t, target, f, 100 if f == 0.5 else 50, "%s.spikeAF%g.dsMT%g" % (prefix, target, f), None) for t, target in enumerate(targets) for f in fracs]
    for c in cells:
        with open(c[4] + ".smCounter.all.txt", "w") as fh:
            fh.write("\t".join(dsaf.HEADER_ALL) + "\n" + "\t".join(_row("33.0")) + "\n")
        with open(c[4] + ".smCounter.cut.txt", "w") as fh:
            fh.write("CHROM\tPOS\tREF\tALT\n")
    counts = [[dict(N=10 + c, V0=0, S=c, READS=2 * c, V1=c) for c in range(4)] for _ in range(2)]
    spike.write_depth_detection(prefix, [V, v2], cells, counts)
    det = [l.split("\t") for l in open(prefix + ".spikeAF.depth.detection.txt").read().splitlines()]
    assert det[0] == list(spike.DEPTH_DETECTION_HEADER) and len(det) == 1 + 2 * 4
    assert [l[4:7] for l in det[1:5]] == [["0.05", "0.5", "100"], ["0.05", "0.25", "50"], ["0.01", "0.5", "100"], ["0.01", "0.25", "50"]]
    assert [l[1] for l in det[1:]] == ["100"] * 4 + ["200"] * 4 and det[2][7:12] == ["11", "0", "1", "2", "1"]
    assert det[1][16] == "33.0" and det[5][16] == ""                                   # (the second variant has no row in the cells' files)
    lods = np.array([0.5, 0.25])
    with_lod = [c[:5] + (lods,) for c in cells]
    spike.write_depth_detection(prefix, [V, v2], with_lod, counts, {("chr1", "100"): 0, ("chr1", "200"): 1})
    det = [l.split("\t") for l in open(prefix + ".spikeAF.depth.detection.txt").read().splitlines()]
    assert det[0][-1] == "LOD" and det[1][-1] == "0.5" and det[8][-1] == "0.25"
    yes, no = _entry(5, 6, "30.0", True), _entry(1, 1, "1.0")
    entries = {(i, c): [yes if (c + j) % 2 else no for j in range(2)] for i in range(2) for c in range(4)}
    full_entries = {(i, t): [yes, yes] for i in range(2) for t in range(2)}
    spike.write_depth_replicates(prefix, [V, v2], cells, [7, 8], entries)
    reps = [l.split("\t") for l in open(prefix + ".spikeAF.depth.replicates.txt").read().splitlines()]
    assert reps[0] == list(spike.DEPTH_REPLICATES_HEADER) and len(reps) == 1 + 2 * 4 * 2
    assert [l[DS.REP] for l in reps[1:5]] == ["0", "1", "0", "1"] and [l[DS.SEED] for l in reps[1:3]] == ["7", "8"]
    spike.write_depth_sensitivity(prefix, [V, v2], cells, entries)
    sens = [l.split("\t") for l in open(prefix + ".spikeAF.depth.sensitivity.txt").read().splitlines()]
    assert sens[0] == list(spike.DEPTH_SENSITIVITY_HEADER) and sens[1:] == DS.sensitivity_from(reps[1:], [V, v2], [(c[1], c[2]) for c in cells], 2, dsaf.frac_text)
    spike.write_depth_curve(prefix, [V, v2], targets, fracs, [(200, None), (200, None)], cells, full_entries, entries)
    curve = [l.split("\t") for l in open(prefix + ".spikeAF.depth.curve.txt").read().splitlines()]
    assert curve[0] == list(spike.depth_curve_header(targets)) and len(curve) == 1 + 2 * 3
    assert [l[4] for l in curve[1:4]] == ["full", "0.5", "0.25"] and [l[5] for l in curve[1:4]] == ["200", "100", "50"]
    full_lines = [spike.replicate_line(v, t, j, j, *e).split("\t") for i, v in enumerate([V, v2]) for k, t in enumerate(targets)
                  for j, e in enumerate(full_entries[(i, k)])]
    assert curve[1:] == DS.curve_from(full_lines, [200, 200], reps[1:], [V, v2], targets, fracs, 2, dsaf.frac_text)
