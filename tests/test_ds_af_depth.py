"""--dsAFDepth without a GPU: the flag and its refusals, the cells' prefixes and mtDepths, the cell rule's properties on the
restatement (tests/ds_af_depth_restate.py: nested kept sets, f = 1, the binomial widths on a synthetic BAM with planted variants),
the restatement's depth draw against the library's host Philox, the T95 rule, the four line formats on hand-made rows, the ABI."""
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, bamio, cli, devplanes, dsaf, fasta
from smcounter_amd.rows import HEADER_ALL
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_depth_restate as DR  # noqa: E402
import ds_af_reps_restate as RR  # noqa: E402
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402

SEED = 7                        # (test_deviation_bounds...: a seed for which the RESTATEMENT holds the bounds, verified on the CPU)
TARGETS = (0.05, 0.1)
FRACS = (0.25, 0.5)


def _args(tmp, **kw):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp))
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    vfile = str(tmp / "v.txt")
    open(vfile, "w").write("%s\t%d\tA\tG\n" % loci[0])
    d = dict(outPrefix=str(tmp / "o"), bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, refGenome=fa, dsAF="0.05,0.2", dsAFVariants=vfile,
             dsAFDepth="0.5,0.25")
    d.update(kw)
    return {k: v for k, v in d.items() if v is not None}


def _ns(args):
    return cli.build_parser().parse_args(["--%s=%s" % kv for kv in args.items()])


def test_parser_accepts_the_flag_and_names_the_cells(tmp_path):
    args = _args(tmp_path, mtDepth=3000)
    ns = _ns(args)
    assert ns.dsAFDepth == "0.5,0.25"
    targets = cli.ds_af_targets(ns)
    fracs, cells = cli.ds_af_depth_cells(ns, targets)
    assert fracs == [0.5, 0.25]
    o = args["outPrefix"]
    # targets outer, fractions inner; the mtDepth --dsMT f gets from the target's: max(1, round(f x mtDepth))
    assert cells == [(0, 0.05, 0.5, 1500, o + ".dsAF0.05.dsMT0.5"), (0, 0.05, 0.25, 750, o + ".dsAF0.05.dsMT0.25"),
                     (1, 0.2, 0.5, 1500, o + ".dsAF0.2.dsMT0.5"), (1, 0.2, 0.25, 750, o + ".dsAF0.2.dsMT0.25")]
    # --dsAFMtDepth gives a target its depth, and its cells theirs (Python 2 rounding: 2.5 -> 3; never below 1)
    ns = _ns(dict(args, dsAFMtDepth="10,1", dsAFDepth="0.25,1"))
    _, cells = cli.ds_af_depth_cells(ns, cli.ds_af_targets(ns))
    assert [c[3] for c in cells] == [3, 10, 1, 1]
    assert [c[3] for c in cells[:1]] == [d for _, d, _ in cli.ds_fractions(_ns(dict(_args(tmp_path, mtDepth=10, dsAF=None, dsAFVariants=None,
                                                                                          dsAFDepth=None), dsMT="0.25")))]
    ns.dsAFDepth = None
    assert cli.ds_af_depth_cells(ns, cli.ds_af_targets(ns)) == (None, [])
    assert "--dsAFDepth" in cli.build_parser().format_help()


@pytest.mark.parametrize("kw,msg", [
    (dict(dsAF=None, dsAFVariants=None), "--dsAFDepth thins the barcodes of the --dsAF dilutions: it needs --dsAF"),
    (dict(dsAFDepth="0.5,0"), "--dsAFDepth: every fraction must lie in (0, 1]"),
    (dict(dsAFDepth="1.5"), "--dsAFDepth: every fraction must lie in (0, 1]"),
    (dict(dsAFDepth="-0.5"), "--dsAFDepth: every fraction must lie in (0, 1]"),
    (dict(dsAFDepth="half"), "--dsAFDepth: comma-separated fractions in (0, 1] expected"),
    (dict(dsAFDepth="0.5,0.25,0.50"), "--dsAFDepth: a fraction is listed twice"),
    (dict(dsAFDepth=",".join("%g" % (0.03 * k) for k in range(1, 18))), "2 targets x 17 fractions = 34 cells, at most 32"),
    (dict(dsAFVariants=None), "it needs --dsAFVariants"),
    (dict(dsAF="0.5,1"), "must lie in (0, 1)"),
    (dict(dsMT="0.5"), "cannot be combined with --dsMT"),
    (dict(dsRpb="2"), "cannot be combined with --dsRpb"),
    (dict(dsAFMtDepth="10"), "1 depths for 2 --dsAF targets"),
    (dict(dsAFReps=1), "must lie in 2 .. 1000, got 1"),
])
def test_cli_refusals_before_any_file(tmp_path, kw, msg):
    args = _args(tmp_path, **kw)
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(args)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_cli_refuses_more_processes(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="runs in one process only"):
        cli.main(_args(tmp_path))
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def _sets(bam_path, fa_path, variants):
    """(covers, carries) identities of the listed variants, by the tool's own file pass, and the identities of every placed barcode."""
    ids = af.unique_idents(bamio.placed_barcodes(bam_path), bam_path)
    vs = [af.Variant(v.chrom, v.pos, v.ref, v.alt, *af.allele_key(v.ref, v.alt)) for v in variants]
    counted = af.count_file(bam_path, vs, fasta.FastaFile(fa_path))
    arr = lambda texts: np.array([ids[t] for t in texts], np.uint64)
    return [arr(c) for c, _ in counted], [arr(sorted(k)) for _, k in counted], np.array(sorted(ids.values()), np.uint64)


def _synth(tmp_path):
    bam, fa, loci, _, _ = R.synth_bam(str(tmp_path))
    variants = R.planted(bam, fa, loci)
    assert len(variants) >= 3
    return _sets(bam, fa, variants)


def test_kept_sets_are_nested_and_f1_is_the_dsaf_set(tmp_path):
    covers, carries, every = _synth(tmp_path)
    targets, fracs, reps = (0.02, 0.05, 0.1), (0.1, 0.25, 0.5, 1.0), 3
    keep, counts = DR.restate(every, covers, carries, targets, fracs, SEED, reps)
    plain, plain_counts, _ = RR.restate(every, covers, carries, targets, SEED, reps)
    assert keep.shape == (reps, 3, 4, len(every)) and counts.shape == (len(covers), reps, 3, 4, 2)
    compared = 0
    for j in range(reps):
        for t in range(3):
            for f in range(4):
                if t:
                    assert not (keep[j, t - 1, f] & ~keep[j, t, f]).any()          # nested in t: kept(t1) within kept(t2), t1 < t2
                if f:
                    assert not (keep[j, t, f - 1] & ~keep[j, t, f]).any()          # nested in f
                compared += 1
            # f = 1: the --dsAF kept set and its counts
            assert np.array_equal(keep[j, t, 3], plain[j, t]) and np.array_equal(counts[:, j, t, 3], plain_counts[:, j, t])
            # the product rule: a cell is the target's set and-ed with the fraction's, whatever the target
            for f in range(4):
                assert np.array_equal(keep[j, t, f], plain[j, t] & DR.depth_keep(every, fracs[f], DR.seeds(SEED, reps)[j]))
    assert compared == reps * 12
    assert keep[0, 0, 0].sum() < keep[0, 0, 1].sum() < keep[0, 0, 2].sum() < keep[0, 0, 3].sum() < len(every)
    assert not np.array_equal(keep[0], keep[1])                                    # (another seed, another draw)


def test_deviation_bounds_on_a_synthetic_bam_with_planted_variants(tmp_path):
    """|N' - f N| <= 4 sqrt(N f (1 - f)) and |V' - f k V| <= 4 sqrt(V f k (1 - f k)) for every planted variant and cell: the binomials'
    own widths.  N' also loses the carriers the dilution drops - (1 - k) V of the variant's own, and in this BAM, whose planted
    variants lie within a read's length of each other, those of every other listed variant too - so each planted variant is listed
    ALONE here, at targets and fractions that keep its own loss inside the width; f = 1, where the width is 0, is the equality test
    above.  Input and SEED are fixed: the restatement holds the bounds, verified here on the CPU; the device's counts are bit-equal to
    it and held to the same bounds (tests/test_gpu_ds_af_depth.py)."""
    covers, carries, every = _synth(tmp_path)
    assert check_bounds(lambda cov, car: DR.restate(every, cov, car, TARGETS, FRACS, SEED, 1)[1], covers, carries) >= 12


def check_bounds(counts_of, covers, carries):
    """The two bounds for every variant listed alone; counts_of(covers, carries) -> uint32 [1, 1, T, F, 2] -> cells checked."""
    checked = 0
    for v in range(len(covers)):
        counts = counts_of(covers[v:v + 1], carries[v:v + 1])
        for t, r in enumerate(af.titrate(covers[v:v + 1], carries[v:v + 1], list(TARGETS), SEED)):
            n, nv, k = r["rows"][0]["N"], r["rows"][0]["V"], r["rows"][0]["k"]
            assert n > 100 and nv > 10 and k < 1.0
            for i, f in enumerate(FRACS):
                n2, v2 = (int(x) for x in counts[0, 0, t, i])
                wn, wv = 4 * math.sqrt(n * f * (1 - f)), 4 * math.sqrt(nv * f * k * (1 - f * k))
                print("variant %d t %g f %g: N %d N' %d (f N %.1f, width %.1f); V %d k %.4f V' %d (f k V %.2f, width %.2f)" %
                      (v, TARGETS[t], f, n, n2, f * n, wn, nv, k, v2, f * k * nv, wv))
                assert abs(n2 - f * n) <= wn
                assert abs(v2 - f * k * nv) <= wv
                checked += 1
    return checked


def check_joint_bounds(counts_of, covers, carries):
    """All planted variants listed TOGETHER, as a run lists them.  The depth draw is a stream of its own, so given the dilution at t -
    titrate()'s achieved N2, V2 of the joint listing, which count every listed variant's dropped carriers - a cell's N' is
    Binomial(N2, f) and its V' Binomial(V2, f): |N' - f N2| <= 4 sqrt(N2 f (1 - f)) and |V' - f V2| <= 4 sqrt(V2 f (1 - f)), the
    binomials' own widths.  counts_of(covers, carries) -> uint32 [V, 1, T, F, 2] -> cells checked."""
    counts = counts_of(covers, carries)
    checked = 0
    for t, r in enumerate(af.titrate(covers, carries, list(TARGETS), SEED)):
        for v, row in enumerate(r["rows"]):
            assert row["N2"] < row["N"] and row["V2"] <= row["V"]
            for i, f in enumerate(FRACS):
                n2, v2 = (int(x) for x in counts[v, 0, t, i])
                wn, wv = 4 * math.sqrt(row["N2"] * f * (1 - f)), 4 * math.sqrt(row["V2"] * f * (1 - f))
                print("variant %d t %g f %g: N2 %d N' %d (f N2 %.1f, width %.1f); V2 %d V' %d (f V2 %.2f, width %.2f)" %
                      (v, TARGETS[t], f, row["N2"], n2, f * row["N2"], wn, row["V2"], v2, f * row["V2"], wv))
                assert abs(n2 - f * row["N2"]) <= wn
                assert abs(v2 - f * row["V2"]) <= wv
                checked += 1
    return checked


def test_deviation_bounds_with_all_planted_variants_listed_together(tmp_path):
    """What a run produces: one listing of all six planted variants, whose dilutions drop each other's covering barcodes.  The
    restatement holds the conditional bounds of check_joint_bounds at this input and SEED; the device's counts are held to them too."""
    covers, carries, every = _synth(tmp_path)
    assert check_joint_bounds(lambda cov, car: DR.restate(every, cov, car, TARGETS, FRACS, SEED, 1)[1], covers, carries) >= 12


def test_restated_depth_draw_is_the_dsmt_philox_rule():
    """The numpy draw of the restatement against the library's host Philox in devplanes.philox_keep_host - the rule --dsMT --dsSampler
    philox applies - and the thresholds against devplanes.frac_threshold."""
    L = _lib.load()
    rng = np.random.RandomState(11)
    ids = rng.randint(0, 1 << 62, 500).astype(np.uint64) * np.uint64(5) + np.uint64(3)
    compared = 0
    for seed in (7, (1 << 32) + 5, DR.M64):
        for f in (0.001, 0.3, 0.5, 1.0):
            assert np.array_equal(DR.depth_keep(ids, f, seed), devplanes.philox_keep_host(L, ids, f, seed))
            compared += len(ids)
    assert compared == 12 * 500
    assert DR.MT_DOMAIN == devplanes.DS_DOMAIN != devplanes.AF_DOMAIN
    for f in (1e-9, 0.1, 0.25, 1.0 / 3, 0.999999, 1.0):
        assert DR.frac_thr(f) == devplanes.frac_threshold(f)
    assert DR.frac_thr(1.0) == 1 << 32 and DR.frac_thr(0.5) == 1 << 31
    # the two streams of one barcode are different words
    assert not np.array_equal(DR.depth_draw(ids, 7), af.philox_word0(ids, 7))


def test_t95_rule():
    t = [0.005, 0.01, 0.02, 0.05]
    assert dsaf.t95(t, [0.1, 0.96, 1.0, 1.0]) == 0.01
    assert dsaf.t95(t, [1.0, 0.5, 0.97, 1.0]) == 0.02                # non-monotone: a dip below the level above 0.005 disqualifies it
    assert dsaf.t95(t, [0.96, 0.96, 0.9, 1.0]) == 0.05
    assert dsaf.t95(t, [0.0, 0.5, 0.9, 0.94]) is None                # all below
    assert dsaf.t95(t, [1.0, 1.0, 1.0, 0.0]) is None                 # the largest target itself is not found
    assert dsaf.t95(t, [0.95, 0.95, 1.0, 0.95]) == 0.005             # all above (0.95 counts)
    assert dsaf.t95([0.05, 0.005, 0.02, 0.01], [1.0, 0.1, 1.0, 0.96]) == 0.01     # any order of the targets
    assert dsaf.t95([], []) is None
    rng = np.random.RandomState(3)
    for _ in range(200):
        rates = rng.choice([0.0, 0.9, 0.95, 1.0], 4).tolist()
        assert dsaf.t95(t, rates) == DR.t95(t, rates)
    assert dsaf.T95_RATE == 0.95


def _row(**kw):
    row = [""] * len(HEADER_ALL)
    base = dict(CHROM="chr1", POS="100", REF="A", ALT="G", UMT="1700", VMT="9", VMF="0.0053", PI="31.25", FILTER="PASS")
    base.update(kw)
    for name, val in base.items():
        row[HEADER_ALL.index(name)] = val
    return row


def test_line_formats_on_hand_made_rows():
    v = af.Variant("chr1", 100, "A", "G", "G", af.SNV)
    hit = ("A", ["G"])
    d = dsaf.depth_detection_line(v, 0.005, 0.5, 1806, 1700, 9, 0.25, _row(), hit).split("\t")
    assert len(d) == len(dsaf.DEPTH_DETECTION_HEADER) == 17
    assert list(dsaf.DEPTH_DETECTION_HEADER) == "CHROM POS REF ALT TARGET FRACTION MTDEPTH N V AF K UMT VMT VMF PI FILTER CALLED".split()
    assert d == ["chr1", "100", "A", "G", "0.005", "0.5", "1806", "1700", "9", "0.005294", "0.25", "1700", "9", "0.0053", "31.25", "PASS", "1"]
    # without FRACTION and MTDEPTH it is detection_line()'s, LOD included
    with_lod = dsaf.depth_detection_line(v, 0.005, 0.5, 1806, 1700, 9, 0.25, _row(), hit, lod=0.0042).split("\t")
    assert with_lod[:5] + with_lod[7:] == dsaf.detection_line(v, 0.005, 1700, 9, 0.25, _row(), hit, 0.0042).split("\t") and with_lod[-1] == "0.0042"
    assert dsaf.depth_detection_line(v, 0.005, 1.0, 3612, 0, 0, 1.0, None, None).split("\t")[4:] == \
        ["0.005", "1", "3612", "0", "0", "0.0", "1.0", "", "", "", "", "", "0"]
    r = dsaf.depth_replicate_line(v, 0.005, 0.25, 903, 3, DR.M64, 850, 4, 0.25, _row(), None).split("\t")
    assert list(dsaf.DEPTH_REPLICATES_HEADER) == "CHROM POS REF ALT TARGET FRACTION MTDEPTH REP SEED N V AF K UMT VMT VMF PI FILTER CALLED".split()
    assert r[4:11] == ["0.005", "0.25", "903", "3", "18446744073709551615", "850", "4"] and r[-1] == "0" and len(r) == 19
    assert r[:7] + r[9:] == dsaf.depth_detection_line(v, 0.005, 0.25, 903, 850, 4, 0.25, _row(), None).split("\t")
    reps = [(850, 4, _row(PI="31.25"), hit), (860, 2, _row(PI="12.5"), None), (840, 6, _row(PI="40.0"), hit), (850, 0, None, None)]
    s = dsaf.depth_sensitivity_line(v, 0.005, 0.25, 903, reps).split("\t")
    assert list(dsaf.DEPTH_SENSITIVITY_HEADER) == ("CHROM POS REF ALT TARGET FRACTION MTDEPTH REPS CALLED RATE LO95 HI95 AF_MEAN AF_MIN AF_MAX "
                                                  "V_MIN V_MAX PI_MEAN PI_MIN N_MEAN").split()
    assert len(s) == 20 and s[4:10] == ["0.005", "0.25", "903", "4", "2", "0.5"] and s[-1] == "850.0"
    assert s[:5] + s[7:19] == dsaf.sensitivity_line(v, 0.005, reps).split("\t")
    lo, hi = RR.wilson(2, 4)
    assert s[10:12] == [dsaf.frac_text(lo), dsaf.frac_text(hi)]
    assert dsaf.depth_sensitivity_line(v, 0.005, 0.25, 903, reps, lod=0.011).split("\t")[19:] == ["850.0", "0.011"]
    # the curve: RATE@ in ascending target order whatever the order given, T95 by the rule, NA when no target qualifies
    targets = [0.02, 0.005, 0.01]
    all_hit, none_hit = [(800, 5, _row(), hit)] * 4, [(820, 1, _row(), None)] * 4
    assert dsaf.curve_header(targets) == ("CHROM", "POS", "REF", "ALT", "DEPTH", "MTDEPTH", "N_MEAN", "RATE@0.005", "RATE@0.01", "RATE@0.02", "T95")
    assert dsaf.curve_header(targets, True)[-2:] == ("T95", "LOD")
    c = dsaf.curve_line(v, 0.25, [903, 903, 903], targets, [all_hit, none_hit, reps]).split("\t")
    assert c == ["chr1", "100", "A", "G", "0.25", "903", dsaf.frac_text((800 + 820 + 850) / 3.0), "0.0", "0.5", "1.0", "0.02"]
    c = dsaf.curve_line(v, None, [3612, 3000, 3612], targets, [none_hit, all_hit, all_hit], lod=0.003).split("\t")
    assert c[4:6] == ["full", "3612,3000,3612"] and c[7:] == ["1.0", "1.0", "0.0", "NA", "0.003"]


def test_the_four_files_on_hand_made_rows(tmp_path):
    """Headers, the order of the lines (variants outer; cells: targets outer, fractions inner; replicates ascending; the curve: full
    first, then the fractions), the LOD columns."""
    v0 = af.Variant("chr1", 100, "A", "G", "G", af.SNV)
    v1 = af.Variant("chr1", 200, "C", "CTT", "INS|C|CTT", af.INS)
    targets, fracs, seeds = [0.05, 0.01], [0.5, 0.25], dsaf.rep_seeds(7, 2)
    ks = [[0.5, 1.0], [0.05, 0.25]]
    prefix = str(tmp_path / "o")
    lods = np.array([0.001, 0.002])
    cells, row = [], _row()
    for t, target in enumerate(targets):
        for f in fracs:
            p = "%s.dsAF%g.dsMT%g" % (prefix, target, f)
            open(p + ".smCounter.all.txt", "w").write("\t".join(HEADER_ALL) + "\n" + "\t".join(row) + "\n")
            open(p + ".smCounter.cut.txt", "w").write("CHROM\tPOS\tREF\tALT\n" + ("chr1\t100\tA\tG\n" if f == 0.5 else ""))
            cells.append((t, target, f, int(3000 * f), p, lods * (1 + len(cells))))
    loc_index = {("chr1", "100"): 0, ("chr1", "200"): 1}
    counts = np.arange(2 * 4 * 2).reshape(2, 4, 2) + 100
    dsaf.write_depth_detection(prefix, [v0, v1], cells, counts, ks, loc_index)
    det = [l.split("\t") for l in open(prefix + ".dsAF.depth.detection.txt").read().splitlines()]
    assert det[0] == list(dsaf.DEPTH_DETECTION_HEADER) + ["LOD"] and len(det) == 1 + 2 * 4
    assert [(l[1], l[4], l[5], l[6]) for l in det[1:]] == [(p, t, f, d) for p in ("100", "200") for t in ("0.05", "0.01")
                                                           for f, d in (("0.5", "1500"), ("0.25", "750"))]
    assert [l[7:9] for l in det[1:3]] == [["100", "101"], ["102", "103"]] and det[3][10] == "0.05" and det[5][10] == "1.0" and det[7][10] == "0.25"
    assert [l[16] for l in det[1:5]] == ["1", "0", "1", "0"] and det[5][11:17] == ["", "", "", "", "", "0"]      # (v1 has no row)
    assert [l[17] for l in det[1:]] == ["0.001", "0.002", "0.003", "0.004", "0.002", "0.004", "0.006", "0.008"]
    hit = ("A", ["G"])
    entries = {(i, c): [(900 - c, 9 - j, row if i == 0 else None, hit if (i == 0 and j == 0 and c != 3) else None) for j in range(2)]
               for i in range(2) for c in range(4)}
    dsaf.write_depth_replicates(prefix, [v0, v1], cells, seeds, ks, entries)
    rep = [l.split("\t") for l in open(prefix + ".dsAF.depth.replicates.txt").read().splitlines()]
    assert rep[0] == list(dsaf.DEPTH_REPLICATES_HEADER) and len(rep) == 1 + 2 * 4 * 2
    assert [(l[1], l[4], l[5], l[7], l[8]) for l in rep[1:5]] == [("100", "0.05", "0.5", "0", "7"), ("100", "0.05", "0.5", "1", "8"),
                                                                  ("100", "0.05", "0.25", "0", "7"), ("100", "0.05", "0.25", "1", "8")]
    assert rep[1][9:11] == ["900", "9"] and rep[1][-1] == "1" and rep[2][-1] == "0"
    dsaf.write_depth_sensitivity(prefix, [v0, v1], cells, entries, loc_index)
    sens = [l.split("\t") for l in open(prefix + ".dsAF.depth.sensitivity.txt").read().splitlines()]
    assert sens[0] == list(dsaf.DEPTH_SENSITIVITY_HEADER) + ["LOD"] and len(sens) == 1 + 2 * 4
    assert [(l[1], l[4], l[5], l[7], l[8], l[9]) for l in sens[1:5]] == [("100", "0.05", "0.5", "2", "1", "0.5"), ("100", "0.05", "0.25", "2", "1", "0.5"),
                                                                         ("100", "0.01", "0.5", "2", "1", "0.5"), ("100", "0.01", "0.25", "2", "0", "0.0")]
    assert sens[1] == dsaf.depth_sensitivity_line(v0, 0.05, 0.5, 1500, entries[(0, 0)], 0.001).split("\t")
    full_entries = {(i, t): [(1000, 20, row if i == 0 else None, hit if i == 0 else None)] * 2 for i in range(2) for t in range(2)}
    full = [(3000, lods * 10), (3000, lods * 10)]
    dsaf.write_depth_curve(prefix, [v0, v1], targets, fracs, full, cells, full_entries, entries, loc_index)
    cur = [l.split("\t") for l in open(prefix + ".dsAF.depth.curve.txt").read().splitlines()]
    assert cur[0] == ["CHROM", "POS", "REF", "ALT", "DEPTH", "MTDEPTH", "N_MEAN", "RATE@0.01", "RATE@0.05", "T95", "LOD"]
    assert len(cur) == 1 + 2 * 3 and [(l[1], l[4], l[5]) for l in cur[1:]] == [(p, d, m) for p in ("100", "200")
                                                                               for d, m in (("full", "3000"), ("0.5", "1500"), ("0.25", "750"))]
    assert cur[1][6:] == ["1000.0", "1.0", "1.0", "0.01", "0.01"]
    assert cur[2][6:] == [dsaf.frac_text((900 + 898) / 2.0), "0.5", "0.5", "NA", "0.001"]       # (the LOD of the largest target's cell)
    assert cur[3][6:] == [dsaf.frac_text((899 + 897) / 2.0), "0.0", "0.5", "NA", "0.002"]
    assert cur[4][6:] == ["1000.0", "0.0", "0.0", "NA", "0.02"]
    # without LODs: no LOD column in any of the four
    cells = [c[:5] + (None,) for c in cells]
    dsaf.write_depth_detection(prefix, [v0, v1], cells, counts, ks)
    dsaf.write_depth_sensitivity(prefix, [v0, v1], cells, entries)
    dsaf.write_depth_curve(prefix, [v0, v1], targets, fracs, [(3000, None)] * 2, cells, full_entries, entries)
    for name, header in (("detection", dsaf.DEPTH_DETECTION_HEADER), ("sensitivity", dsaf.DEPTH_SENSITIVITY_HEADER),
                         ("curve", dsaf.curve_header(targets))):
        assert open("%s.dsAF.depth.%s.txt" % (prefix, name)).readline().rstrip("\n").split("\t") == list(header)


def test_header_symbols_and_abi():
    h = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"\bint smc_af_depth_masks\(smc_ctx\* ctx,", h) and re.search(r"\bint smc_af_depth_counts\(smc_ctx\* ctx,", h)
    assert re.search(r"#define SMC_ABI_VERSION 11\b", h)
    assert "#define SMC_AF_DEPTH_MAX_CELLS %d" % cli.GRID_MAX_CELLS in h
    assert "smc_af_depth_masks" in _lib.SYMBOLS and "smc_af_depth_counts" in _lib.SYMBOLS
    L = _lib.load()
    assert L.smc_abi_version() == 11 and hasattr(L, "smc_af_depth_masks") and hasattr(L, "smc_af_depth_counts")
    assert os.path.exists(os.path.join(ROOT, "smcounter_amd", "csrc", "k_af_depth.inc"))
    rule = devplanes.DsRule(0.5, None, af=0.01, dropped_idents=np.zeros(0, np.uint64), bc_thr=1 << 31, depth=object(), cell=3)
    assert rule.flag == "--dsAFDepth" and rule.label == "allele fraction 0.01 x fraction 0.5" and rule.level == "barcode"
    assert devplanes.DsRule(1.0, None, af=0.01, dropped_idents=np.zeros(0, np.uint64)).flag == "--dsAF"
