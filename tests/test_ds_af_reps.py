"""--dsAFReps without a GPU: the flag and its refusals, the sensitivity table's arithmetic (Wilson interval against a hand-computed
table), the carrier table against tools.ds_allele_fraction.titrate's dropped sets, the two writers on hand-made rows, the ABI."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, cli, dsaf
from smcounter_amd.rows import HEADER_ALL
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_reps_restate as RR  # noqa: E402
import ds_restate  # noqa: E402


def _args(tmp, **kw):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp))
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    vfile = str(tmp / "v.txt")
    open(vfile, "w").write("%s\t%d\tA\tG\n" % loci[0])
    d = dict(outPrefix=str(tmp / "o"), bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, refGenome=fa, dsAF="0.05", dsAFVariants=vfile,
             dsAFReps=4)
    d.update(kw)
    return {k: v for k, v in d.items() if v is not None}


def test_parser_accepts_the_flag_with_dsaf(tmp_path):
    args = _args(tmp_path)
    ns = cli.build_parser().parse_args(["--%s=%s" % kv for kv in args.items()])
    assert ns.dsAFReps == 4
    targets = cli.ds_af_targets(ns)
    assert cli.ds_af_reps(ns, targets) == 4
    ns.dsAFReps = None
    assert cli.ds_af_reps(ns, targets) is None
    for r in (dsaf.REPS_MIN, dsaf.REPS_MAX):
        ns.dsAFReps = r
        assert cli.ds_af_reps(ns, targets) == r
    assert (cli.REPS_MIN, cli.REPS_MAX) == (dsaf.REPS_MIN, dsaf.REPS_MAX) == (2, 1000)


@pytest.mark.parametrize("kw,msg", [
    (dict(dsAF=None, dsAFVariants=None), "--dsAFReps replicates the dilutions of --dsAF: it needs --dsAF"),
    (dict(dsAFReps=1), "must lie in 2 .. 1000, got 1"),
    (dict(dsAFReps=0), "must lie in 2 .. 1000, got 0"),
    (dict(dsAFReps=1001), "must lie in 2 .. 1000, got 1001"),
    (dict(dsAFVariants=None), "it needs --dsAFVariants"),
    (dict(dsAF="0.5,1"), "must lie in (0, 1)"),
    (dict(dsMT="0.5"), "cannot be combined with --dsMT"),
    (dict(dsAFMtDepth="10,20"), "2 depths for 1 --dsAF targets"),
])
def test_cli_refusals_before_any_file(tmp_path, kw, msg):
    args = _args(tmp_path, **kw)
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(args)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


# z = 1.959963984540054, by hand from (2c + z^2 -/+ z sqrt(z^2 + 4c(n - c)/n)) / (2(n + z^2)) in 40-digit decimals
WILSON = {(0, 10): (0.0, 0.2775327998628892045), (10, 10): (0.7224672001371107955, 1.0),
          (3, 7): (0.1582198552514697076, 0.7495416354723427782), (500, 1000): (0.4690696003681041844, 0.5309303996318958156)}


def test_wilson_interval_against_the_hand_computed_table():
    n = 0
    for (c, r), (lo, hi) in WILSON.items():
        got = dsaf.wilson(c, r)
        assert abs(got[0] - lo) < 1e-12 and abs(got[1] - hi) < 1e-12, (c, r, got)
        assert 0.0 <= got[0] <= got[1] <= 1.0
        assert abs(RR.wilson(c, r)[0] - lo) < 1e-12 and abs(RR.wilson(c, r)[1] - hi) < 1e-12
        n += 1
    assert n == 4
    assert dsaf.WILSON_Z == 1.959963984540054


def _row(**kw):
    row = [""] * len(HEADER_ALL)
    base = dict(CHROM="chr1", POS="100", REF="A", ALT="G", UMT="3500", VMT="17", VMF="0.0049", PI="31.25", FILTER="PASS")
    base.update(kw)
    for name, val in base.items():
        row[HEADER_ALL.index(name)] = val
    return row


def test_sensitivity_line_arithmetic_and_format():
    v = af.Variant("chr1", 100, "A", "G", "G", af.SNV)
    hit, miss = ("A", ["G"]), None
    reps = [(1000, 10, _row(PI="31.25"), hit), (1000, 4, _row(PI="12.5"), miss), (998, 7, _row(PI="20.0"), hit), (1000, 0, None, None),
            (1000, 5, _row(PI="18.0"), ("A", ["T"])), (999, 6, _row(PI="40.0"), ("A", ["T", "G"])), (1000, 9, _row(PI="22.0"), ("C", ["G"]))]
    f = dsaf.sensitivity_line(v, 0.005, reps).split("\t")
    assert len(f) == len(dsaf.SENSITIVITY_HEADER) == 17
    assert f[:7] == ["chr1", "100", "A", "G", "0.005", "7", "3"]
    assert f[7:10] == [dsaf.frac_text(3.0 / 7), "0.15822", "0.749542"]
    afs = [10 / 1000., 4 / 1000., 7 / 998., 0.0, 5 / 1000., 6 / 999., 9 / 1000.]
    assert f[10:13] == [dsaf.frac_text(sum(afs) / 7), "0.0", "0.01"]
    assert f[13:15] == ["0", "10"]
    pis = [31.25, 12.5, 20.0, 0.0, 18.0, 40.0, 22.0]                      # (a replicate without a row counts as PI 0)
    assert f[15:] == [dsaf.frac_text(sum(pis) / 7), "0.0"]
    assert dsaf.sensitivity_line(v, 0.005, reps, lod=0.0021).split("\t")[17:] == ["0.0021"]
    # the left-alone variant: every replicate is the same, the rate is 0 or 1 and the interval is Wilson's of 0 / R or R / R
    same = [(1000, 12, _row(), hit)] * 10
    g = dsaf.sensitivity_line(v, 0.9, same).split("\t")
    assert g[4:10] == ["0.9", "10", "10", "1.0", "0.722467", "1.0"] and g[10:15] == ["0.012", "0.012", "0.012", "12", "12"]
    g = dsaf.sensitivity_line(v, 0.9, [(1000, 0, _row(PI="0.0"), None)] * 10).split("\t")
    assert g[5:10] == ["10", "0", "0.0", "0.0", "0.277533"] and g[13:] == ["0", "0", "0.0", "0.0"]


def test_carrier_table_is_the_min_threshold_rule_of_titrate():
    """One barcode range carries two listed variants with different k: the table's threshold is the smaller, and u >= it is exactly
    titrate()'s dropped set - for several seeds, two targets (one leaves variant 1 alone: thr 2^32)."""
    ids = np.arange(1, 101, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    covers = [ids[:100], ids[14:64]]
    carries = [ids[:20], ids[14:39]]
    targets = [0.05, 0.3]
    thr = RR.thresholds(covers, carries, targets)
    assert thr[0][0] != thr[0][1] and thr[1][0] == 1 << 32 and thr[1][1] < 1 << 32
    table_ids, table = dsaf.carrier_table(carries, thr)
    assert table.dtype == np.uint64 and table.shape == (39, 2)
    assert np.array_equal(table_ids, np.unique(ids[:39])) and (np.diff(table_ids.astype(object)) > 0).all()
    shared = np.isin(table_ids, ids[14:20])
    only0, only1 = np.isin(table_ids, ids[:14]), np.isin(table_ids, ids[20:39])
    assert shared.sum() == 6 and only0.sum() == 14 and only1.sum() == 19
    for t in range(2):
        assert (table[shared, t] == min(thr[t])).all() and (table[only0, t] == thr[t][0]).all() and (table[only1, t] == thr[t][1]).all()
    compared = 0
    for seed in (7, 8, (1 << 32) + 5, RR.M64):
        res = af.titrate(covers, carries, targets, seed)
        u = af.philox_word0(table_ids, seed)
        for t, r in enumerate(res):
            assert np.array_equal(table_ids[u >= table[:, t]], r["dropped"])
            compared += 1
    assert compared == 8
    assert any(len(r["dropped"]) for r in af.titrate(covers, carries, targets, 7))
    # no carrier at all: an empty table
    e_ids, e_tab = dsaf.carrier_table([ids[:0], ids[:0]], thr)
    assert len(e_ids) == 0 and e_tab.shape == (0, 2)
    assert dsaf.rep_seeds(RR.M64 - 1, 3) == [RR.M64 - 1, RR.M64, 0] == RR.seeds(RR.M64 - 1, 3)


def test_the_two_files_on_hand_made_rows(tmp_path):
    """Header, order of lines (variants outer, targets, replicates ascending), REP / SEED, a replicate without a row."""
    v0 = af.Variant("chr1", 100, "A", "G", "G", af.SNV)
    v1 = af.Variant("chr1", 200, "C", "CTT", "INS|C|CTT", af.INS)
    targets, seeds = [0.05, 0.01], dsaf.rep_seeds(RR.M64, 3)
    ks = [[0.473684210526, 1.0], [0.0452261306533, 0.25]]
    raw = "\t".join(_row(FILTER=";"))
    row, cut = dsaf.replicate_entry(raw, 20, {}, {})
    assert row == _row() and cut == ("A", ["G"])                                   # (';' -> PASS, PI 31.25 >= 20: in the cut file)
    assert dsaf.replicate_entry(raw, 32, {}, {}) == (_row(), None)                 # (below the threshold: printed, not cut)
    assert dsaf.replicate_entry("\t".join(_row(ALT="DEL", FILTER=";")), 20, {}, {})[1] is None
    assert dsaf.replicate_entry(None, 20, {}, {}) == (None, None)
    entries = {}
    for i in range(2):
        for t in range(2):
            entries[(i, t)] = [(3400 - j, 160 - 10 * j - t, None if (i, t, j) == (1, 1, 2) else row, cut if j != 1 else None) for j in range(3)]
    prefix = str(tmp_path / "o")
    dsaf.write_replicates(prefix, [v0, v1], targets, seeds, ks, entries)
    lines = [l.split("\t") for l in open(prefix + ".dsAF.replicates.txt").read().splitlines()]
    assert lines[0] == list(dsaf.REPLICATES_HEADER) == "CHROM POS REF ALT TARGET REP SEED N V AF K UMT VMT VMF PI FILTER CALLED".split()
    assert len(lines) == 1 + 2 * 2 * 3
    assert [(l[1], l[4], l[5]) for l in lines[1:]] == [(p, t, "%d" % j) for p in ("100", "200") for t in ("0.05", "0.01") for j in range(3)]
    assert [l[6] for l in lines[1:4]] == ["18446744073709551615", "0", "1"]
    # a line without its REP and SEED fields is detection_line()'s
    first = lines[1]
    assert "\t".join(first[:5] + first[7:]) == dsaf.detection_line(v0, 0.05, 3400, 160, ks[0][0], row, cut)
    assert first[7:11] == ["3400", "160", "0.047059", "0.473684"] and first[-1] == "1" and lines[2][-1] == "0"
    assert lines[-1][7:] == ["3398", "139", dsaf.frac_text(139.0 / 3398), "0.25", "", "", "", "", "", "0"]      # (no row)
    assert lines[7][-1] == "0"                                                     # (v1's ALT is CTT: the row's cut names G)
    dsaf.write_sensitivity(prefix, [v0, v1], targets, entries)
    sens = [l.split("\t") for l in open(prefix + ".dsAF.sensitivity.txt").read().splitlines()]
    assert sens[0] == list(dsaf.SENSITIVITY_HEADER) and len(sens) == 1 + 2 * 2
    assert [(l[1], l[4], l[5], l[6]) for l in sens[1:]] == [("100", "0.05", "3", "2"), ("100", "0.01", "3", "2"), ("200", "0.05", "3", "0"),
                                                           ("200", "0.01", "3", "0")]
    assert sens[1] == dsaf.sensitivity_line(v0, 0.05, entries[(0, 0)]).split("\t")
    dsaf.write_sensitivity(prefix, [v0, v1], targets, entries, lods=[[0.001, 0.002], [0.003, 0.004]])
    sens = [l.split("\t") for l in open(prefix + ".dsAF.sensitivity.txt").read().splitlines()]
    assert sens[0][-1] == "LOD" and [l[-1] for l in sens[1:]] == ["0.001", "0.003", "0.002", "0.004"]


def test_header_symbols_and_help():
    h = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"\bint smc_af_rep_masks\(smc_ctx\* ctx,", h) and re.search(r"\bint smc_af_rep_counts\(smc_ctx\* ctx,", h)
    assert re.search(r"#define SMC_ABI_VERSION 11\b", h)
    assert "#define SMC_AF_REP_MAX_REPS %d" % dsaf.REPS_MAX in h
    assert "smc_af_rep_masks" in _lib.SYMBOLS and "smc_af_rep_counts" in _lib.SYMBOLS
    L = _lib.load()
    assert L.smc_abi_version() == 11 and hasattr(L, "smc_af_rep_masks") and hasattr(L, "smc_af_rep_counts")
    assert os.path.exists(os.path.join(ROOT, "smcounter_amd", "csrc", "k_af_depth.inc"))
    assert "--dsAFReps" in cli.build_parser().format_help()
