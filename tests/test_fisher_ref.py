"""The exact Fisher reference (tests/fisher_exact_ref.py) against scipy's own numbers, and the CPU restatement
(oracle/smc_oracle.c: fisher_exact) against the reference - RELATIVELY, under the bound the GPU is held to
(fisher_exact_ref.bound: 16 ulp of log((n1 + n2)!) + 1e-12), on the table families tests/test_gpu_fisher.py runs on the device.
No GPU needed."""
import math
from fractions import Fraction

import numpy as np
import pytest

from conftest import golden_files, load_golden
import fisher_exact_ref as F

import oracle_lib


def _families():
    fams = [("small", F.small_tables()), ("support", F.support_tables()), ("symmetric", F.symmetric_tables()),
            ("gates", [t for g in F.GATES for pair in F.STRADDLERS[g] for t in pair]), ("deep", F.deep_tables())]
    return fams + [("random<=%d" % top, F.random_tables(top, count, seed)) for top, count, seed in F.RANDOM_FAMILIES]


def test_reference_known_values():
    # by hand: [[3, 0], [0, 3]] has weights 1 9 9 1 of 20, the observed one is an end: 2 / 20; [[1, 1], [1, 1]]: 1 4 1, the middle
    assert F.report(3, 0, 0, 3).p_exact == Fraction(1, 10) and F.report(1, 1, 1, 1).p_exact == 1
    assert F.report(2, 1, 1, 2).p_exact == Fraction(1, 1)                        # 1 9 9 1: a middle weight, everything counts
    assert F.report(10, 0, 0, 10).p_exact == Fraction(2, math.comb(20, 10))
    for t, want in (((10, 0, 0, 10), 1.0825e-05), ((11, 0, 0, 10), 2.835e-06), ((2000, 2000, 0, 17), 1.4785e-05), ((2000, 2000, 0, 18), 7.366e-06)):
        assert abs(F.report(*t).p - want) <= 1e-4 * want, (t, F.report(*t).p)
    R = F.report(0, 4, 0, 9)
    assert math.isnan(R.oddsratio) and R.p == 1.0 and R.usable
    assert F.report(5, 0, 2, 3).oddsratio == math.inf and F.report(0, 5, 2, 3).oddsratio == 0.0 and F.report(6, 2, 3, 4).oddsratio == 4.0
    # a symmetric table is usable (an exact tie), and its p holds the mirrored tail: twice the one-sided sum
    R = F.report(4, 6, 6, 4)
    assert R.usable and R.p_exact == R.p_slack == 2 * Fraction(sum(math.comb(10, k) ** 2 for k in range(5)), math.comb(20, 10))


def test_reference_matches_the_captured_scipy_calls():
    """scipy.stats.fisher_exact's own (oddsratio, p) of the ~ 500 calls the reference made for the goldens: relative, wherever
    scipy's p is at least 1e-290."""
    n, worst = 0, 0.0
    for path in golden_files():
        for e in load_golden(path)[4]:
            for (tab, orat, p) in e["fisher"]:
                t = (int(tab[0][0]), int(tab[0][1]), int(tab[1][0]), int(tab[1][1]))
                R = F.report(*t)
                assert (math.isnan(orat) and math.isnan(R.oddsratio)) or orat == R.oddsratio, (t, orat, R.oddsratio)
                if p < 1e-290 or not R.usable:
                    continue
                r = abs(p - R.p) / R.p / F.bound(*t)
                worst = max(worst, r)
                assert r <= 1.0, (t, p, R.p, r)
                n += 1
    assert n > 450, n


def test_reference_matches_scipy_on_the_families():
    stats = pytest.importorskip("scipy.stats")
    for name, tables in _families():
        if name == "deep":
            tables = [t for t in tables if F.report(*t).n_support <= 1000]      # (scipy walks the long ones for seconds)
        got = [stats.fisher_exact([[t[0], t[1]], [t[2], t[3]]]) for t in tables]
        F.check_family("scipy, " + name, tables, [g[0] for g in got], [g[1] for g in got])


def test_the_deep_form_matches_the_integer_form():
    for t in [(1490, 1510, 1510, 1490), (450, 550, 550, 450), (4000, 4000, 3990, 4010), (3000, 2000, 700, 900), (37, 4100, 2500, 1),
              (2999, 3001, 3001, 2999), (6000, 5000, 0, 800)]:
        a, b = F.report(*t, form="integer"), F.report(*t, form="deep")
        assert abs(a.p_exact - Fraction(b.p_exact)) <= a.p_exact * Fraction(1, 10 ** 50), t
        assert abs(a.p_slack - Fraction(b.p_slack)) <= a.p_slack * Fraction(1, 10 ** 50), t
        assert a.usable == b.usable and (a.gap == b.gap or abs(a.gap - b.gap) <= 1e-12 * a.gap), (t, a, b)


def test_unusable_tables_are_recognised():
    # 125000 + 125000 reference reads against 3 + 2: the weights of k = 2 and k = 3 differ by 8e-6 relative - a pmf rounded at
    # 1e-9 still tells them apart, one at 1e-5 would not: not a table to hold an implementation to
    R = F.report(125000, 125000, 3, 2)
    assert not R.usable and 0 < R.gap < F.TIE_GAP
    assert F.report(15000, 15000, 3, 2).usable


def test_every_random_family_keeps_99_percent_usable():
    for top, count, seed in F.RANDOM_FAMILIES:
        tables = F.random_tables(top, count, seed)
        usable = sum(F.report(*t).usable for t in tables)
        assert usable >= 0.99 * len(tables), (top, usable, len(tables))


def test_the_listed_gate_pairs_straddle_their_gates():
    for gate in F.GATES:
        pairs = F.STRADDLERS[gate]
        assert len(pairs) >= 20
        for t, u in pairs:
            Rt, Ru = F.report(*t), F.report(*u)
            assert sum(abs(x - y) for x, y in zip(t, u)) == 1 and Rt.usable and Ru.usable
            assert Rt.p >= gate * (1 + 1e-6) and Ru.p < gate * (1 - 1e-6), (t, u, Rt.p, Ru.p)
        ors = [F.report(*t).oddsratio for pair in pairs for t in pair]
        assert 50.0 in ors and 0.02 in ors and any(40 <= o < 50 for o in ors) and any(50 < o < 80 for o in ors)
        assert any(0.0125 <= o < 0.02 for o in ors)
        totals = [sum(t) for pair in pairs for t in pair]
        assert min(totals) < 100 and any(1000 < s < 20000 for s in totals) and max(totals) > 100000


@pytest.mark.parametrize("name,tables", _families(), ids=[f[0] for f in _families()])
def test_restatement_within_the_bound_of_the_exact_reference(name, tables):
    got = [oracle_lib.fisher(*t) for t in tables]
    worst, at, n_use = F.check_family("restatement, " + name, tables, [g[0] for g in got], [g[1] for g in got])
    print("restatement %-14s worst rel / bound %.3g at %r (%d usable of %d)" % (name, worst, at, n_use, len(tables)))


def test_restatement_decides_the_gates_as_the_reference_does():
    for gate in F.GATES:
        for pair in F.STRADDLERS[gate]:
            for t in pair:
                assert (oracle_lib.fisher(*t)[1] < gate) == (F.report(*t).p < gate), (t, gate)


def test_strand_bias_gate_in_the_restated_pipeline():
    """The loci tests/test_gpu_fisher.py sends through the kernels, through the restatement: the tallies are the tables, the
    candidate goes through the filters, p_sb is the exact p within the bound and SB is set as the reference decides."""
    from smcounter_amd import abi, features
    from smcounter_amd.params import VcParams
    P = VcParams(mtDepth=1000, rpb=8.0)
    rows = oracle_lib.call_batch(features.extract_features(F.sb_pileup(F.SB_PIPELINE), P), abi.c_params(P), abi.ROW_DTYPE)
    check_sb_rows(rows, F.SB_PIPELINE)


def check_sb_rows(rows, tables):
    from smcounter_amd import abi
    assert len(rows) == len(tables)
    n_set = 0
    for R, t in zip(rows, tables):
        C = R["cand"][0]
        assert R["status"] == abi.ST_OK and C["flt_applied"] == 1 and C["allele"] == 1, (t, R["status"], C["allele"])
        assert (R["ref_tal"][abi.T_REV], R["ref_tal"][abi.T_FWD], C["tal"][abi.T_REV], C["tal"][abi.T_FWD]) == t
        rep, sb = F.sb_expected(t)
        assert rep.usable and abs(rep.p - 1e-5) > 1e-11
        assert F.rel_error(float(C["p_sb"]), rep) <= F.bound(*t), (t, float(C["p_sb"]), rep.p)
        assert bool(C["flt"] & abi.F_SB) == sb, (t, float(C["p_sb"]), rep.p, rep.oddsratio)
        n_set += sb
    assert 0 < n_set < len(tables)
