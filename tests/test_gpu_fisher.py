"""The Fisher exact tests of csrc/k_filter_loci.inc (wave_fisher, d_lfact, k_lfact_table) against EXACT arithmetic
(tests/fisher_exact_ref.py), on tables built on purpose and handed to the device function through smc_fisher_tables /
smc_lfact_values.  The p-value is compared relatively, under fisher_exact_ref.bound (16 ulp of log((n1 + n2)!) + 1e-12) - never
against the CPU restatement, which shares the kernel's structure.  Each family is one call; the host reference is the cost."""
import math
import random

import numpy as np
import pytest

import fisher_exact_ref as F
from smcounter_amd import _lib, features, pileup
from smcounter_amd.params import VcParams
from test_fisher_ref import check_sb_rows

pytestmark = pytest.mark.gpu


def _run(engine0, name, tables, need_usable=None):
    orat, p = engine0.fisher_tables(tables)
    assert not np.isnan(p).any()
    worst, at, n_use = F.check_family("GPU, " + name, tables, orat, p, need_usable)
    print("GPU %-14s worst rel / bound %.3g at %r (%d usable of %d)" % (name, worst, at, n_use, len(tables)))
    return orat, p


def test_every_small_table(engine0):
    tables = F.small_tables()
    assert len(tables) == 2401
    orat, p = _run(engine0, "small", tables, need_usable=1.0)
    for t, o, q in zip(tables, orat, p):
        a, b, c, d = t
        if a + b == 0 or c + d == 0 or a + c == 0 or b + d == 0:
            assert math.isnan(o) and q == 1.0, t
        elif b * c == 0:
            assert o == math.inf, t
        assert 0.0 < q <= 1.0


def test_support_lengths_and_lane_chunks(engine0):
    tables = F.support_tables()
    lens = {(F.report(*t).n_support, t[0] - t[3] > 0) for t in tables}                    # (lo = max(0, n - n2) = max(0, a - d))
    assert {l for l, _ in lens} == {0, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097}     # (0: the one-cell supports, a zero margin)
    assert all((l, True) in lens and (l, False) in lens for l in (2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097))
    orat, p = _run(engine0, "support", tables, need_usable=1.0)
    assert math.isnan(orat[0]) and p[0] == 1.0 and math.isnan(orat[1]) and p[1] == 1.0


def test_symmetric_tables_include_the_mirrored_tail(engine0):
    tables = F.symmetric_tables()
    assert {sum(t) for t in tables} >= {20, 2000, 60000}
    orat, p = _run(engine0, "symmetric", tables, need_usable=1.0)
    for t, q in zip(tables, p):
        R = F.report(*t)
        # without the mirrored cell and what lies beyond it the sum is half the exact p (the tie is exact: only the slack, or a
        # `<=` that rounding happens to satisfy, takes it in)
        assert q > 0.75 * R.p, (t, q, R.p)


@pytest.mark.parametrize("gate", F.GATES)
def test_gate_straddlers_are_decided_as_the_reference_decides(engine0, gate):
    pairs = F.STRADDLERS[gate]
    assert len(pairs) >= 20
    tables = [t for pair in pairs for t in pair]
    orat, p = _run(engine0, "gate %g" % gate, tables, need_usable=1.0)
    for i, t in enumerate(tables):
        R = F.report(*t)
        assert abs(R.p - gate) >= 1e-6 * gate
        assert (p[i] < gate) == (R.p < gate) == bool(i & 1), (t, p[i], R.p)
        assert (orat[i] >= 50) == (R.oddsratio >= 50) and (orat[i] <= 1.0 / 50) == (R.oddsratio <= 1.0 / 50) and \
               (orat[i] < 0.05) == (R.oddsratio < 0.05), (t, orat[i])


def test_log_factorials(engine0):
    rng = random.Random(4711)
    ns = list(range(41)) + list(range(65530, 65542)) + [2 ** k for k in range(31)] + \
        [rng.randrange(0, 65536) for _ in range(100)] + [rng.randrange(65536, 2 ** 30) for _ in range(100)]
    got = engine0.lfact_values(ns)
    computed = engine0.lfact_values(ns, computed=True)
    worst = 0.0
    for n, g, c in zip(ns, got, computed):
        # the table's entries are what the series (the constants below 8) gives at the same argument, bit for bit
        assert np.float64(g).tobytes() == np.float64(c).tobytes(), (n, g, c)
        want = math.lgamma(n + 1.0)
        tol = 2 * math.ulp(want) + 1e-12
        worst = max(worst, abs(g - want) / tol)
        assert abs(g - want) <= tol, (n, g, want)
        if n <= 3000:                                        # exact: log of the integer n!, correctly rounded by math.log
            exact = math.log(math.factorial(n))
            assert abs(g - exact) <= 2 * math.ulp(exact) + 1e-12, (n, g, exact)
    assert got[0] == 0.0 and got[1] == 0.0
    print("log(n!): worst error / (2 ulp + 1e-12) = %.3g" % worst)
    assert len(engine0.lfact_values([])) == 0
    with pytest.raises(_lib.SmcError, match="smc_lfact_values"):
        engine0.lfact_values([3, -1])


def test_deep_tables(engine0):
    tables = F.deep_tables()
    assert 35 <= len(tables) <= 45 and min(sum(t) for t in tables) >= 8000 and max(sum(t) for t in tables) >= 262144
    orat, p = _run(engine0, "deep", tables, need_usable=0.95)
    assert sum(F.report(*t).p < F.TINY for t in tables) >= 5               # (the range below the doubles is visited)


@pytest.mark.parametrize("top,count,seed", F.RANDOM_FAMILIES, ids=["<=%d" % f[0] for f in F.RANDOM_FAMILIES])
def test_random_tables(engine0, top, count, seed):
    assert sum(f[1] for f in F.RANDOM_FAMILIES) == 2000
    _run(engine0, "random<=%d" % top, F.random_tables(top, count, seed), need_usable=0.99)


def test_results_do_not_depend_on_the_batch(engine0):
    tables = F.random_tables(700, 300, 99) + F.support_tables()[:40] + F.symmetric_tables() + F.deep_tables()[:10]
    o1, p1 = engine0.fisher_tables(tables)
    o2, p2 = engine0.fisher_tables(tables)
    assert o1.tobytes() == o2.tobytes() and p1.tobytes() == p2.tobytes()
    order = list(range(len(tables)))
    random.Random(5).shuffle(order)
    o3, p3 = engine0.fisher_tables([tables[i] for i in order])
    assert o3.tobytes() == o1[order].tobytes() and p3.tobytes() == p1[order].tobytes()


def test_refusals(engine0):
    with pytest.raises(_lib.SmcError, match="smc_fisher_tables.*negative"):
        engine0.fisher_tables([(1, 2, 3, 4), (1, -2, 3, 4)])
    with pytest.raises(_lib.SmcError, match="smc_fisher_tables.*2\\^31"):
        engine0.fisher_tables([(2 ** 30, 2 ** 30, 1, 1)])
    with pytest.raises(_lib.SmcError, match="smc_fisher_tables.*2\\^31"):
        engine0.fisher_tables([(2 ** 40, 0, 1, 1)])
    orat, p = engine0.fisher_tables(np.zeros((0, 4), np.int64))
    assert len(orat) == 0 and len(p) == 0
    assert engine0.L.smc_fisher_tables(engine0.ctx, None, 0, None, None) == 0
    orat, p = engine0.fisher_tables([(2 ** 31 - 4, 1, 1, 1), (3, 0, 0, 3)])             # (the largest total, and the context still works)
    assert orat[0] == 2.0 ** 31 - 4 and abs(p[1] - 0.1) < 1e-15


P_SB = VcParams(mtDepth=1000, rpb=8.0)


def test_strand_bias_gate_in_the_pipeline_one_locus_per_workgroup(engine0):
    """The gate-straddling strand-bias tables as loci through k_call_v2 and k_filter_loci: a short worklist, flt_locus<true> (the four
    tests side by side in a workgroup)."""
    db = features.extract_features(F.sb_pileup(F.SB_PIPELINE), P_SB)
    check_sb_rows(engine0.call_batch_host(db, P_SB), F.SB_PIPELINE)


def test_strand_bias_gate_in_the_pipeline_one_locus_per_wavefront(engine0):
    """The same loci 700 times over in one batch: more queued loci than the filter kernel's grid has wavefronts (2048 x 4), so
    flt_locus<false> runs (a locus per wavefront, the tests one after the other)."""
    reps = 700
    pb = F.sb_pileup(F.SB_PIPELINE)
    assert reps * pb.n_loci > 2048 * 4
    db = features.extract_features(pileup.concat([pb] * reps), P_SB)
    rows = engine0.call_batch_host(db, P_SB)
    assert int((rows["cand"][:, 0]["flt_applied"] != 0).sum()) == reps * pb.n_loci
    n = pb.n_loci
    check_sb_rows(rows[:n], F.SB_PIPELINE)
    check_sb_rows(rows[-n:], F.SB_PIPELINE)
    cand = rows["cand"][:, 0]
    for name in ("p_sb", "p_r1", "p_r2", "p_pr", "flt"):                                 # every copy of a locus gets the same bits
        col = np.ascontiguousarray(cand[name]).reshape(reps, n)
        assert col.tobytes() == np.ascontiguousarray(col[0]).tobytes() * reps, name
