"""The barcode posteriors of csrc/k_call_v2.inc (calProb and the PI / consensus step, every route of its U stage) against EXACT
arithmetic (tests/calprob_exact_ref.py), on barcodes built on purpose: one locus per barcode, through features.extract_features and
call_batch_host.  pi[0..3] and cand[0].pi are held to calprob_exact_ref's bound, K (2^-53 (1 + 1 / x) / ln 10 + ulp(pred)) +
2^-(fxshift + 1) with the K measured on the CPU restatements (16) - never to the restatements themselves, which share the kernel's
view of the algorithm.  umt / vsm must be the reference's wherever the reference alone decides them.  Each family is a batch or two.

Worst error / bound on an MI355X, families 1 to 7: 0.51, 0.51, 0.53, 0.53, 0.39, 0.64, 0.41."""
import numpy as np
import pytest

import calprob_exact_ref as X
from smcounter_amd import features

pytestmark = pytest.mark.gpu


def _run(eng, n, label="", expect_underflow=None):
    """Family n through the kernels, twice: identical bytes, and the rows inside the bound of the exact ones."""
    worst_all, excused_all, rows_all = 0.0, [], []
    for i, B in enumerate(X.family(n)):
        db = features.extract_features(X.build_pileup(B), B.params)
        rows = eng.call_batch_host(db, B.params)
        assert eng.call_batch_host(db, B.params).tobytes() == rows.tobytes()
        worst, worst1, at, excused = X.check_rows("GPU%s, family %d.%d" % (label, n, i), rows, B,
                                                  expect_underflow=expect_underflow[i] if expect_underflow else None)
        print("GPU%s family %d.%d: worst error / bound %.3g (K = %d) at %r; %d of %d loci excused from the consensus check" % (
            label, n, i, worst, X.K, at, excused, len(B.loci)))
        worst_all = max(worst_all, worst)
        excused_all.append((excused, len(B.loci)))
        rows_all.append((db, rows))
    return worst_all, excused_all, rows_all


def _few_excused(excused):
    for e, n in excused:
        assert e <= 0.05 * n, excused


def test_family1_one_allele_reference(engine0):
    _, excused, _ = _run(engine0, 1)
    _few_excused(excused)


def test_family2_one_allele_other(engine0):
    _, excused, _ = _run(engine0, 2)
    _few_excused(excused)


def test_family3_reference_and_one_other_around_lite_from(engine0):
    _, excused, _ = _run(engine0, 3)
    _few_excused(excused)


def test_family4_three_to_seven_alleles(engine0):
    _, excused, _ = _run(engine0, 4)
    _few_excused(excused)


def test_family5_symmetric_barcodes(engine0):
    _, excused, rows = _run(engine0, 5)
    assert all(e == n for e, n in excused)                  # the reference's own answer is order-dependent: excused in full
    for _, r in rows:
        assert (r["umt"].sum(axis=1) <= 1).all()


def test_family6_sums_parts_and_the_other_alleles_table(engine0):
    _, excused, rows = _run(engine0, 6)
    _few_excused(excused)
    (db, r), = rows
    deep = db.loci["n_reads"] > 24576                        # SMC_ALT_FROM_READS: parts, 512 threads, the major other allele's table
    assert sorted(db.loci["n_reads"][deep].tolist()) == [2 * X.F6_ALT, X.F6_MANY]
    assert r["used_mt"].tolist() == [len(L.barcodes) for L in X.family(6)[0].loci]


def test_family7_underflow_is_flagged_where_the_reference_underflows(engine0):
    _, excused, _ = _run(engine0, 7, expect_underflow=X.F7_EXPECT)
    assert all(e == 0 for e, _ in excused)                  # (the rows that do not underflow are asked their consensus too)


@pytest.fixture
def _experiment_switches(monkeypatch):
    """The switches below are experiment knobs: the library reads them only under SMC_EXPERIMENTAL (tests/test_gpu_parity.py)."""
    monkeypatch.setenv("SMC_EXPERIMENTAL", "1")
    return monkeypatch


def test_family3_without_lite(_experiment_switches):
    from smcounter_amd import engine
    _experiment_switches.setenv("SMC_NO_LITE", "1")
    eng = engine.Engine(0)
    try:
        _, excused, _ = _run(eng, 3, " (SMC_NO_LITE)")
    finally:
        eng.close()
    _few_excused(excused)


def test_family2_without_the_other_alleles_table(_experiment_switches):
    from smcounter_amd import engine
    _experiment_switches.setenv("SMC_NO_ALT", "1")
    eng = engine.Engine(0)
    try:
        _, excused, _ = _run(eng, 2, " (SMC_NO_ALT)")
        _, excused6, _ = _run(eng, 6, " (SMC_NO_ALT)")          # (the locus whose T barcodes the table scores by default: the general path)
    finally:
        eng.close()
    _few_excused(excused)
    _few_excused(excused6)
