"""finish_row (csrc/device_common.inc) and the integer and ratio gates of flt_locus (csrc/k_filter_loci.inc) on the constructed loci of
tests/decision_cases.py, against what the REFERENCE returned for them (tests/golden/decision/): the ranking by PI, the slot order of
exact ties among A, T, G, C, ALT, `biallelic`, which candidates are filtered and every gate from both sides.

abi.compare_rows and abi.near_tie_loci excuse a locus where the two sides pick maxBase / secondMaxBase differently at PIs within
1e-9 - right for ties of summation order, wrong for the exact ties the reference pins.  Here no locus of class `pinned` may be among
the excused ones, and the printed row is the reference's byte for byte.  Every path the stage has gives the same bytes: the
whole-locus classes, the parts path (deep class), the filter tallies by their own kernel, and both forms of the filter kernel
(a locus per workgroup / per wavefront).  Classes, labels and expectations come from the stored fixture."""
import numpy as np
import pytest

import decision_cases as D
from smcounter_amd import abi
from test_decision_ref import check_gate_flags, check_rows_against_the_reference

import oracle_lib

pytestmark = pytest.mark.gpu
PI_TOL = 1e-6
P_TOL = 1e-6


@pytest.fixture(autouse=True)
def _experiment_switches(monkeypatch):
    """The switches below are experiment knobs: the library reads them only under SMC_EXPERIMENTAL (tests/test_gpu_parity.py)."""
    monkeypatch.setenv("SMC_EXPERIMENTAL", "1")


def _check(F, got, what):
    want, fragile = oracle_lib.call_batch(F.db, abi.c_params(F.P), abi.ROW_DTYPE, return_fragile=True)
    assert not fragile.any()
    assert abi.compare_rows(got, want, PI_TOL, P_TOL, fragile) == [], what
    excused = abi.near_tie_loci(got, want)
    assert [F.labels[l] for l in sorted(excused) if F.classes[l] == "pinned"] == [], what          # the hole this file closes
    check_rows_against_the_reference(F, got, what)
    if F.name == "gates":
        check_gate_flags(F, got, what)
    # keys whose PIs are bit-equal in the reference are bit-equal on the device: the fixed-point sums add the same integers
    for l, e in enumerate(F.expected):
        val = dict((k, v) for k, v in e["final"])
        for i, x in enumerate(D.BASES):
            for j, y in enumerate(D.BASES[:i]):
                if x in val and y in val and val[x] == val[y]:
                    assert got["pi"][l][i] == got["pi"][l][j], (what, F.labels[l], x, y)


@pytest.mark.parametrize("name", D.FAMILIES)
def test_rows_are_the_references(engine0, name):
    F = D.family(name)
    got = engine0.call_batch_host(F.db, F.P)
    _check(F, got, name)
    assert engine0.call_batch_host(F.db, F.P).tobytes() == got.tobytes()


@pytest.mark.parametrize("name", D.FAMILIES)
def test_every_path_gives_the_same_bytes(engine0, monkeypatch, name):
    """The parts path with the geometry of test_host_made_and_device_made_plans_report_the_same_shape (loci above 100 reads in the deep
    class, parts of 64 reads) - and with every locus in it, tens of reads too (test_parts_and_chunks_give_identical_rows) - and the
    filter tallies by k_filter_tallies."""
    F = D.family(name)
    base = engine0.call_batch_host(F.db, F.P)
    paths = (("parts", dict(SMC_DEEP_FROM_READS="100", SMC_DEEP_PART_READS="64", SMC_DEEP_FCAP="16")),
             ("parts, every locus", dict(SMC_DEEP_FROM_READS="1", SMC_DEEP_PART_READS="64", SMC_DEEP_FCAP="16")),
             ("tallies later", dict(SMC_TALLIES_LATER="1")))
    for what, env in paths:
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        got = engine0.call_batch_host(F.db, F.P)
        for k in env:
            monkeypatch.delenv(k)
        assert got.tobytes() == base.tobytes(), (name, what)
    _check(F, base, name)


def test_gates_on_a_long_filter_worklist_one_locus_per_wavefront(engine0):
    """The light gate loci (the 1,000-barcode and the DP loci left out) repeated until more loci are queued than the filter kernel's
    grid has wavefronts (2048 x 4): flt_locus<false> runs, the tests of a locus one after the other in one wavefront.  The first and
    the last copy against the reference, and every copy the same bytes."""
    F = D.family("gates")
    light = [l for l in range(len(F.labels)) if F.pb.read_off[l + 1] - F.pb.read_off[l] <= D.LIGHT_READS]
    assert 30 <= len(light) < len(F.labels)
    n_queued = sum(1 for l in light if F.designs[l][1] > 0 or F.designs[l][0] != ";")
    reps = (2048 * 4) // n_queued + 2
    S = D.subset(F, light, reps)
    got = engine0.call_batch_host(S.db, S.P)
    assert int((got["cand"]["flt_applied"] != 0).any(axis=1).sum()) == reps * n_queued > 2048 * 4
    n = len(light)
    one = D.subset(F, light)
    _check(one, got[:n], "first copy")
    _check(one, got[-n:], "last copy")
    copies = np.ascontiguousarray(got).reshape(reps, n)
    first = copies[0].tobytes()
    assert all(copies[r].tobytes() == first for r in range(reps))
    # ... and the short worklist (flt_locus<true>) gives the same bytes
    assert engine0.call_batch_host(one.db, one.P).tobytes() == first
