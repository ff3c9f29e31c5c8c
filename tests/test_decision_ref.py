"""The stage between the barcode posteriors and the output row - ranking by PI, the order of exact ties, ALT, `biallelic`, which
candidates are filtered, and the integer and ratio gates of filterVariants - on the constructed loci of tests/decision_cases.py, against
what the reference itself returned for them (tests/golden/decision/, made by tests/golden/make_decision_golden.py).

No tie excuse anywhere in this file: a locus whose order the reference pins (order class `pinned`, `pinned_indel`) must come out of the
CPU restatements with the reference's maxBase, secondMaxBase and row, byte for byte.  The GPU half is tests/test_gpu_decision.py."""
import itertools

import numpy as np
import pytest

import decision_cases as D
from smcounter_amd import abi, py2compat, rows
from smcounter_amd.pileup import BASE_ALLELES, _PER_READ

import oracle_lib
import vc_port

# Loci of class `pinned_indel` (and the loci of 21 to 30 keys) where oracle/smc_oracle.c - and with it the kernel - picks maxBase /
# secondMaxBase differently from what the harness's Py2Dict recorded: label -> ((reference's maxBase, secondMaxBase), (the oracle's)).
# A documented non-parity: an indel key's hash can take a base's slot, and from 22 keys on the dict has 128 slots.
# EMPTY: through the harness as it stands no locus of the fixture shows either effect at a tie that decides anything.
EXPECTED_DIFFERENCES = {}

ORDER_8 = ["A", "C", "DEL", "T", "G", "N"]          # slot order of the fixed keys in a dict of 8, 32 and 128 slots
ORDER_32 = ["A", "C", "G", "N", "DEL", "T"]
ORDER_128 = ["DEL", "A", "C", "G", "N", "T"]


@pytest.mark.parametrize("name", D.FAMILIES)
def test_stored_fixture_is_what_decision_cases_builds_and_keeps_the_generators_conditions(name):
    F = D.family(name)
    pb, chroms, P, labels, designs = getattr(D, name)()
    assert labels == F.labels and P == F.P and chroms == F.extra["chroms"]
    assert [list(d) if d else d for d in designs] == F.designs
    assert pb.chrom == F.pb.chrom and pb.ref == F.pb.ref and pb.alleles == F.pb.alleles
    for k in ("pos", "read_off") + _PER_READ:
        assert np.array_equal(getattr(pb, k), getattr(F.pb, k)), k
    D.check_fixture(name, F.extra)
    assert set(F.classes) <= {"pinned", "pinned_indel", "unpinned"}


def test_the_fixture_holds_the_cases_the_families_are_for():
    t8, t32, ti, g = (D.family(n) for n in D.FAMILIES)
    assert len(t8.labels) == 128 and len(t32.labels) == 64
    kinds = {lab.split(":")[2].split("-")[0] for lab in t8.labels}
    assert kinds == {"clean", "one", "two", "pair", "first", "ref"}
    for F in (t8, t32):                                      # every reference base, every pair of the others, at both places
        for ref in D.BASES:
            for x, y in itertools.combinations([b for b in D.BASES if b != ref], 2):
                for kind in ("pair", "first"):
                    assert any(lab.split(":")[1:] in ([ref, "%s-%s%s" % (kind, x, y)], [ref, "%s-%s%s" % (kind, y, x)]) for lab in F.labels)
    n_keys = {lab: len(e["final"]) for lab, e in zip(ti.labels, ti.expected)}
    assert [n_keys["ti:keys%d" % n] for n in D.N_KEYS_AROUND_GROWTH] == list(D.N_KEYS_AROUND_GROWTH)
    assert {n for lab, n in n_keys.items() if "keys" not in lab} == {5, 6, 7, 8}
    tied = sum(D.has_tie_at_top(e["final"]) for e, c in zip(ti.expected, ti.classes) if c == "pinned_indel")
    assert tied >= 150                                       # the designed ties survive the indel keys, bit for bit
    # (the FIRST barcode carries the indel read in half of them: its keys go into finalDict before the bases of the later barcodes)
    assert sum(lab.split(":")[0].endswith("f") for lab in ti.labels) == sum(lab.split(":")[0].endswith("l") for lab in ti.labels) == 96
    assert len(g.labels) == 40 and max(np.diff(g.pb.read_off)) < 3000


def test_what_the_harness_recorded_of_displaced_bases_and_of_the_128_slot_dict():
    """The finding the fixture is there to record: through the harness no indel key displaces a base key - the fixed
    keys of every `ties_indel` locus below 22 keys stand in the order of the device's tables -, and from 22 keys on they stand in the
    128-slot order, DEL in front of A; at 30 keys an insertion key sits where N probes and N moves behind T - the one displaced
    fixed key of the fixture, and no base among A, T, G, C.  A fixture regenerated with another result fails here first."""
    ti = D.family("ties_indel")
    seen_128 = 0
    for lab, e in zip(ti.labels, ti.expected):
        keys = [k for k, _ in e["final"]]
        table = ORDER_8 if len(keys) <= 5 else ORDER_32 if len(keys) < 22 else ORDER_128
        if lab == "ti:keys30":
            table = ["DEL", "A", "C", "G", "T", "N"]
        assert [k for k in keys if k in D.FIXED_KEYS] == [k for k in table if k in keys], (lab, keys)
        seen_128 += len(keys) >= 22
    assert seen_128 == 3


def _dict_of(size, keys):
    d = py2compat.Py2Dict()
    d.size, d.slots = size, [None] * size
    for k in keys:
        assert d._place(d.slots, size, k)
    return d


def test_rank_tables_from_first_principles():
    """The one independent derivation the slot constants have: CPython 2.7's string hash and dictobject probing (py2compat).  Every
    insertion order of every set of fixed keys gives ONE key order per table size, and vc_port.R8 / R32 (the same numbers as rank() in
    csrc/device_common.inc and tie_rank() in oracle/smc_oracle.c) are exactly the slots."""
    ids = {k: i for i, k in enumerate(BASE_ALLELES)}
    for size, table, order in ((8, vc_port.R8, ORDER_8), (32, vc_port.R32, ORDER_32)):
        assert sorted(table) == list(range(6))
        assert [BASE_ALLELES[a] for a in sorted(table, key=table.get)] == order
        for n in range(1, 7):
            for keys in itertools.combinations(BASE_ALLELES, n):
                want = sorted(keys, key=lambda k: table[ids[k]])
                for perm in itertools.permutations(keys):
                    d = _dict_of(size, perm)
                    assert d.keys() == want, (size, perm)
                    assert all(d.slots[table[ids[k]]] == k for k in keys), (size, perm)      # (the constants ARE the slot numbers)
    # through the whole model - growth included - as finalDict is filled: up to five keys stay in 8 slots, the sixth moves them to 32
    for n in range(2, 7):
        for keys in itertools.combinations(BASE_ALLELES, n):
            table = vc_port.R8 if n <= 5 else vc_port.R32
            want = sorted(keys, key=lambda k: table[ids[k]])
            assert all(py2compat.py2_dict_order(perm) == want for perm in itertools.permutations(keys)), keys
    # from 22 keys on the dict has 128 slots and DEL moves in front of A: documented, not in the device's tables
    fill = ["INS|A|A%s" % t for t in ("C", "G", "T", "CC", "CG", "CT", "GC", "GG", "GT", "TC", "TG", "TT", "CCC", "GGG", "TTT", "CGT")]
    for n_fill, order in ((15, ORDER_32), (16, ORDER_128)):
        got = py2compat.py2_dict_order(list(BASE_ALLELES) + fill[:n_fill])
        assert len(got) == 6 + n_fill and [k for k in got if k in BASE_ALLELES] == order, (n_fill, got)
    assert [k for k in _dict_of(128, BASE_ALLELES).keys()] == ORDER_128


def _strict_port_check(F, rows_py, R, loci):
    """vc_port's rows against the C restatement's with no tie excuse: every integer field, both candidates whole."""
    for l in loci:
        r = rows_py[l]
        lab = F.labels[l]
        for k in ("status", "cvg", "all_mt", "all_frag", "used_mt", "used_frag", "mt3", "mt5", "mt7", "mt10", "n_touched", "max_allele",
                  "second_allele", "biallelic"):
            assert r[k] == R[k][l], (lab, k, r[k], R[k][l])
        assert r["dp"] == R["dp"][l].tolist() and r["umt"] == R["umt"][l].tolist() and r["vsm"] == R["vsm"][l].tolist(), lab
        assert np.abs(np.array(r["pi"]) - R["pi"][l]).max() <= 1e-9, lab
        for ci, key in ((0, "cand0"), (1, "cand1")):
            c, C = r[key], R["cand"][l][ci]
            if c is None:
                assert C["allele"] == -1, (lab, key)
                continue
            for k in ("allele", "vdp", "vmt", "vsm", "flt_applied", "flt", "vmf_lt_099"):
                assert c[k] == C[k], (lab, key, k, c[k], C[k])
            assert abs(c["pi"] - C["pi"]) <= 1e-9, (lab, key)
            for a, b in zip(c["p"], (C["p_sb"], C["p_r1"], C["p_r2"], C["p_pr"])):
                assert (np.isnan(a) and np.isnan(b)) or abs(a - b) <= 1e-9, (lab, key)


def check_rows_against_the_reference(F, R, what):
    """Rows of family F (any producer) against what the reference returned: maxBase / secondMaxBase of every locus the reference pins,
    the printed row byte for byte, the unrounded PIs; the differences listed in EXPECTED_DIFFERENCES, and only those, exactly as
    listed.  -> the loci compared."""
    text = rows.format_rows(R, F.db, F.P, F.refp)
    seen, compared = set(), []
    for l, (lab, cls, e) in enumerate(zip(F.labels, F.classes, F.expected)):
        if cls == "unpinned":
            continue
        got = (F.allele_text(l, int(R["max_allele"][l])), F.allele_text(l, int(R["second_allele"][l])))
        want = F.reference_choice(l)
        if lab in EXPECTED_DIFFERENCES:
            assert cls == "pinned_indel" and EXPECTED_DIFFERENCES[lab] == (want, got) and want != got, (what, lab, want, got)
            seen.add(lab)
            continue
        assert got == want, "%s, %s: maxBase, secondMaxBase %r, the reference has %r (%r)" % (what, lab, got, want, e["final"])
        assert text[l] == e["row"], "%s, %s: the row differs from the reference's own output" % (what, lab)
        d = max(max(abs(e["pi_raw"][k] - R["pi"][l][k]) for k in range(4)), abs(e["pi_raw"][4] - R["cand"][l][0]["pi"]))
        assert d <= 1e-6, (what, lab, d)
        compared.append(l)
    assert seen == {lab for lab in EXPECTED_DIFFERENCES if lab in F.labels}
    return compared


def check_gate_flags(F, R, what):
    """flt_applied of a gate locus as designed: a candidate is filtered iff the reference ran its Fisher tests or printed a FILTER."""
    for l, (lab, (flt, n_fisher)) in enumerate(zip(F.labels, F.designs)):
        applied = int((R["cand"][l]["flt_applied"] != 0).sum())
        assert (applied > 0) == (n_fisher > 0 or flt != ";"), (what, lab)
        assert applied == (2 if n_fisher == 8 else applied and 1), (what, lab)
        if "af-61" in lab:                                   # above 60 % the strand-bias test is not made, R1CP / R2CP cannot fire
            c = R["cand"][l][0]
            assert np.isnan(c["p_sb"]) and not np.isnan(c["p_r1"]) and not (int(c["flt"]) & (abi.F_SB | abi.F_R1CP | abi.F_R2CP)), (what, lab)
        if "af-60" in lab:
            c = R["cand"][l][0]
            assert not np.isnan(c["p_sb"]) and (int(c["flt"]) & (abi.F_SB | abi.F_R1CP)) == abi.F_SB | abi.F_R1CP, (what, lab)


@pytest.mark.parametrize("name", D.FAMILIES)
def test_oracle_and_port_decide_as_the_reference(name):
    F = D.family(name)
    R, fragile = oracle_lib.call_batch(F.db, abi.c_params(F.P), abi.ROW_DTYPE, return_fragile=True)
    assert not fragile.any()                                 # no barcode of these loci hangs on rounding
    compared = check_rows_against_the_reference(F, R, "oracle")
    assert len(compared) >= (len(F.labels) if name != "ties_indel" else len(F.labels) // 2)
    if name == "gates":
        check_gate_flags(F, R, "oracle")
    pinned = [l for l, c in enumerate(F.classes) if c != "unpinned"]
    _strict_port_check(F, vc_port.call_batch(F.db, F.P, n_cpu=1), R, pinned)


def test_expected_differences_name_loci_of_the_fixture():
    labels = set(D.family("ties_indel").labels) | set(D.family("gates").labels)
    assert set(EXPECTED_DIFFERENCES) <= labels
