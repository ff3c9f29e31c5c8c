"""The exact calProb reference (tests/calprob_exact_ref.py) held to account, and the two CPU restatements (oracle/smc_oracle.c through
oracle_lib.call_batch, oracle/vc_port.py's cal_prob) held to it under the bound the GPU is held to - on the barcode families
tests/test_gpu_calprob.py sends through k_call_v2.  The bound's K is measured here.  No GPU needed."""
import math

import pytest

import calprob_exact_ref as X
from calprob_exact_ref import A_, T_, G_, C_, N_, DEL_, INS_

import oracle_lib
import vc_port

FAMILIES = (1, 2, 3, 4, 5, 6, 7)


def _oracle_rows(batch):
    from smcounter_amd import abi, features
    db = features.extract_features(X.build_pileup(batch), batch.params)
    return db, oracle_lib.call_batch(db, abi.c_params(batch.params), abi.ROW_DTYPE)


def test_known_answers():
    P = X._params()
    # one lone reference fragment: uniqBase A T G C, pcr(c) = 10^(-6 (c + .5) / 3); 1 - post(A) = 3 pcr(1) / (pne 0.9 / 0.9 + pcr(0) + 3 pcr(1))
    E = X.exact([(A_, None)], 0, P.smt)
    pcr0, pcr1 = 10.0 ** -1.0, 10.0 ** -3.0
    by_hand = -math.log10(3 * pcr1 / (0.99997 + pcr0 + 3 * pcr1))
    assert abs(E.pred_f[A_] - by_hand) < 1e-14 and abs(E.pred_f[A_] - 2.565442445) < 5e-10, E.pred_f
    assert E.keys == (A_, T_, G_, C_) and E.top == A_ and E.cons == A_ and not E.strong and not E.underflow
    assert E.pred[T_] == E.pred[G_] == E.pred[C_]
    # a one-allele barcode, whatever the allele and the qualities: the closed form of csrc/device_common.inc's comment,
    # post = (pne + pcr(0)) / (pne + pcr(0) + 3 pcr(nf)), pcr(c) = 10^(-6 (c + .5) / (nf + 2))
    mp = X.MP
    for nf in (1, 2, 7, 128, 4097):
        for a, q in ((A_, None), (T_, 30), (INS_, 93), (DEL_, 20)):
            E = X.exact([(a, q)] * nf, 0, P.smt)
            pcr = lambda c: mp.power(10, -6 * (mp.mpf(2 * c + 1) / (2 * nf + 4)))
            pne = 1 - mp.mpf(3) / 100000
            x = 3 * pcr(nf) / (pne + pcr(0) + 3 * pcr(nf))
            assert abs(E.x[a] / x - 1) < mp.mpf(10) ** -70 and abs(E.pred[a] + mp.log10(x)) < mp.mpf(10) ** -70, (nf, a, q)
            assert E.keys == tuple(sorted({a, A_, T_, G_} if a > C_ else {A_, T_, G_, C_}))
    # dropped barcodes (:28-32): four zeros, counted for their fragment's allele only when it is alone (:521-523)
    E = X.exact([(T_, 30)], 1, P.smt)
    assert E.dropped and set(E.pred_f.values()) == {0.0} and E.top is None and E.cons == T_ and X.firm(E)
    E = X.exact([(T_, 30), (T_, 30)], 2, P.smt)
    assert E.dropped and E.cons is None
    # two alleles, by hand: A lone, T lone -> symmetric, an exact tie; no consensus
    E = X.exact([(A_, None), (T_, None)], 0, P.smt)
    assert E.pred[A_] == E.pred[T_] and E.top is None and E.cons is None and not X.firm(E)
    # five alleles: no padding, every key exists
    E = X.exact([(A_, None), (T_, None), (G_, 30), (N_, None), (INS_, 30)], 0, P.smt)
    assert E.keys == (A_, T_, G_, N_, INS_)
    assert X.lite_from_for(20) == 27 and X.lite_from_for(8) != 27 and X.lite_from_for(0) is None
    assert [X.fxshift_for(n, 40000) for n in (1, 63, 64, 65, 4096, 30000)] == [48, 48, 48, 48, 45, 43]


def test_every_family_contains_its_sizes_and_routes():
    nfs = lambda fam: {len(L.barcodes[0]) for B in fam for L in B.loci}
    f1, f2 = X.family(1), X.family(2)
    assert nfs(f1[:1]) == set(X.NF_LIST) >= {1, 2, 3, 5, 26, 27, 127, 128, 129, 1000, 4095, 4096, 4097}
    assert f1[0].params.mtDrop == 0 and f1[1].params.mtDrop == 1 and {1, 2} <= nfs(f1[1:])
    for B in f1:
        for nf in nfs([B]):
            assert {q for L in B.loci if len(L.barcodes[0]) == nf for _, q in L.barcodes[0]} == {None, B.params.minBQ, 30, 93}
        assert all({a for a, _ in L.barcodes[0]} == {L.ref} for L in B.loci)
    for a in (A_, T_, G_, C_, DEL_, INS_):
        mine = [L for L in f2[0].loci if L.barcodes[0][0][0] == a]
        assert {len(L.barcodes[0]) for L in mine} == set(X.NF_LIST) and all(L.ref != a and len({f for f in L.barcodes[0]}) == 1 for L in mine)
        assert {L.barcodes[0][0][1] is None for L in mine} == {True, False}
    f3 = X.family(3)
    assert [B.params.minBQ for B in f3] == [20, 8]
    for B in f3:
        lf = X.lite_from_for(B.params.minBQ)
        crs, tot = set(), set()
        for L in B.loci:
            bc = L.barcodes[0]
            cr = sum(a == L.ref for a, _ in bc)
            assert len({a for a, _ in bc}) == 2 and 1 <= len(bc) - cr <= 3
            crs.add(cr); tot.add(len(bc))
            if lf - 2 <= cr <= lf + 1:
                crs.add((cr, bc[0][1], len(bc) - cr, bc[-1][1]))
        for cr in range(lf - 2, lf + 2):
            assert all((cr, rq, na, aq) in crs for rq in (None, B.params.minBQ, 93) for na in (1, 2, 3) for aq in (None, 30)), cr
        assert {lf - 20, lf - 19} <= crs and {127, 128, 129} <= tot and min(tot) < 10
    assert X.lite_from_for(20) != X.lite_from_for(8)
    f4 = X.family(4)[0]
    lf = X.lite_from_for(20)
    seen = set()
    for L in f4.loci:
        cnt = {}
        for a, _ in L.barcodes[0]:
            cnt[a] = cnt.get(a, 0) + 1
        top = sorted(cnt.values(), reverse=True)
        seen.add((len(cnt), L.ref in cnt, cnt.get(L.ref, 0) >= lf, top[0] == top[1]))
    for n in (3, 4, 5, 6, 7):
        assert any(s[0] == n for s in seen), n
    for n in (3, 4, 5):
        assert any(s[0] == n and not s[1] for s in seen) and any(s[0] == n and s[2] for s in seen) and any(s[0] == n and s[3] for s in seen), n
    assert any(s[0] == 6 and s[2] for s in seen) and any(s[0] == 6 and s[3] for s in seen)
    assert {a for L in f4.loci for a, _ in L.barcodes[0]} == {A_, T_, G_, C_, N_, DEL_, INS_}
    assert {len(L.barcodes[0]) // 2 for L in X.family(5)[0].loci} == {1, 15, 64}
    f6 = X.family(6)[0]
    assert {len(L.barcodes) for L in f6.loci} == {1, 63, 64, 65, 4096, 13000, 30000}
    assert sorted(L.n_reads for L in f6.loci)[-2:] == [26000, 30000] and f6.params.ds >= 30000
    f7 = X.family(7)[0]
    assert [(len(L.barcodes[0]), L.barcodes[0][0]) for L in f7.loci] == [(600, (A_, 3)), (940, (A_, 3)), (1050, (A_, 3)), (1200, (A_, 3)), (2000, (A_, 3)),
                                                                         (940, (T_, 3)), (1200, (T_, 3)), (7000, (G_, None))]
    # the table's gate (csrc/host_abi.inc, simple_to_for, restated): 995 at minBQ 3, the whole table from minBQ 9 on; one-allele reference
    # barcodes of merged pairs at minBQ sit within 6 % of it on either side, every one decided by the exact rightP
    assert [X.simple_to_for(q) for q in (0, 3, 6, 8, 9, 20)] == [1, 995, 2395, 4015, 4096, 4096]
    for B, expect in zip(X.family(7), X.F7_EXPECT):
        q = B.params.minBQ
        assert q in X.F7_SIZES and len(expect) == len(B.loci)
        gate = X.simple_to_for(q)
        ref_only = sorted(len(L.barcodes[0]) for L in B.loci if L.barcodes[0][0] == (L.ref, q))
        below, above = [n for n in ref_only if n < gate], [n for n in ref_only if n >= gate]
        assert below and above and max(below) >= 0.94 * gate and min(above) <= 1.07 * gate, (q, gate, ref_only)
        for L, e in zip(B.loci, expect):
            E = X.exact(L.barcodes[0], 0, B.params.smt)
            assert E.underflow == e and (e or len(L.barcodes[0]) < gate or L.barcodes[0][0][0] != L.ref), L.note
    for n in FAMILIES:
        assert sum(len(B.loci) for B in X.family(n)) <= 300, n


def test_the_smallest_x_keeps_the_bound_meaningful():
    for n in (1, 2, 3, 4, 5, 6):
        assert X.min_x_of(n) > 2.0 ** -40, n


def test_the_reference_alone_decides_the_consensus_of_95_percent():
    for n in (1, 2, 3, 4, 6, 7):                      # (family 7: the rows that do not underflow are asked their consensus too)
        for B in X.family(n):
            soft = [L.note for L in B.loci if not X.locus_exact(L, B.params).firm]
            assert len(soft) <= 0.05 * len(B.loci), (n, soft)
    B = X.family(5)[0]
    assert not any(X.locus_exact(L, B.params).firm for L in B.loci)


import functools


@functools.lru_cache(maxsize=None)
def _oracle_family(n):
    """Family n through smc_oracle.c, held to the bound -> the worst error / bound(K = 1) of each of its batches"""
    out = []
    for i, B in enumerate(X.family(n)):
        db, rows = _oracle_rows(B)
        if n == 6:
            assert sorted(db.loci["n_reads"].tolist())[-2] > 24576
        worst, worst1, at, excused = X.check_rows("smc_oracle.c, family %d.%d" % (n, i), rows, B, expect_underflow=X.F7_EXPECT[i] if n == 7 else None,
                                                  sum_slack=True)
        print("smc_oracle.c  family %d.%d: worst error / bound %.3g, / bound(K = 1) %.3g at %r; %d of %d excused" % (n, i, worst, worst1, at, excused, len(B.loci)))
        out.append(worst1)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _vc_port_family(n):
    """Every distinct barcode of family n through vc_port.cal_prob, held to the bound -> the worst error / bound(K = 1) per batch"""
    out = []
    for i, B in enumerate(X.family(n)):
        P, worst1, at = B.params, 0.0, None
        for L in B.loci:
            for g in {X.canonical(bc) for bc in L.barcodes}:
                frags = [(a, None if q < 0 else q) for (a, q), m in g for _ in range(m)]
                E = X.exact(frags, P.mtDrop, P.smt)
                if E.underflow:
                    continue
                post = vc_port.cal_prob([[a, 0.1 if q is None else pow(10.0, -q / 10.0), q is not None] for a, q in frags], P.mtDrop)
                assert tuple(sorted(post)) == E.keys, L.note
                for k, p in post.items():
                    x = 1.0 - p
                    pred = -math.log10(x) if x > 0.0 else 16.0
                    r1 = abs(pred - E.pred_f[k]) / X.key_bound(E, k, 1)
                    if r1 > worst1:
                        worst1, at = r1, (L.note, k)
                    assert abs(pred - E.pred_f[k]) <= X.key_bound(E, k), (L.note, k, pred, E.pred_f[k], r1)
        print("vc_port       family %d.%d: worst error / bound(K = 1) %.3g at %r" % (n, i, worst1, at))
        out.append(worst1)
    return tuple(out)


@pytest.mark.parametrize("n", FAMILIES)
def test_oracle_within_the_bound_of_the_exact_reference(n):
    _oracle_family(n)


@pytest.mark.parametrize("n", FAMILIES)
def test_vc_port_cal_prob_within_the_bound_of_the_exact_reference(n):
    _vc_port_family(n)


def test_K_is_four_times_the_restatements_worst_ratio():
    """K = 4 x the worst error / bound(K = 1) of the plain IEEE restatements over every family (computed here, or taken from the tests
    above where they ran), rounded up to a power of two, at least 8; never tuned to the kernel."""
    ratios = {(who, n, i): r for who, f in (("oracle", _oracle_family), ("vc_port", _vc_port_family)) for n in FAMILIES for i, r in enumerate(f(n))}
    who = max(ratios, key=ratios.get)
    worst = ratios[who]
    need = max(8, 2 ** math.ceil(math.log2(4 * worst)))
    print("worst error / bound(K = 1) of the restatements: %.3g (%r); oracle alone %.3g; K = %d (module: %d)" % (
        worst, who, max(v for k, v in ratios.items() if k[0] == "oracle"), need, X.K))
    assert worst <= X.K / 4.0 and need == X.K
