"""calProb and the PI / consensus step (smCounter.py:26-98, :506-532) in EXACT arithmetic - the reference the barcode posteriors of
csrc/k_call_v2.inc, and the two CPU restatements (oracle/smc_oracle.c, oracle/vc_port.py), are held against.  mpmath at 80 digits;
nothing here is shared with the kernel, oracle/ or vc_port.py: the likelihoods are formed from the fragments' error probabilities as
the reference's lines form them (equal fragments taken as a power - exact arithmetic has no multiplication order), no table, no
shortcut for one allele, no odds form, no series.

  input    a barcode is a list of fragments (allele id, quality): quality None is a lone read (error probability exactly 1/10,
           :67-68), an integer q a merged pair whose smaller read quality is q (exactly 10^(-q/10), :469-473).  pcr_no_error is
           exactly 0.99997.
  output   `exact(frags, mt_drop, smt)`: per key of uniqBase the exact pred = -log10(1 - post) and x = 1 - post; whether the top pred
           is unique and by how much it leads, whether it exceeds smt, the allele MTCnt counts (:514-523), and whether the
           reference's own double products leave the normal range (rightP < 2^-1000, the threshold of smc_oracle.c and the kernel).
  bound    a computed pred is held to   K (2^-53 (1 + 1 / x) / ln 10 + ulp(pred)) + 2^-(fxshift + 1):
           1 / x is the conditioning of 1 - post, the last term the rounding of the kernel's fixed-point PI sums (fxshift 48 for a
           locus of one barcode).  K is MEASURED on the CPU, never on the kernel: the worst error / bound(K = 1) that the two plain IEEE
           restatements show over every family is 2.34 (smc_oracle.c and vc_port.cal_prob alike, at a barcode of 100 + 30 + 5 lone
           reads of three alleles; 2.25 to 2.29 in families 1 to 3), times 4 for what the kernel adds beyond IEEE operations
           (fast_div, the device exp10, neg_log10_unit's polynomial, the tree order of grpN_mul), rounded up to a power of two,
           at least 8:   K = 16.  tests/test_calprob_ref.py repeats the measurement and fails if the restatements exceed K / 4.
  families the barcodes tests/test_gpu_calprob.py sends through the kernel (and tests/test_calprob_ref.py through the restatements):
           every route of k_call_v2's U stage on both sides of its boundaries - see `family1` .. `family7`.

A family is a list of batches (one per parameter set), a batch a list of loci, a locus a reference letter and its barcodes;
`build_pileup` turns a batch into a PileupBatch: one fragment per read id, mates as F_READ1 / F_READ2, the way
fisher_exact_ref.sb_pileup builds its loci.  Over families 1 to 6 the smallest x is above 2^-40 (asserted here: the PCR terms keep
every likelihood within 1e-6 or so of the largest), so the bound means something and the `x <= 0 -> 16.0` cap (:510) is
unreachable in this domain."""
from __future__ import annotations

import math
from collections import Counter

import mpmath

MP = mpmath.mp.clone()
MP.dps = 80
K = 16                           # see the docstring: measured, 4 x the restatements' worst ratio rounded up to a power of two
A_, T_, G_, C_, N_, DEL_, INS_ = range(7)
INS_TEXT = "INS|A|AT"            # allele id 6 of every locus built here
_TEN, _ONE = MP.mpf(10), MP.mpf(1)
_PNE = _ONE - MP.mpf(3) / 100000                 # pcr_no_error, :20
_TWO_M1000 = MP.mpf(2) ** -1000


def lite_from_for(min_bq):
    """The host's rule (csrc/host_abi.inc, lite_from_for) restated: reference fragments from which the general path takes `lite`;
    None where it never does."""
    e = 10.0 ** (-0.1 * max(0, min_bq))
    if not e < 0.5:
        return None
    rho = max(1.0 / 9.0, e / (1.0 - e))
    return int(math.ceil(24.0 / -math.log10(rho))) + 1


def fxshift_for(n_umi, ds):
    """k_call_v2's rule for the scale of the fixed-point PI sums, restated"""
    return min(48, 58 - min(n_umi, ds).bit_length())


class Exact(object):
    """nf, keys (uniqBase, ascending ids), pred / x (mpf per key), pred_f / x_f (floats), top (the allele of the largest pred; None
    when it is not unique), lead (float: largest pred minus the runner-up), strong (top pred > smt), cons (the allele MTCnt counts,
    None: nobody), underflow."""
    __slots__ = ("nf", "keys", "pred", "x", "pred_f", "x_f", "top", "lead", "smt_gap", "strong", "cons", "underflow", "dropped")


_CACHE = {}


def canonical(frags):
    return tuple(sorted(Counter((a, -1 if q is None else q) for a, q in frags).items()))


def exact(frags, mt_drop, smt):
    key = (canonical(frags), mt_drop, smt)
    E = _CACHE.get(key)
    if E is None:
        E = _CACHE[key] = _exact(key[0], mt_drop, smt)
    return E


def _exact(groups, mt_drop, smt):
    E = Exact()
    nf = E.nf = sum(c for _, c in groups)
    E.dropped = nf <= mt_drop
    if E.dropped:                                                       # :28-32
        E.keys = (A_, T_, G_, C_)
        E.pred = {k: MP.mpf(0) for k in E.keys}
        E.x = {k: _ONE for k in E.keys}
        E.underflow = False
    else:
        exist = sorted({a for (a, _), _ in groups})
        uniq = list(exist)
        if len(uniq) < 4:                                               # :49-54
            for b in (A_, T_, G_, C_):
                if b not in uniq:
                    uniq.append(b)
                    if len(uniq) == 4:
                        break
        uniq.sort()
        prod = {k: _ONE for k in uniq}
        cnt = {k: 0 for k in uniq}
        right = _ONE
        for (a, q), c in groups:                                        # :62-77, c equal fragments at once
            p = _ONE / 10 if q < 0 else MP.power(_TEN, MP.mpf(-q) / 10)
            good, bad = MP.power(_ONE - p, c), MP.power(p, c)
            for k in uniq:
                prod[k] *= good if k == a else bad
            cnt[a] += c
            right *= good
        pcr = {k: MP.power(_TEN, -6 * (MP.mpf(2 * cnt[k] + 1) / (2 * nf + len(uniq)))) for k in uniq}     # :79-81
        tmp = {}
        for k in uniq:                                                  # :83-93
            if k in exist:
                tmp[k] = _PNE * prod[k] + right * min(pcr[c] for c in uniq if c != k)
            else:
                t = right
                for c in exist:
                    if c != k:
                        t *= pcr[c]
                tmp[k] = t
        total = sum(tmp.values())
        assert total > 0
        E.keys = tuple(uniq)
        E.x = {k: (total - tmp[k]) / total for k in uniq}               # 1 - post without the cancellation
        E.pred = {k: -MP.log10(E.x[k]) for k in uniq}
        E.underflow = bool(right < _TWO_M1000)
        assert not (_TWO_M1000 / 2 ** 40 < right < _TWO_M1000 * 2 ** 40), "a barcode too near the underflow threshold to be decided"
    E.pred_f = {k: float(v) for k, v in E.pred.items()}
    E.x_f = {k: float(v) for k, v in E.x.items()}
    order = sorted(E.keys, key=lambda k: E.pred[k], reverse=True)
    E.lead = float(E.pred[order[0]] - E.pred[order[1]])
    E.top = order[0] if E.pred[order[0]] > E.pred[order[1]] else None
    E.smt_gap = abs(float(E.pred[order[0]] - smt))
    E.strong = bool(E.pred[order[0]] > smt)
    if E.top is not None:                                               # :514-523
        E.cons = E.top
    elif nf == 1:
        E.cons = groups[0][0][0]
    else:
        E.cons = None
    return E


def key_bound(E, k, K_=K, fxshift=48):
    """The bound on one barcode's pred of key k (see the docstring); fxshift None: without the fixed-point term."""
    b = K_ * (2.0 ** -53 * (1.0 + 1.0 / E.x_f[k]) / math.log(10.0) + math.ulp(E.pred_f[k]))
    return b + (2.0 ** -(fxshift + 1) if fxshift is not None else 0.0)


def firm(E, K_=K):
    """The reference ALONE decides the barcode's consensus: the top pred leads by more than twice the bound and is further than the
    bound from smt (a dropped barcode's four zeros are zeros in any arithmetic: firm)."""
    if E.dropped:
        return True
    if E.top is None:
        return False
    order = sorted(E.keys, key=lambda k: E.pred[k], reverse=True)
    b = max(key_bound(E, order[0], K_), key_bound(E, order[1], K_))
    return E.lead > 2 * b and E.smt_gap > b


# ---- loci, batches, families ----------------------------------------------------------------------------------------------------

class Locus(object):
    def __init__(self, ref, barcodes, note=""):
        self.ref, self.barcodes, self.note = ref, barcodes, note

    @property
    def n_reads(self):
        return sum(1 if q is None else 2 for bc in self.barcodes for _, q in bc)


class Batch(object):
    def __init__(self, params, loci):
        self.params, self.loci = params, loci


def _params(**kw):
    from smcounter_amd.params import VcParams
    d = dict(mtDepth=1000, rpb=8.0)
    d.update(kw)
    return VcParams(**d)


def build_pileup(batch):
    """The batch's loci as a PileupBatch: barcode u of a locus is umi u, its fragment j read id j; a lone read is F_READ1 (every third
    one F_READ2) at a quality of 30, 37 or 93 - whatever it is, the fragment counts 0.1 -, a merged pair F_READ1 + F_READ2 of the same
    allele at q and min(q + 7, 93), the smaller one first or second in turn; READ2 is on the reverse strand.  In-deletion reads
    ('DEL', id 5) carry any quality - the batch gives them minBQ (:418) -, so a merged DEL fragment has q = minBQ."""
    import numpy as np
    from smcounter_amd import pileup
    P = batch.params
    umi, frag, flag, allele, bq = [], [], [], [], []
    off = [0]
    lone_q = (30, 37, 93)
    for L in batch.loci:
        for u, bc in enumerate(L.barcodes):
            for j, (a, q) in enumerate(bc):
                if q is None:
                    r2 = j % 3 == 2
                    umi.append(u); frag.append(j); allele.append(a); bq.append(max(P.minBQ, lone_q[j % 3]))
                    flag.append(pileup.F_READ2 | pileup.F_REVERSE if r2 else pileup.F_READ1)
                else:
                    assert q >= P.minBQ and (a != DEL_ or q == P.minBQ), (a, q)
                    hi = min(q + 7, 93)
                    qs = (q, hi) if j & 1 else (hi, q)
                    for m in range(2):
                        umi.append(u); frag.append(j); allele.append(a); bq.append(qs[m])
                        flag.append(pileup.F_READ2 | pileup.F_REVERSE if m else pileup.F_READ1)
        off.append(len(umi))
    n, nl = off[-1], len(batch.loci)
    al = np.array(allele, np.uint8)
    z = lambda dt, v=0: np.full(n, v, dt)
    return pileup.PileupBatch(
        chrom=["c"] * nl, pos=np.arange(100, 100 + nl, dtype=np.int64), ref=[pileup.BASE_ALLELES[L.ref] for L in batch.loci],
        alleles=[list(pileup.BASE_ALLELES) + [INS_TEXT] for _ in range(nl)], read_off=np.array(off, np.int64),
        umi=np.array(umi, np.uint32), frag=np.array(frag, np.uint32), flag=np.array(flag, np.uint8), mq=z(np.uint8, 60), nm=z(np.uint32),
        n_indel=z(np.uint32), left_sp=z(np.uint32), qlen=z(np.uint32, 100), qalen=z(np.uint32, 100), qpos=z(np.int32, 50),
        indel=(al == INS_).astype(np.int32), is_del=al == DEL_, allele=al, bq=np.array(bq, np.uint8))


NF_LIST = (1, 2, 3, 5, 26, 27, 127, 128, 129, 1000, 4095, 4096, 4097)


def family1():
    """One allele, the reference: the per-count table below 4096 fragments, the general path from there on."""
    out = []
    for mt_drop, nfs in ((0, NF_LIST), (1, (1, 2, 3, 128, 4096))):       # (mtDrop 0: nf = mtDrop is no barcode; mtDrop 1: nf 1 is dropped)
        P, loci = _params(mtDrop=mt_drop), []
        for i, nf in enumerate(nfs):
            for q in (None, 20, 30, 93):
                ref = (i + (q or 0)) % 4
                loci.append(Locus(ref, [[(ref, q)] * nf], "nf %d q %r" % (nf, q)))
        out.append(Batch(P, loci))
    return out


def family2():
    """One allele, not the reference (the general path's n_exist == 1): the letters, in-deletion reads and an insertion."""
    loci = []
    for a, ref in ((T_, A_), (A_, T_), (G_, A_), (C_, G_), (DEL_, A_), (INS_, C_)):
        for nf in NF_LIST:
            for q in (None, 20 if a == DEL_ else 30):
                loci.append(Locus(ref, [[(a, q)] * nf], "allele %d nf %d q %r" % (a, nf, q)))
    return [Batch(_params(), loci)]


F3_MINBQ = (20, 8)


def family3_cr(min_bq):
    lf = lite_from_for(min_bq)
    core = [lf - 2, lf - 1, lf, lf + 1]
    return lf, core, [1, 2, lf - 20, lf - 19, 60, 124, 125, 126, 127, 130]


def family3():
    """The reference plus one other allele (n_exist == 2): reference fragments around lite_from (the full cross of the qualities and
    the other allele's fragments), far below it (where a lowered lite_from would show), and up to totals on both sides of 128."""
    out = []
    for min_bq in F3_MINBQ:
        lf, core, extra = family3_cr(min_bq)
        alts = [(n, q) for n in (1, 2, 3) for q in (30, None)]
        loci, i = [], 0
        for cr in core + extra:
            full = cr in core
            for rq in ((None, min_bq, 93) if full else ((None, 93) if cr & 1 else (min_bq, None))):
                for na, aq in (alts if full else (alts[0], alts[3], alts[4])):
                    ref = i % 4
                    alt = INS_ if i % 5 == 4 else (ref + 1 + i % 3) % 4
                    loci.append(Locus(ref, [[(ref, rq)] * cr + [(alt, aq)] * na], "cr %d rq %r alt %d x %d q %r" % (cr, rq, alt, na, aq)))
                    i += 1
        out.append(Batch(_params(minBQ=min_bq), loci))
    return out


F4_COMPS = (   # (counts by allele id, reference letter, the two largest counts tie)
    ({A_: 5, T_: 2, G_: 1}, A_, False), ({A_: 30, T_: 2, G_: 1}, A_, False), ({A_: 2, T_: 2, G_: 1}, A_, True),
    ({T_: 3, G_: 3, C_: 1}, A_, True), ({A_: 130, T_: 1, G_: 1}, A_, False), ({T_: 100, G_: 30, C_: 5}, A_, False),
    ({A_: 4, T_: 3, G_: 2, C_: 1}, A_, False), ({A_: 28, T_: 1, G_: 1, C_: 1}, A_, False), ({A_: 3, T_: 3, G_: 1, N_: 1}, T_, True),
    ({T_: 2, G_: 2, C_: 1, DEL_: 1}, A_, True), ({A_: 40, T_: 1, DEL_: 1, INS_: 1}, A_, False), ({G_: 126, T_: 1, INS_: 1}, G_, False),
    ({A_: 3, T_: 2, G_: 2, C_: 1, N_: 1}, A_, False), ({A_: 30, T_: 1, G_: 1, C_: 1, DEL_: 1}, A_, False),
    ({T_: 2, G_: 2, C_: 1, N_: 1, INS_: 1}, A_, True), ({A_: 2, T_: 2, G_: 1, C_: 1, N_: 1, DEL_: 1}, A_, True),
    ({C_: 29, T_: 2, G_: 1, A_: 1, DEL_: 1, INS_: 2}, C_, False), ({A_: 3, T_: 1, G_: 1, C_: 1, N_: 1, DEL_: 1, INS_: 2}, A_, False),
    ({A_: 1, T_: 1, G_: 1, C_: 1, N_: 1, DEL_: 1, INS_: 3}, G_, False),
    # a fragment or two of each of three or four alleles: posteriors of a third or so, 1 - post far from a power of two - where the
    # polynomial of the kernel's own logarithm matters (near 1 - post = 1/2 or 1 its argument is near 0)
    ({A_: 1, T_: 1, G_: 1}, A_, True), ({A_: 1, T_: 1, G_: 1, C_: 1}, T_, True), ({A_: 2, T_: 1, G_: 1}, A_, False),
    ({T_: 1, G_: 1, INS_: 1}, A_, True))
# qualities by allele id; equal qualities make tied counts an exact tie of the posteriors (family 5's subject): not used for those
F4_MODES = ((None,) * 7, (30, 30, 30, 30, 30, 20, 30), (None, 30, 20, 37, None, 20, 25), (93, None, 41, 20, 22, None, None))


def family4():
    """Three and four alleles (pass B, full and lite), five to seven in one barcode (the route of its own)."""
    loci = []
    for comp, ref, tie in F4_COMPS:
        for mode in (F4_MODES[2:] if tie else F4_MODES):
            bc = [(a, mode[a]) for a in sorted(comp) for _ in range(comp[a])]
            loci.append(Locus(ref, [bc], "%r ref %d" % (comp, ref)))
    return [Batch(_params(), loci)]


def family5():
    """k fragments of A and k of T at one quality: the reference's own answer depends on its multiplication order."""
    return [Batch(_params(), [Locus(ref, [[(A_, q)] * k + [(T_, q)] * k], "k %d q %r" % (k, q))
                              for k in (1, 15, 64) for q in (None, 30) for ref in (A_, G_)])]


F6_COUNTS = (1, 63, 64, 65, 4096)
F6_MANY, F6_ALT = 30000, 13000


def family6():
    """Sums: B equal barcodes in a locus (one through the general path, one through the table), 30,000 one-fragment barcodes (parts,
    512 threads), and 13,000 merged one-fragment barcodes, every other one T: the table route of the major other allele."""
    general, table = [(A_, 30), (A_, 30), (T_, None)], [(A_, None), (A_, 30)]
    loci = [Locus(A_, [list(bc) for _ in range(B)], "B %d" % B) for B in F6_COUNTS for bc in (general, table)]
    loci.append(Locus(A_, [[(A_, None)] for _ in range(F6_MANY)], "B %d" % F6_MANY))
    loci.append(Locus(A_, [[(T_ if u & 1 else A_, 30)] for u in range(F6_ALT)], "B %d, half T" % F6_ALT))
    return [Batch(_params(mtDepth=20000), loci)]


def simple_to_for(min_bq):
    """The host's rule (csrc/host_abi.inc, simple_to_for) restated: the fragment count from which a one-allele barcode leaves the
    per-count table for the general path, because rightP >= (1 - max(0.1, 10^(-minBQ/10)))^nf may be below 2^-1000 from there on."""
    e = max(0.1, 10.0 ** (-0.1 * max(0, min_bq)))
    if not e < 1.0:
        return 1
    return int(min(4096.0, max(1.0, math.floor(1000.0 * math.log(2.0) / -math.log1p(-e)) - 1.0)))


F7_SIZES = {3: (600, 940, 1050, 1200, 2000), 6: (2290, 2500)}      # merged fragments at quality minBQ, on both sides of simple_to_for
F7_EXPECT = ((False, False, True, True, True, False, True, True), (False, True, False, True))


def family7():
    """Underflow.  Merged Q3 fragments at minBQ 3 (rightP = 0.4988^nf: 2^-602, 2^-943, 2^-1054, 2^-1204, 2^-2007 - the table gives
    way at 995 fragments), one-allele barcodes of the reference and of another allele, and 7,000 lone reads (0.9^7000 = 2^-1064); merged
    Q6 fragments at minBQ 6 (0.7488^nf: 2^-956, 2^-1043; the table gives way at 2,395)."""
    out = []
    for min_bq, sizes in sorted(F7_SIZES.items()):
        loci = [Locus(A_, [[(A_, min_bq)] * nf], "nf %d Q%d" % (nf, min_bq)) for nf in sizes]
        if min_bq == 3:
            loci.append(Locus(A_, [[(T_, 3)] * 940], "T nf 940 Q3"))
            loci.append(Locus(A_, [[(T_, 3)] * 1200], "T nf 1200 Q3"))
            loci.append(Locus(G_, [[(G_, None)] * 7000], "nf 7000 lone"))
        else:
            loci += [Locus(C_, [[(T_, 6)] * nf], "T nf %d Q6" % nf) for nf in sizes]
        out.append(Batch(_params(minBQ=min_bq), loci))
    return out


_FAMILIES = {}


def family(n):
    if n not in _FAMILIES:
        _FAMILIES[n] = (family1, family2, family3, family4, family5, family6, family7)[n - 1]()
    return _FAMILIES[n]


# ---- a locus's exact row, and the check of computed rows against it ----------------------------------------------------------------

class LocusExact(object):
    __slots__ = ("pi", "bound1", "fx", "umt", "vsm", "firm", "underflow", "fxshift", "min_x")


def locus_exact(L, P, K_=K):
    """PI per key (floats of the exact sums), its bound split as bound = K_ * bound1 + fx (the rounding of the fixed-point terms is
    not K's), consensus counts, whether every barcode's consensus is firm, whether a barcode underflows."""
    R = LocusExact()
    groups = Counter(canonical(bc) for bc in L.barcodes)
    R.fxshift = fxshift_for(len(L.barcodes), P.ds)
    assert len(L.barcodes) <= P.ds
    pi, b1, n_terms = {}, {}, {}
    R.umt, R.vsm, R.firm, R.underflow, R.min_x = Counter(), Counter(), True, False, math.inf
    for g, c in groups.items():
        frags = [(a, None if q < 0 else q) for (a, q), m in g for _ in range(m)]
        E = exact(frags, P.mtDrop, P.smt)
        R.underflow |= E.underflow
        R.firm &= firm(E, K_)
        R.min_x = min(R.min_x, min(E.x_f.values()))
        for k in E.keys:
            pi[k] = pi.get(k, 0) + c * E.pred[k]
            b1[k] = b1.get(k, 0.0) + c * key_bound(E, k, 1, None)
            n_terms[k] = n_terms.get(k, 0) + c
        if E.cons is not None:
            R.umt[E.cons] += c
            if E.top is not None and E.strong:
                R.vsm[E.cons] += c
    R.pi = {k: float(v) for k, v in pi.items()}
    R.bound1 = b1
    R.fx = {k: n_terms[k] * 2.0 ** -(R.fxshift + 1) for k in pi}
    return R


def check_rows(label, rows, batch, K_=K, expect_underflow=None, sum_slack=False):
    """Hold computed rows against the exact ones: pi[0..3] and cand[0].pi within the bound, status ST_OK (or ST_UNDERFLOW exactly where
    `expect_underflow` says - such rows are asked nothing else), cand[0] the best allele other than the reference, umt / vsm as the
    reference decides wherever it alone decides.  `sum_slack`: the rows come from a restatement that adds a locus's barcodes as doubles,
    one after the other: half an ulp of the total per term is allowed on top (never for the kernel, whose sums are integers).  The
    allowance enters the K = 1 ratio too: the measurement of K is of the per-barcode arithmetic and leaves the accumulation error of
    summed loci out (their ratios, 0.16 and 0.79, are far from the worst, which comes from loci of one barcode, where it is zero).
    -> (worst error / bound, worst error / bound(K = 1), where, loci excused from the consensus check); AssertionError with the figures."""
    from smcounter_amd import abi
    P = batch.params
    assert len(rows) == len(batch.loci)
    bad, worst, worst1, at, excused = [], 0.0, 0.0, None, 0
    for l, (L, row) in enumerate(zip(batch.loci, rows)):
        X = locus_exact(L, P, K_)
        st = int(row["status"])
        if expect_underflow is not None:
            assert X.underflow == expect_underflow[l], (label, L.note)
            if bool(st & abi.ST_UNDERFLOW) != X.underflow or (st & ~abi.ST_UNDERFLOW) != abi.ST_OK:
                bad.append((L.note, "status", st, "underflow expected: %r" % X.underflow))
            if X.underflow:
                continue
        elif st != abi.ST_OK:
            bad.append((L.note, "status", st))

        def hold(what, got, k):
            nonlocal worst, worst1, at
            if k not in X.pi:
                if got != 0.0:
                    bad.append((L.note, what, got, "not a key"))
                return
            slack = len(L.barcodes) * 0.5 * math.ulp(X.pi[k]) if sum_slack and len(L.barcodes) > 1 else 0.0
            err = abs(got - X.pi[k])
            r, r1 = err / (K_ * X.bound1[k] + X.fx[k] + slack), err / (X.bound1[k] + X.fx[k] + slack)
            if r > worst:
                worst, worst1, at = r, r1, (L.note, what)
            if not r <= 1.0:
                bad.append((L.note, what, got, X.pi[k], "error / bound = %.3g" % r))
        for k in range(4):
            hold("pi[%d]" % k, float(row["pi"][k]), k)
        C = row["cand"][0]
        ca = int(C["allele"])
        others = sorted((k for k in X.pi if k != L.ref), key=lambda k: X.pi[k], reverse=True)
        if ca not in others:
            bad.append((L.note, "cand[0].allele", ca, others))
        else:
            hold("cand[0].pi", float(C["pi"]), ca)
            tot = lambda k: K_ * X.bound1[k] + X.fx[k]
            if len(others) > 1 and X.pi[others[0]] - X.pi[others[1]] > tot(others[0]) + tot(others[1]) and ca != others[0]:
                bad.append((L.note, "cand[0].allele", ca, "the best other allele is %d" % others[0]))
        if not X.firm:
            excused += 1
            if int(row["umt"].sum()) > len(L.barcodes):
                bad.append((L.note, "umt", row["umt"].tolist()))
            continue
        for f, want in (("umt", X.umt), ("vsm", X.vsm)):
            if [int(v) for v in row[f]] != [want[k] for k in range(4)]:
                bad.append((L.note, f, row[f].tolist(), dict(want)))
        if ca in others and (int(C["vmt"]), int(C["vsm"])) != (X.umt[ca], X.vsm[ca]):
            bad.append((L.note, "cand[0].vmt / vsm", int(C["vmt"]), int(C["vsm"]), X.umt[ca], X.vsm[ca]))
    msg = "%s: worst error / bound %.3g (K = %d; / bound(K = 1): %.3g) at %r; %d of %d loci excused from the consensus check" % (
        label, worst, K_, worst1, at, excused, len(batch.loci))
    assert not bad, msg + "; %d off: %r" % (len(bad), bad[:6])
    return worst, worst1, at, excused


def min_x_of(n):
    return min(locus_exact(L, B.params).min_x for B in family(n) for L in B.loci)
