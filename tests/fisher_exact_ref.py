"""Two-sided Fisher exact test in exact arithmetic - the reference the Fisher tests of csrc/k_filter_loci.inc and their CPU
restatement (oracle/smc_oracle.c) are held against.  Standard library only; nothing here is shared with either of them: no
log-factorial, no exp, no floating-point sum.

The hypergeometric weights of a table [[a, b], [c, d]] with margins n1 = a + b, n2 = c + d, n = a + c are the integers
w(k) = C(n1, k) C(n2, n - k), k = lo .. hi, and sum(w) = C(n1 + n2, n).  scipy.stats.fisher_exact's two-sided p-value is
sum(w(k) : w(k) <= w(a) (1 + 1e-7)) / C(n1 + n2, n), capped at 1 (the slack makes up for the rounding of ITS pmf).

  integer form   w walked from w(lo) by exact integer division, the sum checked against C(n1 + n2, n), p as a Fraction.
  deep form      where that is too slow (support length x total beyond DEEP_COST: big integers of a quarter of a million bits over
                 a hundred thousand steps): the ratios r(k) = w(k) / w(a) walked in both directions from the observed cell in `decimal` at
                 60 digits (a step rounds at 1e-60, the longest walk has 2^18 of them), anchored by the exact pmf of the observed
                 cell (the prime factorisation of its factorials, evaluated at 60 digits), and checked by sum(r) pmf(a) = 1.  tests/test_fisher_ref.py holds it against
                 the integer form.

A table's `report` also says whether the reference ALONE decides its answer (`usable`): the strict rule w(k) <= w(a) and the slack
rule w(k) 10^7 <= w(a) (10^7 + 1) give the same sum, and no weight that differs from w(a) lies within 1e-5 relative of it - an
implementation whose pmf is off by far less than that then includes the same cells whatever its rounding.  Exact ties (the
mirrored cell of a symmetric table) are usable: any slack at all includes them, none does not.

Run as a program it searches the gate-straddling pairs tests/test_gpu_fisher.py lists."""
from __future__ import annotations

import decimal
import math
import random
from fractions import Fraction

DEEP_COST = 2 * 10 ** 8          # support length x total above which the deep form is used (~ 0.1 s of big-integer walking)
TIE_GAP = 1e-5                   # a table is usable when no unequal weight is nearer to the observed one than this (relative)
_CTX = decimal.Context(prec=60, Emax=decimal.MAX_EMAX, Emin=decimal.MIN_EMIN)
_DEC_TIE = decimal.Decimal("1e-40")   # deep form: ratios this close to 1 are the observed weight itself (exact ties; rounding is 1e-54)


class Report(object):
    """oddsratio, p (float, the exact value correctly rounded), p_exact (Fraction, or Decimal in the deep form), p_slack (the same
    under the slack rule), gap (smallest relative distance of an unequal weight to the observed one; inf if there is none), usable,
    n_support, form ('margin', 'integer' or 'deep')."""
    __slots__ = ("table", "oddsratio", "p", "p_exact", "p_slack", "gap", "usable", "n_support", "form")

    def __repr__(self):
        return "Report(%r: or=%r p=%r gap=%.3g usable=%r %s)" % (self.table, self.oddsratio, self.p, self.gap, self.usable, self.form)


def oddsratio(a, b, c, d):
    """The sample odds ratio as scipy returns it: nan at a zero margin, inf when b * c == 0 (true division of the exact products)."""
    if a + b == 0 or c + d == 0 or a + c == 0 or b + d == 0:
        return math.nan
    return (a * d) / (b * c) if b * c else math.inf


_PRIMES = [2, 3]


def _primes_to(m):
    """the primes <= m (a sieve, kept and grown)"""
    if _PRIMES[-1] < m:
        top = max(m, 2 * _PRIMES[-1])
        sieve = bytearray([1]) * (top + 1)
        sieve[0:2] = b"\0\0"
        for q in range(2, math.isqrt(top) + 1):
            if sieve[q]:
                sieve[q * q::q] = bytes(len(range(q * q, top + 1, q)))
        _PRIMES[:] = [q for q in range(top + 1) if sieve[q]]
    return _PRIMES


def _legendre(m, q):
    """the exponent of the prime q in m!"""
    e = 0
    while m:
        m //= q
        e += m
    return e


def _prime_powers(plus, minus):
    """[(prime, exponent)] of prod(m! for m in plus) / prod(m! for m in minus), exponents != 0: integer arithmetic only"""
    out, top = [], max(plus + minus + (2,))
    for q in _primes_to(top):
        if q > top:
            break
        e = 0
        for m in plus:
            e += _legendre(m, q)
        for m in minus:
            e -= _legendre(m, q)
        if e:
            out.append((q, e))
    return out


def _tree_product(xs):
    while len(xs) > 1:
        xs = [xs[i] * xs[i + 1] for i in range(0, len(xs) - 1, 2)] + ([xs[-1]] if len(xs) & 1 else [])
    return xs[0] if xs else 1


def binom(m, k):
    """C(m, k) from its prime factorisation (math.comb multiplies k growing integers one after the other)"""
    if m < 3000:
        return math.comb(m, k)
    return _tree_product([q ** e for q, e in _prime_powers((m,), (k, m - k))])


def _integer_form(n1, n2, n, a):
    lo, hi = max(0, n - n2), min(n, n1)
    w = binom(n1, lo) * binom(n2, n - lo)
    ws = [w]
    for k in range(lo, hi):
        w, rem = divmod(w * ((n1 - k) * (n - k)), (k + 1) * (n2 - n + k + 1))
        assert rem == 0
        ws.append(w)
    total = sum(ws)
    assert total == binom(n1 + n2, n), "the weights do not add up to C(n1 + n2, n)"
    wo = ws[a - lo]
    top = wo * (10 ** 7 + 1) // 10 ** 7                  # (w integer: w 10^7 <= wo (10^7 + 1) is w <= the floor of the quotient)
    strict = sum(w for w in ws if w <= wo)
    slack = sum(w for w in ws if w <= top)
    below, above = [w for w in ws if w < wo], [w for w in ws if w > wo]
    dist = ([wo - max(below)] if below else []) + ([min(above) - wo] if above else [])
    gap = (min(dist) * 10 ** 30 // wo) / 1e30 if dist else math.inf
    return Fraction(strict, total), Fraction(slack, total), strict / total, gap, strict == slack


def _deep_form(n1, n2, n, a):
    lo, hi = max(0, n - n2), min(n, n1)
    D = decimal.Decimal
    mul, div, add = _CTX.multiply, _CTX.divide, _CTX.add
    # the exact pmf of the observed cell n1! n2! n! (N - n)! / (N! a! b! c! d!) from the prime factorisation of its nine factorials
    # (Legendre's formula: integers), evaluated at 60 digits - some 23,000 factors at 2^18, each rounded at 1e-60
    p_obs = D(1)
    for q, e in _prime_powers((n1, n2, n, n1 + n2 - n), (n1 + n2, a, n1 - a, n - a, n2 - n + a)):
        p_obs = mul(p_obs, _CTX.power(D(q), D(e)))
    one, slack_top = D(1), D(10 ** 7 + 1) / D(10 ** 7)
    total = strict = slack = one
    gap = None

    def take(r):
        nonlocal total, strict, slack, gap
        total = add(total, r)
        dr = abs(r - one)
        if dr <= _DEC_TIE:
            strict = add(strict, r)
            slack = add(slack, r)
            return
        if gap is None or dr < gap:
            gap = dr
        if r < one:
            strict = add(strict, r)
        if r <= slack_top:
            slack = add(slack, r)
    r = one
    for k in range(a, hi):                              # w(k + 1) / w(k) = (n1 - k)(n - k) / ((k + 1)(n2 - n + k + 1))
        r = div(mul(r, D((n1 - k) * (n - k))), D((k + 1) * (n2 - n + k + 1)))
        take(r)
    r = one
    for k in range(a, lo, -1):                          # w(k - 1) / w(k) = k (n2 - n + k) / ((n1 - k + 1)(n - k + 1))
        r = div(mul(r, D(k * (n2 - n + k))), D((n1 - k + 1) * (n - k + 1)))
        take(r)
    assert abs(mul(total, p_obs) - one) < D("1e-50"), "the weights do not add up to 1"
    p, ps = mul(strict, p_obs), mul(slack, p_obs)
    return p, ps, float(p), (float(gap) if gap is not None else math.inf), strict == slack


_CACHE = {}


def report(a, b, c, d, form=None):
    """The Report of the table [[a, b], [c, d]]; `form`: 'integer' / 'deep' to force one (the tests compare the two)."""
    key = (a, b, c, d, form)
    R = _CACHE.get(key)
    if R is not None:
        return R
    assert min(a, b, c, d) >= 0
    R = Report()
    R.table, R.oddsratio = (a, b, c, d), oddsratio(a, b, c, d)
    n1, n2, n = a + b, c + d, a + c
    if min(n, b + d) > min(n1, n2):                      # the transposed table has the same weights, out of smaller integers:
        n1, n2, n = a + c, b + d, a + b                   # C(N, n) with n the smallest of the four margins
    if math.isnan(R.oddsratio):
        R.p, R.p_exact, R.p_slack, R.gap, R.usable, R.n_support, R.form = 1.0, Fraction(1), Fraction(1), math.inf, True, 0, "margin"
    else:
        R.n_support = min(n, n1) - max(0, n - n2) + 1
        R.form = form or ("integer" if R.n_support * (n1 + n2) <= DEEP_COST else "deep")
        R.p_exact, R.p_slack, R.p, R.gap, same = (_integer_form if R.form == "integer" else _deep_form)(n1, n2, n, a)
        R.usable = same and R.gap >= TIE_GAP
    _CACHE[key] = R
    return R


def bound(a, b, c, d):
    """The relative bound a computed p-value is held to: an anchor pmf is made of nine log-factorials, each rounded at the magnitude
    of L = log((n1 + n2)!), a Stirling truncation below 1e-12, and a walk of multiplications each within an ulp."""
    return 16 * math.ulp(math.lgamma(a + b + c + d + 1.0)) + 1e-12


def rel_error(p, R):
    """|p - exact| / exact against the Report R, in float: the exact value is rounded once (1.1e-16, far below any bound)."""
    return abs(p - R.p) / R.p if R.p > 0 else (0.0 if p == 0 else math.inf)


TINY = 1e-290                    # below this the double range ends: a computed p is only asked to be tiny too (< 1e-280) and not NaN


def check_family(name, tables, oddsratios, pvalues, need_usable=None):
    """Hold computed (oddsratio, p) of `tables` against the reference: the odds ratio equal (nan / inf / the correctly rounded
    quotient - the products of the tests' tables are exact in double), p within `bound` relative on usable tables (below TINY: tiny,
    not NaN).  -> (worst rel / bound, its table, usable tables); AssertionError with the figures otherwise.  `need_usable`: the
    smallest share of the tables that must be usable."""
    worst, at, n_use, bad = 0.0, None, 0, []
    for t, o, p in zip(tables, oddsratios, pvalues):
        R = report(*t)
        o, p = float(o), float(p)
        same_or = (math.isnan(o) and math.isnan(R.oddsratio)) or o == R.oddsratio
        if not same_or:
            bad.append((t, "oddsratio", o, R.oddsratio))
        if not R.usable:
            continue
        n_use += 1
        if R.p < TINY:
            if not (0.0 <= p < 1e-280):
                bad.append((t, "p below the double range", p, R.p_exact))
            continue
        r = rel_error(p, R) / bound(*t)
        if r > worst:
            worst, at = r, t
        if not r <= 1.0:
            bad.append((t, "p", p, R.p, "rel / bound = %.3g" % r))
    msg = "%s: worst rel / bound %.3g at %r; %d of %d tables usable" % (name, worst, at, n_use, len(tables))
    assert not bad, msg + "; %d off: %r" % (len(bad), bad[:6])
    if need_usable is not None:
        assert n_use >= need_usable * len(tables), msg
    return worst, at, n_use


# ---- table families (shared by tests/test_fisher_ref.py and tests/test_gpu_fisher.py) -----------------------------------------

def small_tables(top=6):
    r = range(top + 1)
    return [(a, b, c, d) for a in r for b in r for c in r for d in r]


def support_tables():
    """Supports of length 1, 2, 63 .. 4097, each with lo == 0 and with lo > 0; the observed cell at lo, hi, the mode and at the
    first and last k of lanes' chunks (the kernel cuts the support into 64 chunks of ceil(length / 64): the last lanes' chunks are
    short or empty).  A support of ONE cell is a table with an empty column: (nan, 1)."""
    out = [(5, 0, 3, 0), (0, 41, 0, 7)]                      # length 1: lo == hi == 0 and lo == hi == n
    for length in (2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097):
        for lo in (0, 37):
            n = lo + length - 1                              # k = lo .. n
            n1 = n + (5 if lo else 0)
            n2 = n - lo if lo else n + 3
            chunk = (length + 63) // 64
            ks = {lo, n, min(max(((n + 1) * (n1 + 1)) // (n1 + n2 + 2), lo), n)}
            for lane in (0, 1, 31, 62, 63, (length - 1) // chunk):
                ks.update(k for k in (lo + chunk * lane, lo + chunk * lane + chunk - 1) if lo <= k <= n)
            out += [(k, n1 - k, n - k, n2 - n + k) for k in sorted(ks)]
    assert all(min(t) >= 0 for t in out)
    return out


def symmetric_tables():
    """(a, b, b, a): the mirrored cell k = b has exactly the observed weight - only the slack (or a `<=` that rounding happens to
    satisfy) puts the far tail into the sum."""
    out = []
    for q, firsts in ((10, (1, 2, 3, 4)), (1000, (499, 480, 450, 400)), (3000, (1490, 1450)), (30000, (14999, 14900, 14700, 14500))):
        out += [(a, q - a, q - a, a) for a in firsts]
    return out


def random_tables(top, count, seed):
    rng = random.Random(seed)
    return [tuple(rng.randint(0, top) for _ in range(4)) for _ in range(count)]


# (largest count, tables, seed): 2,000 tables; fewer of the large ones - the exact walk of one takes 20 ms
RANDOM_FAMILIES = ((12, 500, 1201), (70, 500, 1202), (130, 450, 1203), (700, 400, 1204), (5000, 150, 1205))


def deep_tables():
    """About 40 tables of 8,000 to 262,144 reads in the shapes of the filters: a reference row of thousands against an alternate row of
    5 to 500, balanced and one-sided strands, counts on both sides of 65536 (the end of the kernel's log-factorial table)."""
    out = []
    for ref in (8000, 30000, 65530, 65536, 131000, 250000):
        h = ref // 2
        out += [(h, ref - h, 3, 2), (h, ref - h, 0, 40), (h + ref // 8, ref - h - ref // 8, 140, 360), (ref - 7, 7, 5, 0),
                (ref - 300, 300, 30, 170)]
    out += [(65535, 65536, 200, 300), (65536, 65537, 1, 499), (65534, 2, 65536, 500), (65537, 65535, 65536, 65536),
            (4000, 4000, 3990, 4010), (60000, 71072, 65536, 65536), (131072, 0, 131000, 72), (100000, 31072, 31072, 100000),
            (65535, 1, 1, 65535), (20000, 45536, 45535, 20001)]
    return out


GATES = (1e-5, 1e-3)


def one_count_neighbours(t):
    for i in range(4):
        u = list(t)
        u[i] += 1
        yield tuple(u)


def find_straddlers(gate, bases, margin=1e-6):
    """Pairs (t, u) one count apart with p(t) >= gate > p(u), both at least `margin` relative away from it and usable, among the
    tables `bases` and their one-count neighbours."""
    out = []
    for t in bases:
        Rt = report(*t)
        if not (Rt.usable and Rt.p >= gate * (1 + margin)):
            continue
        for u in one_count_neighbours(t):
            Ru = report(*u)
            if Ru.usable and Ru.p < gate * (1 - margin):
                out.append((t, u))
    return out


def straddler_bases():
    """Where the search looks: one-sided alternates against balanced reference rows of tens, thousands and tens of thousands; the
    pure diagonal; odds ratios of exactly 50 and 1 / 50 ((50x, y, x, y): a d / (b c) = 50 x y / (x y)) and their neighbours."""
    bases = []
    for r in (12, 40, 2000, 5000, 30000, 70000):
        bases += [(r, r, 0, j) for j in range(5, 40)] + [(r, r + r // 3, j, 0) for j in range(5, 40)]
        bases += [(r, r, 1, j) for j in range(8, 40)]
    bases += [(k, 0, 0, m) for k in range(3, 30) for m in range(3, 14)]
    for x in (1, 2, 3, 5, 8):
        for y in range(1, 90):
            bases += [(50 * x, y, x, y), (x, y, 50 * x, y), (50 * x, y, x, y - 1), (x, y, 50 * x, y - 1)][:4 if y > 1 else 2]
    return bases


# Pairs the search above found (gate, then (p >= gate, p < gate) one count apart): supports of tens, thousands and tens of
# thousands, infinite and zero odds ratios, and odds ratios of 50, 1 / 50 and either side of them
STRADDLERS = {
    1e-5: [((10, 0, 0, 10), (11, 0, 0, 10)), ((10, 0, 0, 10), (10, 0, 0, 11)), ((9, 0, 0, 10), (9, 0, 0, 11)), ((23, 0, 0, 5), (24, 0, 0, 5)),
           ((16, 0, 0, 6), (17, 0, 0, 6)), ((7, 0, 0, 13), (7, 0, 0, 14)), ((12, 12, 0, 29), (12, 12, 0, 30)), ((12, 12, 0, 29), (13, 12, 0, 29)),
           ((12, 16, 20, 0), (12, 16, 21, 0)), ((12, 12, 1, 38), (12, 12, 1, 39)), ((40, 40, 0, 20), (40, 40, 0, 21)), ((40, 53, 15, 0), (40, 53, 16, 0)),
           ((40, 40, 1, 25), (41, 40, 1, 25)), ((2000, 2000, 0, 17), (2000, 2000, 0, 18)), ((2000, 2666, 13, 0), (2000, 2666, 14, 0)),
           ((2000, 2000, 1, 21), (2000, 2000, 1, 22)), ((5000, 5000, 1, 21), (5000, 5000, 1, 22)), ((30000, 30000, 0, 17), (30000, 30000, 0, 18)),
           ((30000, 40000, 13, 0), (30000, 40000, 14, 0)), ((70000, 70000, 1, 21), (70000, 70000, 1, 22)), ((70000, 93333, 13, 0), (70000, 93333, 14, 0)),
           ((50, 8, 1, 8), (50, 8, 1, 9)), ((1, 8, 50, 8), (1, 9, 50, 8)), ((50, 10, 1, 9), (50, 10, 1, 10)), ((100, 7, 2, 6), (100, 7, 2, 7)),
           ((2, 5, 100, 5), (2, 6, 100, 5)), ((150, 5, 3, 5), (150, 5, 3, 6)), ((3, 4, 150, 3), (3, 5, 150, 3)), ((400, 5, 8, 4), (400, 5, 8, 5)),
           ((8, 4, 400, 4), (8, 5, 400, 4))],
    1e-3: [((3, 0, 0, 10), (4, 0, 0, 10)), ((4, 0, 0, 9), (4, 0, 0, 10)), ((6, 0, 0, 6), (7, 0, 0, 6)), ((9, 0, 0, 4), (10, 0, 0, 4)),
           ((16, 0, 0, 3), (17, 0, 0, 3)), ((12, 12, 0, 14), (13, 12, 0, 14)), ((12, 12, 0, 14), (12, 12, 0, 15)), ((12, 16, 10, 0), (12, 16, 11, 0)),
           ((12, 12, 1, 19), (12, 12, 1, 20)), ((40, 40, 0, 11), (40, 40, 0, 12)), ((40, 53, 8, 0), (40, 53, 9, 0)), ((40, 40, 1, 15), (41, 40, 1, 15)),
           ((2000, 2000, 0, 10), (2000, 2000, 0, 11)), ((2000, 2666, 8, 0), (2000, 2666, 9, 0)), ((2000, 2000, 1, 13), (2000, 2000, 1, 14)),
           ((5000, 6666, 8, 0), (5000, 6666, 9, 0)), ((30000, 30000, 0, 10), (30000, 30000, 0, 11)), ((30000, 30000, 1, 13), (30000, 30000, 1, 14)),
           ((70000, 70000, 0, 10), (70000, 70000, 0, 11)), ((70000, 93333, 8, 0), (70000, 93333, 9, 0)), ((50, 3, 1, 3), (50, 3, 1, 4)),
           ((1, 3, 50, 3), (1, 4, 50, 3)), ((50, 5, 1, 4), (50, 5, 1, 5)), ((100, 2, 2, 2), (100, 2, 2, 3)), ((2, 2, 100, 1), (2, 3, 100, 1)),
           ((100, 4, 2, 3), (100, 4, 2, 4)), ((150, 3, 3, 2), (150, 3, 3, 3)), ((5, 2, 250, 2), (5, 3, 250, 2)), ((400, 3, 8, 2), (400, 3, 8, 3)),
           ((8, 2, 400, 1), (8, 3, 400, 1))],
}
# a dozen strand-bias tables of the 1e-5 list for the pipeline (reference reverse / forward, alternate reverse / forward): both sides of
# the gate, with the odds ratio beyond 50 (or 1 / 50), exactly there, and short of it
SB_PIPELINE = [(10, 0, 0, 10), (11, 0, 0, 10), (12, 12, 0, 29), (12, 12, 0, 30), (40, 53, 15, 0), (40, 53, 16, 0), (50, 8, 1, 8), (50, 8, 1, 9),
               (50, 10, 1, 9), (50, 10, 1, 10), (1, 8, 50, 8), (1, 9, 50, 8),
               (49, 10, 1, 10), (1, 10, 49, 10)]      # (and two below the gate whose odds ratio stays inside: 49 and 1 / 49)


def sb_pileup(tables):
    """One locus per table (a, b, c, d) in a PileupBatch: reference allele A with a reverse and b forward reads, alternate T with c
    and d, so that the strand-bias test of filterVariants sees exactly [[a, b], [c, d]].  Reads go in pairs - one fragment (number 0 of its own
    barcode) each, Q30 (a left-over read is a fragment of its own): the alternate has five barcodes or more and becomes the candidate.
    Where the alternate would be more than 55 % of the coverage (the test is made at af <= 60 only) reads of a third letter below
    minBQ are added: they count in the coverage and in nothing else."""
    import numpy as np
    from smcounter_amd import pileup
    per = {k: [] for k in ("umi", "frag", "flag", "allele", "bq")}
    off = [0]
    for (a, b, c, d) in tables:
        reads = [(pileup.A_, 1)] * a + [(pileup.A_, 0)] * b + [(pileup.T_, 1)] * c + [(pileup.T_, 0)] * d
        n_f = 0
        for al in (pileup.A_, pileup.T_):
            mine = [r for r in reads if r[0] == al]
            for i, (_, rev) in enumerate(mine):
                per["umi"].append(n_f + i // 2)
                per["frag"].append(0)
                per["flag"].append((pileup.F_READ2 if i & 1 else pileup.F_READ1) | (pileup.F_REVERSE if rev else 0))
                per["allele"].append(al)
                per["bq"].append(30)
            n_f += (len(mine) + 1) // 2
        pad = 0
        while 100 * (c + d) > 55 * (a + b + c + d + pad):
            pad += 1
        for i in range(pad):
            per["umi"].append(n_f + i)
            per["frag"].append(0)
            per["flag"].append(pileup.F_READ1)
            per["allele"].append(pileup.G_)
            per["bq"].append(5)
        off.append(len(per["umi"]))
    n, nl = off[-1], len(tables)
    z = lambda dt, v=0: np.full(n, v, dt)
    return pileup.PileupBatch(
        chrom=["c"] * nl, pos=np.arange(100, 100 + nl, dtype=np.int64), ref=["A"] * nl, alleles=[list(pileup.BASE_ALLELES) for _ in range(nl)],
        read_off=np.array(off, np.int64), umi=np.array(per["umi"], np.uint32), frag=np.array(per["frag"], np.uint32),
        flag=np.array(per["flag"], np.uint8), mq=z(np.uint8, 60), nm=z(np.uint32), n_indel=z(np.uint32), left_sp=z(np.uint32),
        qlen=z(np.uint32, 100), qalen=z(np.uint32, 100), qpos=z(np.int32, 50), indel=z(np.int32), is_del=z(bool),
        allele=np.array(per["allele"], np.uint8), bq=np.array(per["bq"], np.uint8))


def sb_expected(t):
    """(exact p, SMC_F_SB expected) of a strand-bias table: smCounter.py:215-216"""
    R = report(*t)
    return R, R.p < 1e-5 and (R.oddsratio >= 50 or R.oddsratio <= 1.0 / 50)


if __name__ == "__main__":
    for g in GATES:
        pairs = find_straddlers(g, straddler_bases())
        print("# gate %g: %d pairs" % (g, len(pairs)))
        for t, u in pairs:
            print("    (%r, %r),   # %.6g  %.6g   or %.6g %.6g" % (t, u, report(*t).p, report(*u).p, report(*t).oddsratio, report(*u).oddsratio))
