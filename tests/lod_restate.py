"""The algorithm of csrc/k_lod.inc in plain Python floats: the direct-sum binomial CDF the kernel uses, through the tool's own `zeroin`
(tools.mt_depths_lod: R's R_zeroin2).  Pins the kernel's formulation on the CPU against the tool's scipy incomplete-beta CDF."""
import math

from smcounter_amd.tools import mt_depths_lod as tool

MT_DEPTHS = (450, 1000, 3612, 8000)


def pbinom(k: int, n: int, p: float) -> float:
    """P(X <= k), X ~ Binomial(n, p): the first k + 1 terms, each from the one before (lod_pbinom)."""
    if p <= 0.0:
        return 1.0
    if p >= 1.0:
        return 1.0 if k >= n else 0.0
    t = math.exp(n * math.log1p(-p))
    s = t
    r = p / (1.0 - p)
    for i in range(k):
        t = t * (n - i) / (i + 1) * r
        s += t
    return s


def find_root(depth: int, needed: int):
    """(root before rounding, passes of zeroin's loop as k_lod_table counts them) - 1.0 and 0 where no search is made."""
    if depth < 5:
        return 1.0, 0
    calls = [0]

    def f(p):
        calls[0] += 1
        return pbinom(needed - 1, depth, p) - 0.05
    f_lo, f_hi = f(0.0), f(1.0)
    if not (f_lo * f_hi <= 0):
        return 1.0, 0
    calls[0] = 0
    try:
        root = tool.zeroin(f, 0.0, 1.0, f_lo, f_hi, tool.EPSILON ** 0.25)
    except RuntimeError:
        return 1.0, 1001
    return root, calls[0] + 1          # (the pass that returns evaluates nothing)


def find_lod(depth: int, needed: int) -> float:
    return round(find_root(depth, needed)[0], 4)


def depths_checked(mt_depth: int, sparse_step: int):
    """Every depth 0 .. 2 x mtDepth for the two shallow settings, every `sparse_step`-th for the two deep ones."""
    return range(0, 2 * mt_depth + 1, 1 if mt_depth <= 1000 else sparse_step)
