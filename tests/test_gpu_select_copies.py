"""smc_select_alignments_copies on the GPU: every selection of a batch (copies x fractions) against smc_select_alignments on that copy
with that seed and fraction, byte for byte - the kept records, their orig_index, all descriptors, the summary -, nothing written
anywhere else, two calls alike, the refusals, and devplanes.select_copies against devplanes.select_run.

The runs are hand-made records (the selection reads pos, end and bc_gid alone): 1, 1023, 1025 and 2500 alignments - one block short of
and just over its 1024 items, and three blocks -, alignments that start before start0 and end behind the last locus, and a run whose
positions within one block span more than the 4096 loci of the difference array's LDS window.  Every case is computed once, both ways,
and shared by the tests."""
import ctypes

import numpy as np
import pytest

from smcounter_amd import _lib, abi, devplanes
from smcounter_amd.engine import DevBuf

pytestmark = pytest.mark.gpu

E_INPUT = -4
POISON = 0xA5
FRACS = (1.0, 0.5, 1e-12)            # everything; about half; floor(f x 2^32) = 0: nothing
SEEDS = (11, 2 ** 63 + 5, 77)        # one per copy
# name: (alignments, loci, start0, the positions' range in loci)
CASES = {"one": (1, 40, 1000, 40), "short": (1023, 300, 5000, 300), "over": (1025, 300, 5000, 300), "three": (2500, 700, 123456, 700),
         "wide": (1500, 12000, 2000, 12000)}
MODES = ("strided", "shared")


def _records(name):
    n, nl, start0, span = CASES[name]
    rng = np.random.default_rng(n)
    a = np.zeros(n, abi.DEV_ALN_DTYPE)
    # (sorted by position, as the decoder leaves them; some start before start0, some end behind the last locus)
    a["pos"] = np.sort(rng.integers(start0 - 60, start0 + span + 30, n))
    a["end"] = a["pos"] + rng.integers(1, 150, n)
    n_bc = max(1, n // 3)
    a["bc_gid"] = rng.integers(0, n_bc, n)
    a["pair_gid"] = rng.integers(0, n, n)
    for f in ("cig_off", "seq_off", "n_cig", "oflag", "mapq", "left_sp", "qalen", "l_seq"):
        a[f] = rng.integers(0, 200, n)
    if name != "one":
        assert (a["pos"] < start0).any() and (a["end"] > start0 + nl).any()
    if name == "wide":
        assert int(a["pos"][1023]) - int(a["pos"][0]) > 4096
    idents = devplanes.fnv64_array(["bc%d" % g for g in range(n_bc)])
    return a, idents, nl, start0


def _copies(a, mode):
    """The three copies' records and their byte stride: with a stride every copy has seq_off of its own (a field the selection does
    not read: a selection made of the wrong copy shows in the bytes)."""
    if mode == "shared":
        return [a, a, a], 0
    cs = []
    for c in range(3):
        b = a.copy()
        b["seq_off"] = a["seq_off"] + 100000 * (c + 1)
        cs.append(b)
    return cs, (36 * len(a) + 255) & ~255


class _Out(object):
    """Poisoned outputs of `n_sel` selections, with a guard stretch behind each array."""
    GUARD = 512

    def __init__(self, eng, n_sel, n, nl):
        self.sizes = (36 * n * n_sel, 4 * n * n_sel, 16 * nl * n_sel, 16 * n_sel)
        self.bufs = [DevBuf(eng, s + self.GUARD).upload(np.full(s + self.GUARD, POISON, np.uint8)) for s in self.sizes]

    def ptrs(self):
        return [b.data_ptr() for b in self.bufs]

    def take(self):
        got = [b.download(np.uint8, s + self.GUARD) for b, s in zip(self.bufs, self.sizes)]
        for b in self.bufs:
            b.free()
        return got


def _single(eng, d_aln, n, nl, start0, d_id, n_ids, seed, frac):
    out = _Out(eng, 1, n, nl)
    _lib.check(eng.L.smc_select_alignments(eng.ctx, d_aln, n, None, nl, start0, None, d_id, n_ids, ctypes.c_uint64(seed), float(frac), *out.ptrs(),
                                           None), "smc_select_alignments")
    return out.take()


def _batch(eng, d_aln, stride, n_copies, n, nl, start0, d_id, n_ids, seeds, fracs):
    out = _Out(eng, n_copies * len(fracs), n, nl)
    s = np.array(seeds, np.uint64)
    f = np.array(fracs, np.float64)
    _lib.check(eng.L.smc_select_alignments_copies(eng.ctx, d_aln, stride, n_copies, n, None, nl, start0, d_id, n_ids, s.ctypes.data, f.ctypes.data,
                                                  len(f), *out.ptrs(), None), "smc_select_alignments_copies")
    return out.take()


_DONE = {}


def _results(eng, name, mode):
    """-> dict(single: {(f, c): the four arrays of the single call}, batch, again: the four arrays of two batched calls, n, nl)."""
    if (name, mode) in _DONE:
        return _DONE[name, mode]
    a, idents, nl, start0 = _records(name)
    cs, stride = _copies(a, mode)
    n = len(a)
    flat = np.zeros(max(stride, 36 * n) * 3 + 256, np.uint8)
    for c, b in enumerate(cs):
        flat[c * stride:c * stride + 36 * n] = b.view(np.uint8)
    d_aln = DevBuf(eng, len(flat)).upload(flat)
    d_id = DevBuf(eng, 8 * len(idents) + 256).upload(idents)
    args = (n, nl, start0, d_id.data_ptr(), len(idents))
    single = {(f, c): _single(eng, d_aln.data_ptr() + c * stride, *args, SEEDS[c], FRACS[f]) for f in range(len(FRACS)) for c in range(3)}
    batch = _batch(eng, d_aln.data_ptr(), stride, 3, *args, SEEDS, FRACS)
    again = _batch(eng, d_aln.data_ptr(), stride, 3, *args, SEEDS, FRACS)
    d_aln.free(); d_id.free()
    _DONE[name, mode] = dict(single=single, batch=batch, again=again, n=n, nl=nl, copies=cs)
    return _DONE[name, mode]


def _kept(summary_bytes, s=0):
    return summary_bytes[16 * s:16 * s + 12].view(np.uint32)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_every_selection_is_the_single_calls(engine0, name, mode):
    r = _results(engine0, name, mode)
    n, nl = r["n"], r["nl"]
    aln, orig, loc, summ = r["batch"]
    for (f, c), (aln1, orig1, loc1, summ1) in r["single"].items():
        s = f * 3 + c
        what = "%s/%s fraction %g copy %d" % (name, mode, FRACS[f], c)
        kept = int(_kept(summ1)[0])
        assert _kept(summ, s).tobytes() == _kept(summ1).tobytes(), what
        assert aln[36 * n * s:36 * (n * s + kept)].tobytes() == aln1[:36 * kept].tobytes(), what
        assert orig[4 * n * s:4 * (n * s + kept)].tobytes() == orig1[:4 * kept].tobytes(), what
        assert loc[16 * nl * s:16 * nl * (s + 1)].tobytes() == loc1[:16 * nl].tobytes(), what
        # the cases are what they are meant to be: everything, a proper part (where there is more than one barcode), nothing
        if FRACS[f] == 1.0:
            assert kept == n
            assert aln1[:36 * n].tobytes() == r["copies"][c].tobytes()
        elif FRACS[f] == 0.5:
            assert n < 100 or 0 < kept < n
        else:
            assert kept == 0 and not loc1[:16 * nl].view(abi.DEV_LOCUS_DTYPE)["n"].any()
    if n > 100:
        halves = [aln[36 * n * (3 + c):36 * n * (3 + c) + 36 * int(_kept(summ, 3 + c)[0])].tobytes() for c in range(3)]
        assert len(set(halves)) == 3                       # (three seeds - and with a stride three arrays -: three selections)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(CASES))
def test_nothing_is_written_elsewhere_and_two_calls_agree(engine0, name, mode):
    r = _results(engine0, name, mode)
    n, nl = r["n"], r["nl"]
    aln, orig, loc, summ = r["batch"]
    for s in range(9):
        kept = int(_kept(summ, s)[0])
        assert (aln[36 * (n * s + kept):36 * n * (s + 1)] == POISON).all()
        assert (orig[4 * (n * s + kept):4 * n * (s + 1)] == POISON).all()
        assert (summ[16 * s + 12:16 * (s + 1)] == POISON).all()          # (the fourth word is the caller's)
    for got, size in zip(r["batch"], (36 * n * 9, 4 * n * 9, 16 * nl * 9, 16 * 9)):
        assert len(got) == size + _Out.GUARD and (got[size:] == POISON).all()
    for x, y in zip(r["batch"], r["again"]):
        assert x.tobytes() == y.tobytes()


def test_refusals_launch_nothing(engine0):
    eng = engine0
    a, idents, nl, start0 = _records("short")
    n = len(a)
    d_aln = DevBuf(eng, 36 * n + 256).upload(a.view(np.uint8))
    d_id = DevBuf(eng, 8 * len(idents) + 256).upload(idents)
    out = _Out(eng, 4, n, nl)
    seeds = np.arange(2048, dtype=np.uint64)
    fr = np.full(2049, 0.5, np.float64)

    def call(n_copies=2, n_fracs=2, stride=0, fracs=fr, outs=None):
        p = outs if outs is not None else out.ptrs()
        return eng.L.smc_select_alignments_copies(eng.ctx, d_aln.data_ptr(), stride, n_copies, n, None, nl, start0, d_id.data_ptr(), len(idents),
                                                  seeds.ctypes.data, fracs.ctypes.data, n_fracs, *p, None)
    bad = [dict(n_copies=0), dict(n_fracs=0), dict(n_copies=-1), dict(n_copies=2048, n_fracs=2), dict(n_copies=1, n_fracs=2049),
           dict(fracs=np.array([0.5, 0.0])), dict(fracs=np.array([1.5, 0.5])), dict(fracs=np.array([0.5, -0.25])),
           dict(fracs=np.array([np.nan, 0.5])), dict(stride=-36), dict(stride=36 * n + 2)]
    for k in range(4):
        p = out.ptrs()
        p[k] = None
        bad.append(dict(outs=p))
    for kw in bad:
        assert call(**kw) == E_INPUT, kw
        assert b"smc_select_alignments_copies" in eng.L.smc_last_error()
    got = out.take()
    assert all((g == POISON).all() for g in got)           # (take() synchronises: nothing was launched)
    d_aln.free(); d_id.free()


def test_select_copies_gives_select_runs_selections(engine0):
    """The wrapper over copies at a stride (as _SpikedCopies lays them out): views, counts - with the gather of a run that has status
    bit 0 - and one summary table."""
    eng = engine0
    a, idents, nl, start0 = _records("three")
    cs, stride = _copies(a, "strided")
    n = len(a)
    flat = np.zeros(stride * 3, np.uint8)
    for c, b in enumerate(cs):
        flat[c * stride:c * stride + 36 * n] = b.view(np.uint8)
    d_aln = DevBuf(eng, len(flat) + 256).upload(flat)
    A = dict(nl=nl, n_bc=len(idents), n_pair=n, status=1, aln=a, n_slots=0)
    d_loc = DevBuf(eng, 16 * nl + 256)                    # (the input windows: handed on, never read)
    runs = [devplanes.RunOnDevice(devplanes._BufView(d_aln, c * stride), None, None, d_loc, None, n, None) for c in range(3)]
    fracs = [0.5, 0.25]
    sels = devplanes.select_copies(eng, runs, A, start0, idents, SEEDS, fracs)
    assert sels.summary.shape == (2, 3, 3)
    for f, frac in enumerate(fracs):
        for c in range(3):
            sel, counts, d_orig = sels.of[f][c]
            one, counts1, d_orig1 = devplanes.select_run(eng, runs[c], A, start0, idents=idents, frac=frac, seed=SEEDS[c])
            k = one.n_aln
            assert sel.n_aln == k and 0 < k < n and tuple(sels.summary[f, c]) == (k, counts1["deepest"], counts1["n_slots"])
            assert {x: counts[x] for x in counts if x != "aln"} == {x: counts1[x] for x in counts1 if x != "aln"}
            assert counts["aln"].tobytes() == counts1["aln"].tobytes() and len(counts["aln"]) == k
            assert sel.aln.download(np.uint8, 36 * k).tobytes() == one.aln.download(np.uint8, 36 * k).tobytes()
            assert d_orig.download(np.uint32, k).tobytes() == d_orig1.download(np.uint32, k).tobytes()
            assert sel.loc.download(np.uint8, 16 * nl).tobytes() == one.loc.download(np.uint8, 16 * nl).tobytes()
            one.aln.free(); one.loc.free(); d_orig1.free()
        # (nested in the fraction: what 0.25 keeps of a copy, 0.5 keeps)
    for c in range(3):
        half = set(sels.of[0][c][2].download(np.uint32, sels.of[0][c][0].n_aln).tolist())
        quarter = set(sels.of[1][c][2].download(np.uint32, sels.of[1][c][0].n_aln).tolist())
        assert quarter < half
    sels.free()
    d_aln.free(); d_loc.free()
    with pytest.raises(ValueError):
        devplanes.select_copies(eng, runs, A, start0, idents, SEEDS[:2], fracs)
