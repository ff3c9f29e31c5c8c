"""smc_select_alignments_reads_copies on the GPU: every selection of a batch (copies x keep masks) against
smc_select_alignments_keyed at SMC_SEL_KEY_READ on that copy with that mask, byte for byte - the kept records with their renumbered
ids, their orig_index, all descriptors, three summary words -, nothing written anywhere else, two calls alike, the refusals, and
devplanes.select_copies_reads against devplanes.select_run(level="read", d_mask=...).

The runs are the hand-made shapes of test_gpu_select_copies.py: 1, 1023, 1025 and 2500 alignments - one block short of and just over
its 1024 items, and three blocks -, alignments that start before start0 and end behind the last locus, and a run whose positions
within one block span more than the 4096 loci of the difference array's LDS window.  Here a read name belongs to one barcode and a
barcode has several names, so that a selection can drop a barcode's first read and keep a later one.  Every case is computed once,
both ways, and shared by the tests."""
import numpy as np
import pytest

from smcounter_amd import _lib, abi, devplanes
from smcounter_amd.engine import DevBuf

pytestmark = pytest.mark.gpu

E_INPUT = -4
POISON = 0xA5
N_COPIES = 3
N_MASKS = 3                          # all ones; about half the read names, drawn per copy; all zeros
# name: (alignments, loci, start0, the positions' range in loci)
CASES = {"one": (1, 40, 1000, 40), "short": (1023, 300, 5000, 300), "over": (1025, 300, 5000, 300), "three": (2500, 700, 123456, 700),
         "wide": (1500, 12000, 2000, 12000)}
# strided: every copy its own records and masks; shared: one record array (stride 0); shared_masks: one mask set (copy stride 0);
# short_ids: n_ids below n_pair - the read names at or beyond it are dropped whatever the masks say
VARIANTS = ("strided", "shared", "shared_masks", "short_ids")


def _records(name):
    n, nl, start0, span = CASES[name]
    rng = np.random.default_rng(n + 7)
    a = np.zeros(n, abi.DEV_ALN_DTYPE)
    # (sorted by position, as the decoder leaves them; some start before start0, some end behind the last locus)
    a["pos"] = np.sort(rng.integers(start0 - 60, start0 + span + 30, n))
    a["end"] = a["pos"] + rng.integers(1, 150, n)
    n_pair = max(1, (n + 1) // 2)
    n_bc = max(1, n_pair // 4)
    bc_of = rng.integers(0, n_bc, n_pair)                 # a read name belongs to one barcode
    a["pair_gid"] = rng.integers(0, n_pair, n)
    a["bc_gid"] = bc_of[a["pair_gid"]]
    for f in ("cig_off", "seq_off", "n_cig", "oflag", "mapq", "left_sp", "qalen", "l_seq"):
        a[f] = rng.integers(0, 200, n)
    if name != "one":
        assert (a["pos"] < start0).any() and (a["end"] > start0 + nl).any()
    if name == "wide":
        assert int(a["pos"][1023]) - int(a["pos"][0]) > 4096
    return a, n_bc, n_pair, nl, start0


def _copies(a, variant):
    """The three copies' records and their byte stride: with a stride every copy has seq_off of its own (a field the selection does
    not read: a selection made of the wrong copy shows in the bytes)."""
    if variant == "shared":
        return [a, a, a], 0
    cs = []
    for c in range(N_COPIES):
        b = a.copy()
        b["seq_off"] = a["seq_off"] + 100000 * (c + 1)
        cs.append(b)
    return cs, (36 * len(a) + 255) & ~255


def _masks(n_pair, variant, seed):
    """-> (bool [copies, masks, n_pair], uint32 words of the whole buffer, words per mask, copy stride in words).  A mask has a word
    more than it needs and the copies' sets a gap between them: neither stride is the tight one."""
    rng = np.random.default_rng(seed)
    mw = (n_pair + 31) // 32 + 1
    keep = np.zeros((N_COPIES, N_MASKS, n_pair), bool)
    keep[:, 0] = True
    for c in range(N_COPIES):
        keep[c, 1] = rng.random(n_pair) < 0.5
    if variant == "shared_masks":
        keep[:] = keep[0]
        cstride = 0
    else:
        cstride = N_MASKS * mw + 5
    words = np.full((N_COPIES - 1) * cstride + N_MASKS * mw + 8, 0xFFFFFFFF, np.uint32)    # (bits beyond n_pair are set: never read)
    for c in range(N_COPIES if cstride else 1):
        for m in range(N_MASKS):
            bits = np.ones(32 * mw, bool)
            bits[:n_pair] = keep[c, m]
            words[c * cstride + m * mw:c * cstride + (m + 1) * mw] = np.packbits(bits, bitorder="little").view(np.uint32)
    return keep, words, mw, cstride


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


def _single(eng, d_aln, n, nl, start0, n_bc, n_pair, d_mask, n_ids):
    out = _Out(eng, 1, n, nl)
    _lib.check(eng.L.smc_select_alignments_keyed(eng.ctx, d_aln, n, None, nl, start0, 1, n_bc, n_pair, d_mask, None, n_ids, 0, 1.0, *out.ptrs(), None),
               "smc_select_alignments_keyed")
    return out.take()


def _batch(eng, d_aln, stride, n, nl, start0, n_bc, n_pair, d_masks, mw, cstride, n_ids):
    out = _Out(eng, N_COPIES * N_MASKS, n, nl)
    _lib.check(eng.L.smc_select_alignments_reads_copies(eng.ctx, d_aln, stride, N_COPIES, n, None, nl, start0, n_bc, n_pair, d_masks, mw, cstride,
                                                        N_MASKS, n_ids, *out.ptrs(), None), "smc_select_alignments_reads_copies")
    return out.take()


def _first_read_dropped(a, keep_names):
    """Whether some barcode's first alignment is dropped while a later one of it is kept (what the renumbering exists for)."""
    kept = keep_names[a["pair_gid"]]
    _, first = np.unique(a["bc_gid"], return_index=True)
    dropped_first = set(a["bc_gid"][first[~kept[first]]].tolist())
    return bool(dropped_first & set(a["bc_gid"][kept].tolist()))


_DONE = {}


def _results(eng, name, variant):
    """-> dict(single: {(m, c): the four arrays of the single call}, batch, again: the four arrays of two batched calls, ...)."""
    if (name, variant) in _DONE:
        return _DONE[name, variant]
    a, n_bc, n_pair, nl, start0 = _records(name)
    cs, stride = _copies(a, variant)
    n = len(a)
    keep, words, mw, cstride = _masks(n_pair, variant, n)
    n_ids = n_pair // 2 if variant == "short_ids" else n_pair
    flat = np.zeros(max(stride, 36 * n) * N_COPIES + 256, np.uint8)
    for c, b in enumerate(cs):
        flat[c * stride:c * stride + 36 * n] = b.view(np.uint8)
    d_aln = DevBuf(eng, len(flat)).upload(flat)
    d_masks = DevBuf(eng, words.nbytes + 256).upload(words)
    single = {(m, c): _single(eng, d_aln.data_ptr() + c * stride, n, nl, start0, n_bc, n_pair,
                              d_masks.data_ptr() + 4 * (c * cstride + m * mw), n_ids) for m in range(N_MASKS) for c in range(N_COPIES)}
    args = (d_aln.data_ptr(), stride, n, nl, start0, n_bc, n_pair, d_masks.data_ptr(), mw, cstride, n_ids)
    batch = _batch(eng, *args)
    again = _batch(eng, *args)
    d_aln.free(); d_masks.free()
    keep = keep.copy()
    keep[:, :, n_ids:] = False
    if n > 100:
        assert any(_first_read_dropped(a, keep[c, 1]) for c in range(N_COPIES))
    _DONE[name, variant] = dict(single=single, batch=batch, again=again, n=n, nl=nl, copies=cs, keep=keep, n_ids=n_ids, n_pair=n_pair)
    return _DONE[name, variant]


def _kept(summary_bytes, s=0):
    return summary_bytes[16 * s:16 * s + 12].view(np.uint32)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_every_selection_is_the_single_calls(engine0, name, variant):
    r = _results(engine0, name, variant)
    n, nl = r["n"], r["nl"]
    aln, orig, loc, summ = r["batch"]
    for (m, c), (aln1, orig1, loc1, summ1) in r["single"].items():
        s = m * N_COPIES + c
        what = "%s/%s mask %d copy %d" % (name, variant, m, c)
        kept = int(_kept(summ1)[0])
        src = r["copies"][c]
        assert kept == int(r["keep"][c, m][src["pair_gid"]].sum()), what             # (the single call keeps what the mask says)
        assert _kept(summ, s).tobytes() == _kept(summ1).tobytes(), what
        assert aln[36 * n * s:36 * (n * s + kept)].tobytes() == aln1[:36 * kept].tobytes(), what
        assert orig[4 * n * s:4 * (n * s + kept)].tobytes() == orig1[:4 * kept].tobytes(), what
        assert loc[16 * nl * s:16 * nl * (s + 1)].tobytes() == loc1[:16 * nl].tobytes(), what
        # the kept records are the copy's own, with ids dense from 0 by first kept appearance
        got = aln[36 * n * s:36 * (n * s + kept)].view(abi.DEV_ALN_DTYPE)
        idx = orig[4 * n * s:4 * (n * s + kept)].view(np.uint32)
        assert (got["seq_off"] == src["seq_off"][idx]).all() and (np.diff(idx.astype(np.int64)) > 0).all(), what
        for f in ("bc_gid", "pair_gid"):
            _, first, inv = np.unique(src[f][idx], return_index=True, return_inverse=True)
            assert (got[f] == np.argsort(np.argsort(first))[inv]).all(), what
        if m == 0 and r["n_ids"] == r["n_pair"]:
            assert kept == n
        elif m == 2:
            assert kept == 0 and not loc1[:16 * nl].view(abi.DEV_LOCUS_DTYPE)["n"].any()
    if n > 100 and variant != "shared_masks":
        halves = [orig[4 * n * (3 + c):4 * (n * (3 + c) + int(_kept(summ, 3 + c)[0]))].tobytes() for c in range(N_COPIES)]
        assert len(set(halves)) == N_COPIES                # (three masks: a selection made with another copy's mask shows)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("name", list(CASES))
def test_nothing_is_written_elsewhere_and_two_calls_agree(engine0, name, variant):
    r = _results(engine0, name, variant)
    n, nl = r["n"], r["nl"]
    aln, orig, loc, summ = r["batch"]
    S = N_COPIES * N_MASKS
    for s in range(S):
        kept = int(_kept(summ, s)[0])
        assert (aln[36 * (n * s + kept):36 * n * (s + 1)] == POISON).all()
        assert (orig[4 * (n * s + kept):4 * n * (s + 1)] == POISON).all()
        assert (summ[16 * s + 12:16 * (s + 1)] == POISON).all()          # (the fourth word is the caller's)
    for got, size in zip(r["batch"], (36 * n * S, 4 * n * S, 16 * nl * S, 16 * S)):
        assert len(got) == size + _Out.GUARD and (got[size:] == POISON).all()
    for x, y in zip(r["batch"], r["again"]):
        assert x.tobytes() == y.tobytes()


def test_refusals_launch_nothing(engine0):
    eng = engine0
    a, n_bc, n_pair, nl, start0 = _records("short")
    n = len(a)
    _, words, mw, cstride = _masks(n_pair, "strided", 1)
    d_aln = DevBuf(eng, 36 * n + 256).upload(a.view(np.uint8))
    d_masks = DevBuf(eng, words.nbytes + 256).upload(words)
    out = _Out(eng, 4, n, nl)

    def call(n_copies=2, n_masks=2, stride=0, masks=d_masks.data_ptr(), mask_words=mw, copy_stride=cstride, bc=n_bc, pair=n_pair, ids=n_pair,
             outs=None):
        p = outs if outs is not None else out.ptrs()
        return eng.L.smc_select_alignments_reads_copies(eng.ctx, d_aln.data_ptr(), stride, n_copies, n, None, nl, start0, bc, pair, masks,
                                                        mask_words, copy_stride, n_masks, ids, *p, None)
    bad = [dict(n_copies=0), dict(n_masks=0), dict(n_copies=-1), dict(n_masks=-3), dict(n_copies=2048, n_masks=2), dict(n_copies=1, n_masks=2049),
           dict(stride=-36), dict(stride=36 * n + 2), dict(copy_stride=-1), dict(mask_words=(n_pair + 31) // 32 - 1), dict(mask_words=0),
           dict(bc=-1), dict(pair=-1), dict(ids=-1), dict(masks=None)]
    for k in range(4):
        p = out.ptrs()
        p[k] = None
        bad.append(dict(outs=p))
    for kw in bad:
        assert call(**kw) == E_INPUT, kw
        assert b"smc_select_alignments_reads_copies" in eng.L.smc_last_error()
    got = out.take()
    assert all((g == POISON).all() for g in got)           # (take() synchronises: nothing was launched)
    d_aln.free(); d_masks.free()


def test_select_copies_reads_gives_select_runs_selections(engine0):
    """The wrapper over copies at a stride (as _SpikedCopies lays them out): views, counts - with the gather of a run that has status
    bit 0 - and one summary table."""
    eng = engine0
    a, n_bc, n_pair, nl, start0 = _records("three")
    cs, stride = _copies(a, "strided")
    n = len(a)
    keep, words, mw, cstride = _masks(n_pair, "strided", 3)
    flat = np.zeros(stride * N_COPIES, np.uint8)
    for c, b in enumerate(cs):
        flat[c * stride:c * stride + 36 * n] = b.view(np.uint8)
    d_aln = DevBuf(eng, len(flat) + 256).upload(flat)
    d_masks = DevBuf(eng, words.nbytes + 256).upload(words)
    A = dict(nl=nl, n_bc=n_bc, n_pair=n_pair, status=1, aln=a, n_slots=0)
    d_loc = DevBuf(eng, 16 * nl + 256)                    # (the input windows: handed on, never read)
    runs = [devplanes.RunOnDevice(devplanes._BufView(d_aln, c * stride), None, None, d_loc, None, n, None) for c in range(N_COPIES)]
    sels = devplanes.select_copies_reads(eng, runs, A, start0, d_masks.data_ptr(), mw, cstride, 2)
    assert sels.summary.shape == (2, N_COPIES, 3)
    for m in range(2):
        for c in range(N_COPIES):
            sel, counts, d_orig = sels.of[m][c]
            one, counts1, d_orig1 = devplanes.select_run(eng, runs[c], A, start0, level="read",
                                                         d_mask=d_masks.data_ptr() + 4 * (c * cstride + m * mw))
            k = one.n_aln
            assert k == int(keep[c, m][a["pair_gid"]].sum()) and (m == 0 or 0 < k < n)
            assert sel.n_aln == k and tuple(sels.summary[m, c]) == (k, counts1["deepest"], counts1["n_slots"])
            assert {x: counts[x] for x in counts if x != "aln"} == {x: counts1[x] for x in counts1 if x != "aln"}
            assert counts["aln"].tobytes() == counts1["aln"].tobytes() and len(counts["aln"]) == k
            assert sel.aln.download(np.uint8, 36 * k).tobytes() == one.aln.download(np.uint8, 36 * k).tobytes()
            assert d_orig.download(np.uint32, k).tobytes() == d_orig1.download(np.uint32, k).tobytes()
            assert sel.loc.download(np.uint8, 16 * nl).tobytes() == one.loc.download(np.uint8, 16 * nl).tobytes()
            one.aln.free(); one.loc.free(); d_orig1.free()
    sels.free()
    d_aln.free(); d_masks.free(); d_loc.free()
