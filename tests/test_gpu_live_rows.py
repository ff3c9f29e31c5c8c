"""The plane builder drops the window rows that cover none of a tile's loci (k_bp_sort_seg: an alignment that ends at or before the
tile's first position takes no part in the sort, the walks end the tile's list at its live rows - BpArgs.n_live, bp_wave).  Runs
made by hand - three tiles, spans between 1 and 150, half of the second and third tile's windows dead - through smc_build_planes /
smc_build_planes_w16 / the raw-field planes:
  * the rows of the locus kernels against the same alignments through oracle/aln_planes.c + oracle/smc_oracle.c;
  * byte for byte against the same build with the dead rows kept (SMC_BP_KEEP_DEAD_ROWS): words, umi_start, u_gid, u_finc, descriptors, extras
    (and the raw-field planes);
  * the live row counts the builder reports (smc_build_live_rows) against the definition: the window's alignments with end > the
    tile's first position where one workgroup sorts the tile's window, every window row elsewhere.
All with the builder's scratch poisoned (SMC_BP_POISON_SCRATCH): nothing may read a count or a state of a stretch the count walk has
not written this run."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, devplanes, synth
from smcounter_amd.engine import DevBuf
from smcounter_amd.params import VcParams

sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_gpu_build_listed import LOCUS, counts_of, make_run, read  # noqa: E402

import oracle_lib  # noqa: E402

pytestmark = pytest.mark.gpu
TILE, SUB, PART = 64, 64, 256          # loci per tile; rows per wavefront of the walk that writes; rows per wavefront of the count walk
SORT_LDS_MAX, LSORT_MAX = 6144, 16384  # window rows up to which the small / the large one-workgroup sort takes a tile
P = VcParams(minBQ=20, minMQ=0, mtDepth=4000, rpb=3.0, hpLen=8, mismatchThr=100.0, mtDrop=0, maxMT=0, primerDist=20)
NL = 192


@pytest.fixture(autouse=True)
def _switches(monkeypatch):
    monkeypatch.setenv("SMC_EXPERIMENTAL", "1")
    monkeypatch.setenv("SMC_BP_POISON_SCRATCH", str(0xA5))


# ---- the runs.  Read 1 (the anchor) covers offsets 0 .. 149 and is the second alignment of the file: the windows of tiles 1 and 2
# start at it, so tile 1's window is every later alignment with pos <= 127 and tile 2's every later alignment - a row is dead in
# tile 1 when it ends at or before offset 64, in tile 2 at or before 128.
def live_rows_run(n1, n2, seed, fill1=200, fill2=0, tail=0):
    """n1 / n2: live rows of tile 1 / tile 2 (before `tail`); fill1: one- to 60-base reads inside tile 0 (dead in tiles 1 and 2);
    fill2: short reads inside tile 1 (dead in tile 2); tail: one-base reads inside tile 2 (live there)."""
    rng = np.random.RandomState(seed)
    pool = ["P%02d" % k for k in range(24)]
    quiet = "P07"                                   # every row of this barcode is dead in tiles 1 and 2; P06 and P08 are live there

    def seq(n):
        return "".join("ACGT"[k] for k in rng.randint(0, 4, n))

    def plain(pos, span, bc, name, **kw):
        return read(pos, [(0, span)], seq(span), bc, name, qual=[int(q) for q in rng.randint(10, 41, span)], **kw)
    reads = [plain(0, 64, "Z", "z0"),               # barcode 0 of the run: outside the windows of tiles 1 and 2 ...
             plain(0, 150, "anchor", "a0")]
    reads.append(plain(5, 3, "Z", "z1"))            # ... and this row of it inside them, dead: the FIRST entry of their unfiltered lists
    for k, bc in enumerate(pool):                   # the pool's barcodes in order, each by a row that is dead in tiles 1 and 2
        reads.append(plain(6 + k, 1 + k % 40, bc, "i%d" % k, rev=bool(k & 1)))
    # general CIGARs: a dead one (a deletion; ends at 22) and, below, a live one (an insertion) in tile 1; a soft clip
    reads.append(read(10, [(0, 5), (2, 3), (0, 4)], seq(9), "P03", "gd", qual=31))
    reads.append(read(12, [(4, 2), (0, 6)], seq(8), "P04", "gs", qual=33))
    # a pair whose first mate is dead in tile 1 and whose second is live there
    reads.append(plain(40, 20, "P05", "pair"))
    reads.append(plain(70, 30, "P05", "pair", r2=True, rev=True))
    n_fixed_dead = len(reads)
    for k in range(max(0, fill1 - (n_fixed_dead - 2))):
        pos = int(rng.randint(31, 61))
        reads.append(plain(pos, int(rng.randint(1, 65 - pos)), pool[int(rng.randint(len(pool)))], "f%d" % int(rng.randint(0, 40)), r2=bool(rng.randint(2)),
                           rev=bool(rng.randint(2))))
    reads.append(plain(62, 2, "last", "l0"))        # the run's last barcode, dead in tiles 1 and 2: the LAST entry of their unfiltered lists
    busy = [b for b in pool if b != quiet]
    # tile 1's live rows: the anchor, the pair's second mate, the general CIGAR, P06 and P08, five rows that reach into tile 2, the rest
    t1 = [read(80, [(0, 10), (1, 2), (0, 20)], seq(32), "P09", "gl", qual=35),
          plain(66, 40, "P06", "n6"), plain(67, 7, "P08", "n8", r2=True)]
    cross = [plain(100 + 5 * k, 60 + k, busy[k], "x%d" % k, rev=bool(k & 1)) for k in range(5)]
    for k in range(n1 - 2 - len(t1) - len(cross)):
        pos = int(rng.randint(31, 127))
        lo_end = max(pos + 1, 65)
        end = int(rng.randint(lo_end, 129))
        t1.append(plain(pos, end - pos, busy[int(rng.randint(len(busy)))], "t%d" % int(rng.randint(0, 30)), r2=bool(rng.randint(2)), rev=bool(rng.randint(2))))
    mid = [plain(int(rng.randint(64, 121)), int(rng.randint(1, 8)), pool[int(rng.randint(len(pool)))], "m%d" % int(rng.randint(0, 60)), r2=bool(rng.randint(2)))
           for k in range(fill2)]
    t2 = []
    for k in range(n2 - 1 - len(cross)):
        pos = int(rng.randint(128, 192))
        t2.append(plain(pos, int(rng.choice([1, 2, 30, 100, 150])), busy[int(rng.randint(len(busy)))], "u%d" % int(rng.randint(0, 30)), r2=bool(rng.randint(2)),
                        rev=bool(rng.randint(2))))
    far = [plain(int(rng.randint(128, 192)), 1, busy[int(rng.randint(len(busy)))], "w%d" % int(rng.randint(0, 200)), r2=bool(rng.randint(2))) for k in range(tail)]
    A = make_run(reads + t1 + cross + mid + t2 + far, NL)
    A["seq"], A["qual"] = A["bq"][0::2], A["bq"][1::2]
    A["reads"] = int(A["loc"]["n"].sum())
    return A


def tile_lists(A):
    """Per tile: (the window's alignment indices in the sort's order, which of them are dead)."""
    aln, loc, out = A["aln"], A["loc"], []
    for t in range((A["nl"] + TILE - 1) // TILE):
        l0, l1 = t * TILE, min(A["nl"], (t + 1) * TILE) - 1
        w0, w1 = int(loc["w0"][l0]), max(int(loc["w0"][l0]), int(loc["w1"][l1]))
        idx = np.arange(w0, w1)
        order = idx[np.lexsort((idx, aln["pair_gid"][idx], aln["bc_gid"][idx]))]
        out.append((order, aln["end"][order] <= A["start0"] + l0))
    return out


def expected_live(A, filtered=True, seg_tiles=1):
    return [int((~dead).sum()) if filtered and seg_tiles == 1 and len(order) <= LSORT_MAX else len(order) for order, dead in tile_lists(A)]


# ---- one build of the run in HBM -> host arrays, the rows of the locus kernels, the live row counts
def build(eng, up, A, mode):
    """mode: 16 / 32 (read words alone) / "raw" (32-bit words and the four raw-field planes)."""
    cnt, lo = counts_of(A), A["start0"]
    nl, ns = cnt["nl"], cnt["n_slots"]
    cp = abi.c_params(P)
    nu = ns + nl + 64
    d_w, d_us, d_g, d_f = DevBuf(eng, 4 * ns + 256), DevBuf(eng, 4 * nu), DevBuf(eng, 4 * nu), DevBuf(eng, 4 * nu)
    raw = [DevBuf(eng, 4 * ns + 256) for _ in range(4)] if mode == "raw" else []
    xcap = devplanes.build_xcap(nl)
    d_l, d_x, d_c = DevBuf(eng, 32 * nl), DevBuf(eng, 20 * xcap), DevBuf(eng, 8)
    bufs = [d_w, d_us, d_g, d_f, d_l, d_x, d_c] + raw
    for b in bufs[:4] + raw:                                                    # (what no build writes is the same bytes in both arms)
        b.upload(np.zeros(b.nbytes, np.uint8))
    bi = abi.SmcBuildIn(up.aln.data_ptr(), up.cig.data_ptr(), up.bq.data_ptr(), up.loc.data_ptr(), up.ref.data_ptr(), lo, nl, cnt["n_bc"], cnt["n_pair"],
                        cnt["deepest"], up.n_aln, A["loc"].ctypes.data)
    try:
        if mode == 16:
            _lib.check(eng.L.smc_build_planes_w16(eng.ctx, ctypes.byref(cp), ctypes.byref(bi), 0, 0, d_w.data_ptr(), d_us.data_ptr(), d_g.data_ptr(),
                                                  d_f.data_ptr(), d_l.data_ptr(), d_x.data_ptr(), xcap, d_c.data_ptr(), None), "smc_build_planes_w16")
            d_w.word_bits = 16
        else:
            rp = [b.data_ptr() for b in raw] if raw else [None] * 4
            _lib.check(eng.L.smc_build_planes(eng.ctx, ctypes.byref(cp), ctypes.byref(bi), 0, 0, d_w.data_ptr(), rp[0], rp[1], rp[2], rp[3], d_us.data_ptr(),
                                              d_g.data_ptr(), d_f.data_ptr(), d_l.data_ptr(), d_x.data_ptr(), xcap, d_c.data_ptr(), None), "smc_build_planes")
        c = d_c.download(np.uint32, 2)
        assert int(c[0]) <= xcap and int(c[1]) == 0, c
        live, n_lists = np.zeros(64, np.uint32), ctypes.c_int32()
        _lib.check(eng.L.smc_build_live_rows(eng.ctx, live.ctypes.data, len(live), ctypes.byref(n_lists)), "smc_build_live_rows")
        x = d_x.download(np.uint32, 5 * int(c[0])).reshape(-1, 5)
        out = dict(words=d_w.download(np.uint16 if mode == 16 else np.uint32, ns), us=d_us.download(np.uint32, nu), gid=d_g.download(np.uint32, nu), finc=d_f.download(np.uint32, nu),
                   loci=d_l.download(LOCUS, nl),
                   x=x[np.lexsort(x.T[::-1])], live=live[:n_lists.value].tolist(), raw=[b.download(np.uint32, ns) for b in raw])
        plan = eng.make_plan_dev(d_l, nl)
        out["rows"] = plan.run_devbuf([d_w, d_us], P).copy()
        plan.close()
        return out
    finally:
        for b in bufs:
            b.free()


_ORACLE = {}


def oracle_rows(key, A):
    """The oracle's rows of a run, made once and shared by the cases that build it."""
    if key not in _ORACLE:
        cores = min(8, len(os.sched_getaffinity(0)))
        db = oracle_lib.aln_planes(A, P, 0, A["nl"], n_threads=cores)
        assert int(db.loci["n_umi"].max()) <= P.ds
        _ORACLE[key] = (db.loci["n_alleles"].copy(),) + tuple(oracle_lib.call_batch_mt(db, abi.c_params(P), abi.ROW_DTYPE, cores, return_fragile=True, return_pi_all=True))
    return _ORACLE[key]


def check_run(eng, monkeypatch, key, A, modes, want_live, seg_tiles=None):
    n_al, want, fragile, pi_all = oracle_rows(key, A)
    if seg_tiles is not None:
        monkeypatch.setenv("SMC_BP_SEG_TILES", str(seg_tiles))
    up = devplanes.upload_run(eng, A, synth.aln_ref_fetch(A["start0"], A["start0"] + A["nl"]))
    try:
        for mode in modes:
            monkeypatch.delenv("SMC_BP_KEEP_DEAD_ROWS", raising=False)
            got = build(eng, up, A, mode)
            monkeypatch.setenv("SMC_BP_KEEP_DEAD_ROWS", "1")
            kept = build(eng, up, A, mode)
            monkeypatch.delenv("SMC_BP_KEEP_DEAD_ROWS")
            assert got["live"] == want_live, (mode, got["live"], want_live)
            assert kept["live"] == [len(order) for order, dead in tile_lists(A)], (mode, kept["live"])
            for k in ("words", "us", "gid", "finc", "loci", "x"):
                assert got[k].tobytes() == kept[k].tobytes(), "%s differs from the build that keeps the dead rows (%r)" % (k, mode)
            for a, b in zip(got["raw"], kept["raw"]):
                assert a.tobytes() == b.tobytes()
            assert (got["loci"]["n_alleles"] == n_al).all()
            assert abi.compare_rows(got["rows"], want, 1e-6, 1e-6, fragile, pi_all) == [], mode
    finally:
        up.free()


MODES = (16, 32, "raw")


@pytest.mark.parametrize("n1,n2", [(63, 255), (64, 256), (65, 257)])
def test_live_counts_at_the_batch_and_the_part_boundary(engine0, monkeypatch, n1, n2):
    """Tile 1 has 63 / 64 / 65 live rows (one batch of the walks is 64), tile 2 has 255 / 256 / 257 (a part of the count walk is 256) of
    windows of 512 rows and more: the last part of both is wholly dead.  In the unfiltered lists a dead row is the first entry, a
    dead row the last, a barcode between two live ones has dead rows only, a pair's first mate is dead and its second live, a dead
    and a live general CIGAR share tile 1 - and (checked here on the host) a dead row stands where a part of the walk begins."""
    A = live_rows_run(n1, n2, 1000 + n1)
    L = tile_lists(A)
    want = expected_live(A)
    assert want[1:] == [n1, n2] and want[0] == len(L[0][0])
    assert len(L[2][0]) >= 2 * PART and (len(L[2][0]) - 1) // PART > (n2 - 1) // PART          # a last part without a live row
    assert min(float(d.mean()) for o, d in L[1:]) > 0.25
    aln = A["aln"]
    for order, dead in L[1:]:
        assert dead[0] and dead[-1]
        bc = aln["bc_gid"][order]
        quiet = [g for g in np.unique(bc) if dead[bc == g].all() and 0 < g < bc.max() and not dead[bc == g - 1].all() and not dead[bc == g + 1].all()]
        assert quiet, "no barcode with dead rows only between two live ones"
    o1, d1 = L[1]
    pair = [g for g in np.unique(aln["pair_gid"][o1]) if (aln["pair_gid"][o1] == g).sum() == 2 and d1[aln["pair_gid"][o1] == g].tolist() == [True, False]]
    assert pair, "no pair with a dead first and a live second mate"
    gen = aln["n_cig"][o1] > 1
    assert (gen & d1).any() and (gen & ~d1).any()
    starts = [bool(d[j]) for o, d in L[1:] for j in range(SUB, len(o), SUB)]
    assert any(starts) and not all(starts)                                                # a part begins on a dead row, another on a live one
    check_run(engine0, monkeypatch, ("edge", n1, n2), A, MODES, want)


def test_both_instantiations_of_the_sort_filter(engine0, monkeypatch):
    """Tile 0's window holds fewer than 6,144 rows, those of tiles 1 and 2 more (short reads inside tile 1): a run that launches both
    instantiations of k_bp_sort_seg, and both drop their dead rows."""
    A = live_rows_run(140, 300, 77, fill1=300, fill2=6500)
    sizes = [len(o) for o, d in tile_lists(A)]
    assert 0 < sizes[0] <= SORT_LDS_MAX < sizes[1] <= sizes[2] <= LSORT_MAX
    want = expected_live(A)
    assert want[2] == 300 and want[1] == 140 + 6500
    check_run(engine0, monkeypatch, "both", A, MODES, want)


@pytest.mark.parametrize("seg_tiles", [1, None])
def test_a_tile_beyond_the_one_workgroup_sort_keeps_every_row(engine0, monkeypatch, seg_tiles):
    """Tile 2's window holds more than 16,384 rows.  With one tile per segment (SMC_BP_SEG_TILES=1) the multi-launch passes sort it
    and it keeps every window row, while tile 1 - sorted by one workgroup in the same run - drops its dead ones; by default such a
    run takes the deep path (segments of several tiles, a list per tile), which keeps every row of every tile."""
    A = live_rows_run(100, 200, 99, tail=16400)
    sizes = [len(o) for o, d in tile_lists(A)]
    assert sizes[1] <= SORT_LDS_MAX and sizes[2] > LSORT_MAX
    want = expected_live(A) if seg_tiles == 1 else sizes
    assert want[2] == sizes[2] and (want[1] == 100) == (seg_tiles == 1)
    check_run(engine0, monkeypatch, "beyond", A, MODES if seg_tiles == 1 else (16,), want, seg_tiles=seg_tiles)
