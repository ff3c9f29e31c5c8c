"""smc_scan_detect on the GPU, on rows made in numpy: B = 3 copies of nl = 70 loci (no multiple of 64), G = 9 listed loci.  Every
verdict of CALLED or NOT against the host path on the same rows (vc._strings, dsaf.replicate_entry, spike._called); every HOST
verdict one of the three documented reasons; the list of HOST records; nothing written outside the record and list buffers; two calls
alike.

The list's ORDER is that of the kernel's atomic appends and is not fixed from call to call (csrc/k_scan_detect.inc), so the list is
compared as a sorted array - as devplanes.scan_detect hands it out; the records are compared byte for byte."""
import collections
import ctypes

import numpy as np
import pytest

from smcounter_amd import _lib, abi, devplanes, vc
from smcounter_amd.engine import DevBuf
from smcounter_amd.params import VcParams
from smcounter_amd.pileup import BASE_ALLELES
from smcounter_amd.tools import ds_allele_fraction as af

pytestmark = pytest.mark.gpu
B, NL, THR = 3, 70, 17
OFFSETS = (0, 5, 11, 23, 37, 42, 64, 65, NL - 1)        # (the first and the last locus of a copy among them)
G = len(OFFSETS)
EDGE = THR - 0.005
LO, HI = EDGE - 1e-6, EDGE + 1e-6
INDEL_KEY = "INS|A|AT"                                    # allele id 6 at the locus that meets it
ZERO_COVERAGE = abi.ST_ZERO_COVERAGE
# (what cand[0] holds: "alt" the planted letter, "other" another letter, or an allele id; PI; bi-allelic; status) -> the verdict
CASES = [
    ("alt", HI + 10.0, 0, 0, abi.SCAN_CALLED),
    ("alt", 3.0, 0, 0, abi.SCAN_NOT),
    ("alt", EDGE, 0, 0, abi.SCAN_HOST),                   # exactly thr - 0.005
    ("alt", LO, 0, 0, abi.SCAN_HOST),                     # the guard band's edges belong to it
    ("alt", HI, 0, 0, abi.SCAN_HOST),
    ("alt", float(np.nextafter(LO, -np.inf)), 0, 0, abi.SCAN_NOT),       # just outside, both sides
    ("alt", float(np.nextafter(HI, np.inf)), 0, 0, abi.SCAN_CALLED),
    ("alt", THR - 0.0049, 0, 0, abi.SCAN_CALLED),         # py2 round(PI, 2) = thr
    ("alt", THR - 0.0051, 0, 0, abi.SCAN_NOT),            # ... = thr - 0.01
    ("other", 40.0, 0, 0, abi.SCAN_NOT),
    (6, 40.0, 0, 0, abi.SCAN_NOT),                        # an indel key
    (4, 40.0, 0, 0, abi.SCAN_NOT),                        # N
    (5, 40.0, 0, 0, abi.SCAN_NOT),                        # DEL: the .cut files never hold it
    (-1, 40.0, 0, 0, abi.SCAN_NOT),
    ("other", 40.0, 1, 0, abi.SCAN_HOST),                 # bi-allelic, the second candidate the planted letter
    ("alt", 40.0, 1, 0, abi.SCAN_HOST),
    ("alt", 40.0, 0, ZERO_COVERAGE, abi.SCAN_HOST),       # a status that is not 0
    ("alt", 1e6, 0, 0, abi.SCAN_CALLED),
    ("alt", 0.0, 0, 0, abi.SCAN_NOT),
]


def _make():
    """-> (rows [B, NL], listed, per listed locus (REF, ALT letters), the case of every (copy, listed locus))."""
    rng = np.random.default_rng(5)
    rows = np.zeros((B, NL), abi.ROW_DTYPE)
    # every row a callable locus whose candidate is a called G: a lane that read the wrong row would say so
    rows["cvg"], rows["all_frag"], rows["all_mt"], rows["used_frag"], rows["used_mt"] = 400, 400, 120, 380, 100
    rows["mt3"], rows["mt5"], rows["mt7"], rows["mt10"] = 90, 80, 70, 60
    rows["dp"], rows["umt"], rows["vsm"], rows["pi"] = 100, 25, 20, 1.5
    rows["cand"]["allele"][:, :, 0], rows["cand"]["allele"][:, :, 1] = 2, -1
    rows["cand"]["vdp"], rows["cand"]["vmt"], rows["cand"]["vsm"], rows["cand"]["pi"] = 40, 12, 9, 55.0
    rows["used_mt"] += rng.integers(0, 50, (B, NL)).astype(np.int32)
    rows["cand"]["vmt"][:, :, 0] += rng.integers(0, 12, (B, NL)).astype(np.int32)
    listed = np.zeros(G, abi.SCAN_LOCUS_DTYPE)
    letters, case_of = [], {}
    for g, off in enumerate(OFFSETS):
        alt = g % 4
        listed[g] = (off, alt)
        letters.append((BASE_ALLELES[(alt + 1) % 4], BASE_ALLELES[alt]))
        for c in range(B):
            case = CASES[(c * G + g) % len(CASES)]
            case_of[(c, g)] = case
            what, pi, bi, status, _ = case
            cand = rows["cand"]
            cand["allele"][c, off, 0] = alt if what == "alt" else (alt + 2) % 4 if what == "other" else what
            cand["pi"][c, off, 0], rows["biallelic"][c, off], rows["status"][c, off] = pi, bi, status
            if bi:
                cand["allele"][c, off, 1] = alt if what == "other" else (alt + 2) % 4
                cand["pi"][c, off, 1] = 45.0
    assert B * G >= len(CASES)
    return rows, listed, letters, case_of


@pytest.fixture(scope="module")
def made():
    return _make()


def _host_called(rows, listed, letters, c, g):
    off = int(listed["offset"][g])
    ref, alt = letters[g]
    table = list(BASE_ALLELES) + [INDEL_KEY]
    view = vc.LocusView(["chrT"], [off + 1], [ref], [table])
    text = vc._strings(rows[c, off:off + 1].copy(), view, VcParams(mtDepth=250, rpb=3.0), None)
    assert not text[0].startswith(vc.EXC_PREFIX), text[0]
    nothing = (collections.defaultdict(list), collections.defaultdict(list))
    return devplanes.scan_called_host(text[0], af.Variant("chrT", off + 1, ref, alt, alt, af.SNV), THR, nothing)


def test_verdicts_equal_the_host_path_and_host_records_have_a_documented_reason(engine0, made):
    rows, listed, letters, case_of = made
    d_rows = DevBuf(engine0, rows.nbytes + 256).upload(rows.view(np.uint8).reshape(-1))
    try:
        rec, todo = devplanes.scan_detect(engine0, d_rows, B, NL, listed, THR)
        again, todo2 = devplanes.scan_detect(engine0, d_rows, B, NL, listed, THR)
    finally:
        d_rows.free()
    assert rec.shape == (B, G) and rec.tobytes() == again.tobytes() and np.array_equal(todo, todo2)
    verdict = rec["mt_verdict"] >> 30
    seen = collections.Counter()
    for c in range(B):
        for g in range(G):
            r = rows[c, OFFSETS[g]]
            what, pi, bi, status, want = case_of[(c, g)]
            v = int(verdict[c, g])
            print("copy %d locus %d: cand %r PI %.17g biallelic %d status %d -> %d" % (c, OFFSETS[g], what, pi, bi, status, v))
            assert v == want, (c, g, case_of[(c, g)])
            seen[v] += 1
            # the record: cand[0]'s PI unrounded and its VMT, the used MT below the verdict
            assert rec[c, g]["pi"].tobytes() == r["cand"][0]["pi"].tobytes()
            assert int(rec[c, g]["vmt"]) == int(r["cand"][0]["vmt"])
            assert int(rec[c, g]["mt_verdict"]) & abi.SCAN_MT_MASK == int(r["used_mt"])
            if v == abi.SCAN_HOST:
                in_band = LO <= float(r["cand"][0]["pi"]) <= HI
                assert int(r["biallelic"]) != 0 or int(r["status"]) != 0 or in_band
            else:
                assert (v == abi.SCAN_CALLED) == _host_called(rows, listed, letters, c, g), (c, g, case_of[(c, g)])
    assert all(seen[v] >= 3 for v in (abi.SCAN_NOT, abi.SCAN_CALLED, abi.SCAN_HOST)), seen
    # the list: exactly the HOST records, each once
    assert todo.dtype == np.uint32 and todo.tolist() == np.flatnonzero(verdict.reshape(-1) == abi.SCAN_HOST).tolist()
    # (a bi-allelic row whose second candidate is the planted letter IS called on the host: why the kernel must not say NOT there)
    c, g = next(k for k, case in case_of.items() if case[0] == "other" and case[2])
    assert _host_called(rows, listed, letters, c, g)


def _raw(eng, d_rows, listed, d_listed, d_out, d_list, d_n, n_listed=None):
    _lib.check(eng.L.smc_scan_detect(eng.ctx, d_rows.data_ptr(), B, NL, d_listed.data_ptr(), listed.ctypes.data,
                                     len(listed) if n_listed is None else n_listed, float(THR), d_out.data_ptr(), d_list.data_ptr(),
                                     d_n.data_ptr(), ctypes.c_void_p(0)), "smc_scan_detect")


def test_nothing_else_is_written_and_a_second_call_gives_the_same_bytes(engine0, made):
    rows, listed, _, _ = made
    n, pad, fill = B * G, 512, 0xA5
    flat = rows.view(np.uint8).reshape(-1)
    bufs = [DevBuf(engine0, flat.nbytes + pad), DevBuf(engine0, listed.nbytes + pad), DevBuf(engine0, 16 * n + pad),
            DevBuf(engine0, 4 * n + pad), DevBuf(engine0, 4 + pad)]
    d_rows, d_listed, d_out, d_list, d_n = bufs
    sizes = (flat.nbytes + pad, listed.nbytes + pad, 16 * n + pad, 4 * n + pad, 4 + pad)
    try:
        def reset():
            for b, size in zip(bufs, sizes):
                b.upload(np.full(size, fill, np.uint8))
            d_rows.upload(flat)
            d_listed.upload(listed.view(np.uint8).reshape(-1))

        def state():
            return [b.download(np.uint8, size) for b, size in zip(bufs, sizes)]
        reset()
        _raw(engine0, d_rows, listed, d_listed, d_out, d_list, d_n)
        first = state()
        n_host = int(first[4][:4].view(np.uint32)[0])
        assert 0 < n_host < n
        # the inputs as they went up, the outputs' tails and the list behind its last entry untouched
        assert np.array_equal(first[0][:flat.nbytes], flat) and (first[0][flat.nbytes:] == fill).all()
        assert first[1][:listed.nbytes].tobytes() == listed.tobytes() and (first[1][listed.nbytes:] == fill).all()
        assert (first[2][16 * n:] == fill).all() and (first[3][4 * n_host:] == fill).all() and (first[4][4:] == fill).all()
        _raw(engine0, d_rows, listed, d_listed, d_out, d_list, d_n)
        second = state()
        assert second[2].tobytes() == first[2].tobytes() and second[4].tobytes() == first[4].tobytes()
        assert np.array_equal(np.sort(second[3][:4 * n_host].view(np.uint32)), np.sort(first[3][:4 * n_host].view(np.uint32)))
        assert (second[3][4 * n_host:] == fill).all()
        # G = 0: the cursor is zeroed, nothing else is touched
        reset()
        _raw(engine0, d_rows, listed, d_listed, d_out, d_list, d_n, n_listed=0)
        empty = state()
        assert int(empty[4][:4].view(np.uint32)[0]) == 0 and (empty[4][4:] == fill).all()
        assert (empty[2] == fill).all() and (empty[3] == fill).all()
        rec, todo = devplanes.scan_detect(engine0, d_rows, B, NL, listed[:0], THR)
        assert rec.shape == (B, 0) and len(todo) == 0
        # refusals launch nothing
        reset()
        for bad, msg in (((NL, 0), "names offset %d of %d" % (NL, NL)), ((3, 4), "allele id 4")):
            wrong = listed.copy()
            wrong[G - 1] = bad
            with pytest.raises(_lib.SmcError, match=msg):
                _raw(engine0, d_rows, wrong, d_listed, d_out, d_list, d_n)
        assert (state()[2] == fill).all() and (state()[4] == fill).all()
    finally:
        for b in bufs:
            b.free()
