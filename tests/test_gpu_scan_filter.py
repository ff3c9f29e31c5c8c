"""smc_scan_filter on the GPU, on rows made in numpy: B = 3 copies of nl = 70 loci (no multiple of 64), G = 9 listed loci - the shape of
test_gpu_scan_detect.py.  Every word against the host twin spike.scan_filter_host (which test_spike_scan_filter.py holds against the
printed FILTER column), under nine assignments of the gate and always words to the listed loci, so that every row case meets every
word; bit 31 with its documented reason; nothing written outside the output; two calls alike; every refusal, with nothing launched."""
import ctypes

import numpy as np
import pytest

from smcounter_amd import _lib, abi, devplanes, spike
from smcounter_amd.engine import DevBuf

pytestmark = pytest.mark.gpu
B, NL = 3, 70
OFFSETS = (0, 5, 11, 23, 37, 42, 64, 65, NL - 1)        # (the first and the last locus of a copy among them)
G = len(OFFSETS)
EDGE = 4.995
LO, HI = EDGE - 1e-6, EDGE + 1e-6
HOST = abi.SCAN_FLT_HOST
GARBAGE = 0xFFFFFFFF
ALL = abi.SCAN_FLT_DEVICE_MASK
GATES = (0, abi.F_HP, abi.F_LOWC, abi.F_HP | abi.F_LOWC)
ALWAYS = (0, abi.F_REPT, abi.F_REPS, abi.F_SL, abi.F_OTHER_REPEAT, abi.F_LOWC, abi.F_REPT | abi.F_REPS | abi.F_SL,
          abi.F_LOWC | abi.F_REPT | abi.F_REPS | abi.F_SL | abi.F_OTHER_REPEAT)
# (flt_applied, flt, vmf_lt_099, PI, bi-allelic, status) -> is the word left to the host
CASES = [(1, bit, 1, 40.0, 0, 0, False) for bit, _ in abi.FILTER_NAMES] + [        # each SMC_F_* bit alone ...
    (1, ALL, 1, 40.0, 0, 0, False),                       # ... and all together
    (1, ALL | 0xFFFFFC00, 0, 40.0, 0, 0, False),          # bits above the ten are not the device's
    (0, GARBAGE, 1, 40.0, 0, 0, False),                   # filterVariants did not run: garbage in flt must not show
    (0, GARBAGE, 0, 3.0, 0, 0, False),
    (1, 0, 0, 40.0, 0, 0, False),                         # the gate closed / open, nothing else
    (1, 0, 1, 40.0, 0, 0, False),
    (1, 0, 7, 5.0, 0, 0, False),                          # vmf_lt_099 is a truth value
    (0, 0, 1, EDGE, 0, 0, True),                          # exactly 4.995
    (0, 0, 1, LO, 0, 0, True),                            # the band's edges belong to it
    (0, 0, 1, HI, 0, 0, True),
    (0, 0, 1, float(np.nextafter(LO, -np.inf)), 0, 0, False),    # one ulp outside, both sides
    (0, 0, 1, float(np.nextafter(HI, np.inf)), 0, 0, False),
    (0, 0, 1, float("nan"), 0, 0, True),
    (1, abi.F_SB, 1, 40.0, 1, 0, True),                   # bi-allelic
    (1, abi.F_SB, 1, 40.0, 0, abi.ST_ZERO_COVERAGE, True),      # a status that is not 0
    (2, abi.F_SB, 1, 40.0, 0, 0, True),                   # flt_applied neither 0 nor 1
    (-1, abi.F_SB, 1, 40.0, 0, 0, True),
]
assert len(CASES) <= B * G


def _make():
    rng = np.random.default_rng(11)
    rows = np.zeros((B, NL), abi.ROW_DTYPE)
    # every row one with all ten bits and a PI far above 5: a lane that read the wrong row would say so
    rows["cand"]["flt_applied"], rows["cand"]["flt"], rows["cand"]["vmf_lt_099"], rows["cand"]["pi"] = 1, ALL, 1, 55.0
    rows["used_mt"] = rng.integers(50, 150, (B, NL)).astype(np.int32)
    case_of = {}
    for c in range(B):
        for g, off in enumerate(OFFSETS):
            case = CASES[(c * G + g) % len(CASES)]
            case_of[(c, g)] = case
            cand = rows["cand"]
            (cand["flt_applied"][c, off, 0], cand["flt"][c, off, 0], cand["vmf_lt_099"][c, off, 0], cand["pi"][c, off, 0],
             rows["biallelic"][c, off], rows["status"][c, off]) = case[:6]
            # (cand[1] must not matter)
            cand["flt_applied"][c, off, 1], cand["flt"][c, off, 1], cand["pi"][c, off, 1] = 1, GARBAGE & ALL, 4.995
    return rows, case_of


@pytest.fixture(scope="module")
def made():
    return _make()


def _words(shift):
    gate = np.array([GATES[(g + shift) % len(GATES)] for g in range(G)], np.uint32)
    always = np.array([ALWAYS[(g + 2 * shift) % len(ALWAYS)] for g in range(G)], np.uint32)
    return gate, always


def test_every_word_equals_the_host_twin_and_bit_31_has_a_documented_reason(engine0, made):
    rows, case_of = made
    offsets = np.array(OFFSETS, np.uint32)
    d_rows = DevBuf(engine0, rows.nbytes + 256).upload(rows.view(np.uint8).reshape(-1))
    met = set()
    try:
        for shift in range(9):
            gate, always = _words(shift)
            got = devplanes.scan_filter(engine0, d_rows, B, NL, offsets, gate, always)
            again = devplanes.scan_filter(engine0, d_rows, B, NL, offsets, gate, always)
            assert got.shape == (B, G) and got.dtype == np.uint32 and got.tobytes() == again.tobytes()
            for c in range(B):
                for g in range(G):
                    applied, flt, below, pi, bi, status, host = case_of[(c, g)]
                    w, ga, al = int(got[c, g]), int(gate[g]), int(always[g])
                    want = spike.scan_filter_host(rows[c, OFFSETS[g]], ga, al)
                    assert w == want, (shift, c, g, case_of[(c, g)], hex(w), hex(want))
                    assert bool(w & HOST) == host and not w & ~(abi.SCAN_FLT_NAMES_MASK | HOST)
                    if w & HOST:
                        assert bi or status or applied not in (0, 1) or pi != pi or LO <= pi <= HI
                    # the rule itself, beside the twin
                    low = ((flt & ALL) | (ga if below else 0)) if applied else 0
                    assert w & abi.SCAN_FLT_NAMES_MASK == low | (al if pi > HI else 0)
                    if not applied:
                        assert not w & ALL & ~al, "flt shows although filterVariants did not run"
                    met.add((CASES.index(case_of[(c, g)]), ga, al))
        print("%d (row case, gate, always) triples met" % len(met))
        for k in range(len(CASES)):
            assert {ga for i, ga, _ in met if i == k} == set(GATES) and len({al for i, _, al in met if i == k}) >= 4, k
        # G = 0 and B = 0: no-ops that succeed
        assert devplanes.scan_filter(engine0, d_rows, B, NL, offsets[:0], [], []).shape == (B, 0)
        assert devplanes.scan_filter(engine0, d_rows, 0, NL, offsets, *_words(0)).shape == (0, G)
    finally:
        d_rows.free()


def _raw(eng, d_rows, d_in, host, d_out, n_listed=None, null=None):
    """host: uint32 [3, G] (offsets, gate, always), uploaded as it is; null: the device array passed as NULL."""
    n = host.shape[1]
    at = d_in.data_ptr()
    dev = [at, at + 4 * n, at + 8 * n]
    if null is not None:
        dev[null] = None
    _lib.check(eng.L.smc_scan_filter(eng.ctx, d_rows.data_ptr(), B, NL, dev[0], host[0].ctypes.data, dev[1], host[1].ctypes.data, dev[2],
                                     host[2].ctypes.data, n if n_listed is None else n_listed, d_out.data_ptr(), ctypes.c_void_p(0)),
               "smc_scan_filter")


def test_nothing_else_is_written_and_refusals_launch_nothing(engine0, made):
    rows, _ = made
    n, pad, fill = B * G, 512, 0xA5
    flat = rows.view(np.uint8).reshape(-1)
    host = np.ascontiguousarray(np.stack([np.array(OFFSETS, np.uint32)] + list(_words(3))))
    sizes = (flat.nbytes + pad, host.nbytes + pad, 4 * n + pad)
    bufs = [DevBuf(engine0, s) for s in sizes]
    d_rows, d_in, d_out = bufs
    try:
        def reset():
            for b, size in zip(bufs, sizes):
                b.upload(np.full(size, fill, np.uint8))
            d_rows.upload(flat)
            d_in.upload(host.view(np.uint8).reshape(-1))

        def state():
            return [b.download(np.uint8, size) for b, size in zip(bufs, sizes)]
        reset()
        _raw(engine0, d_rows, d_in, host, d_out)
        first = state()
        assert np.array_equal(first[0][:flat.nbytes], flat) and (first[0][flat.nbytes:] == fill).all()
        assert first[1][:host.nbytes].tobytes() == host.tobytes() and (first[1][host.nbytes:] == fill).all()
        assert (first[2][4 * n:] == fill).all()
        want = devplanes.scan_filter(engine0, d_rows, B, NL, host[0], host[1], host[2])
        assert first[2][:4 * n].tobytes() == want.tobytes() and (want != 0xA5A5A5A5).all()
        _raw(engine0, d_rows, d_in, host, d_out)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(state(), first))
        # G = 0: nothing is touched
        reset()
        _raw(engine0, d_rows, d_in, host, d_out, n_listed=0)
        assert (state()[2] == fill).all()
        # refusals launch nothing
        for row, col, value, msg in ((0, G - 1, NL, "names offset %d of %d" % (NL, NL)), (0, 0, 0xFFFFFFFF, "names offset"),
                                     (1, 4, abi.F_SB, "gate bits"), (1, 4, abi.F_REPT, "gate bits"), (1, 0, HOST, "gate bits"),
                                     (2, 2, abi.F_HP, "always bits"), (2, 2, 1 << 14, "always bits"), (2, 8, HOST, "always bits")):
            wrong = host.copy()
            wrong[row, col] = value
            with pytest.raises(_lib.SmcError, match=msg):
                _raw(engine0, d_rows, d_in, wrong, d_out)
        for null in range(3):
            with pytest.raises(_lib.SmcError, match="NULL argument"):
                _raw(engine0, d_rows, d_in, host, d_out, null=null)
        rc = engine0.L.smc_scan_filter(engine0.ctx, d_rows.data_ptr(), B, NL, d_in.data_ptr(), None, d_in.data_ptr(), host[1].ctypes.data,
                                       d_in.data_ptr(), host[2].ctypes.data, G, d_out.data_ptr(), ctypes.c_void_p(0))
        assert rc == -4 and b"smc_scan_filter" in engine0.L.smc_last_error()          # SMC_E_INPUT
        rc = engine0.L.smc_scan_filter(engine0.ctx, d_rows.data_ptr(), B, NL, d_in.data_ptr(), host[0].ctypes.data, d_in.data_ptr() + 4 * G,
                                       host[1].ctypes.data, d_in.data_ptr() + 8 * G, host[2].ctypes.data, G, None, ctypes.c_void_p(0))
        assert rc == -4
        assert (state()[2] == fill).all()
    finally:
        for b in bufs:
            b.free()
