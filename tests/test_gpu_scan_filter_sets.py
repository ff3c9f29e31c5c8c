"""smc_scan_filter_sets on the GPU, on rows made in numpy as test_gpu_scan_filter.py makes them, cycling through its CASES (every branch
of the member rule: flt_applied 0 / 1 / other, vmf_lt_099, PI below / inside / above the 4.995 band and NaN, a status that is not 0,
bi-allelic rows): B = 3 copies of nl = 70 loci (no multiple of 64), the listed loci tiled by sets of every size 1 .. 8; 33 and 65 sets of
one member (32 sets fill a workgroup: these straddle it); one set.  The member words must be smc_scan_filter's on the same rows, word
for word; the joint words the numpy rule (abi.scan_filter_joint_rule) of them; every joint bit 31 traces to a member's; nothing is
written outside the two outputs; two calls alike; every refusal returns SMC_E_INPUT with nothing launched."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, devplanes
from smcounter_amd.engine import DevBuf

sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_scan_filter as TF  # noqa: E402  (its CASES, GATES, ALWAYS and the rows' background)

pytestmark = pytest.mark.gpu
B, NL = TF.B, TF.NL
SIZES = (1, 2, 3, 4, 5, 6, 7, 8)
SET_OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint32)
G, S = int(SET_OFF[-1]), len(SIZES)
# (the first and the last locus of a copy among them, neighbours as an MNV's members are, and not in ascending order throughout)
OFFSETS = tuple([0] + list(range(5, 5 + 17)) + list(range(40, 40 + 17)) + [NL - 1])
assert len(OFFSETS) == G == 36 and len(set(OFFSETS)) == G
HOST, NAMES, SHIFT = abi.SCAN_FLT_HOST, abi.SCAN_FLT_NAMES_MASK, abi.SCAN_FLT_MEMBER_SHIFT
E_INPUT = -4


def _rows(offsets, start=0):
    """TF._make's rows with the listed loci at `offsets`: copy c's listed locus g gets CASES[(start + c * len(offsets) + g) % len(CASES)]."""
    rng = np.random.default_rng(11)
    rows = np.zeros((B, NL), abi.ROW_DTYPE)
    rows["cand"]["flt_applied"], rows["cand"]["flt"], rows["cand"]["vmf_lt_099"], rows["cand"]["pi"] = 1, TF.ALL, 1, 55.0
    rows["used_mt"] = rng.integers(50, 150, (B, NL)).astype(np.int32)
    cand = rows["cand"]
    for c in range(B):
        for g, off in enumerate(offsets):
            case = TF.CASES[(start + c * len(offsets) + g) % len(TF.CASES)]
            (cand["flt_applied"][c, off, 0], cand["flt"][c, off, 0], cand["vmf_lt_099"][c, off, 0], cand["pi"][c, off, 0],
             rows["biallelic"][c, off], rows["status"][c, off]) = case[:6]
            cand["flt_applied"][c, off, 1], cand["flt"][c, off, 1], cand["pi"][c, off, 1] = 1, TF.GARBAGE & TF.ALL, 4.995
    return rows


def _words(n, shift):
    gate = np.array([TF.GATES[(g + shift) % len(TF.GATES)] for g in range(n)], np.uint32)
    always = np.array([TF.ALWAYS[(g + 2 * shift) % len(TF.ALWAYS)] for g in range(n)], np.uint32)
    return gate, always


@pytest.fixture(scope="module")
def made():
    return _rows(OFFSETS, start=1)       # (rotated by one: a set whose members are all PASS is among them)


def _up(eng, rows):
    return DevBuf(eng, rows.nbytes + 256).upload(rows.view(np.uint8).reshape(-1))


def _held(joint, mem, want_mem, set_off):
    """Checks 1 and 2 on one call's output."""
    assert mem.dtype == np.uint32 and mem.tobytes() == want_mem.tobytes()
    want = abi.scan_filter_joint_rule(want_mem, set_off)
    assert joint.dtype == np.uint32 and joint.shape == want.shape and np.array_equal(joint, want)
    off = np.asarray(set_off, np.int64)
    for c in range(joint.shape[0]):
        for s in range(len(off) - 1):
            w, mine = int(joint[c, s]), [int(x) for x in want_mem[c, off[s]:off[s + 1]]]
            assert bool(w & HOST) == any(x & HOST for x in mine), (c, s)                   # every bit 31 traces to a member's
            assert w & NAMES == int(np.bitwise_or.reduce(np.array(mine) & NAMES))
            assert [bool(w >> (SHIFT + m) & 1) for m in range(len(mine))] == [bool(x & NAMES) for x in mine]
            assert not w & ~(NAMES | HOST | (((1 << len(mine)) - 1) << SHIFT))
    return want


def test_member_words_are_scan_filters_and_the_joint_words_the_numpy_rule(engine0, made):
    rows = made
    offsets = np.array(OFFSETS, np.uint32)
    d_rows = _up(engine0, rows)
    seen = set()
    try:
        for shift in range(4):
            gate, always = _words(G, shift)
            want_mem = devplanes.scan_filter(engine0, d_rows, B, NL, offsets, gate, always)
            joint, mem = devplanes.scan_filter_sets(engine0, d_rows, B, NL, offsets, gate, always, SET_OFF)
            joint2, mem2 = devplanes.scan_filter_sets(engine0, d_rows, B, NL, offsets, gate, always, SET_OFF)
            _, mem0 = devplanes.scan_filter_sets(engine0, d_rows, B, NL, offsets, gate, always, SET_OFF, members_of=[2])
            assert joint.shape == (B, S) and mem.shape == (B, G)
            assert joint.tobytes() == joint2.tobytes() and mem.tobytes() == mem2.tobytes()
            assert mem0.shape == (1, G) and mem0[0].tobytes() == want_mem[2].tobytes()
            _held(joint, mem, want_mem, SET_OFF)
            for c in range(B):
                for s in range(S):
                    w = int(joint[c, s])
                    print("shift %d copy %d set %d (%d members): joint word %#010x" % (shift, c, s, SIZES[s], w))
                    n_bad = bin(w >> SHIFT & 0xFF).count("1")
                    seen.add(("host" if w & HOST else "device", "pass" if not n_bad else "one" if n_bad == 1 else "all" if n_bad == SIZES[s]
                              else "some"))
        # the layout meets PASS sets, sets with exactly one member that is not PASS, mixed sets, and both with and without bit 31
        assert {("device", "pass"), ("device", "one"), ("device", "some"), ("host", "some")} <= seen, sorted(seen)
        # no set and no copy: no-ops that succeed
        joint, mem = devplanes.scan_filter_sets(engine0, d_rows, B, NL, offsets[:0], [], [], [0])
        assert joint.shape == (B, 0) and mem.shape == (B, 0)
        joint, mem = devplanes.scan_filter_sets(engine0, d_rows, 0, NL, offsets, *_words(G, 0), SET_OFF)
        assert joint.shape == (0, S) and mem.shape == (0, G)
    finally:
        d_rows.free()


@pytest.mark.parametrize("n", [33, 65])
def test_sets_of_one_member_straddling_a_workgroup(engine0, n):
    """n sets of one member (a workgroup takes 32 sets); then the same loci as sets of 8 with a shorter last one."""
    offsets = np.array([(7 * g) % NL for g in range(n)], np.uint32)       # (7 and 70 share a factor: some loci are listed more than once)
    rows = _rows(sorted(set(int(o) for o in offsets)), start=n)
    gate, always = _words(n, 1)
    d_rows = _up(engine0, rows)
    try:
        want_mem = devplanes.scan_filter(engine0, d_rows, B, NL, offsets, gate, always)
        for off in (np.arange(n + 1), np.concatenate([np.arange(0, n, 8), [n]])):
            joint, mem = devplanes.scan_filter_sets(engine0, d_rows, B, NL, offsets, gate, always, off)
            want = _held(joint, mem, want_mem, off)
            assert len(set(want.reshape(-1).tolist())) >= 3
    finally:
        d_rows.free()


def test_one_set(engine0, made):
    offsets = np.array(OFFSETS[:5], np.uint32)
    gate, always = _words(5, 2)
    d_rows = _up(engine0, made)
    try:
        want_mem = devplanes.scan_filter(engine0, d_rows, B, NL, offsets, gate, always)
        joint, mem = devplanes.scan_filter_sets(engine0, d_rows, B, NL, offsets, gate, always, [0, 5])
        assert joint.shape == (B, 1)
        _held(joint, mem, want_mem, [0, 5])
    finally:
        d_rows.free()


def _raw(eng, bufs, host, set_off, n_copies=B, n_listed=None, n_sets=None, null=None):
    """host: uint32 [3, G] (offsets, gate, always) as uploaded; null: the index of the device array passed as NULL."""
    d_rows, d_in, d_off, d_mem, d_joint = bufs
    n = host.shape[1]
    at = d_in.data_ptr()
    dev = [at, at + 4 * n, at + 8 * n, d_off.data_ptr(), d_mem.data_ptr(), d_joint.data_ptr()]
    if null is not None:
        dev[null] = None
    return eng.L.smc_scan_filter_sets(eng.ctx, d_rows.data_ptr(), n_copies, NL, dev[0], host[0].ctypes.data, dev[1], host[1].ctypes.data,
                                      dev[2], host[2].ctypes.data, n if n_listed is None else n_listed, dev[3], set_off.ctypes.data,
                                      len(set_off) - 1 if n_sets is None else n_sets, dev[4], dev[5], ctypes.c_void_p(0))


def test_nothing_else_is_written_two_calls_are_alike_and_refusals_launch_nothing(engine0, made):
    rows = made
    n, ns, pad, fill = B * G, B * S, 512, 0xA5
    flat = rows.view(np.uint8).reshape(-1)
    host = np.ascontiguousarray(np.stack([np.array(OFFSETS, np.uint32)] + list(_words(G, 3))))
    sizes = (flat.nbytes + pad, host.nbytes + pad, SET_OFF.nbytes + pad, 4 * n + 2 * pad, 4 * ns + 2 * pad)
    allocs = [DevBuf(engine0, size) for size in sizes]
    # (the two outputs stand `pad` bytes into their allocations: a guard stretch on both sides)
    bufs = allocs[:3] + [b.view(pad) for b in allocs[3:]]
    try:
        def reset():
            for b, size in zip(allocs, sizes):
                b.upload(np.full(size, fill, np.uint8))
            allocs[0].upload(flat)
            allocs[1].upload(host.view(np.uint8).reshape(-1))
            allocs[2].upload(SET_OFF.view(np.uint8))

        def state():
            return [b.download(np.uint8, size) for b, size in zip(allocs, sizes)]

        def outputs_untouched(st):
            return all((st[i] == fill).all() for i in (3, 4))
        reset()
        _lib.check(_raw(engine0, bufs, host, SET_OFF), "smc_scan_filter_sets")
        first = state()
        assert np.array_equal(first[0][:flat.nbytes], flat) and (first[0][flat.nbytes:] == fill).all()
        assert first[1][:host.nbytes].tobytes() == host.tobytes() and (first[1][host.nbytes:] == fill).all()
        assert first[2][:SET_OFF.nbytes].tobytes() == SET_OFF.tobytes() and (first[2][SET_OFF.nbytes:] == fill).all()
        for i, used in ((3, 4 * n), (4, 4 * ns)):
            assert (first[i][:pad] == fill).all() and (first[i][pad + used:] == fill).all(), i
        want_mem = devplanes.scan_filter(engine0, allocs[0], B, NL, host[0], host[1], host[2])
        assert first[3][pad:pad + 4 * n].tobytes() == want_mem.tobytes()
        assert first[4][pad:pad + 4 * ns].tobytes() == abi.scan_filter_joint_rule(want_mem, SET_OFF).tobytes()
        assert (first[4][pad:pad + 4 * ns].view(np.uint32) != 0xA5A5A5A5).all()
        _lib.check(_raw(engine0, bufs, host, SET_OFF), "smc_scan_filter_sets")
        assert all(a.tobytes() == b.tobytes() for a, b in zip(state(), first))
        # no listed locus: nothing is touched
        reset()
        _lib.check(_raw(engine0, bufs, host, SET_OFF[:1].copy(), n_listed=0), "smc_scan_filter_sets")
        assert outputs_untouched(state())
        # the refusals return SMC_E_INPUT and launch nothing
        many = np.arange(32770, dtype=np.uint32)                           # 65535 copies x 32769 sets >= 2^31
        calls = []
        for row, col, value, msg in ((0, G - 1, NL, "names offset %d of %d" % (NL, NL)), (0, 0, 0xFFFFFFFF, "names offset"),
                                     (1, 4, abi.F_SB, "gate bits"), (1, 0, HOST, "gate bits"), (2, 2, abi.F_HP, "always bits"),
                                     (2, 2, 1 << 14, "always bits")):      # what smc_scan_filter refuses
            wrong = host.copy()
            wrong[row, col] = value
            calls.append((lambda wrong=wrong: _raw(engine0, bufs, wrong, SET_OFF), msg))
        calls += [(lambda k=k: _raw(engine0, bufs, host, SET_OFF, null=k), "NULL argument") for k in range(6)]
        calls += [(lambda: _raw(engine0, bufs, host, SET_OFF, n_copies=65536), "at most 65535"),
                  (lambda: _raw(engine0, bufs, host, many, n_copies=65535), "2\\^31"),
                  # what smc_scan_detect_sets refuses about the tiling
                  (lambda: _raw(engine0, bufs, host, np.array([0, 1, 3, 6, 10, 15, 21, 28, G - 1], np.uint32)), "must tile"),
                  (lambda: _raw(engine0, bufs, host, np.array([1, 1, 3, 6, 10, 15, 21, 28, G], np.uint32)), "must tile"),
                  (lambda: _raw(engine0, bufs, host, np.array([0, 0, 3, 6, 10, 15, 21, 28, G], np.uint32)), "has 0 members"),
                  (lambda: _raw(engine0, bufs, host, np.array([0, 1, 3, 6, 10, 15, 21, 27, G], np.uint32)), "has 9 members"),
                  (lambda: _raw(engine0, bufs, host, np.array([0, 3, 2, 6, 10, 15, 21, 28, G], np.uint32)), "members")]
        for call, msg in calls:
            rc = call()
            assert rc == E_INPUT, (rc, msg)
            with pytest.raises(_lib.SmcError, match=msg):
                _lib.check(rc, "smc_scan_filter_sets")
        final = state()
        assert outputs_untouched(final)
        assert np.array_equal(final[0][:flat.nbytes], flat)
    finally:
        for b in allocs:
            b.free()
