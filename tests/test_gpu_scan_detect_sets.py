"""smc_scan_detect_sets on the GPU, on rows made in numpy as test_gpu_scan_detect.py makes them, cycling through its CASES: B = 3
copies of nl = 70 loci (no multiple of 64), the listed records tiled by sets of 1, 2, 3 and 8 members.  The member records must be
smc_scan_detect's on the same rows, byte for byte; the joint words and the sorted list must be the numpy rule (abi.scan_joint_rule)
applied to that output.  The list's order is that of the kernel's atomic appends, so it is compared sorted."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, devplanes
from smcounter_amd.engine import DevBuf

sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_scan_detect as TD  # noqa: E402  (its CASES and the rows' background)

pytestmark = pytest.mark.gpu
B, NL, THR = TD.B, TD.NL, TD.THR
SIZES = (1, 2, 3, 8)
SET_OFF = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.uint32)
G = int(SET_OFF[-1])
OFFSETS = (0, 5, 6, 11, 12, 13, 23, 24, 25, 26, 27, 28, 29, NL - 1)        # (the first and the last locus of a copy among them)
CALLED, NOT = ("alt", TD.HI + 10.0, 0, 0, abi.SCAN_CALLED), ("alt", 3.0, 0, 0, abi.SCAN_NOT)
BAND, NAN = ("alt", TD.EDGE, 0, 0, abi.SCAN_HOST), ("alt", float("nan"), 0, 0, abi.SCAN_HOST)
STATUS = ("alt", 40.0, 0, TD.ZERO_COVERAGE, abi.SCAN_HOST)
LO_EDGE, HI_EDGE = ("alt", TD.LO, 0, 0, abi.SCAN_HOST), ("alt", TD.HI, 0, 0, abi.SCAN_HOST)
ABOVE = ("alt", float(np.nextafter(TD.HI, np.inf)), 0, 0, abi.SCAN_CALLED)
BELOW = ("alt", float(np.nextafter(TD.LO, -np.inf)), 0, 0, abi.SCAN_NOT)
# per copy and set the members' cases, and the joint verdict they must give
LAYOUT = {
    (0, 0): ([CALLED], abi.SCAN_CALLED),
    (0, 1): ([BAND, NOT], abi.SCAN_NOT),                              # one HOST beside one NOT: nothing listed
    (0, 2): ([CALLED, BAND, CALLED], abi.SCAN_HOST),                  # one HOST, the rest CALLED: that member listed
    (0, 3): (TD.CASES[:8], abi.SCAN_NOT),
    (1, 0): ([BAND], abi.SCAN_HOST),
    (1, 1): ([CALLED, CALLED], abi.SCAN_CALLED),
    (1, 2): ([CALLED, CALLED, NOT], abi.SCAN_NOT),
    (1, 3): ([CALLED] * 8, abi.SCAN_CALLED),
    (2, 0): ([BELOW], abi.SCAN_NOT),
    (2, 1): ([NAN, ABOVE], abi.SCAN_HOST),
    (2, 2): ([STATUS, LO_EDGE, HI_EDGE], abi.SCAN_HOST),
    (2, 3): ([CALLED] * 7 + [STATUS], abi.SCAN_HOST),
}


def _rows(n_copies, cases_at, alts):
    """TD._make's rows: every row a called G, then at (copy, offset) of `cases_at` the case's cand[0] with the planted letter alts[offset]."""
    rng = np.random.default_rng(5)
    rows = np.zeros((n_copies, NL), abi.ROW_DTYPE)
    rows["cvg"], rows["all_frag"], rows["all_mt"], rows["used_frag"], rows["used_mt"] = 400, 400, 120, 380, 100
    rows["dp"], rows["umt"], rows["vsm"], rows["pi"] = 100, 25, 20, 1.5
    rows["cand"]["allele"][:, :, 0], rows["cand"]["allele"][:, :, 1] = 2, -1
    rows["cand"]["vdp"], rows["cand"]["vmt"], rows["cand"]["vsm"], rows["cand"]["pi"] = 40, 12, 9, 55.0
    rows["used_mt"] += rng.integers(0, 50, (n_copies, NL)).astype(np.int32)
    rows["cand"]["vmt"][:, :, 0] += rng.integers(0, 12, (n_copies, NL)).astype(np.int32)
    cand = rows["cand"]
    for (c, off), (what, pi, bi, status, _) in cases_at.items():
        alt = alts[off]
        cand["allele"][c, off, 0] = alt if what == "alt" else (alt + 2) % 4 if what == "other" else what
        cand["pi"][c, off, 0], rows["biallelic"][c, off], rows["status"][c, off] = pi, bi, status
    return rows


@pytest.fixture(scope="module")
def made():
    """-> (rows [B, NL], listed [G], the member case of every (copy, listed record))."""
    listed = np.zeros(G, abi.SCAN_LOCUS_DTYPE)
    for g, off in enumerate(OFFSETS):
        listed[g] = (off, g % 4)
    alts = {off: g % 4 for g, off in enumerate(OFFSETS)}
    case_of = {}
    for (c, s), (cases, _) in LAYOUT.items():
        assert len(cases) == SIZES[s]
        for m, case in enumerate(cases):
            case_of[(c, int(SET_OFF[s]) + m)] = case
    rows = _rows(B, {(c, OFFSETS[g]): case for (c, g), case in case_of.items()}, alts)
    return rows, listed, case_of


def _up(eng, rows):
    return DevBuf(eng, rows.nbytes + 256).upload(rows.view(np.uint8).reshape(-1))


def test_member_records_are_scan_detects_and_the_joint_words_the_numpy_rule(engine0, made):
    rows, listed, case_of = made
    d_rows = _up(engine0, rows)
    try:
        want_rec, want_todo = devplanes.scan_detect(engine0, d_rows, B, NL, listed, THR)
        joint, todo, rec = devplanes.scan_detect_sets(engine0, d_rows, B, NL, listed, SET_OFF, THR)
        joint2, todo2, rec2 = devplanes.scan_detect_sets(engine0, d_rows, B, NL, listed, SET_OFF, THR)
        _, _, rec0 = devplanes.scan_detect_sets(engine0, d_rows, B, NL, listed, SET_OFF, THR, records_of=[2])
    finally:
        d_rows.free()
    assert rec.shape == (B, G) and rec.tobytes() == want_rec.tobytes()
    assert rec0.shape == (1, G) and rec0[0].tobytes() == want_rec[2].tobytes()
    assert joint.tobytes() == joint2.tobytes() and np.array_equal(todo, todo2) and rec.tobytes() == rec2.tobytes()
    verdict = (want_rec["mt_verdict"] >> 30).astype(np.int64)
    for (c, g), case in sorted(case_of.items()):
        print("copy %d record %d: cand %r PI %.17g biallelic %d status %d -> %d" % ((c, g) + tuple(case[:4]) + (int(verdict[c, g]),)))
        assert int(verdict[c, g]) == case[4], (c, g, case)
    words, listed_host = abi.scan_joint_rule(verdict, SET_OFF)
    assert joint.dtype == np.uint32 and joint.shape == (B, len(SIZES)) and np.array_equal(joint, words)
    assert todo.dtype == np.uint32 and np.array_equal(todo, listed_host)
    for (c, s), (_, want) in sorted(LAYOUT.items()):
        print("copy %d set %d: joint word %#010x" % (c, s, int(joint[c, s])))
        assert int(joint[c, s]) >> 30 == want, (c, s)
    # the four named cases, spelled out
    assert int(joint[1, 3]) == (abi.SCAN_CALLED << 30) | 0xFF                             # all members CALLED
    assert int(joint[1, 2]) == (abi.SCAN_NOT << 30) | 0x3 | (0x4 << 16)                   # one NOT
    assert int(joint[0, 2]) == (abi.SCAN_HOST << 30) | 0x5 | (0x2 << 8)                   # one HOST, the rest CALLED: that member listed
    assert 0 * G + int(SET_OFF[2]) + 1 in todo.tolist()
    assert int(joint[0, 1]) == (abi.SCAN_NOT << 30) | (0x1 << 8) | (0x2 << 16)            # one HOST beside one NOT: nothing listed
    assert not set(todo.tolist()) & {0 * G + 1, 0 * G + 2}
    host_members = set(np.flatnonzero(verdict.reshape(-1) == abi.SCAN_HOST).tolist())
    assert set(todo.tolist()) < host_members, "every HOST member was listed: the layout holds no HOST member beside a NOT one"


def test_one_set_and_sets_of_one_straddling_a_workgroup(engine0):
    """n_sets = 1, and 3 x 100 sets of one member (a workgroup takes 32 sets): records listed more than once share a row."""
    n = 100
    alts = {off: off % 4 for off in range(NL)}
    rows = _rows(B, {(c, off): TD.CASES[(c * NL + off) % len(TD.CASES)] for c in range(B) for off in range(NL)}, alts)
    listed = np.zeros(n, abi.SCAN_LOCUS_DTYPE)
    for g in range(n):
        listed[g] = (g % NL, (g % NL) % 4)
    d_rows = _up(engine0, rows)
    try:
        for lst, off in ((listed, np.arange(n + 1)), (listed[:5], [0, 5]), (listed, np.concatenate([np.arange(0, n, 8), [n]]))):
            want_rec, _ = devplanes.scan_detect(engine0, d_rows, B, NL, lst, THR)
            joint, todo, rec = devplanes.scan_detect_sets(engine0, d_rows, B, NL, lst, off, THR)
            assert rec.tobytes() == want_rec.tobytes()
            words, listed_host = abi.scan_joint_rule(want_rec["mt_verdict"] >> 30, off)
            assert np.array_equal(joint, words) and np.array_equal(todo, listed_host)
            assert len({int(w) >> 30 for w in words.reshape(-1)}) >= 2 or len(off) == 2
    finally:
        d_rows.free()


def _raw(eng, bufs, listed, set_off, n_copies=B, n_listed=None, n_sets=None):
    d_rows, d_listed, d_off, d_out, d_joint, d_list, d_n = bufs
    return eng.L.smc_scan_detect_sets(eng.ctx, d_rows.data_ptr(), n_copies, NL, d_listed.data_ptr(), listed.ctypes.data,
                                      len(listed) if n_listed is None else n_listed, d_off.data_ptr(), set_off.ctypes.data,
                                      len(set_off) - 1 if n_sets is None else n_sets, float(THR), d_out.data_ptr(), d_joint.data_ptr(),
                                      d_list.data_ptr(), d_n.data_ptr(), ctypes.c_void_p(0))


def test_nothing_else_is_written_two_calls_are_alike_and_refusals_launch_nothing(engine0, made):
    rows, listed, _ = made
    n, ns, pad, fill = B * G, B * len(SIZES), 512, 0xA5
    flat = rows.view(np.uint8).reshape(-1)
    sizes = (flat.nbytes + pad, listed.nbytes + pad, SET_OFF.nbytes + pad, 16 * n + 2 * pad, 4 * ns + 2 * pad, 4 * n + 2 * pad, 4 + 2 * pad)
    allocs = [DevBuf(engine0, size) for size in sizes]
    # (the three outputs and the cursor stand `pad` bytes into their allocations: a guard stretch on both sides)
    bufs = allocs[:3] + [b.view(pad) for b in allocs[3:]]
    try:
        def reset():
            for b, size in zip(allocs, sizes):
                b.upload(np.full(size, fill, np.uint8))
            allocs[0].upload(flat)
            allocs[1].upload(listed.view(np.uint8).reshape(-1))
            allocs[2].upload(SET_OFF.view(np.uint8))

        def state():
            return [b.download(np.uint8, size) for b, size in zip(allocs, sizes)]

        def outputs_untouched(st, cursor=False):
            return all((st[i] == fill).all() for i in (3, 4, 5)) and (cursor or (st[6] == fill).all())
        reset()
        _lib.check(_raw(engine0, bufs, listed, SET_OFF), "smc_scan_detect_sets")
        first = state()
        n_host = int(first[6][pad:pad + 4].view(np.uint32)[0])
        assert 0 < n_host < n
        assert np.array_equal(first[0][:flat.nbytes], flat) and (first[0][flat.nbytes:] == fill).all()
        assert first[1][:listed.nbytes].tobytes() == listed.tobytes() and (first[1][listed.nbytes:] == fill).all()
        assert first[2][:SET_OFF.nbytes].tobytes() == SET_OFF.tobytes() and (first[2][SET_OFF.nbytes:] == fill).all()
        for i, used in ((3, 16 * n), (4, 4 * ns), (5, 4 * n_host), (6, 4)):
            assert (first[i][:pad] == fill).all() and (first[i][pad + used:] == fill).all(), i
        _lib.check(_raw(engine0, bufs, listed, SET_OFF), "smc_scan_detect_sets")
        second = state()
        assert all(second[i].tobytes() == first[i].tobytes() for i in (3, 4, 6))
        assert np.array_equal(np.sort(second[5][pad:pad + 4 * n_host].view(np.uint32)), np.sort(first[5][pad:pad + 4 * n_host].view(np.uint32)))
        assert (second[5][pad + 4 * n_host:] == fill).all()
        # no set: the cursor is zeroed, nothing else is touched
        reset()
        _lib.check(_raw(engine0, bufs, listed, SET_OFF[:1].copy(), n_listed=0), "smc_scan_detect_sets")
        empty = state()
        assert int(empty[6][pad:pad + 4].view(np.uint32)[0]) == 0 and (empty[6][:pad] == fill).all() and (empty[6][pad + 4:] == fill).all()
        assert outputs_untouched(empty, cursor=True)
        joint, todo, rec = devplanes.scan_detect_sets(engine0, allocs[0], B, NL, listed[:0], [0], THR)
        assert joint.shape == (B, 0) and len(todo) == 0 and rec.shape == (B, 0)
        # the refusals launch nothing (the cursor is not zeroed either)
        reset()
        wrong = listed.copy()
        wrong[G - 1] = (NL, 0)                                             # what smc_scan_detect refuses
        many = np.arange(32770, dtype=np.uint32)                           # 65535 copies x 32769 sets >= 2^31
        for call, msg in ((lambda: _raw(engine0, bufs, wrong, SET_OFF), "names offset %d of %d" % (NL, NL)),
                          (lambda: _raw(engine0, bufs, listed, np.array([0, 1, 3, 6, G - 1], np.uint32)), "must tile"),
                          (lambda: _raw(engine0, bufs, listed, np.array([1, 1, 3, 6, G], np.uint32)), "must tile"),
                          (lambda: _raw(engine0, bufs, listed, np.array([0, 0, 3, 6, G], np.uint32)), "has 0 members"),
                          (lambda: _raw(engine0, bufs, listed, np.array([0, 1, 2, 3, 5, G], np.uint32)), "has 9 members"),
                          (lambda: _raw(engine0, bufs, listed, np.array([0, 3, 2, 6, G], np.uint32)), "members"),
                          (lambda: _raw(engine0, bufs, listed, many, n_copies=65535), "2\\^31")):
            with pytest.raises(_lib.SmcError, match=msg):
                _lib.check(call(), "smc_scan_detect_sets")
        assert outputs_untouched(state())
    finally:
        for b in allocs:
            b.free()
