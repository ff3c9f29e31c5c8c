"""smc_scan_phase_rpb_counts on the GPU: word for word against BOTH smc_spike_phase_rpb_counts on spike_joint_records' CSR of the same
made run (the existing host path) AND the numpy rule (abi.scan_phase_rpb_counts_rule) - the made runs of tests/scan_phase_rpb_made.py,
whose record lists are those of tests/test_gpu_spike_phase_rpb.py laid out as one decoded run; the refusals, which leave a poisoned
output as it is."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import devplanes
from smcounter_amd.engine import DevBuf

sys.path.insert(0, os.path.join(ROOT, "tests"))
import scan_phase_rpb_made as MR  # noqa: E402
from test_gpu_spike_phase_rpb import _device  # noqa: E402

pytestmark = pytest.mark.gpu
ZR, PR, ONE = MR.ZR, MR.PR, MR.ONE
SEED = ZR.SEED


def _scan(eng, run, lead, seeds, thr, rthr, rows=None, joint=None):
    """The made run's order and bits go up, the entry runs once, everything is freed."""
    order = devplanes.RunOrder(eng, run.order, run.idents)
    d_bits = DevBuf(eng, run.bits.size + 256).upload(run.bits.reshape(-1) if run.bits.size else np.zeros(4, np.uint8))
    try:
        return devplanes.scan_phase_rpb_counts(eng, order, d_bits, run.n_var, run.rows if rows is None else rows,
                                               run.joint if joint is None else joint, lead, seeds, thr, rthr)
    finally:
        d_bits.free()
        order.free()


def _three_ways(eng, rows, run, lead, seeds, thr, rthr, detail=None):
    """-> the entry's words, after holding them against the existing entry on the host's CSR and against the numpy rule."""
    got = _scan(eng, run, lead, seeds, thr, rthr)
    csr, joint, _ = _device(eng, rows, lead, seeds, thr, rthr)
    rule = run.rule(lead, seeds, thr, rthr, detail=detail)
    assert [len(j[0]) for j in joint] == [len(j) for j in run.joint]
    assert got.shape == csr.shape == rule.shape and got.dtype == np.uint32
    assert np.array_equal(got, csr), np.argwhere(got != csr)[:5]
    assert np.array_equal(got, rule), np.argwhere(got != rule)[:5]
    return got


def test_sets_of_one_two_and_eight_members_a_set_nobody_covers_and_member_rows_behind_them(engine0):
    eng = engine0
    rows = MR._made([(1, 70, 0), (2, 0, 25), (8, 130, 40), (2, 90, 30)])
    run = MR.MadeRun(rows, seed=3)
    lead, seeds = [11, 5000, 1 << 20, 77], PR.seeds(SEED, 3)
    thr, rthr = [PR.threshold(t) for t in (0.1, 0.5)], [PR.threshold(0.2), PR.threshold(0.7), ONE]
    detail = []
    got = _three_ways(eng, rows, run, lead, seeds, thr, rthr, detail)
    assert [len(j) for j in run.joint] == [70, 0, 130, 90] and (run.bits.sum(axis=0) == 0).any()
    assert not got[1].any() and got[0].any() and got[2].any() and got[3].any()
    # thinning bites in these inputs: a barcode out of one member's pileup only, a majority that flips at one member only
    assert all(MR.thinning_bites(detail, 2))
    # a record that spans both members: one alignment with a byte at two bit rows
    assert ((run.bits[run.rows[3][0]] & 1) & (run.bits[run.rows[3][1]] & 1)).any()
    # two calls, the same words; the joint lists in descending id order
    assert np.array_equal(_scan(eng, run, lead, seeds, thr, rthr), got)
    assert np.array_equal(_scan(eng, run, lead, seeds, thr, rthr, joint=[j[::-1].copy() for j in run.joint]), got)
    # member rows of one behind the set rows in one call: the set rows are those of the call without them, the member rows listed variants
    singles = [[v] for r in run.rows for v in r]
    bc = run.A["aln"]["bc_gid"]
    covers = [np.flatnonzero(np.bincount(bc[(run.bits[v[0]] & 1) != 0], minlength=run.A["n_bc"])).astype(np.uint32) for v in singles]
    both = _scan(eng, run, lead + [9] * len(singles), seeds, thr, rthr, rows=run.rows + singles, joint=run.joint + covers)
    assert np.array_equal(both[:4], got)
    alone = ZR.counts_from([[m] for members in rows for m in members], [9] * len(singles), thr, rthr, seeds)
    assert np.array_equal(both[4:], alone) and alone.any()


def test_three_hundred_joint_barcodes_and_a_barcode_deep_at_one_member(engine0):
    rng = np.random.RandomState(9)
    rows = MR._made([(3, 300, 20)], seed=4)[0]
    deep = [MR._rec(rng, "DEEPACGT", "q:DEEPACGT:%d" % i, i == 17, False) for i in range(200)]
    rows[0] += deep
    rows[1] += [MR._rec(rng, "DEEPACGT", "q:DEEPACGT:199", False, False)]                 # (200 records at one member, 1 at another)
    rows[2] += deep[:3]
    run = MR.MadeRun([rows], seed=5)
    assert len(run.joint[0]) == 301 and int(np.diff(run.order["bc_start"].astype(np.int64)).max()) >= 200
    lead, seeds = [9], PR.seeds(SEED, 3)
    thr, rthr = [PR.threshold(t) for t in (0.2, 0.9)], [0, PR.threshold(0.01), PR.threshold(0.4), ONE]
    got = _three_ways(engine0, [rows], run, lead, seeds, thr, rthr)
    assert (got[0, :, :, 3, 0] == 301).all() and (got[0, :, :, 0, 0] < 301).all()


def test_barcodes_of_first_names_only_and_barcodes_without_one(engine0):
    firsts = MR._made([(2, 150, 10)], seed=3, records=(1, 4), p_first=1.0)
    none = MR._made([(2, 150, 10), (3, 40, 0)], seed=3, records=(1, 4), p_first=0.0)
    seeds, thr, rthr = PR.seeds(SEED, 2), [PR.threshold(0.5)], [0, PR.threshold(0.3), ONE]
    got = _three_ways(engine0, firsts, MR.MadeRun(firsts, seed=7, strangers=0), [300], seeds, thr, rthr)
    assert (got[0, :, :, :, 0] == 150).all()                                              # (a first name stays at every threshold)
    got = _three_ways(engine0, none, MR.MadeRun(none, seed=8, strangers=0), [300, 301], seeds, thr, rthr)
    assert not got[:, :, :, 0].any()                                                      # (threshold 0 keeps first names only: nobody is there)
    assert (got[:, :, 0, 2, 0] == np.array([[150], [40]])).all() and 0 < got[0, 0, 0, 1, 0] < 150


def test_thirty_two_cells_and_more_replicates_than_the_grid_is_deep(engine0):
    rows = MR._made([(2, 300, 10), (4, 65, 5)])
    thr = [PR.threshold(t) for t in (0.01, 0.05, 0.1, 0.2, 0.4, 0.6, 0.8, 1.0)]
    rthr = [PR.threshold(p) for p in (0.1, 0.25, 0.5)] + [ONE]
    seeds = PR.seeds(PR.M64 - 3, 70)                                                    # (70 replicates > the 64 the entry launches; the seeds wrap)
    run = MR.MadeRun(rows, seed=9)
    got = _scan(engine0, run, [101, 202], seeds, thr, rthr)
    assert got.shape == (2, 70, 8, 4, 4)
    assert np.array_equal(got, _device(engine0, rows, [101, 202], seeds, thr, rthr)[0])
    assert np.array_equal(got, run.rule([101, 202], seeds, thr, rthr))
    assert len({got[:, j].tobytes() for j in range(70)}) > 60


def test_nine_read_thresholds_take_the_wide_instance(engine0):
    rows = MR._made([(2, 130, 9), (8, 9, 3)])
    run = MR.MadeRun(rows, seed=10)
    lead, seeds = [55, 66], PR.seeds(SEED, 2)
    thr, rthr = [PR.threshold(t) for t in (0.3, 0.6)], [PR.threshold(k / 8.0) for k in range(8)] + [ONE]
    got = _three_ways(engine0, rows, run, lead, seeds, thr, rthr)
    assert got.shape == (2, 2, 2, 9, 4)
    ends = [PR.threshold(k / 31.0) for k in range(31)] + [ONE]                           # (32 read thresholds, one target)
    got = _three_ways(engine0, rows, run, lead, seeds, thr[:1], ends)
    assert got.shape == (2, 2, 1, 32, 4) and (np.diff(got[:, :, :, :, 0].astype(np.int64), axis=3) >= 0).all()


def test_the_call_zeroes_a_poisoned_output_and_an_index_beyond_the_run_reads_nothing(engine0):
    eng = engine0
    rows = MR._made([(2, 40, 5)], seed=12)
    run = MR.MadeRun(rows, seed=11)
    lead, seeds, thr, rthr = [31], PR.seeds(SEED, 2), [0, PR.threshold(0.4)], [PR.threshold(0.5), ONE]      # (target 0: S_ALL' is 0, a word no atomic touches)
    want = run.rule(lead, seeds, thr, rthr)
    order = devplanes.RunOrder(eng, run.order, run.idents)
    d_bits = DevBuf(eng, run.bits.size + 256).upload(run.bits.reshape(-1))
    row_off, joint_off = np.array([0, 2], np.uint32), np.array([0, len(run.joint[0]) + 1], np.uint32)
    row_var = np.array(run.rows[0], np.uint32)
    gids = np.concatenate([run.joint[0], [run.A["n_bc"] + 7]]).astype(np.uint32)         # (an id that is not below n_bc: no records, no count)
    n_out = want.size
    ups = [devplanes._up8(eng, a) for a in (row_off, row_var, joint_off, gids, np.array(lead, np.uint32), np.array(seeds, np.uint64))]
    out = DevBuf(eng, 4 * n_out + 256).upload(np.full(4 * n_out + 256, 0x5A, np.uint8))
    t, q = np.array(thr, np.uint64), np.array(rthr, np.uint64)
    try:
        o = order.bufs
        rc = eng.L.smc_scan_phase_rpb_counts(eng.ctx, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), order.n_aln, o[3].data_ptr(),
                                             order.host["bc_start"].ctypes.data, o[4].data_ptr(), order.n_bc, d_bits.data_ptr(), run.n_var,
                                             ups[0].data_ptr(), row_off.ctypes.data, ups[1].data_ptr(), row_var.ctypes.data, ups[2].data_ptr(),
                                             joint_off.ctypes.data, ups[3].data_ptr(), ups[4].data_ptr(), 1, ups[5].data_ptr(), len(seeds),
                                             t.ctypes.data, len(t), q.ctypes.data, len(q), out.data_ptr(), None)
        assert rc == 0, eng.L.smc_last_error()
        got = out.download(np.uint32, n_out).reshape(want.shape)
        tail = out.download(np.uint8, 256, 4 * n_out)
    finally:
        for b in ups + [out, d_bits]:
            b.free()
        order.free()
    assert np.array_equal(got, want) and want.any() and (want == 0).any() and (tail == 0x5A).all()


def test_refusals_launch_nothing(engine0):
    eng = engine0
    size = 8192
    out = DevBuf(eng, size).upload(np.full(size, 0x5A, np.uint8))
    src = DevBuf(eng, size).upload(np.zeros(size, np.uint8))
    half, above = np.full(40, 1 << 31, np.uint64), np.full(40, 1 << 31, np.uint64)
    above[1] = ONE + 1
    row_off, row_var = np.array([0, 2, 5], np.uint32), np.array([0, 1, 2, 3, 4], np.uint32)
    joint_off, bc_start = np.array([0, 2, 3], np.uint32), np.array([0, 3, 3, 9], np.uint32)

    def counts(row_off=row_off, row_var=row_var, joint_off=joint_off, bc_start=bc_start, n_aln=9, n_bc=3, n_var=5, n_rows=2, n_reps=2, thr=half,
               n_targets=2, rthr=half, n_rthr=2):
        p = src.data_ptr()
        return eng.L.smc_scan_phase_rpb_counts(eng.ctx, p, p, p, n_aln, p, bc_start.ctypes.data, p, n_bc, p, n_var, p, row_off.ctypes.data, p,
                                               row_var.ctypes.data, p, joint_off.ctypes.data, p, p, n_rows, p, n_reps, thr.ctypes.data,
                                               n_targets, rthr.ctypes.data, n_rthr, out.data_ptr(), None)
    many = np.zeros(4098, np.uint32)
    for kw, msg in ((dict(row_off=np.array([0, 3, 2], np.uint32)), "row offsets decrease at row 1"),
                    (dict(joint_off=np.array([0, 3, 2], np.uint32)), "joint offsets decrease at row 1"),
                    (dict(row_off=np.array([0, 2, 11], np.uint32)), "row 1 has 9 members, 1 .. 8 expected"),
                    (dict(row_off=np.array([0, 0, 3], np.uint32)), "row 0 has 0 members"),
                    (dict(row_var=np.array([0, 1, 2, 5, 4], np.uint32)), "member 3 names bit row 5 of 5"),
                    (dict(n_var=4), "member 4 names bit row 4 of 4"),
                    (dict(bc_start=np.array([0, 4, 3, 9], np.uint32)), "barcode starts decrease at barcode 1"),
                    (dict(bc_start=np.array([0, 3, 3, 8], np.uint32)), "barcode starts end at 8, not at the 9 alignments"),
                    (dict(n_aln=10), "barcode starts end at 9, not at the 10 alignments"),
                    (dict(thr=above), "target 1: a threshold above 2^32"), (dict(rthr=above), "read threshold 1 is above 2^32"),
                    (dict(n_rthr=0), "0 read thresholds"), (dict(n_rthr=-1), "-1 read thresholds"),
                    (dict(n_targets=3, n_rthr=11), "3 targets x 11 read thresholds, at most 32 cells"),
                    (dict(n_targets=32, n_rthr=2), "at most 32 cells"), (dict(n_targets=33, n_rthr=1), "33 targets, at most 32"),
                    (dict(n_reps=1001), "1001 replicates, at most 1000"),
                    # (an output of 2^32 - 256 words or more: checked, and out of reach - 4096 rows x 1000 replicates x 32 cells x 4 is below it)
                    (dict(n_rows=4097, row_off=many, joint_off=many), "4097 rows, at most 4096")):
        assert counts(**kw) == -4 and msg.encode() in eng.L.smc_last_error(), (msg, eng.L.smc_last_error())            # SMC_E_INPUT
        assert eng.L.smc_last_error().startswith(b"smc_scan_phase_rpb_counts:")
    eng.L.smc_device_sync(eng.ctx)
    assert (out.download(np.uint8, size) == 0x5A).all()                                       # nothing zeroed, nothing launched
    out.free(); src.free()
