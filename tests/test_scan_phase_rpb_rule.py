"""abi.scan_phase_rpb_counts_rule - the numpy twin of smc_scan_phase_rpb_counts, on the entry's own arrays - against the restatement
of --spikePhaseRpb (tests/spike_phase_rpb_restate.py: counts_from, per record, from the record lists alone) on made runs; and the
barcode-major arrays of a run (devplanes.run_barcode_major)."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, devplanes
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import scan_phase_rpb_made as MR  # noqa: E402

ZR, PR, ONE = MR.ZR, MR.PR, MR.ONE
SEED = ZR.SEED


@pytest.fixture(scope="module")
def made():
    """Sets of 1, 2 and 8 members and a set nobody covers jointly: a few hundred alignments, computed once and only read."""
    rows = MR._made([(1, 30, 0), (2, 0, 12), (8, 25, 10), (2, 40, 15)], seed=6)
    return rows, MR.MadeRun(rows, seed=2)


def test_the_barcode_major_arrays_are_a_stable_permutation(made):
    _, run = made
    o, bc = run.order, run.A["aln"]["bc_gid"].astype(np.int64)
    n = len(bc)
    assert 300 < n < 1500 and not np.array_equal(np.sort(bc), bc)                         # (the barcode ids are shuffled in file order)
    assert o["bm_aln"].dtype == np.uint32 and np.array_equal(np.sort(o["bm_aln"]), np.arange(n))
    walk = bc[o["bm_aln"]]
    assert (np.diff(walk) >= 0).all()
    same = np.diff(walk) == 0
    assert (np.diff(o["bm_aln"].astype(np.int64))[same] > 0).all() and same.any()         # (file order inside a barcode)
    per = np.bincount(bc, minlength=run.A["n_bc"])
    assert o["bc_start"].dtype == np.uint32 and len(o["bc_start"]) == run.A["n_bc"] + 1
    assert np.array_equal(o["bc_start"], np.concatenate([[0], np.cumsum(per)])) and int(o["bc_start"][-1]) == n
    pair = run.A["aln"]["pair_gid"][o["bm_aln"]]
    assert o["bm_name"].dtype == np.uint64 and np.array_equal(o["bm_name"], run.p_idents[pair])
    assert o["bm_first"].dtype == np.uint8 and np.array_equal(o["bm_first"], run.first[pair].astype(np.uint8))
    assert 0 < int(o["bm_first"].sum()) < n
    with pytest.raises(ValueError, match="a record of barcode"):
        devplanes.run_barcode_major(dict(run.A, n_bc=run.A["n_bc"] - 1), run.p_idents, run.first)
    empty = devplanes.run_barcode_major(dict(aln=np.zeros(0, MR.ALN_DTYPE), n_bc=3), np.zeros(0, np.uint64), np.zeros(0, bool))
    assert len(empty["bm_aln"]) == 0 and np.array_equal(empty["bc_start"], np.zeros(4, np.uint32))


def test_the_rule_equals_the_restatement(made):
    rows, run = made
    assert [len(r) for r in run.rows] == [1, 2, 8, 2] and [len(j) for j in run.joint] == [30, 0, 25, 40]
    assert (run.bits.sum(axis=0) == 0).any()                                              # (alignments of another amplicon lie in the walk)
    lead, seeds = [11, 5000, 1 << 20, 77], PR.seeds(SEED, 3)
    thr, rthr = [PR.threshold(t) for t in (0.1, 0.5)], [0, PR.threshold(0.2), PR.threshold(0.7), ONE]
    detail = []
    got = run.rule(lead, seeds, thr, rthr, detail=detail)
    want = ZR.counts_from(rows, lead, thr, rthr, seeds)
    assert got.shape == want.shape == (4, 3, 2, 4, 4) and got.dtype == np.uint32
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert not got[1].any() and got[0].any() and got[2].any() and got[3].any()
    assert len({got[:, j].tobytes() for j in range(3)}) == 3 and (got[3, :, :, 0, 0] < got[3, :, :, 3, 0]).all()
    assert [d.shape for d in detail] == [(3, 30, 1, 4, 3), (3, 0, 2, 4, 3), (3, 25, 8, 4, 3), (3, 40, 2, 4, 3)]
    assert all(MR.thinning_bites(detail, 3))
    # rows are independent: member rows of one behind the set rows leave the set rows as they are and equal sets of one member
    singles = [[v] for r in run.rows for v in r]
    covers = [np.flatnonzero(np.bincount(run.A["aln"]["bc_gid"][(run.bits[v[0]] & 1) != 0], minlength=run.A["n_bc"])) for v in singles]
    both = run.rule(lead + [9] * len(singles), seeds, thr, rthr, rows=run.rows + singles, joint=run.joint + covers)
    assert np.array_equal(both[:4], got)
    alone = ZR.counts_from([[m] for members in rows for m in members], [9] * len(singles), thr, rthr, seeds)
    assert np.array_equal(both[4:], alone) and alone.any()
    # the joint ids in any order, and an id beyond the run's barcodes reads nothing
    back = [j[::-1] for j in run.joint]
    assert np.array_equal(run.rule(lead, seeds, thr, rthr, joint=back), got)
    beyond = [np.concatenate([j, [run.A["n_bc"] + 5]]).astype(np.uint32) for j in run.joint]
    assert np.array_equal(run.rule(lead, seeds, thr, rthr, joint=beyond), got)


def test_the_draws_are_the_packages(made):
    ids = np.array([0, 1, 0xFFFFFFFFFFFFFFFF, 0x123456789ABCDEF0], np.uint64)
    for seed in (0, SEED, (1 << 64) - 1):
        assert np.array_equal(abi.philox_word0(ids, abi.SPIKE_DRAW_DOMAIN, 1234, seed), sv.draw(ids, seed, 1234))
        assert np.array_equal(abi.philox_word0(ids, abi.READ_DRAW_DOMAIN, 0, seed), MR.XR.RR.rp.draws(ids, seed))
    assert abi.SPIKE_DRAW_DOMAIN == sv.SPIKE_DOMAIN and abi.READ_DRAW_DOMAIN == devplanes.RPB_DOMAIN


def test_the_entry_is_declared_bound_and_a_second_source_of_the_one_body():
    text = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"#define SMC_ABI_VERSION 11\b", text)
    assert re.search(r"\bint smc_scan_phase_rpb_counts\(smc_ctx\* ctx, const uint32_t\* d_bm_aln, const uint64_t\* d_bm_name,", text)
    assert "--spikeScanMnvRpb" in text and "smc_scan_phase_rpb_counts" in _lib.SYMBOLS
    L = _lib.load()
    assert L.smc_abi_version() == 11 and len(L.smc_scan_phase_rpb_counts.argtypes) == 28
    kernels = open(os.path.join(ROOT, "smcounter_amd", "csrc", "k_spike_rpb.inc")).read()
    host = open(os.path.join(ROOT, "smcounter_amd", "csrc", "host_abi.inc")).read()
    # ONE body: both kernels are a record source handed to spr_counts, which alone holds the walk, the draws and the reduction
    assert len(re.findall(r"void spr_counts\(", kernels)) == 1 and len(re.findall(r"rg_draw\(src\.name\(i\), seed\)", kernels)) == 1
    assert len(re.findall(r"spr_counts<MAXR, \w+, \w+>\(src,", kernels)) == 2 and len(re.findall(r"__ballot\(there && hit\)", kernels)) == 2
    assert "k_spr_run_counts<8>" in host and "k_spr_run_counts<SMC_RG_MAX_TARGETS>" in host and "asm" not in kernels
    assert devplanes.SCAN_BITS_BUDGET == 256 << 20
    assert devplanes.scan_set_chunks(10, 2, 1 << 20, 8 << 20) == [(0, 4), (4, 8), (8, 10)]
    assert devplanes.scan_set_chunks(3, 2, 1 << 30) == [(0, 1), (1, 2), (2, 3)] and devplanes.scan_set_chunks(0, 2, 5) == []
