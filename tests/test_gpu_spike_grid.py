"""--spikeGrid on the GPU: smc_spike_grid_counts word for word against the restatement (tests/spike_grid_restate.py) on made-up
record lists - the kernel's edges, both instances, thresholds of the replicate's own - and on the synthetic BAM; its identities with
smc_spike_rpb_counts and smc_spike_depth_counts; smc_read_groups_counts_frac_seeds against single calls and the restatement; the
refusals of both entries."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import bamio, devplanes
from smcounter_amd.engine import DevBuf

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import spike_depth_restate as DS  # noqa: E402
import spike_grid_restate as G  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_rpb_restate as RR  # noqa: E402
import test_gpu_spike_rpb as TR  # noqa: E402  (its made-up records and its way from a BAM to the device's records)

pytestmark = pytest.mark.gpu
SEED = RR.SEED
ONE = 1 << 32
# rows of 1, 63, 64, 65 and 257 covering barcodes (a wavefront's edge, one barcode over a workgroup) and one nobody covers
SIZES = (1, 63, 0, 64, 65, 257)
POS = (3, 1 << 20, 77, 4000, 4001, 123456)


def _rows():
    """Per row of SIZES its records: barcodes of 1 .. 5 records in random order, and in the last row barcodes of 1, 2 and 70 records."""
    recs = TR._made(SIZES, seed=17)
    rng = np.random.RandomState(4)
    for name, n in (("LONE", 1), ("PAIR", 2), ("DEEP", 70)):
        recs[-1] += [RR.Rec(name + "ACGT", "q:%sACGT:%d" % (name, i), i == 0, bool(rng.rand() < 0.5), bool(rng.rand() < 0.9)) for i in range(n)]
    return recs


def _csr_with_empty(rows, empty=()):
    """TR._csr, with the barcodes `empty` added behind the others: covering barcodes of no record."""
    ident, (off, names, flags) = TR._csr(rows)
    if not empty:
        return ident, (off, names, flags)
    return (np.concatenate([ident, PR.idents(list(empty))]),
            (np.concatenate([off, np.full(len(empty), off[-1], np.uint32)]), names, flags))


def _device(eng, recs, pos, seeds, thr, bc_thr, rd_thr, empty=()):
    made = [_csr_with_empty(rows, empty if i == len(recs) - 1 else ()) for i, rows in enumerate(recs)]
    return devplanes.spike_grid_counts(eng, pos, [c for c, _ in made], [r for _, r in made], seeds, thr, bc_thr, rd_thr)


def _thresholds(n_reps, n_frac, n_rr, seed=1):
    """Barcode thresholds that end at f = 1 (2^32), and read thresholds that differ per replicate and include 0 and 2^32."""
    rng = np.random.RandomState(seed)
    bc = sorted(int(x) for x in rng.randint(ONE // 8, ONE, size=n_frac - 1).astype(np.int64)) + [ONE]
    rd = rng.randint(0, ONE, size=(n_reps, n_frac, n_rr)).astype(np.uint64)
    rd[0, 0, 0] = 0
    rd[-1, -1, -1] = ONE
    return bc, rd


@pytest.mark.parametrize("n_tgt,n_frac,n_rr,n_reps", [(1, 1, 1, 1), (3, 2, 4, 3), (3, 3, 3, 3), (1, 4, 8, 1), (1, 1, 9, 3)],
                         ids=["1x1x1", "3x8pairs", "3x9pairs", "32pairs", "9reads"])
def test_counts_equal_the_restatement_on_made_up_rows(engine0, n_tgt, n_frac, n_rr, n_reps):
    """(8 pairs: the small instance at its limit; 9 and 32: the large one at both ends)"""
    recs = _rows()
    seeds = PR.seeds(SEED, n_reps)
    thr = [PR.threshold(t) for t in (0.5, 0.05, 0.9)[:n_tgt]]
    bc, rd = _thresholds(n_reps, n_frac, n_rr)
    want = G.counts_from(recs, POS, thr, bc, rd, seeds)
    got = _device(engine0, recs, POS, seeds, thr, bc, rd, empty=("NOBODYACGT", "NOBODYTTTT"))
    assert got.shape == want.shape == (len(SIZES), n_reps, n_tgt, n_frac, n_rr, 5) and got.dtype == np.uint32
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(_device(engine0, recs, POS, seeds, thr, bc, rd, empty=("NOBODYACGT", "NOBODYTTTT")), got)     # (two calls, the same bytes)
    assert not got[2].any() and got[0].any() and got[5].any()                                # (the row nobody covers)
    assert (got[:, :, :, -1, :, 0].max(axis=(1, 2, 3)) <= np.array(SIZES) + np.array([0, 0, 0, 0, 0, 3])).all()
    if n_reps > 1 and n_frac * n_rr > 1:
        assert len({got[:, j].tobytes() for j in range(n_reps)}) == n_reps                  # (every replicate draws and thins on its own)


def test_a_majority_that_flips_and_a_barcode_that_leaves(engine0):
    """FLIP: a first name that shows ALT and two more reads that do not - carries the variant at read threshold 0 only.  GONE: no
    first name among its covering records - not there at read threshold 0.  DROP: whatever it holds, not there at barcode threshold 0."""
    rows = [RR.Rec("FLIPACGT", "q:FLIPACGT:0", True, True, True), RR.Rec("FLIPACGT", "q:FLIPACGT:1", False, False, True),
            RR.Rec("FLIPACGT", "q:FLIPACGT:2", False, False, False),
            RR.Rec("GONEACGT", "q:GONEACGT:1", False, True, True), RR.Rec("GONEACGT", "q:GONEACGT:2", False, True, True)]
    seeds = PR.seeds(SEED, 2)
    rd = np.array([[[0, ONE], [0, ONE]]] * 2, np.uint64)                                     # [R = 2][F = 2][Rr = 2]
    got = _device(engine0, [rows], [99], seeds, [0, ONE], [0, ONE], rd)
    assert np.array_equal(got, G.counts_from([rows], [99], [0, ONE], [0, ONE], rd, seeds))
    assert not got[0, :, :, 0].any()                                                         # (barcode threshold 0 keeps nobody)
    for j in range(2):
        # never hit (t = 0): read threshold 0 -> FLIP alone, carrying (1 of 1 ALT); 2^32 -> both there, GONE alone carrying (FLIP 1 of 3)
        assert got[0, j, 0, 1, 0].tolist() == [1, 1, 0, 0, 1] and got[0, j, 0, 1, 1].tolist() == [2, 1, 0, 0, 1]
        # always hit (t = 1): single letters 1 of 1 at 0; at 2^32 FLIP 2 of 3 and GONE 2 of 2 - READS' = 4, both carry when spiked
        assert got[0, j, 1, 1, 0].tolist() == [1, 1, 1, 1, 1] and got[0, j, 1, 1, 1].tolist() == [2, 1, 2, 4, 2]


def test_one_fraction_of_one_and_equal_thresholds_is_the_reads_per_barcode_entry(engine0):
    recs = _rows()
    seeds = PR.seeds(SEED, 3)
    thr = [PR.threshold(t) for t in (0.1, 0.6)]
    for rthr in ([0, PR.threshold(0.3), ONE], [PR.threshold(k / 11.0) for k in range(11)] + [ONE]):     # (3 pairs, 12 pairs: both instances)
        rd = np.tile(np.array(rthr, np.uint64), (len(seeds), 1, 1))
        got = _device(engine0, recs, POS, seeds, thr, [ONE], rd)
        rpb = TR._device(engine0, recs, POS, seeds, thr, rthr)
        assert got.shape == (len(SIZES), 3, 2, 1, len(rthr), 5) and np.array_equal(got[:, :, :, 0], rpb)


def test_one_read_threshold_of_one_is_the_depth_entry_on_the_barcode_sums(engine0):
    recs = _rows()
    seeds = PR.seeds(SEED, 3)
    thr, fracs = [PR.threshold(t) for t in (0.1, 0.6)], [0, DS.frac_thr(0.25), DS.frac_thr(0.5), ONE]
    counters = [RR.barcode_counters(rows) for rows in recs]
    depth = devplanes.spike_depth_counts(engine0, POS, [PR.idents(t) for t, _ in counters], [c for _, c in counters], seeds, thr, fracs)
    got = _device(engine0, recs, POS, seeds, thr, fracs, np.full((3, 4, 1), ONE, np.uint64))
    assert got.shape == (len(SIZES), 3, 2, 4, 1, 5) and np.array_equal(got[:, :, :, :, 0], depth)
    assert np.array_equal(depth, DS.counts_from(counters, POS, thr, fracs, seeds))


def test_more_replicates_than_the_grid_is_deep(engine0):
    recs = TR._made([130, 9])
    seeds = PR.seeds(PR.M64 - 3, 70)                                                        # (70 > the 64 the entry launches; the seeds wrap)
    bc, rd = _thresholds(70, 2, 2, seed=8)
    thr = [PR.threshold(0.4)]
    got = _device(engine0, recs, [55, 66], seeds, thr, bc, rd)
    assert got.shape == (2, 70, 1, 2, 2, 5) and np.array_equal(got, G.counts_from(recs, [55, 66], thr, bc, rd, seeds))


def _table(eng, path, chunk=1 << 20):
    groups = devplanes.ReadGroups(eng)
    bam = bamio.NativeBam(path)
    try:
        for first, keys in bam.name_keys(chunk, 4):
            groups.add(keys, first)
    finally:
        bam.close()
    groups.finish()
    assert groups.status() == 0
    return groups


@pytest.mark.parametrize("name", ("case", "bam_cigars"))
def test_counts_frac_seeds_equals_single_calls_and_the_restatement(engine0, tmp_path, name):
    path = (ds_restate.make_case(str(tmp_path)) if name == "case" else ds_restate.load_fixture(name, str(tmp_path)))[0]
    fracs = (0.1, 0.5, 1.0)
    bthr = [G.frac_threshold(f) for f in fracs]
    file_groups = RR.file_groups(path)
    groups = _table(engine0, path)
    try:
        for seeds in (PR.seeds(SEED, 1), PR.seeds(SEED, 3), PR.seeds(PR.M64 - 2, 70)):
            got = groups.counts_frac_seeds(seeds, bthr)
            assert got.shape == (len(seeds), 3, 4) and got.dtype == np.uint64
            for j, s in enumerate(seeds[:5]):
                single = groups.counts_frac(s, bthr)
                assert got[j].tolist() == [[c[k] for k in G.F_NAMES] for c in single]
            assert np.array_equal(got[:5].astype(np.int64), G.seed_counters(file_groups, fracs, seeds[:5]))
            assert np.array_equal(groups.counts_frac_seeds(seeds, bthr), got)
        assert len({got[j].tobytes() for j in range(70)}) > 1                                  # (the barcode draw moves with the seed)
        assert groups.counts_frac_seeds([], bthr).shape == (0, 3, 4) and groups.counts_frac_seeds([1, 2], []).shape == (2, 0, 4)
    finally:
        groups.close()


def test_thresholds_and_counts_equal_the_restatement_on_the_synthetic_bam(engine0, tmp_path):
    """From the file to the counters the device's way: the table, ONE counts_frac_seeds launch, probKeep and the thresholds on the host
    as philox_grid_rules makes them for one seed, the records as --spikeRpb makes them, one smc_spike_grid_counts call."""
    bam, fa, P, variants = RR.synth_inputs(str(tmp_path))
    targets, fracs, rpb, reps = (0.2, 0.05), (1.0, 0.5), (1.5, 3.0), 4
    seeds = PR.seeds(SEED, reps)
    assert G.keeps_a_multi_name_barcode(RR.file_groups(bam), fracs, seeds)
    want, recs, rd_thr, prob = G.restate_counts(bam, fa, variants, targets, fracs, rpb, SEED, reps)
    covers, records, _, seen, _ = TR._device_records(engine0, bam, fa, variants, P, rpb)
    groups = _table(engine0, bam)
    try:
        thr, p = devplanes.grid_read_thresholds(groups, seeds, fracs, rpb)
        assert thr.dtype == np.uint64 and np.array_equal(thr, rd_thr) and np.array_equal(p, prob)
        assert len({thr[j].tobytes() for j in range(reps)}) == reps and (thr[:, 0] == thr[0, 0]).all()      # (f = 1 keeps every barcode under any seed)
        cells = [(f, r) for f in fracs for r in rpb]
        for j, s in enumerate(seeds[:2]):                                                      # (one seed: philox_grid_rules' own thresholds)
            rules = devplanes.philox_grid_rules(bam, cells, [P] * len(cells), s, groups)
            assert [r.thr for r in rules] == [int(x) for x in thr[j].reshape(-1)]
            assert [r.bc_thr for r in rules] == [G.frac_threshold(f) for f, _ in cells]
    finally:
        groups.close()
    got = devplanes.spike_grid_counts(engine0, [v.pos for v in variants], covers, records, seeds, [PR.threshold(t) for t in targets],
                                      [G.frac_threshold(f) for f in fracs], thr)
    assert got.shape == want.shape == (len(variants), reps, 2, 2, 2, 5)
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert (got[:, :, :, 1, :, 0] < got[:, :, :, 0, :, 0]).all()                              # (half the barcodes: fewer are there)
    assert got[..., 0, 3].sum() < got[..., 1, 3].sum()                                       # (the thinning takes records the rewrite would change)


def test_refusals_launch_nothing(engine0, tmp_path):
    eng = engine0
    size = 8192
    out = DevBuf(eng, size).upload(np.full(size, 0x5A, np.uint8))
    src = DevBuf(eng, size).upload(np.zeros(size, np.uint8))
    half, above = np.full(80, 1 << 31, np.uint64), np.full(80, 1 << 31, np.uint64)
    above[1] = ONE + 1
    off = np.array([0, 3, 5], np.uint32)
    rec_off = np.array([0, 2, 2, 5, 6, 9], np.uint32)

    def counts(off=off, rec_off=rec_off, n_rec=9, n_var=2, n_reps=2, thr=half, n_targets=2, bthr=half, n_fracs=2, rthr=half, n_rthr=2):
        return eng.L.smc_spike_grid_counts(eng.ctx, src.data_ptr(), src.data_ptr(), off.ctypes.data, src.data_ptr(), rec_off.ctypes.data,
                                           src.data_ptr(), src.data_ptr(), n_rec, src.data_ptr(), n_var, src.data_ptr(), n_reps, thr.ctypes.data,
                                           n_targets, bthr.ctypes.data, n_fracs, src.data_ptr(), rthr.ctypes.data, n_rthr, out.data_ptr(), None)
    for kw, msg in ((dict(n_targets=33, n_fracs=1, n_rthr=1), "33 targets, at most 32"), (dict(n_reps=1001), "1001 replicates, at most 1000"),
                    (dict(thr=above), "target 1: a threshold above 2^32"), (dict(off=np.array([0, 3, 2], np.uint32)), "offsets decrease"),
                    (dict(n_var=4097), "at most 4096"), (dict(bthr=above), "depth threshold 1 is above 2^32"),
                    (dict(rthr=above), "read threshold 1 of replicate 0 is above 2^32"), (dict(n_rthr=0), "0 read thresholds"),
                    (dict(n_fracs=0), "0 fractions"), (dict(n_targets=3, n_fracs=3, n_rthr=4), "3 targets x 12 fraction x read-threshold pairs, at most 32 cells"),
                    (dict(n_targets=1, n_fracs=3, n_rthr=11), "at most 32 cells"),
                    (dict(rec_off=np.array([0, 2, 1, 5, 6, 9], np.uint32)), "record offsets decrease at covering barcode 1"),
                    (dict(n_rec=8), "record offsets end at 9, beyond the 8 records")):
        assert counts(**kw) == -4 and msg.encode() in eng.L.smc_last_error(), msg            # SMC_E_INPUT
    assert counts(n_fracs=-1) == -1 and counts(n_rthr=-1) == -1                              # SMC_E_ARG
    eng.L.smc_device_sync(eng.ctx)
    assert (out.download(np.uint8, size) == 0x5A).all()                                       # nothing zeroed, nothing launched
    # an accepted call zeroes its counters, whatever was there: one variant nobody covers
    none = np.zeros(2, np.uint32)
    assert counts(off=none, rec_off=np.zeros(1, np.uint32), n_rec=0, n_var=1) == 0
    eng.L.smc_device_sync(eng.ctx)
    back = out.download(np.uint8, size)
    n = 4 * 1 * 2 * 2 * 2 * 2 * 5
    assert not back[:n].any() and (back[n:] == 0x5A).all()
    out.free(); src.free()
    # the table's entry: a table that is not finished, too many seeds, a threshold above 2^32
    groups = devplanes.ReadGroups(eng)
    try:
        with pytest.raises(devplanes._lib.SmcError, match="the table is not finished"):
            groups.counts_frac_seeds([1], [ONE])
        groups.finish()
        with pytest.raises(devplanes._lib.SmcError, match="1001 seeds, at most 1000"):
            groups.counts_frac_seeds(range(1001), [ONE])
        with pytest.raises(devplanes._lib.SmcError, match="a threshold above 2\\^32"):
            groups.counts_frac_seeds([1], [ONE + 1])
        assert not groups.counts_frac_seeds([1, 2], [ONE, 5]).any()                           # (an empty file keeps nothing)
    finally:
        groups.close()
