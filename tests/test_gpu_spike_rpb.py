"""--spikeRpb on the GPU: smc_spike_read_bits byte for byte and smc_spike_rpb_counts word for word against the restatement
(tests/spike_rpb_restate.py) on the hand-made BAM, bam_cigars and the synthetic BAM; made-up record lists for the kernel's edges; the
refusals of both entries."""
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import devplanes, fasta
from smcounter_amd.engine import DevBuf
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import spike_depth_restate as DS  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402
import spike_rpb_restate as RR  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = RR.SEED
REPS, TARGETS, RPB = 3, (0.05, 0.3, 0.7), RR.RPB_TARGETS
ONE = 1 << 32


def _inputs(name, tmp):
    """-> (bam, fasta path, VcParams, the listed SNVs)."""
    if name == "case":
        bam, fa, loci, P, variants = SR.make_case(tmp)
        return bam, fa, P, variants
    if name == "synth":
        return RR.synth_inputs(tmp)
    bam, fa, loci, P = ds_restate.load_fixture(name, tmp)
    return bam, fa, P, SR.pick_positions(bam, fa, loci, 3)


def _device_records(eng, bam, fa, variants, P, rpb_targets):
    """The device's way from the file to what smc_spike_rpb_counts takes, every step checked on the way: the pre-pass's runs
    (devplanes.spike_rules: covers and (reads, alt0, single) per covering barcode), smc_spike_read_bits over each, the first names
    from the file-wide table at threshold 0, the CSR -> (covers, records, read thresholds, per variant the bytes of its covering
    records in file order, their name identities, their first bits; the pre-pass's counters)."""
    vs = [af.Variant(v.chrom, v.pos, v.ref, v.alt, v.alt, af.SNV) for v in variants]
    fasta_file = fasta.FastaFile(fa)
    keep = {}
    rules = devplanes.philox_read_rules(bam, list(rpb_targets), [P] * len(rpb_targets), SEED, eng)
    records, seen = [None] * len(vs), [None] * len(vs)
    try:
        devplanes.spike_rules(bam, fasta_file, vs, [0.5], [P], SEED, eng, keep=keep)
        for run in keep["runs"]:
            A = run.A
            var, ins = devplanes.af_run_variants([vs[k] for k in run.group], run.chrom, run.lo, fasta_file)
            bits = devplanes.spike_read_bits(eng, run.up, A, run.lo, var)
            assert bits.shape == (len(run.group), len(A["aln"])) and bits.dtype == np.uint8 and not (bits & ~np.uint8(7)).any()
            assert not (bits[(bits & 1) == 0]).any()                                      # (alt and single only on a covering record)
            _, _, cnt = devplanes.allele_carriers_run(eng, run.up, A, run.lo, var, ins, counts=True)
            p_idents, shared = run.bam.pair_idents(A["n_pair"])
            assert not shared
            first = devplanes.run_first_names(eng, rules[0].groups, p_idents, run.chrom, run.lo, run.nl)
            bc = A["aln"]["bc_gid"].astype(np.int64)
            for r, k in enumerate(run.group):
                sums = np.stack([np.bincount(bc, weights=(bits[r] >> s) & 1, minlength=int(A["n_bc"])) for s in range(3)], axis=1).astype(np.uint32)
                # per barcode the three bits sum to smc_allele_carriers' (reads, alt) and the pre-pass's `single`
                assert np.array_equal(sums[:, :2], cnt[r]), variants[k]
                gids = np.flatnonzero(sums[:, 0])
                assert np.array_equal(run.idents[gids], keep["covers"][k])
                assert np.array_equal(sums[gids], keep["counters"][k]), variants[k]
                records[k] = devplanes.spike_rpb_records(A, bits[r], gids, p_idents, first)
                idx = np.flatnonzero(bits[r])
                pair = A["aln"]["pair_gid"][idx]
                seen[k] = (bits[r][idx], p_idents[pair], first[pair])
        covers = keep["covers"]
    finally:
        devplanes.free_af_runs(keep.get("runs"))
        devplanes.close_rules(rules)
    return covers, records, [r.thr for r in rules], seen, keep["counters"]


@pytest.mark.parametrize("name", ("case", "bam_cigars", "synth"))
def test_bits_and_counts_equal_the_restatement(engine0, tmp_path, name):
    bam, fa, P, variants = _inputs(name, str(tmp_path))
    want, recs, rthr = RR.restate_counts(bam, fa, variants, TARGETS, RPB, SEED, REPS)
    covers, records, dev_rthr, seen, counters = _device_records(engine0, bam, fa, variants, P, RPB)
    assert dev_rthr == rthr and rthr[0] < ONE == rthr[-1]                                 # (one target thins, one has probKeep >= 1)
    # entry 1: every byte, no record skipped - the covering records in file order, their names and first bits
    compared = 0
    for k, rows in enumerate(recs):
        got_bytes, got_names, got_first = seen[k]
        assert len(got_bytes) == len(rows) > 0
        assert np.array_equal(got_bytes, RR.record_bytes(rows)), variants[k]
        assert np.array_equal(got_names, RR.rp.fnv64([r.name for r in rows]))
        assert np.array_equal(got_first, np.array([r.first for r in rows], bool))
        compared += len(rows)
    assert compared == sum(len(rows) for rows in recs)
    # entry 2: every (v, j, t, r)
    pos, seeds, thr = [v.pos for v in variants], PR.seeds(SEED, REPS), [PR.threshold(t) for t in TARGETS]
    got = devplanes.spike_rpb_counts(engine0, pos, covers, records, seeds, thr, rthr)
    assert got.shape == want.shape == (len(variants), REPS, len(TARGETS), len(RPB), 5) and got.dtype == np.uint32
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(devplanes.spike_rpb_counts(engine0, pos, covers, records, seeds, thr, rthr), got)      # (two calls, the same words)
    assert len({got[:, j].tobytes() for j in range(REPS)}) >= 2                           # (the replicates draw differently)
    assert got[:, :, 2, 0, 3].sum() < got[:, :, 2, 2, 3].sum()                            # (the thinning takes records the rewrite would change)
    # the full read threshold: smc_spike_depth_counts at one depth threshold of 2^32, from the pre-pass's counters
    depth = devplanes.spike_depth_counts(engine0, pos, covers, counters, seeds, thr, [ONE])
    assert np.array_equal(got[:, :, :, 2:3], depth)


def test_a_window_wider_than_a_workgroup(engine0, tmp_path):
    cfg = dataclasses.replace(R.SYNTH_CFG, n_umi=300, rpb=2)
    bam, fa, loci, P, A = R.synth_bam(str(tmp_path), cfg, 24)
    variants = SR.pick_positions(bam, fa, loci[8:12], 2)
    want, recs, rthr = RR.restate_counts(bam, fa, variants, TARGETS[:2], (1.5,), SEED, 2)
    assert min(len(rows) for rows in recs) > 256 and any(len(rows) % 64 for rows in recs)
    covers, records, dev_rthr, seen, counters = _device_records(engine0, bam, fa, variants, P, (1.5,))
    for k, rows in enumerate(recs):
        assert np.array_equal(seen[k][0], RR.record_bytes(rows)) and np.array_equal(seen[k][1], RR.rp.fnv64([r.name for r in rows]))
    got = devplanes.spike_rpb_counts(engine0, [v.pos for v in variants], covers, records, PR.seeds(SEED, 2), [PR.threshold(t) for t in TARGETS[:2]], rthr)
    assert dev_rthr == rthr and np.array_equal(got, want)


def _made(sizes, seed=5, records=(1, 6), p_first=0.3):
    """Records without a BAM: per variant `sizes[v]` barcodes of records[0] .. records[1] - 1 records each, random flags (alt only on
    a single-letter record) -> [[Rec]]."""
    rng = np.random.RandomState(seed)
    out = []
    for v, n in enumerate(sizes):
        rows = []
        for b in range(n):
            for i in range(rng.randint(*records)):
                single = rng.rand() < 0.8
                rows.append(RR.Rec("V%dB%dACGT" % (v, b), "q:V%dB%dACGT:%d" % (v, b, i), bool(rng.rand() < p_first), bool(single and rng.rand() < 0.4), bool(single)))
        rng.shuffle(rows)
        out.append(rows)
    return out


def _csr(rows):
    """[Rec] of one variant -> (covers, (offsets, name identities, flags)) as devplanes.spike_rpb_counts takes them."""
    texts = list(dict.fromkeys(r.barcode for r in rows))
    per = {b: [] for b in texts}
    for r in rows:
        per[r.barcode].append(r)
    flat = [r for b in texts for r in per[b]]
    off = np.zeros(len(texts) + 1, np.uint32)
    off[1:] = np.cumsum([len(per[b]) for b in texts])
    flags = np.array([(1 if r.first else 0) | (2 if r.alt else 0) | (4 if r.single else 0) for r in flat], np.uint8)
    return PR.idents(texts), (off, RR.rp.fnv64([r.name for r in flat]) if flat else np.zeros(0, np.uint64), flags)


def _device(eng, recs, pos, seeds, thr, rthr):
    made = [_csr(rows) for rows in recs]
    return devplanes.spike_rpb_counts(eng, pos, [c for c, _ in made], [r for _, r in made], seeds, thr, rthr)


def test_a_variant_nobody_covers_between_two_that_are_covered(engine0):
    recs = _made([70, 0, 130])                                                           # (offsets 0, 70, 70, 200: not aligned to a wavefront)
    pos, seeds = [11, 5000, 1 << 20], PR.seeds(SEED, 2)
    thr, rthr = [PR.threshold(t) for t in (0.1, 0.5)], [PR.threshold(p) for p in (0.2, 0.7)]
    got = _device(engine0, recs, pos, seeds, thr, rthr)
    assert np.array_equal(got, RR.counts_from(recs, pos, thr, rthr, seeds))
    assert not got[1].any() and got[0].any() and got[2].any()
    assert int(got[0, :, :, :, 0].max()) <= 70 and int(got[2, :, :, :, 0].max()) <= 130


def test_a_barcode_of_two_hundred_records_and_barcodes_of_one_first_name(engine0):
    rng = np.random.RandomState(9)
    deep = [RR.Rec("DEEPACGT", "q:DEEPACGT:%d" % i, i == 17, bool(rng.rand() < 0.5), bool(rng.rand() < 0.9)) for i in range(200)]
    ones = [RR.Rec("ONE%dACGT" % b, "q:ONE%dACGT:0" % b, True, bool(b % 3 == 0), bool(b % 3 != 1)) for b in range(90)]
    recs = [deep + ones, ones, deep]
    pos, seeds = [7, 8, 9], PR.seeds(SEED, 3)
    thr, rthr = [PR.threshold(t) for t in (0.2, 0.9)], [0, PR.threshold(0.01), PR.threshold(0.4)]
    got = _device(engine0, recs, pos, seeds, thr, rthr)
    assert np.array_equal(got, RR.counts_from(recs, pos, thr, rthr, seeds))
    assert (got[1, :, :, :, 0] == 90).all()                                               # (a first name stays at every threshold)
    assert (got[2, :, :, :, 0] == 1).all() and got[2, :, 1, 2, 3].max() > 20             # (the one barcode's kept single-letter records)


def test_barcodes_with_no_first_name_among_their_covering_records(engine0):
    recs = _made([150, 40], seed=3, records=(1, 4), p_first=0.0)
    pos, seeds = [300, 301], PR.seeds(SEED, 2)
    thr, rthr = [PR.threshold(0.5)], [0, PR.threshold(0.3), ONE]
    got = _device(engine0, recs, pos, seeds, thr, rthr)
    assert np.array_equal(got, RR.counts_from(recs, pos, thr, rthr, seeds))
    assert not got[:, :, :, 0].any()                                                      # (threshold 0 keeps first names only: nobody is there)
    assert (got[:, :, 0, 2, 0] == np.array([[150], [40]])).all() and 0 < got[0, 0, 0, 1, 0] < 150


def test_thirty_two_cells_and_more_replicates_than_the_grid_is_deep(engine0):
    recs = _made([300, 65])
    pos = [101, 202]
    thr = [PR.threshold(t) for t in (0.01, 0.05, 0.1, 0.2, 0.4, 0.6, 0.8, 1.0)]
    rthr = [PR.threshold(p) for p in (0.1, 0.25, 0.5)] + [ONE]
    seeds = PR.seeds(PR.M64 - 3, 70)                                                    # (70 replicates > the 64 the entry launches; the seeds wrap)
    got = _device(engine0, recs, pos, seeds, thr, rthr)
    assert got.shape == (2, 70, 8, 4, 5)
    assert np.array_equal(got, RR.counts_from(recs, pos, thr, rthr, seeds))
    assert len({got[:, j].tobytes() for j in range(70)}) > 60


def test_more_than_eight_read_thresholds(engine0):
    """(the kernel's second instance: up to 32 read thresholds)"""
    recs = _made([130, 9])
    pos, seeds = [55, 66], PR.seeds(SEED, 2)
    thr, rthr = [PR.threshold(t) for t in (0.3, 0.6)], [PR.threshold(k / 12.0) for k in range(12)] + [ONE] * 4
    got = _device(engine0, recs, pos, seeds, thr, rthr)
    assert got.shape == (2, 2, 2, 16, 5) and np.array_equal(got, RR.counts_from(recs, pos, thr, rthr, seeds))
    ends = [PR.threshold(k / 31.0) for k in range(31)] + [ONE]                           # (32 read thresholds, one target)
    got = _device(engine0, recs, pos, seeds, thr[:1], ends)
    assert got.shape == (2, 2, 1, 32, 5) and np.array_equal(got, RR.counts_from(recs, pos, thr[:1], ends, seeds))


def test_one_replicate_and_the_ends_of_both_axes(engine0):
    recs = _made([210, 77], seed=11)
    pos, seeds = [1000, 2000], PR.seeds(SEED, 1)
    ends = _device(engine0, recs, pos, seeds, [0, ONE], [0, ONE])
    assert ends.shape == (2, 1, 2, 2, 5) and np.array_equal(ends, RR.counts_from(recs, pos, [0, ONE], [0, ONE], seeds))
    assert np.array_equal(_device(engine0, recs, pos, seeds, [0, ONE], [0, ONE]), ends)   # (two identical calls)
    counters = [RR.barcode_counters(rows) for rows in recs]
    depth = devplanes.spike_depth_counts(engine0, pos, [PR.idents(t) for t, _ in counters], [c for _, c in counters], seeds, [0, ONE], [ONE])
    assert np.array_equal(ends[:, :, :, 1:], depth)                                       # (read threshold 2^32: the whole barcodes' numbers)
    assert np.array_equal(depth, DS.counts_from(counters, pos, [0, ONE], [ONE], seeds))
    for i, rows in enumerate(recs):
        with_first = {r.barcode for r in rows if r.first}
        assert ends[i, 0, 0, 0, 0] == ends[i, 0, 1, 0, 0] == len(with_first) < len(counters[i][0])      # (read threshold 0: first names only)
        assert ends[i, 0, 0, 0, 2] == 0 and ends[i, 0, 1, 0, 2] == len(with_first)
        assert ends[i, 0, 1, 0, 3] == sum(r.single for r in rows if r.first)


def test_refusals_launch_nothing(engine0):
    eng = engine0
    size = 8192
    out = DevBuf(eng, size).upload(np.full(size, 0x5A, np.uint8))
    src = DevBuf(eng, size).upload(np.zeros(size, np.uint8))
    half, above = np.full(40, 1 << 31, np.uint64), np.full(40, 1 << 31, np.uint64)
    above[1] = ONE + 1
    off = np.array([0, 3, 5], np.uint32)
    rec_off = np.array([0, 2, 2, 5, 6, 9], np.uint32)

    def counts(off=off, rec_off=rec_off, n_rec=9, n_var=2, n_reps=2, thr=half, n_targets=2, rthr=half, n_rthr=2):
        return eng.L.smc_spike_rpb_counts(eng.ctx, src.data_ptr(), src.data_ptr(), off.ctypes.data, src.data_ptr(), rec_off.ctypes.data,
                                          src.data_ptr(), src.data_ptr(), n_rec, src.data_ptr(), n_var, src.data_ptr(), n_reps, thr.ctypes.data,
                                          n_targets, rthr.ctypes.data, n_rthr, out.data_ptr(), None)
    for kw, msg in ((dict(n_targets=33, n_rthr=1), "33 targets, at most 32"), (dict(n_reps=1001), "1001 replicates, at most 1000"),
                    (dict(thr=above), "target 1: a threshold above 2^32"), (dict(off=np.array([0, 3, 2], np.uint32)), "offsets decrease"),
                    (dict(n_var=4097), "at most 4096"), (dict(rthr=above), "read threshold 1 is above 2^32"), (dict(n_rthr=0), "0 read thresholds"),
                    (dict(n_rthr=-1), "-1 read thresholds"), (dict(n_targets=3, n_rthr=11), "3 targets x 11 read thresholds, at most 32 cells"),
                    (dict(n_targets=32, n_rthr=2), "at most 32 cells"),
                    (dict(rec_off=np.array([0, 2, 1, 5, 6, 9], np.uint32)), "record offsets decrease at covering barcode 1"),
                    (dict(n_rec=8), "record offsets end at 9, beyond the 8 records")):
        assert counts(**kw) == -4 and msg.encode() in eng.L.smc_last_error(), msg            # SMC_E_INPUT
    var = np.zeros(3, devplanes.abi.AF_VARIANT_DTYPE)
    var["letter"] = ord("A")

    def bits(var=var, n_var=3, n_loci=10):
        return eng.L.smc_spike_read_bits(eng.ctx, src.data_ptr(), 16, src.data_ptr(), 16, src.data_ptr(), 16, src.data_ptr(), n_loci, 0,
                                         src.data_ptr(), var.ctypes.data, n_var, out.data_ptr(), None)
    beyond, indel = var.copy(), var.copy()
    beyond[2]["locus"], indel[1]["kind"] = 10, af.INS
    for kw, msg in ((dict(var=beyond), "variant 2 names locus 10 of 10"), (dict(var=indel), "variant 1 has kind 1, an SNV expected"),
                    (dict(n_var=4097), "at most 4096")):
        assert bits(**kw) == -4 and msg.encode() in eng.L.smc_last_error(), msg
    eng.L.smc_device_sync(eng.ctx)
    assert (out.download(np.uint8, size) == 0x5A).all()                                       # nothing zeroed, nothing launched
    out.free(); src.free()
