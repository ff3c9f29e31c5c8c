"""--spikeIndelRpb on the GPU: smc_spike_indel_read_bits byte for byte - every byte of every row - and smc_spike_indel_rpb_counts word
for word against the restatement (tests/spike_indel_rpb_restate.py) on the hand-made BAM, bam_cigars and the synthetic BAM (whose
windows are wider than a workgroup); the bits' per-barcode sums against the pre-pass's four counters; made-up record lists for the
kernel's edges; an SNV-only list against smc_spike_rpb_counts; the refusals of both entries."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import abi, bamio, devplanes, fasta
from smcounter_amd.engine import DevBuf
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import spike_indel_reps_restate as QR  # noqa: E402
import spike_indel_restate as IR  # noqa: E402
import spike_indel_rpb_restate as XR  # noqa: E402
import spike_reps_restate as PR  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = XR.SEED
REPS, TARGETS, RPB = 3, (0.05, 0.3, 0.7), XR.RPB_TARGETS
ONE = 1 << 32


def _inputs(name, tmp):
    """-> (bam, fasta path, VcParams, the listed variants: SNVs, insertions and deletions)."""
    if name == "case":
        bam, fa, loci, P, variants = IR.make_case(tmp)
        return bam, fa, P, variants
    if name == "synth":
        return XR.synth_inputs(tmp)
    bam, fa, loci, P = ds_restate.load_fixture(name, tmp)
    return bam, fa, P, IR.pick_variants(bam, fa, loci, 4, gap=8)


def _device_records(eng, bam, fa, variants, P, rpb_targets):
    """The device's way from the file to what smc_spike_indel_rpb_counts takes, every step checked on the way: the pre-pass's runs
    (devplanes.spike_rules with four counters: alt1 from smc_allele_carriers on the copy spiked at 2^32, touch from
    smc_spike_indel_touch), smc_spike_indel_read_bits over each - EVERY byte of every row against the restatement of the run's records
    -, the first names from the file-wide table, the CSR -> (covers, records, read thresholds, per variant the bytes of its covering
    records in file order, their name identities, their first bits; the pre-pass's counters).  `rpb_targets` None (the hand-made
    BAM: one read name per barcode, a file the philox read sampler refuses - no probKeep is defined): no table, every name is its
    barcode's first, and the caller gives read thresholds of its own."""
    fasta_file = fasta.FastaFile(fa)
    keep = {}
    rules = devplanes.philox_read_rules(bam, list(rpb_targets), [P] * len(rpb_targets), SEED, eng) if rpb_targets is not None else []
    records, seen = [None] * len(variants), [None] * len(variants)
    py = bamio.BamFile(bam)
    try:
        devplanes.spike_rules(bam, fasta_file, variants, [0.5], [P], SEED, eng, keep=keep, indel_counters=True)
        spikes = keep["spikes"]
        for run in keep["runs"]:
            A = run.A
            svar, sorder = spikes.chrom_variants(run.chrom, 0.5)
            var = svar[[sorder.index(k) for k in run.group]]
            bits = devplanes.spike_indel_read_bits(eng, run.up, A, run.lo, var, spikes.ins[run.chrom])
            assert bits.shape == (len(run.group), len(A["aln"])) and bits.dtype == np.uint8 and not (bits & ~np.uint8(15)).any()
            assert not (bits[(bits & 1) == 0]).any()                                      # (the other bits only on a covering record)
            assert np.array_equal(devplanes.spike_indel_read_bits(eng, run.up, A, run.lo, var, spikes.ins[run.chrom]), bits)
            recs = py.fetch(run.chrom, run.lo, run.hi)
            assert len(recs) == len(A["aln"]) and [a.pos for a in recs] == A["aln"]["pos"].tolist()
            p_idents, shared = run.bam.pair_idents(A["n_pair"])
            assert not shared
            first = devplanes.run_first_names(eng, rules[0].groups, p_idents, run.chrom, run.lo, run.nl) if rules else np.ones(len(p_idents), bool)
            bc = A["aln"]["bc_gid"].astype(np.int64)
            for r, k in enumerate(run.group):
                want = np.array([XR.record_bits(a, variants[k], run.chrom, fasta_file)[0] for a in recs], np.uint8)
                assert np.array_equal(bits[r], want), (variants[k], np.flatnonzero(bits[r] != want)[:5])
                sums = np.stack([np.bincount(bc, weights=(bits[r] >> s) & 1, minlength=int(A["n_bc"])) for s in range(4)], axis=1).astype(np.uint32)
                gids = np.flatnonzero(sums[:, 0])
                assert np.array_equal(run.idents[gids], keep["covers"][k])
                assert np.array_equal(sums[gids], keep["counters"][k]), variants[k]      # (reads, alt0, alt1, touch) of the pre-pass
                records[k] = devplanes.spike_rpb_records(A, bits[r], gids, p_idents, first)
                assert not (records[k][2] & ~np.uint8(15)).any()
                idx = np.flatnonzero(bits[r])
                pair = A["aln"]["pair_gid"][idx]
                seen[k] = (bits[r][idx], p_idents[pair], first[pair])
        covers = keep["covers"]
    finally:
        py.close()
        devplanes.free_af_runs(keep.get("runs"))
        devplanes.close_rules(rules)
    return covers, records, [r.thr for r in rules], seen, keep["counters"]


@pytest.mark.parametrize("name", ("case", "bam_cigars", "synth"))
def test_bits_and_counts_equal_the_restatement(engine0, tmp_path, name):
    bam, fa, P, variants = _inputs(name, str(tmp_path))
    assert {v.kind for v in variants} == {af.SNV, af.INS, af.DEL}
    if name == "case":
        # (one read name per barcode: every name a first name, probKeep undefined - the bits are the point here, and the counts entry
        # takes read thresholds of the test's own)
        recs = XR.records(bam, fa, variants)
        assert all(r.first for rows in recs for r in rows)
        rthr = [PR.threshold(0.2), PR.threshold(0.6), ONE]
        want = XR.counts_from(recs, [v.pos for v in variants], [PR.threshold(t) for t in TARGETS], rthr, PR.seeds(SEED, REPS))
        covers, records, _, seen, counters = _device_records(engine0, bam, fa, variants, P, None)
    else:
        want, recs, rthr = XR.restate_counts(bam, fa, variants, TARGETS, RPB, SEED, REPS)
        covers, records, dev_rthr, seen, counters = _device_records(engine0, bam, fa, variants, P, RPB)
        assert dev_rthr == rthr and rthr[0] < ONE == rthr[-1]                             # (one target thins, one has probKeep >= 1)
    # entry 1 once more, through the file: the covering records in file order, their names and first bits
    for k, rows in enumerate(recs):
        got_bytes, got_names, got_first = seen[k]
        assert len(got_bytes) == len(rows) > 0
        assert np.array_equal(got_bytes, XR.record_bytes(rows)), variants[k]
        assert np.array_equal(got_names, XR.rp.fnv64([r.name for r in rows]))
        assert np.array_equal(got_first, np.array([r.first for r in rows], bool))
    if name == "synth":
        assert min(len(rows) for rows in recs) > 256 and any(len(rows) % 64 for rows in recs)     # (a window wider than one workgroup)
        indel = [k for k, v in enumerate(variants) if v.kind != af.SNV]
        assert all(sum(XR.cases(recs[k])[c] for k in indel) for c in XR.CASES)
    if name != "bam_cigars":
        assert any((c[:, 2] != c[:, 3]).any() for c, v in zip(counters, variants) if v.kind != af.SNV)     # (alt1 and touch are two numbers)
    # entry 2: every (v, j, t, r)
    pos, seeds, thr = [v.pos for v in variants], PR.seeds(SEED, REPS), [PR.threshold(t) for t in TARGETS]
    got = devplanes.spike_rpb_counts(engine0, pos, covers, records, seeds, thr, rthr, four=True)
    assert got.shape == want.shape == (len(variants), REPS, len(TARGETS), len(RPB), 5) and got.dtype == np.uint32
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(devplanes.spike_rpb_counts(engine0, pos, covers, records, seeds, thr, rthr, four=True), got)      # (two calls, the same words)
    assert len({got[:, j].tobytes() for j in range(REPS)}) >= 2                           # (the replicates draw differently)
    if name != "case":
        assert got[:, :, 2, 0, 3].sum() < got[:, :, 2, 2, 3].sum()                        # (the thinning takes records the rewrite would change)
    # the full read threshold: smc_spike_indel_counts at one depth threshold of 2^32, from the pre-pass's four counters
    depth = devplanes.spike_indel_counts(engine0, pos, covers, counters, seeds, thr, [ONE])
    assert np.array_equal(got[:, :, :, 2:3], depth)


def _made(sizes, seed=5, records=(1, 6), p_first=0.3, snv=False):
    """Records without a BAM: per variant `sizes[v]` barcodes of records[0] .. records[1] - 1 records each, random bits - an indel's
    (alt1 and touch two sets: a touched record with another anchor letter, an untouched one that shows the key) or, `snv`, alt1 = touch
    and alt0 only on such a record -> [[Rec]]."""
    rng = np.random.RandomState(seed)
    out = []
    for v, n in enumerate(sizes):
        rows = []
        for b in range(n):
            for i in range(rng.randint(*records)):
                touch = rng.rand() < 0.8
                if snv:
                    alt0, alt1 = bool(touch and rng.rand() < 0.4), touch
                else:
                    alt0 = bool(not touch and rng.rand() < 0.5)
                    alt1 = bool(rng.rand() < 0.85) if touch else alt0
                rows.append(XR.Rec("V%dB%dACGT" % (v, b), "q:V%dB%dACGT:%d" % (v, b, i), bool(rng.rand() < p_first), alt0, bool(alt1), bool(touch), None))
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
    flags = np.array([(1 if r.first else 0) | (2 if r.alt0 else 0) | (4 if r.alt1 else 0) | (8 if r.touch else 0) for r in flat], np.uint8)
    return PR.idents(texts), (off, XR.rp.fnv64([r.name for r in flat]) if flat else np.zeros(0, np.uint64), flags)


def _device(eng, recs, pos, seeds, thr, rthr, four=True):
    made = [_csr(rows) for rows in recs]
    return devplanes.spike_rpb_counts(eng, pos, [c for c, _ in made], [r for _, r in made], seeds, thr, rthr, four=four)


def test_a_variant_nobody_covers_between_two_that_are_covered(engine0):
    recs = _made([70, 0, 130])                                                           # (offsets 0, 70, 70, 200: not aligned to a wavefront)
    pos, seeds = [11, 5000, 1 << 20], PR.seeds(SEED, 2)
    thr, rthr = [PR.threshold(t) for t in (0.1, 0.5)], [PR.threshold(p) for p in (0.2, 0.7)]
    got = _device(engine0, recs, pos, seeds, thr, rthr)
    assert np.array_equal(got, XR.counts_from(recs, pos, thr, rthr, seeds))
    assert not got[1].any() and got[0].any() and got[2].any()
    assert int(got[0, :, :, :, 0].max()) <= 70 and int(got[2, :, :, :, 0].max()) <= 130


def test_a_barcode_of_two_hundred_records_and_barcodes_of_one_first_name(engine0):
    rng = np.random.RandomState(9)
    deep = [XR.Rec("DEEPACGT", "q:DEEPACGT:%d" % i, i == 17, bool(rng.rand() < 0.3), bool(rng.rand() < 0.6), bool(rng.rand() < 0.9), None) for i in range(200)]
    ones = [XR.Rec("ONE%dACGT" % b, "q:ONE%dACGT:0" % b, True, bool(b % 3 == 0), bool(b % 3 != 1), bool(b % 2), None) for b in range(90)]
    recs = [deep + ones, ones, deep]
    pos, seeds = [7, 8, 9], PR.seeds(SEED, 3)
    thr, rthr = [PR.threshold(t) for t in (0.2, 0.9)], [0, PR.threshold(0.01), PR.threshold(0.4)]
    got = _device(engine0, recs, pos, seeds, thr, rthr)
    assert np.array_equal(got, XR.counts_from(recs, pos, thr, rthr, seeds))
    assert (got[1, :, :, :, 0] == 90).all()                                               # (a first name stays at every threshold)
    assert (got[2, :, :, :, 0] == 1).all() and got[2, :, 1, 2, 3].max() > 20             # (the one barcode's kept touched records)


def test_barcodes_with_no_first_name_among_their_covering_records(engine0):
    recs = _made([150, 40], seed=3, records=(1, 4), p_first=0.0)
    pos, seeds = [300, 301], PR.seeds(SEED, 2)
    thr, rthr = [PR.threshold(0.5)], [0, PR.threshold(0.3), ONE]
    got = _device(engine0, recs, pos, seeds, thr, rthr)
    assert np.array_equal(got, XR.counts_from(recs, pos, thr, rthr, seeds))
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
    assert np.array_equal(got, XR.counts_from(recs, pos, thr, rthr, seeds))
    assert len({got[:, j].tobytes() for j in range(70)}) > 60


def test_more_than_eight_read_thresholds(engine0):
    """(the kernel's wide instance: up to 32 read thresholds, four counters each)"""
    recs = _made([130, 9])
    pos, seeds = [55, 66], PR.seeds(SEED, 2)
    thr, rthr = [PR.threshold(t) for t in (0.3, 0.6)], [PR.threshold(k / 12.0) for k in range(12)] + [ONE] * 4
    got = _device(engine0, recs, pos, seeds, thr, rthr)
    assert got.shape == (2, 2, 2, 16, 5) and np.array_equal(got, XR.counts_from(recs, pos, thr, rthr, seeds))
    ends = [PR.threshold(k / 31.0) for k in range(31)] + [ONE]                           # (32 read thresholds, one target)
    got = _device(engine0, recs, pos, seeds, thr[:1], ends)
    assert got.shape == (2, 2, 1, 32, 5) and np.array_equal(got, XR.counts_from(recs, pos, thr[:1], ends, seeds))


def test_one_replicate_and_the_ends_of_both_axes(engine0):
    recs = _made([210, 77], seed=11)
    pos, seeds = [1000, 2000], PR.seeds(SEED, 1)
    ends = _device(engine0, recs, pos, seeds, [0, ONE], [0, ONE])
    assert ends.shape == (2, 1, 2, 2, 5) and np.array_equal(ends, XR.counts_from(recs, pos, [0, ONE], [0, ONE], seeds))
    assert np.array_equal(_device(engine0, recs, pos, seeds, [0, ONE], [0, ONE]), ends)   # (two identical calls)
    counters = [XR.barcode_counters(rows) for rows in recs]
    assert any((c[:, 2] != c[:, 3]).any() for _, c in counters)
    depth = devplanes.spike_indel_counts(engine0, pos, [PR.idents(t) for t, _ in counters], [c for _, c in counters], seeds, [0, ONE], [ONE])
    assert np.array_equal(ends[:, :, :, 1:], depth)                                       # (read threshold 2^32: the whole barcodes' numbers)
    assert np.array_equal(depth, QR.counts_from(counters, pos, [0, ONE], seeds, [ONE]))
    for i, rows in enumerate(recs):
        with_first = {r.barcode for r in rows if r.first}
        assert ends[i, 0, 0, 0, 0] == ends[i, 0, 1, 0, 0] == len(with_first) < len(counters[i][0])      # (read threshold 0: first names only)
        assert ends[i, 0, 0, 0, 2] == 0 and ends[i, 0, 1, 0, 2] == len(with_first)
        assert ends[i, 0, 1, 0, 3] == sum(r.touch for r in rows if r.first)


def test_an_snv_only_list_gives_the_words_of_smc_spike_rpb_counts(engine0):
    recs = _made([190, 0, 33], seed=21, snv=True)
    assert all(r.alt1 == r.touch for rows in recs for r in rows)
    pos, seeds = [17, 18, 4000], PR.seeds(SEED, 3)
    thr = [PR.threshold(t) for t in (0.05, 0.5, 1.0)]
    for rthr in ([0, PR.threshold(0.3), ONE], [PR.threshold(k / 9.0) for k in range(10)]):      # (both instances)
        four = _device(engine0, recs, pos, seeds, thr, rthr)
        three = _device(engine0, recs, pos, seeds, thr, rthr, four=False)
        assert np.array_equal(four, three) and np.array_equal(four, XR.counts_from(recs, pos, thr, rthr, seeds)) and four[..., 3].any()
    # and where alt1 and touch differ the SNV entry does not see bit 3: the two entries are two numbers
    mixed = _made([120], seed=2)
    a, b = _device(engine0, mixed, [9], seeds, thr, [ONE]), _device(engine0, mixed, [9], seeds, thr, [ONE], four=False)
    assert not np.array_equal(a[..., 3], b[..., 3]) and np.array_equal(a[..., :3], b[..., :3])


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
        return eng.L.smc_spike_indel_rpb_counts(eng.ctx, src.data_ptr(), src.data_ptr(), off.ctypes.data, src.data_ptr(), rec_off.ctypes.data,
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
        assert b"smc_spike_indel_rpb_counts" in eng.L.smc_last_error()
    ok = np.zeros(3, abi.SPIKE_INDEL_VARIANT_DTYPE)
    ok["pos0"], ok["kind"], ok["ref"], ok["alt"], ok["len"] = [5, 9, 20], [0, 1, 2], ord("A"), [ord("G"), ord("A"), ord("A")], [0, 2, 3]

    def bits(var=ok, n_var=3, n_loci=30, start0=0, n_ins=2):
        var = np.ascontiguousarray(var)
        return eng.L.smc_spike_indel_read_bits(eng.ctx, src.data_ptr(), 16, src.data_ptr(), 16, src.data_ptr(), 16, src.data_ptr(), n_loci, start0,
                                               src.data_ptr(), var.ctypes.data, n_var, src.data_ptr(), n_ins, out.data_ptr(), None)

    def edit(**kw):
        v = ok.copy()
        for k, (i, x) in kw.items():
            v[k][i] = x
        return v
    for kw, msg in ((dict(var=edit(kind=(1, 3))), "variant 1 has kind 3"), (dict(var=edit(pos0=(1, 5))), "not strictly ascending"),
                    (dict(var=ok[::-1]), "not strictly ascending"), (dict(var=edit(pos0=(2, 10))), "footprint overlaps"),
                    (dict(var=edit(ref=(0, ord("N")))), "a letter outside ACGT"), (dict(var=edit(len=(2, 0))), "a length of 0"),
                    (dict(n_ins=1), "2 inserted letters at 0 (pool of 1)"), (dict(n_loci=20), "variant 2 names locus 20 of 20"),
                    (dict(start0=6), "variant 0 names locus -1 of 30"), (dict(var=np.zeros(4097, abi.SPIKE_INDEL_VARIANT_DTYPE), n_var=4097), "at most 4096")):
        assert bits(**kw) == -4 and msg.encode() in eng.L.smc_last_error(), msg
    eng.L.smc_device_sync(eng.ctx)
    assert (out.download(np.uint8, size) == 0x5A).all()                                       # nothing zeroed, nothing launched
    out.free(); src.free()
