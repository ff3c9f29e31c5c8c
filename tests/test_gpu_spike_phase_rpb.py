"""--spikePhaseRpb on the GPU: smc_spike_phase_rpb_counts word for word against the restatement (tests/spike_phase_rpb_restate.py) - on
the synthetic case and bam_cigars through the device's own path (the read bits entry, spike_rpb_records, spike_joint_records) and on
made-up record lists for the kernel's edges; its two equivalences against smc_spike_indel_rpb_counts and smc_spike_indel_phase_counts on
the device; an SNV-only list fed with smc_spike_read_bits' bytes; the refusals."""
import collections
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import devplanes, fasta
from smcounter_amd.engine import DevBuf
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import spike_indel_restate as IR  # noqa: E402
import spike_phase_rpb_restate as ZR  # noqa: E402

pytestmark = pytest.mark.gpu
XR, PR = ZR.XR, ZR.PR
SEED, ONE = ZR.SEED, ZR.ONE
REPS, TARGETS, RPB = 3, (0.05, 0.3, 0.7), ZR.RPB_TARGETS


def _phased(variants, sets):
    return sv.PhasedVariants(variants, [sv.PhaseSet("hap%d" % g, variants[m[0]].chrom, tuple(m)) for g, m in enumerate(sets)])


def _inputs(name, tmp):
    """-> (bam, fasta path, VcParams, the listed variants, the sets as tuples of indexes)."""
    if name == "synth":
        bam, fa, _, P, variants, sets = ZR.synth_case(tmp)
        return bam, fa, P, variants, sets
    bam, fa, loci, P = ds_restate.load_fixture(name, tmp)
    variants = IR.pick_variants(bam, fa, loci, 6, gap=8)                                # (two chromosomes: a set lies on one)
    sets = [(0, 1), (2, 3)]
    assert all(len({variants[k].chrom for k in m}) == 1 for m in sets)
    return bam, fa, P, variants, sets


@pytest.mark.parametrize("name", ("synth", "bam_cigars"))
def test_the_device_path_equals_the_restatement(engine0, tmp_path, name):
    """From the file to the counts the way a run goes: the pre-pass with four counters and the sets' draws, the read bits entry over
    every run - the bits' per-barcode sums against the pre-pass's counters -, the first names from the file-wide table,
    spike_rpb_records per variant, spike_joint_records per set, then the entry."""
    eng = engine0
    bam, fa, P, variants, sets = _inputs(name, str(tmp_path))
    assert {v.kind for v in variants} == {af.SNV, af.INS, af.DEL} and all(len(m) == 2 for m in sets)
    want, recs, rthr = ZR.restate_counts(bam, fa, variants, sets, TARGETS, RPB, SEED, REPS)
    listed = _phased(variants, sets)
    psets = sv.phase_sets(listed)
    keep, records = {}, [None] * len(variants)
    rules = devplanes.philox_read_rules(bam, list(RPB), [P] * len(RPB), SEED, eng)
    try:
        devplanes.spike_rules(bam, fasta.FastaFile(fa), listed, [0.5], [P], SEED, eng, keep=keep, indel_counters=True, phase=dict(sets=psets))
        spikes = keep["spikes"]
        for run in keep["runs"]:
            A = run.A
            svar, sorder = spikes.chrom_variants(run.chrom, 0.5)
            bits = devplanes.spike_indel_read_bits(eng, run.up, A, run.lo, svar[[sorder.index(k) for k in run.group]], spikes.ins[run.chrom])
            p_idents, shared = run.bam.pair_idents(A["n_pair"])
            assert not shared
            first = devplanes.run_first_names(eng, rules[0].groups, p_idents, run.chrom, run.lo, run.nl)
            bc = A["aln"]["bc_gid"].astype(np.int64)
            for r, k in enumerate(run.group):
                sums = np.stack([np.bincount(bc, weights=(bits[r] >> s) & 1, minlength=int(A["n_bc"])) for s in range(4)], axis=1).astype(np.uint32)
                gids = np.flatnonzero(sums[:, 0])
                assert np.array_equal(run.idents[gids], keep["covers"][k])
                assert np.array_equal(sums[gids], keep["counters"][k]), variants[k]      # (reads, alt0, alt1, touch) of the pre-pass
                records[k] = devplanes.spike_rpb_records(A, bits[r], gids, p_idents, first)
        covers = keep["covers"]
        assert [r.thr for r in rules] == rthr and rthr[0] < ONE == rthr[-1]
    finally:
        devplanes.free_af_runs(keep.get("runs"))
        devplanes.close_rules(rules)
    joint = devplanes.spike_joint_records(psets, covers, records)
    for g, (ids, off, names, flags) in enumerate(joint):
        rows = [recs[k] for k in sets[g]]
        assert np.array_equal(ids, np.sort(PR.idents(ZR.joint_names(rows)))) and np.all(np.diff(ids.astype(np.uint64)) > 0)
        assert len(off) == 2 * len(ids) + 1 and int(off[-1]) == len(names) == len(flags) and not (flags & ~np.uint8(15)).any()
    lead = [spikes.lead_pos[ps.members[0]] for ps in psets]
    assert lead == [min(variants[k].pos for k in m) for m in sets]
    seeds, thr = PR.seeds(SEED, REPS), [PR.threshold(t) for t in TARGETS]
    got = devplanes.spike_phase_rpb_counts(eng, lead, [2, 2], joint, seeds, thr, rthr)
    assert got.shape == want.shape == (2, REPS, len(TARGETS), len(RPB), 4) and got.dtype == np.uint32
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(devplanes.spike_phase_rpb_counts(eng, lead, [2, 2], joint, seeds, thr, rthr), got)      # (two calls, the same words)
    assert len({got[:, j].tobytes() for j in range(REPS)}) >= 2
    # the full read threshold: smc_spike_indel_phase_counts at one depth threshold of 2^32, from the pre-pass's joint rows
    whole = devplanes.spike_indel_phase_counts(eng, lead, devplanes.spike_joint(psets, covers, keep["counters"]), seeds, thr, [ONE])
    assert np.array_equal(got[:, :, :, 2:3], whole)
    if name == "synth":
        assert (got[:, :, :, 0, 0] < got[:, :, :, 2, 0]).all()                            # (thinning takes barcodes out of a member's pileup)


# ---- made-up record lists
def _made(shapes, seed=5, records=(1, 6), p_first=0.3, snv=False):
    """Records without a BAM -> per set, per member its [Rec].  shapes[g] = (members, joint barcodes, barcodes that miss a member): a
    barcode owns 1 .. records[1] - 1 read names (each a first name with p_first, the same at every member); at every member it covers
    it shows a random non-empty choice of them, so a name can stand under several members, with bits of that member's own.  One
    barcode in four carries the whole set already: most of its records show the key as they are."""
    rng = np.random.RandomState(seed)
    out = []
    for g, (M, n, part) in enumerate(shapes):
        rows = [[] for _ in range(M)]
        for b in range(n + part):
            bc = "S%dB%dACGT" % (g, b)
            names = [("q:%s:%d" % (bc, i), bool(rng.rand() < p_first)) for i in range(rng.randint(*records))]
            carrier = bool(rng.rand() < 0.25)
            cover = list(range(M))
            if b >= n:
                cover = [m for m in cover if rng.rand() < 0.5][:M - 1] or [int(rng.randint(M))] if M > 1 else []
            for m in cover:
                mine = [x for x in names if rng.rand() < 0.7] or [names[int(rng.randint(len(names)))]]
                for name, first in mine:
                    rows[m].append(_rec(rng, bc, name, first, snv, carrier))
        for r in rows:
            rng.shuffle(r)
        out.append(rows)
    return out


def _rec(rng, bc, name, first, snv=False, carrier=False):
    touch = rng.rand() < 0.8
    if carrier and rng.rand() < 0.9:
        return XR.Rec(bc, name, first, True, True, bool(snv), None)          # (shows the key already: an indel's rewrite leaves it alone)
    if snv:
        alt0, alt1 = bool(touch and rng.rand() < 0.4), touch
    else:
        alt0 = bool(not touch and rng.rand() < 0.5)
        alt1 = bool(rng.rand() < 0.85) if touch else alt0
    return XR.Rec(bc, name, first, alt0, bool(alt1), bool(touch), None)


def _csr(rows, bit3=True):
    """[Rec] of one variant -> (covers, (offsets, name identities, flags)) as devplanes.spike_rpb_counts takes them."""
    texts = list(dict.fromkeys(r.barcode for r in rows))
    per = {b: [] for b in texts}
    for r in rows:
        per[r.barcode].append(r)
    flat = [r for b in texts for r in per[b]]
    off = np.zeros(len(texts) + 1, np.uint32)
    off[1:] = np.cumsum([len(per[b]) for b in texts])
    flags = np.array([(1 if r.first else 0) | (2 if r.alt0 else 0) | (4 if r.alt1 else 0) | (8 if r.touch and bit3 else 0) for r in flat], np.uint8)
    return PR.idents(texts), (off, XR.rp.fnv64([r.name for r in flat]) if flat else np.zeros(0, np.uint64), flags)


class _Set(object):
    def __init__(self, g, members):
        self.name, self.members = "set%d" % g, tuple(members)


def _device(eng, set_rows, lead, seeds, thr, rthr, bit3=True):
    """The sets' members laid out as listed variants one behind the other, then spike_joint_records and the entry."""
    covers, records, sets = [], [], []
    for g, rows in enumerate(set_rows):
        sets.append(_Set(g, range(len(covers), len(covers) + len(rows))))
        for member in rows:
            c, r = _csr(member, bit3)
            covers.append(c); records.append(r)
    joint = devplanes.spike_joint_records(sets, covers, records)
    return devplanes.spike_phase_rpb_counts(eng, lead, [len(rows) for rows in set_rows], joint, seeds, thr, rthr), joint, (sets, covers, records)


def test_sets_of_one_two_and_eight_members_and_a_set_nobody_covers(engine0):
    rows = _made([(1, 70, 0), (2, 0, 25), (8, 130, 40), (2, 90, 30)])                      # (joint offsets 0, 70, 70, 200, 290)
    lead, seeds = [11, 5000, 1 << 20, 77], PR.seeds(SEED, 2)
    thr, rthr = [PR.threshold(t) for t in (0.1, 0.5)], [PR.threshold(p) for p in (0.2, 0.7)]
    got, joint, _ = _device(engine0, rows, lead, seeds, thr, rthr)
    assert [len(j[0]) for j in joint] == [70, 0, 130, 90]
    assert np.array_equal(got, ZR.counts_from(rows, lead, thr, rthr, seeds))
    assert not got[1].any() and got[0].any() and got[2].any() and got[3].any()
    assert got[2, :, :, :, 1].any() or got[3, :, :, :, 1].any()                           # (some barcode carries every member before spiking)
    names = [{r.name for r in member} for member in rows[2]]
    assert names[0] & names[1]                                                            # (a record that appears under two members)


def test_three_hundred_joint_barcodes_and_a_barcode_deep_at_one_member(engine0):
    rng = np.random.RandomState(9)
    rows = _made([(3, 300, 20)], seed=4)[0]
    deep = [_rec(rng, "DEEPACGT", "q:DEEPACGT:%d" % i, i == 17, False) for i in range(200)]
    rows[0] += deep
    rows[1] += [_rec(rng, "DEEPACGT", "q:DEEPACGT:199", False, False)]                    # (200 records at one member, 1 at another)
    rows[2] += deep[:3]
    lead, seeds = [9], PR.seeds(SEED, 3)
    thr, rthr = [PR.threshold(t) for t in (0.2, 0.9)], [0, PR.threshold(0.01), PR.threshold(0.4), ONE]
    got, joint, _ = _device(engine0, [rows], lead, seeds, thr, rthr)
    assert len(joint[0][0]) == 301 and int(np.diff(joint[0][1].astype(np.int64)).max()) == 200
    assert np.array_equal(got, ZR.counts_from([rows], lead, thr, rthr, seeds))
    assert (got[0, :, :, 3, 0] == 301).all() and (got[0, :, :, 0, 0] < 301).all()


def test_barcodes_of_first_names_only_and_barcodes_without_one(engine0):
    firsts, none = _made([(2, 150, 10)], seed=3, records=(1, 4), p_first=1.0), _made([(2, 150, 10), (3, 40, 0)], seed=3, records=(1, 4), p_first=0.0)
    seeds, thr, rthr = PR.seeds(SEED, 2), [PR.threshold(0.5)], [0, PR.threshold(0.3), ONE]
    got, _, _ = _device(engine0, firsts, [300], seeds, thr, rthr)
    assert np.array_equal(got, ZR.counts_from(firsts, [300], thr, rthr, seeds))
    assert (got[0, :, :, :, 0] == 150).all()                                              # (a first name stays at every threshold)
    got, _, _ = _device(engine0, none, [300, 301], seeds, thr, rthr)
    assert np.array_equal(got, ZR.counts_from(none, [300, 301], thr, rthr, seeds))
    assert not got[:, :, :, 0].any()                                                      # (threshold 0 keeps first names only: nobody is there)
    assert (got[:, :, 0, 2, 0] == np.array([[150], [40]])).all() and 0 < got[0, 0, 0, 1, 0] < 150


def test_thirty_two_cells_and_more_replicates_than_the_grid_is_deep(engine0):
    rows = _made([(2, 300, 10), (4, 65, 5)])
    lead = [101, 202]
    thr = [PR.threshold(t) for t in (0.01, 0.05, 0.1, 0.2, 0.4, 0.6, 0.8, 1.0)]
    rthr = [PR.threshold(p) for p in (0.1, 0.25, 0.5)] + [ONE]
    seeds = PR.seeds(PR.M64 - 3, 70)                                                    # (70 replicates > the 64 the entry launches; the seeds wrap)
    got, _, _ = _device(engine0, rows, lead, seeds, thr, rthr)
    assert got.shape == (2, 70, 8, 4, 4)
    assert np.array_equal(got, ZR.counts_from(rows, lead, thr, rthr, seeds))
    assert len({got[:, j].tobytes() for j in range(70)}) > 60


def test_nine_read_thresholds_take_the_wide_instance(engine0):
    rows = _made([(2, 130, 9), (8, 9, 3)])
    lead, seeds = [55, 66], PR.seeds(SEED, 2)
    thr, rthr = [PR.threshold(t) for t in (0.3, 0.6)], [PR.threshold(k / 8.0) for k in range(8)] + [ONE]
    got, _, _ = _device(engine0, rows, lead, seeds, thr, rthr)
    assert got.shape == (2, 2, 2, 9, 4) and np.array_equal(got, ZR.counts_from(rows, lead, thr, rthr, seeds))
    ends = [PR.threshold(k / 31.0) for k in range(31)] + [ONE]                           # (32 read thresholds, one target)
    got, _, _ = _device(engine0, rows, lead, seeds, thr[:1], ends)
    assert got.shape == (2, 2, 1, 32, 4) and np.array_equal(got, ZR.counts_from(rows, lead, thr[:1], ends, seeds))
    assert (np.diff(got[:, :, :, :, 0].astype(np.int64), axis=3) >= 0).all()              # (N_ALL' nested in r)


def test_one_replicate_the_ends_of_both_axes_and_the_two_equivalences(engine0):
    eng = engine0
    rows = _made([(1, 210, 0), (3, 77, 12), (1, 33, 0)], seed=11)
    lead, seeds = [1000, 2000, 3000], PR.seeds(SEED, 1)
    ends, joint, (sets, covers, records) = _device(eng, rows, lead, seeds, [0, ONE], [0, ONE])
    assert ends.shape == (3, 1, 2, 2, 4) and np.array_equal(ends, ZR.counts_from(rows, lead, [0, ONE], [0, ONE], seeds))
    assert np.array_equal(_device(eng, rows, lead, seeds, [0, ONE], [0, ONE])[0], ends)   # (two identical calls)
    assert not ends[:, :, 0, :, 2].any() and np.array_equal(ends[:, :, 1, :, 2], ends[:, :, 1, :, 0])      # (S_ALL' at thresholds 0 and 2^32)
    # M = 1: columns (N', V0', S', V1') of smc_spike_indel_rpb_counts, on the device
    thr, rthr = [PR.threshold(t) for t in (0.2, 0.6)], [0, PR.threshold(0.3), PR.threshold(0.8), ONE]
    got = _device(eng, rows, lead, PR.seeds(SEED, 3), thr, rthr)[0]
    one = [g for g, s in enumerate(sets) if len(s.members) == 1]
    per = devplanes.spike_rpb_counts(eng, [lead[g] for g in one], [covers[sets[g].members[0]] for g in one],
                                     [records[sets[g].members[0]] for g in one], PR.seeds(SEED, 3), thr, rthr, four=True)
    assert np.array_equal(got[one], per[..., [0, 1, 2, 4]]) and per[..., 4].any()
    # one read threshold of 2^32: smc_spike_indel_phase_counts at one depth threshold of 2^32, from the whole barcodes' counters
    counters = []
    for c, (off, _, flags) in zip(covers, records):
        sums = [np.add.reduceat(((flags >> s) & 1).astype(np.int64), off[:-1].astype(np.int64)) for s in (1, 2, 3)]
        counters.append(np.stack([np.diff(off.astype(np.int64))] + sums, axis=1).astype(np.uint32))
    whole = devplanes.spike_indel_phase_counts(eng, lead, devplanes.spike_joint(sets, covers, counters), PR.seeds(SEED, 3), thr, [ONE])
    assert np.array_equal(got[:, :, :, 3:], whole) and whole[1].any()


@pytest.mark.parametrize("n_rthr", (4, 9))
def test_a_set_of_one_member_is_a_listed_variant_in_both_instances(engine0, n_rthr):
    """The two faces of k_spr_counts where they overlap: a set of one member through smc_spike_phase_rpb_counts against the same rows
    as listed variants through smc_spike_indel_rpb_counts (four-bit flags) and smc_spike_rpb_counts (flags without bit 3), both against
    the restatement.  The middle row is one nobody covers; 4 read thresholds take the instance of 8, 9 the wide one."""
    eng = engine0
    rows = _made([(1, 210, 0), (1, 0, 0), (1, 33, 0)], seed=13)
    assert [len({r.barcode for r in s[0]}) for s in rows] == [210, 0, 33]
    per = [n for s in rows for n in collections.Counter(r.barcode for r in s[0]).values()]
    assert min(per) == 1 and 1 < max(per) <= 5                                            # (1 .. 5 records per barcode)
    lead, seeds, thr = [1000, 2000, 3000], PR.seeds(SEED, 3), [PR.threshold(t) for t in (0.2, 0.6)]
    rthr = [PR.threshold(k / float(n_rthr - 1)) for k in range(n_rthr - 1)] + [ONE]
    want = ZR.counts_from(rows, lead, thr, rthr, seeds)
    assert want.shape == (3, 3, 2, n_rthr, 4) and want[0].any() and not want[1].any() and want[2].any()
    for bit3 in (True, False):
        got, joint, (sets, covers, records) = _device(eng, rows, lead, seeds, thr, rthr, bit3=bit3)
        assert [len(j[0]) for j in joint] == [210, 0, 33] and all(len(s.members) == 1 for s in sets)
        listed = devplanes.spike_rpb_counts(eng, lead, covers, records, seeds, thr, rthr, four=bit3)
        assert listed.shape == (3, 3, 2, n_rthr, 5) and listed[..., 3].any()              # (READS': the input is not empty)
        assert np.array_equal(got, listed[..., [0, 1, 2, 4]])
        assert np.array_equal(got, want) and np.array_equal(listed[..., [0, 1, 2, 4]], want)


def test_an_snv_only_list_with_the_bytes_of_smc_spike_read_bits(engine0):
    """(smc_spike_read_bits' bytes have no bit 3: bit 2, single, is an SNV's alt1 - the one entry serves both kinds of list)"""
    rows = _made([(2, 190, 20), (3, 33, 5)], seed=21, snv=True)
    assert all(r.alt1 == r.touch for s in rows for member in s for r in member)
    lead, seeds = [17, 4000], PR.seeds(SEED, 3)
    thr = [PR.threshold(t) for t in (0.05, 0.5, 1.0)]
    for rthr in ([0, PR.threshold(0.3), ONE], [PR.threshold(k / 9.0) for k in range(10)]):      # (both instances)
        three, joint, _ = _device(engine0, rows, lead, seeds, thr, rthr, bit3=False)
        assert not any((j[3] & 8).any() for j in joint)
        four = _device(engine0, rows, lead, seeds, thr, rthr)[0]
        assert np.array_equal(three, four) and np.array_equal(three, ZR.counts_from(rows, lead, thr, rthr, seeds)) and three[..., 3].any()


def test_refusals_launch_nothing(engine0):
    eng = engine0
    size = 8192
    out = DevBuf(eng, size).upload(np.full(size, 0x5A, np.uint8))
    src = DevBuf(eng, size).upload(np.zeros(size, np.uint8))
    half, above = np.full(40, 1 << 31, np.uint64), np.full(40, 1 << 31, np.uint64)
    above[1] = ONE + 1
    off = np.array([0, 2, 3], np.uint32)                                                    # (2 joint barcodes of 2 members, 1 of 3: 7 segments)
    set_m, seg = np.array([2, 3], np.uint32), np.array([0, 4], np.uint32)
    rec_off = np.array([0, 2, 2, 5, 6, 7, 8, 9], np.uint32)

    def counts(off=off, set_m=set_m, seg=seg, rec_off=rec_off, n_rec=9, n_sets=2, n_reps=2, thr=half, n_targets=2, rthr=half, n_rthr=2):
        return eng.L.smc_spike_phase_rpb_counts(eng.ctx, src.data_ptr(), src.data_ptr(), off.ctypes.data, src.data_ptr(), set_m.ctypes.data,
                                                src.data_ptr(), seg.ctypes.data, src.data_ptr(), rec_off.ctypes.data, src.data_ptr(), src.data_ptr(),
                                                n_rec, src.data_ptr(), n_sets, src.data_ptr(), n_reps, thr.ctypes.data, n_targets, rthr.ctypes.data,
                                                n_rthr, out.data_ptr(), None)
    many = np.zeros(4098, np.uint32)
    for kw, msg in ((dict(set_m=np.array([2, 9], np.uint32)), "set 1 has 9 members, 1 .. 8 expected"),
                    (dict(set_m=np.array([0, 3], np.uint32)), "set 0 has 0 members"),
                    (dict(off=np.array([0, 3, 2], np.uint32)), "offsets decrease at set 1"),
                    (dict(seg=np.array([0, 5], np.uint32)), "segments of set 1 start at 5, 4 expected"),
                    (dict(rec_off=np.array([0, 2, 1, 5, 6, 7, 8, 9], np.uint32)), "record offsets decrease at segment 1"),
                    (dict(n_rec=8), "record offsets end at 9, beyond the 8 records"),
                    (dict(thr=above), "target 1: a threshold above 2^32"), (dict(rthr=above), "read threshold 1 is above 2^32"),
                    (dict(n_rthr=0), "0 read thresholds"), (dict(n_rthr=-1), "-1 read thresholds"),
                    (dict(n_targets=3, n_rthr=11), "3 targets x 11 read thresholds, at most 32 cells"),
                    (dict(n_targets=32, n_rthr=2), "at most 32 cells"), (dict(n_targets=33, n_rthr=1), "33 targets, at most 32"),
                    (dict(n_reps=1001), "1001 replicates, at most 1000"),
                    (dict(n_sets=4097, off=many, set_m=many, seg=many), "4097 sets, at most 4096")):
        assert counts(**kw) == -4 and msg.encode() in eng.L.smc_last_error(), msg            # SMC_E_INPUT
        assert eng.L.smc_last_error().startswith(b"smc_spike_phase_rpb_counts:")
    eng.L.smc_device_sync(eng.ctx)
    assert (out.download(np.uint8, size) == 0x5A).all()                                       # nothing zeroed, nothing launched
    out.free(); src.free()
