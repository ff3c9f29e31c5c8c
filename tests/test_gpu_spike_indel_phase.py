"""--spikeIndelPhase on the GPU: smc_spike_indels / smc_spike_indels_reps with `lead` against the restatement (tests/
spike_indel_phase_restate.py) byte for byte - records, both pools up to the totals, NM', n_indel', statistics, totals - on both
listings of the hand-made BAM, on bam_cigars and on a synthetic BAM of a dozen workgroups; `lead` all zero against today's records;
the two refusals of a bad `lead`; smc_spike_indel_phase_counts against the restatement word for word, against smc_spike_phase_counts and smc_spike_indel_counts where
they must agree, its edge sizes and its refusals."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import abi, devplanes
from smcounter_amd.engine import DevBuf

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_depth_restate as DR  # noqa: E402
import ds_restate  # noqa: E402
import spike_indel_phase_restate as XR  # noqa: E402
import spike_indel_restate as IR  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import test_gpu_spike_indels as TG  # noqa: E402  (its decoded run in HBM, its comparison of a copy)

pytestmark = pytest.mark.gpu
SEED = XR.SEED
POISON = 0x5A
ONE, HALF = XR.ONE, XR.HALF


def _single(run, var, ins):
    """smc_spike_indels over the records `var` (their own thresholds) -> TG._assert_copy's dict, statistics in the records' order."""
    A, n = run.A, len(run.A["aln"])
    cap = devplanes.spike_indel_caps(A, var)
    out, stats, totals, nm, n_indel = devplanes.spike_indel_run(run.eng, run.up, A, var, ins, run.idents, SEED, run.P.mismatchThr, run.nm, run.n_indel)
    try:
        return dict(aln=out.aln.download(abi.DEV_ALN_DTYPE, n), bq=out.bq.download(np.uint8, 2 * cap[0] + 64), cig=out.cig.download(np.uint32, cap[1] + 16),
                    nm=nm, n_indel=n_indel, totals=totals, stats=stats)
    finally:
        out.aln.free(); out.bq.free(); out.cig.free()


def _copies(run, var, ins, seeds, thr):
    """smc_spike_indels_reps into buffers filled with POISON -> per copy the same dict (its pools whole, up to the stride)."""
    A, n = run.A, len(run.A["aln"])
    got = devplanes.spike_indel_run_copies(run.eng, run.up, A, var, ins, run.idents, seeds, thr, run.P.mismatchThr, run.nm, run.n_indel, fill=POISON,
                                           mism=True)
    try:
        (sa, sb, sc), B = got["strides"], len(seeds)
        whole = [got[k].download(np.uint8, st * B) for k, st in zip(("aln", "bq", "cig"), (sa, sb, sc))]
    finally:
        for k in ("aln", "bq", "cig"):
            got[k].free()
    out = []
    for c in range(B):
        assert (whole[0][c * sa + 36 * n:(c + 1) * sa] == POISON).all()
        out.append(dict(aln=whole[0][c * sa:c * sa + 36 * n].view(abi.DEV_ALN_DTYPE), bq=whole[1][c * sb:(c + 1) * sb],
                        cig=whole[2][c * sc:(c + 1) * sc].view(np.uint32), nm=got["nm"][c], n_indel=got["n_indel"][c], stats=got["stats"][c],
                        totals=got["totals"][c]))
    return out


def _unchanged(run):
    A, n = run.A, len(run.A["aln"])
    assert run.up.aln.download(abi.DEV_ALN_DTYPE, n).tobytes() == A["aln"].tobytes()
    assert run.up.bq.download(np.uint8, len(A["bq"])).tobytes() == A["bq"].tobytes()
    assert run.up.cig.download(np.uint32, len(A["cig"])).tobytes() == A["cig"].tobytes()


def _against_the_restatement(run, bam_path, fa, variants, sets, thresholds):
    """Both entries with `lead` == the restatement; -> the records relocated over all calls."""
    P, relocated = run.P, 0
    for thr in thresholds:
        var, ins, order = XR.records_with_lead(variants, sets, thr)
        records, stats = XR.restate(bam_path, variants, sets, thr, SEED, P.mismatchThr, fa)
        want = IR.expected_run(run.A, run.recs, records, run.nm, run.n_indel)
        got = _single(run, var, ins)
        TG._assert_copy(got, want, run.A)
        assert got["stats"][:, 0].tolist() == [stats[k]["READS"] for k in order] and got["stats"][:, 1].tolist() == [stats[k]["NMINC"] for k in order]
        relocated += len(want["relocated"])
    # three copies from one call, each with a seed and a threshold of its own, over a fill
    seeds = [SEED + 5, SEED, SEED + 77]
    var, ins, order = XR.records_with_lead(variants, sets, 0)
    copies = _copies(run, var, ins, seeds, list(thresholds)[:3])
    for c, (s, thr) in enumerate(zip(seeds, thresholds)):
        records, stats = XR.restate(bam_path, variants, sets, thr, s, P.mismatchThr, fa)
        want = IR.expected_run(run.A, run.recs, records, run.nm, run.n_indel)
        TG._assert_copy(copies[c], want, run.A)
        assert copies[c]["stats"][:, 0].tolist() == [stats[k]["READS"] for k in order]
        assert copies[c]["stats"][:, 1].tolist() == [stats[k]["NMINC"] for k in order]
        n_pairs, n_cw = want["totals"]
        assert (copies[c]["bq"][2 * n_pairs:] == POISON).all() and (copies[c]["cig"].view(np.uint8)[4 * n_cw:] == POISON).all()
    _unchanged(run)
    return relocated


@pytest.mark.parametrize("listing", ("A", "B"))
def test_rewrite_with_lead_equals_the_restatement_on_the_hand_made_bam(engine0, tmp_path, listing):
    run, bam_path, fa, P, variants = TG._case_run(engine0, tmp_path)
    try:
        sets = XR.LISTINGS[listing]
        var, _, _ = XR.records_with_lead(variants, sets, HALF)
        assert var["lead"].tolist() == ([0, 1, 2, 0] if listing == "A" else [0, 0, 2, 0])
        assert _against_the_restatement(run, bam_path, fa, variants, sets, (0, HALF, ONE)) > 0
        # today's kernels would ignore `lead`: the restatement without sets is another copy
        phased, _ = XR.restate(bam_path, variants, sets, HALF, SEED, P.mismatchThr, fa)
        loose, _ = IR.restate(bam_path, variants, HALF, SEED, P.mismatchThr, fa)
        assert {k: r["applied"] for k, r in loose.items()} != {k: r["applied"] for k, r in phased.items()}
    finally:
        run.close()


@pytest.mark.parametrize("name", ("bam_cigars", "synth"))
def test_rewrite_with_lead_equals_the_restatement_on_a_fixture(engine0, tmp_path, name):
    """IR.pick_variants' four, the first and the last of a run made one set: the others are non-members between two members.  The
    runs of bam_cigars hold about a hundred alignments each; the synthetic BAM's run holds a few thousand - a dozen workgroups - so the
    scan across the workgroups' sums runs with `lead` present and relocated records start from a scanned, non-zero sum."""
    bam_path, fa, loci, P, variants = TG._inputs(name, str(tmp_path))
    done = 0
    for chrom, lo, hi in ds_restate.stretches(loci):
        vs = [v for v in variants if v.chrom == chrom and lo < v.pos <= hi]
        if len(vs) < 2:
            continue
        run = TG.Run(engine0, bam_path, chrom, lo, hi, P)
        try:
            sets = [(0, len(vs) - 1)]
            assert XR.records_with_lead(vs, sets, 0)[0]["lead"].tolist() == [0] * (len(vs) - 1) + [len(vs) - 1]
            done += _against_the_restatement(run, bam_path, fa, vs, sets, (HALF, ONE, 1 << 30))
            if name == "synth":
                records, _ = XR.restate(bam_path, vs, sets, HALF, SEED, P.mismatchThr, fa)
                moved = IR.expected_run(run.A, run.recs, records, run.nm, run.n_indel)["relocated"]
                assert len(run.A["aln"]) > 3 * 256 and len({i // 256 for i in moved}) >= 3
        finally:
            run.close()
    assert done > 0


def test_lead_all_zero_is_the_call_with_todays_records(engine0, tmp_path):
    """A record as the callers before `lead` wrote it - a 32-bit `len` of at most 255 - is the same 24 bytes, and the same copy."""
    run, bam_path, fa, P, variants = TG._case_run(engine0, tmp_path)
    try:
        old = np.dtype([("pos0", "<i4"), ("kind", "u1"), ("ref", "u1"), ("alt", "u1"), ("pad", "u1"), ("len", "<u4"), ("ins_off", "<u4"), ("thr", "<u8")])
        var, ins, _ = XR.records_with_lead(variants, [], HALF)
        assert not var["lead"].any()
        todays = np.zeros(len(var), old)
        for f in old.names:
            todays[f] = var[f]
        assert todays.tobytes() == var.tobytes()
        a, b = _single(run, var, ins), _single(run, todays.view(abi.SPIKE_INDEL_VARIANT_DTYPE), ins)
        for k in ("aln", "bq", "cig", "nm", "n_indel", "stats", "totals"):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k
        records, _ = IR.restate(bam_path, variants, HALF, SEED, P.mismatchThr, fa)
        TG._assert_copy(a, IR.expected_run(run.A, run.recs, records, run.nm, run.n_indel), run.A)
    finally:
        run.close()


def test_a_bad_lead_is_refused_by_both_entries_and_nothing_is_launched(engine0):
    eng = engine0
    n = 8
    ok = np.zeros(3, abi.SPIKE_INDEL_VARIANT_DTYPE)
    ok["pos0"], ok["kind"], ok["ref"], ok["alt"], ok["len"], ok["thr"] = [5, 9, 20], [0, 1, 2], ord("A"), [ord("G"), ord("A"), ord("A")], [0, 2, 3], HALF
    bufs = [DevBuf(eng, 8192).upload(np.full(8192, POISON, np.uint8)) for _ in range(7)]   # aln, bq, cig, nm, n_indel, stats, totals
    src = DevBuf(eng, 4096).upload(np.zeros(4096, np.uint8))
    seeds, thr = np.array([1, 2], np.uint64), np.array([5, 6], np.uint64)

    def calls(var):
        d_var = DevBuf(eng, var.nbytes + 256).upload(np.ascontiguousarray(var).view(np.uint8).reshape(-1))
        b = [x.data_ptr() for x in bufs]
        one = eng.L.smc_spike_indels(eng.ctx, src.data_ptr(), n, src.data_ptr(), 32, src.data_ptr(), 64, d_var.data_ptr(), var.ctypes.data, len(var),
                                     src.data_ptr(), 2, src.data_ptr(), 4, 7, 6.0, src.data_ptr(), src.data_ptr(), 100, 100, *(b + [None]))
        e1 = eng.L.smc_last_error()
        many = eng.L.smc_spike_indels_reps(eng.ctx, src.data_ptr(), n, src.data_ptr(), 32, src.data_ptr(), 64, d_var.data_ptr(), var.ctypes.data, len(var),
                                           src.data_ptr(), 2, src.data_ptr(), 4, seeds.ctypes.data, thr.ctypes.data, 2, 6.0, src.data_ptr(), src.data_ptr(),
                                           100, 100, b[0], 512, b[1], 256, b[2], 512, b[3], b[4], b[5], b[6], None)
        e2 = eng.L.smc_last_error()
        d_var.free()
        return (one, e1, b"smc_spike_indels:"), (many, e2, b"smc_spike_indels_reps:")
    for lead, msg in (([1, 0, 0], "variant 0: lead 1 points in front of the array"), ([0, 2, 0], "variant 1: lead 2 points in front of the array"),
                      ([0, 0, 3], "points in front"), ([0, 1, 1], "variant 2: its leader has a lead of its own")):
        var = ok.copy()
        var["lead"] = lead
        for rc, err, who in calls(var):
            assert rc == -4 and msg.encode() in err and err.startswith(who), (lead, err)      # SMC_E_INPUT
    eng.L.smc_device_sync(eng.ctx)
    for b in bufs:
        assert (b.download(np.uint8, 8192) == POISON).all()                                # nothing copied, nothing launched
    # smc_spike_indel_touch makes no draw and does not read the field
    var = ok.copy()
    var["lead"] = [1, 2, 3]
    d_var = DevBuf(eng, 4096).upload(np.zeros(4096, np.uint8))
    d_out = DevBuf(eng, 4096)
    assert eng.L.smc_spike_indel_touch(eng.ctx, src.data_ptr(), 0, src.data_ptr(), 32, 64, d_var.data_ptr(), var.ctypes.data, len(var), 4,
                                       d_out.data_ptr(), None) == 0
    eng.L.smc_device_sync(eng.ctx)
    for b in bufs + [src, d_var, d_out]:
        b.free()


# ---- smc_spike_indel_phase_counts
TARGETS, FRACS, REPS = (0.05, 0.3, 0.7), (0.2, 0.6, 1.0), 3


def _device(eng, joint, lead, seeds, thr, dthr):
    return devplanes.spike_indel_phase_counts(eng, lead, [(PR.idents(names), cnt) for names, cnt in joint], seeds, thr, dthr)


def _check_counts(eng, joint, lead):
    seeds = PR.seeds(SEED, REPS)
    thr, dthr = [PR.threshold(t) for t in TARGETS], [DR.frac_thr(f) for f in FRACS]
    want = XR.counts_from(joint, lead, thr, dthr, seeds)
    got = _device(eng, joint, lead, seeds, thr, dthr)
    assert got.shape == want.shape == (len(joint), REPS, len(TARGETS), len(FRACS), 4) and got.dtype == np.uint32
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(_device(eng, joint, lead, seeds, thr, dthr), got)              # two identical calls
    ends = _device(eng, joint, lead, seeds[:1], [0, ONE], [0, ONE])                        # (R = 1; thresholds 0 and 2^32 on both axes)
    assert np.array_equal(ends, XR.counts_from(joint, lead, [0, ONE], [0, ONE], seeds[:1]))
    assert not ends[:, :, :, 0].any()
    for g, (names, cnt) in enumerate(joint):
        c = cnt.astype(np.int64)
        v0, v1 = int((2 * c[:, :, 1] > c[:, :, 0]).all(axis=1).sum()), int((2 * c[:, :, 2] > c[:, :, 0]).all(axis=1).sum())
        assert ends[g, 0, 0, 1].tolist() == [len(names), v0, 0, v0] and ends[g, 0, 1, 1].tolist() == [len(names), v0, len(names), v1]
    return got


@pytest.mark.parametrize("name", ("case", "bam_cigars"))
def test_counts_equal_the_restatement(engine0, tmp_path, name):
    bam_path, fa, loci, P, variants = TG._inputs(name, str(tmp_path))
    total = 0
    if name == "case":
        todo = [(variants, [(0, 1, 2), (0, 2), (3,)])]
    else:
        todo = []
        for chrom in sorted({v.chrom for v in variants}):
            vs = [v for v in variants if v.chrom == chrom]
            if len(vs) >= 2:
                todo.append((vs, [tuple(range(len(vs))), (0, len(vs) - 1)]))
    assert todo
    for vs, sets in todo:
        joint = XR.host_joint(bam_path, vs, sets, fa)
        got = _check_counts(engine0, joint, [min(vs[k].pos for k in s) for s in sets])
        total += int(got[..., 0].sum())
        if name == "case":
            # the restatement's other way: the joint barcodes restate() spikes at every member are S_ALL at f = 1
            _, stats = XR.restate(bam_path, vs, sets[:1], PR.threshold(TARGETS[1]), SEED, P.mismatchThr, fa)
            both = set.intersection(*[stats[k]["spiked"] for k in sets[0]]) & set(joint[0][0])
            assert int(got[0, 0, 1, 2, 2]) == len(both) > 0
            # four counters matter here: a member where alt1 and touch differ
            c = np.concatenate([cnt.reshape(-1, 4) for _, cnt in joint]).astype(np.int64)
            assert (c[:, 2] != c[:, 3]).any()
    assert total > 0


def _made_joint(sizes, members, seed=5):
    """Joint barcodes without a BAM: per set `sizes[g]` texts and random (reads, alt0, alt1, touch) per member."""
    rng = np.random.RandomState(seed)
    out = []
    for g, (n, m) in enumerate(zip(sizes, members)):
        reads = rng.randint(1, 6, (n, m))
        touch = np.minimum(reads, rng.randint(0, 6, (n, m)))
        alt0 = np.minimum(reads, rng.randint(0, 4, (n, m)))
        alt1 = np.minimum(reads, rng.randint(0, 6, (n, m)))
        out.append((["S%dB%dACGT" % (g, b) for b in range(n)], np.stack([reads, alt0, alt1, touch], axis=2).astype(np.uint32)))
    return out


def test_with_alt1_and_touch_equal_to_single_the_numbers_are_the_phase_entrys(engine0):
    joint4 = _made_joint([300, 0, 65, 319], [2, 3, 5, 8])
    joint3 = []
    for names, c in joint4:
        c[:, :, 3] = c[:, :, 2]
        joint3.append((PR.idents(names), np.ascontiguousarray(c[:, :, :3])))
    lead, seeds = [101, 7, 202, (1 << 32) - 1], PR.seeds(SEED, 3)
    thr, dthr = [PR.threshold(t) for t in TARGETS], [DR.frac_thr(f) for f in FRACS]
    want = devplanes.spike_phase_counts(engine0, lead, joint3, seeds, thr, dthr)
    got = _device(engine0, joint4, lead, seeds, thr, dthr)
    assert got.shape == (4, 3, 3, 3, 4) and np.array_equal(got, want) and want[0].any() and want[3].any() and not want[1].any()


def test_one_member_equals_the_indel_counts_columns(engine0):
    joint = _made_joint([300, 65, 1], [1, 1, 1])
    pos, seeds = [101, 202, 5], PR.seeds(SEED, 3)
    thr, dthr = [PR.threshold(t) for t in TARGETS], [DR.frac_thr(f) for f in FRACS]
    covers, cnt = [PR.idents(names) for names, _ in joint], [c.reshape(-1, 4) for _, c in joint]
    cells = devplanes.spike_indel_counts(engine0, pos, covers, cnt, seeds, thr, dthr)
    got = _device(engine0, joint, pos, seeds, thr, dthr)
    assert np.array_equal(got, cells[..., [0, 1, 2, 4]]) and got.any()
    # (the column the set entry does not store is the one that reads `touch`)
    assert (cells[..., 3] > 0).any()


def test_eight_members_a_list_of_319_and_a_set_nobody_covers(engine0):
    joint = _made_joint([70, 0, 319], [8, 3, 2])                                          # (rows of 32, 12 and 8 words; a second workgroup, a ragged wavefront)
    lead, seeds = [11, 5000, 1 << 20], PR.seeds(SEED, 2)
    thr, dthr = [PR.threshold(t) for t in (0.1, 0.5)], [DR.frac_thr(f) for f in (0.3, 1.0)]
    got = _device(engine0, joint, lead, seeds, thr, dthr)
    assert np.array_equal(got, XR.counts_from(joint, lead, thr, dthr, seeds))
    assert not got[1].any() and got[0].any() and got[2].any() and int(got[0, ..., 0].max()) <= 70 and int(got[2, ..., 0].max()) == 319
    # with 8 members the conjunction bites: fewer carry all of them than carry the first
    c = joint[0][1].astype(np.int64)
    assert int(got[0, 0, 1, 1, 3]) < int((2 * c[:, 0, 2] > c[:, 0, 0]).sum())
    _check_counts(engine0, joint, lead)


def test_thirty_two_cells_and_more_replicates_than_the_grid_is_deep(engine0):
    joint = _made_joint([300, 65], [2, 5])
    lead = [101, 202]
    thr = [PR.threshold(t) for t in (0.01, 0.05, 0.1, 0.2, 0.4, 0.6, 0.8, 1.0)]
    dthr = [DR.frac_thr(f) for f in (0.1, 0.25, 0.5, 1.0)]
    seeds = PR.seeds(PR.M64 - 3, 70)                                                    # (70 replicates > the 64 the entry launches; the seeds wrap)
    got = _device(engine0, joint, lead, seeds, thr, dthr)
    assert got.shape == (2, 70, 8, 4, 4)
    assert np.array_equal(got, XR.counts_from(joint, lead, thr, dthr, seeds))
    assert len({got[:, j].tobytes() for j in range(70)}) > 60
    assert np.array_equal(_device(engine0, joint, lead, seeds[:1], thr, dthr), got[:, :1])        # (R = 1)


def test_counts_refusals_launch_nothing(engine0):
    eng = engine0
    size = 8192
    out = DevBuf(eng, size).upload(np.full(size, POISON, np.uint8))
    src = DevBuf(eng, size).upload(np.zeros(size, np.uint8))
    half, above = np.full(40, HALF, np.uint64), np.full(40, HALF, np.uint64)
    above[1] = ONE + 1
    off, m = np.array([0, 3, 5], np.uint32), np.array([2, 8], np.uint32)

    def counts(off=off, m=m, n_sets=2, n_reps=2, thr=half, n_targets=2, dthr=half, n_fracs=2):
        return eng.L.smc_spike_indel_phase_counts(eng.ctx, src.data_ptr(), src.data_ptr(), src.data_ptr(), off.ctypes.data, src.data_ptr(), m.ctypes.data,
                                                  src.data_ptr(), src.data_ptr(), n_sets, src.data_ptr(), n_reps, thr.ctypes.data, n_targets,
                                                  dthr.ctypes.data, n_fracs, out.data_ptr(), None)
    big_off = np.zeros(4097, np.uint32)
    for kw, msg in ((dict(m=np.array([2, 0], np.uint32)), "set 1 has 0 members, 1 .. 8 expected"), (dict(m=np.array([9, 1], np.uint32)), "set 0 has 9 members"),
                    (dict(off=np.array([0, 3, 2], np.uint32)), "offsets decrease at set 1"), (dict(n_targets=3, n_fracs=11), "3 targets x 11 fractions, at most 32 cells"),
                    (dict(n_targets=32, n_fracs=2), "at most 32 cells"), (dict(n_targets=33, n_fracs=1), "33 targets, at most 32"),
                    (dict(thr=above), "target 1: a threshold above 2^32"), (dict(dthr=above), "depth threshold 1 is above 2^32"),
                    (dict(n_reps=1001), "1001 replicates, at most 1000"), (dict(n_fracs=0), "0 fractions"),
                    (dict(n_sets=4097, off=big_off, m=np.ones(4097, np.uint32)), "at most 4096")):
        assert counts(**kw) == -4 and msg.encode() in eng.L.smc_last_error(), msg            # SMC_E_INPUT
        assert eng.L.smc_last_error().startswith(b"smc_spike_indel_phase_counts:")
    eng.L.smc_device_sync(eng.ctx)
    assert (out.download(np.uint8, size) == POISON).all()                                     # nothing zeroed, nothing launched
    out.free(); src.free()
    with pytest.raises(ValueError, match="spike_indel_phase_counts: 2 joint barcodes, counters of shape"):
        devplanes.spike_indel_phase_counts(eng, [5], [(np.zeros(2, np.uint64), np.zeros((2, 1, 3), np.uint32))], [1], [HALF], [ONE])
