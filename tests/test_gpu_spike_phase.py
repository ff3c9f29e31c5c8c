"""--spikePhase on the GPU: smc_spike_alleles / smc_spike_alleles_reps with `lead` against the restatement (tests/
spike_phase_restate.py) byte for byte, smc_spike_phase_counts against it word for word with its edge cases and refusals, and the
command line against the tool's --phased BAM, the two-step workflow, separate runs with --dsSeed s_j and the pages' own outputs."""
import argparse
import dataclasses
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import abi, bamio, devplanes, dsaf, fasta, spike
from smcounter_amd.engine import DevBuf
from smcounter_amd.py2compat import py2_round
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import spike_depth_restate as DS  # noqa: E402
import spike_phase_restate as PH  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line)
import test_gpu_spike as TS  # noqa: E402  (its inputs, the expected bytes of a run)
import test_gpu_spike_depth as TD  # noqa: E402  (counters without a BAM)

pytestmark = pytest.mark.gpu
SEED = 20240607
ONE = 1 << 32
SUFFIXES = TL.SUFFIXES
TARGETS, FRACS, REPS = (0.05, 0.3, 0.7), (0.2, 0.6, 1.0), 3


def _other(c, k=1):
    return "ACGT"[("ACGT".index(c) + k) % 4]


def _case(tmp):
    """The hand-made BAM with (P1, P1 + 7) - one MNV line's members - and P3."""
    bam, fa, loci, P, given = SR.make_case(tmp)
    ref = fasta.FastaFile(fa).fetch(SR.CASE_CHROM, SR.P1 - 1, SR.P1 + 7).upper()
    return bam, fa, loci, P, [SR.V(SR.CASE_CHROM, SR.P1, ref[0], _other(ref[0]), _other(ref[0])),
                              SR.V(SR.CASE_CHROM, SR.P1 + 7, ref[7], _other(ref[7]), _other(ref[7])), given[2]]


def _svar(variants, sets, thr):
    """The records as smc_spike_alleles takes them, ascending, with `lead` from the sets (indexes into `variants`)."""
    lead = PH.lead_positions(variants, sets)
    order = sorted(range(len(variants)), key=lambda k: variants[k].pos)
    var = np.zeros(len(variants), abi.SPIKE_VARIANT_DTYPE)
    for j, k in enumerate(order):
        v = variants[k]
        var[j]["pos0"], var[j]["ref"], var[j]["alt"], var[j]["thr"] = v.pos - 1, ord(v.ref), ord(v.alt), thr
        var[j]["lead"] = j - [variants[m].pos for m in order].index(lead[k])
    return var


def _rewrite(eng, nat, py, chrom, lo, hi, P, variants, sets, bam_path, fa, t=0.5):
    """smc_spike_alleles and smc_spike_alleles_reps with `lead` == the restatement, byte for byte; the input run unchanged."""
    A = nat.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
    idents = nat.barcode_idents(A["n_bc"])
    nm, n_indel = nat.run_mismatches(len(A["aln"]))
    var = _svar(variants, sets, sv.threshold(t))
    recs = py.fetch(chrom, lo, hi)
    up = devplanes.upload_run(eng, A, "A" * A["nl"])
    try:
        records, stats = PH.restate(bam_path, fa, variants, sets, t, SEED, P.mismatchThr)
        want_aln, want_bq = TS._expected(A, recs, records)
        out, got = devplanes.spike_run(eng, up, A, var, idents, SEED, P.mismatchThr, nm, n_indel)
        try:
            aln, bq = out.aln.download(abi.DEV_ALN_DTYPE, len(A["aln"])), out.bq.download(np.uint8, len(A["bq"]))
        finally:
            out.aln.free(); out.bq.free()
        assert bq.tobytes() == want_bq.tobytes() and aln.tobytes() == want_aln.tobytes()
        by_pos = sorted(range(len(variants)), key=lambda k: variants[k].pos)
        assert got[:, 0].tolist() == [stats[k]["READS"] for k in by_pos] and got[:, 1].tolist() == [stats[k]["NMINC"] for k in by_pos]
        # two copies from one call, each with a seed and a threshold of its own
        seeds, ts = [SEED + 5, SEED], [0.2, t]
        d_aln, d_bq, (sa, sb), st = devplanes.spike_run_copies(eng, up, A, var, idents, seeds, [sv.threshold(x) for x in ts], P.mismatchThr, nm, n_indel)
        try:
            for c in range(2):
                rc, sc = PH.restate(bam_path, fa, variants, sets, ts[c], seeds[c], P.mismatchThr)
                wa, wb = TS._expected(A, recs, rc)
                assert d_bq.download(np.uint8, sb * 2)[c * sb:c * sb + len(A["bq"])].tobytes() == wb.tobytes()
                assert d_aln.download(np.uint8, sa * 2)[c * sa:c * sa + A["aln"].nbytes].tobytes() == wa.tobytes()
                assert st[c, :, 0].tolist() == [sc[k]["READS"] for k in by_pos]
        finally:
            d_aln.free(); d_bq.free()
        assert up.aln.download(abi.DEV_ALN_DTYPE, len(A["aln"])).tobytes() == A["aln"].tobytes()
        assert up.bq.download(np.uint8, len(A["bq"])).tobytes() == A["bq"].tobytes()
    finally:
        up.free()
    return records, stats


@pytest.mark.parametrize("listed", ("mnv", "mnv_and_singleton"))
def test_rewrite_with_lead_equals_the_restatement_on_the_hand_made_bam(engine0, tmp_path, listed):
    bam_path, fa, loci, P, variants = _case(str(tmp_path))
    variants = variants[:2] if listed == "mnv" else variants
    nat, py = bamio.NativeBam(bam_path), bamio.BamFile(bam_path)
    (chrom, lo, hi), = ds_restate.stretches(loci)
    records, stats = _rewrite(engine0, nat, py, chrom, lo, hi, P, variants, [(0, 1)], bam_path, fa)
    assert any(r["inc"] == 2 for r in records.values())                                  # NM + 2 on one read
    joint = set(PH.host_joint(bam_path, fa, variants, [(0, 1)])[0][0])
    assert stats[0]["spiked"] & joint == stats[1]["spiked"] & joint != set()
    # unphased (lead = 0) the same positions are another file: the restatement without sets differs, and the kernel equals it too
    loose, _ = PH.restate(bam_path, fa, variants, [], 0.5, SEED, P.mismatchThr)
    assert {k: r["edits"] for k, r in loose.items()} != {k: r["edits"] for k, r in records.items()}
    _rewrite(engine0, nat, py, chrom, lo, hi, P, variants, [], bam_path, fa)
    nat.close(); py.close()


def test_rewrite_with_lead_equals_the_restatement_on_bam_cigars(engine0, tmp_path):
    bam_path, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    nat, py = bamio.NativeBam(bam_path), bamio.BamFile(bam_path)
    done = 0
    for chrom, lo, hi in ds_restate.stretches(loci):
        vs = SR.pick_positions(bam_path, fa, [(chrom, p) for p in range(lo + 1, hi + 1)], 3)
        if len(vs) == 3:
            _, stats = _rewrite(engine0, nat, py, chrom, lo, hi, P, vs, [(0, 2)], bam_path, fa)      # (the singleton between the members)
            done += sum(s["READS"] for s in stats)
    assert done > 0
    nat.close(); py.close()


def test_rewrite_refuses_a_bad_lead_and_launches_nothing(engine0):
    eng = engine0
    ok = np.zeros(3, abi.SPIKE_VARIANT_DTYPE)
    ok["pos0"], ok["ref"], ok["alt"], ok["thr"] = [5, 9, 12], ord("A"), ord("G"), 1 << 31
    bufs = [DevBuf(eng, 4096).upload(np.full(4096, 0x5A, np.uint8)) for _ in range(3)]      # aln_out, bq_out, stats
    src = DevBuf(eng, 4096).upload(np.zeros(4096, np.uint8))
    seeds, thr = np.array([1, 2], np.uint64), np.array([5, 6], np.uint64)

    def calls(var):
        d_var = DevBuf(eng, var.nbytes + 256).upload(np.ascontiguousarray(var).view(np.uint8).reshape(-1))
        one = eng.L.smc_spike_alleles(eng.ctx, src.data_ptr(), 8, src.data_ptr(), src.data_ptr(), 64, d_var.data_ptr(), var.ctypes.data, len(var),
                                      src.data_ptr(), 4, 7, 6.0, src.data_ptr(), src.data_ptr(), bufs[0].data_ptr(), bufs[1].data_ptr(),
                                      bufs[2].data_ptr(), None)
        e1 = eng.L.smc_last_error()
        many = eng.L.smc_spike_alleles_reps(eng.ctx, src.data_ptr(), 8, src.data_ptr(), src.data_ptr(), 64, d_var.data_ptr(), var.ctypes.data,
                                            len(var), src.data_ptr(), 4, seeds.ctypes.data, thr.ctypes.data, 2, 6.0, src.data_ptr(),
                                            src.data_ptr(), bufs[0].data_ptr(), 512, bufs[1].data_ptr(), 512, bufs[2].data_ptr(), None)
        e2 = eng.L.smc_last_error()
        d_var.free()
        return (one, e1), (many, e2)
    for lead, msg in (([1, 0, 0], "points in front of the array"), ([0, 2, 0], "points in front of the array"), ([0, 0, 3], "points in front"),
                      ([0, 1, 1], "its leader has a lead of its own")):
        var = ok.copy()
        var["lead"] = lead
        for rc, err in calls(var):
            assert rc == -4 and msg.encode() in err, (lead, err)
    eng.L.smc_device_sync(eng.ctx)
    for b in bufs:
        assert (b.download(np.uint8, 4096) == 0x5A).all()                              # nothing copied, nothing launched
    for b in bufs + [src]:
        b.free()


# ---- smc_spike_phase_counts
def _device(eng, joint, lead, seeds, thr, dthr):
    return devplanes.spike_phase_counts(eng, lead, [(PR.idents(names), cnt) for names, cnt in joint], seeds, thr, dthr)


def _check_counts(eng, joint, lead):
    seeds = PR.seeds(SEED, REPS)
    thr, dthr = [PR.threshold(t) for t in TARGETS], [DS.frac_thr(f) for f in FRACS]
    want = PH.counts_from(joint, lead, thr, dthr, seeds)
    got = _device(eng, joint, lead, seeds, thr, dthr)
    assert got.shape == want.shape == (len(joint), REPS, len(TARGETS), len(FRACS), 4) and got.dtype == np.uint32
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(_device(eng, joint, lead, seeds, thr, dthr), got)              # two identical calls
    ends = _device(eng, joint, lead, seeds[:1], [0, ONE], [0, ONE])                        # (R = 1; thresholds 0 and 2^32 on both axes)
    assert np.array_equal(ends, PH.counts_from(joint, lead, [0, ONE], [0, ONE], seeds[:1]))
    assert not ends[:, :, :, 0].any()
    for g, (names, cnt) in enumerate(joint):
        c = cnt.astype(np.int64)
        v0, v1 = int((2 * c[:, :, 1] > c[:, :, 0]).all(axis=1).sum()), int((2 * c[:, :, 2] > c[:, :, 0]).all(axis=1).sum())
        assert ends[g, 0, 0, 1].tolist() == [len(names), v0, 0, v0] and ends[g, 0, 1, 1].tolist() == [len(names), v0, len(names), v1]
    return got


@pytest.mark.parametrize("name", ("case", "bam_cigars"))
def test_counts_equal_the_restatement(engine0, tmp_path, name):
    total = 0
    if name == "case":
        bam_path, fa, loci, P, variants = _case(str(tmp_path))
        todo = [(variants, [(0, 1), (2,)])]
    else:
        bam_path, fa, loci, P = ds_restate.load_fixture(name, str(tmp_path))
        todo = []
        for chrom, lo, hi in ds_restate.stretches(loci):
            vs = SR.pick_positions(bam_path, fa, [(chrom, p) for p in range(lo + 1, hi + 1)], 3)
            if len(vs) == 3:
                todo.append((vs, [(0, 1, 2), (0, 2)]))
    for variants, sets in todo:
        joint = PH.host_joint(bam_path, fa, variants, sets)
        got = _check_counts(engine0, joint, [min(variants[k].pos for k in s) for s in sets])
        total += int(got[..., 0].sum())
        # the restatement's other way, for the file: the joint barcodes restate() spikes at every member are S_ALL at f = 1
        _, stats = PH.restate(bam_path, fa, variants, sets[:1], TARGETS[1], SEED, P.mismatchThr)
        both = set.intersection(*[stats[k]["spiked"] for k in sets[0]]) & set(joint[0][0])
        assert int(got[0, 0, 1, 2, 2]) == len(both)
    assert total > 0


def test_a_joint_list_wider_than_a_workgroup(engine0, tmp_path):
    cfg = dataclasses.replace(R.SYNTH_CFG, n_umi=300, rpb=2)
    bam, fa, loci, P, A = R.synth_bam(str(tmp_path), cfg, 24)
    vs = SR.pick_positions(bam, fa, loci[18:22], 2)
    joint = PH.host_joint(bam, fa, vs, [(0, 1)])
    n = len(joint[0][0])
    assert n > 256 and n % 64 and n % 256                                                 # (319 joint barcodes: a second workgroup, a ragged last wavefront)
    got = _check_counts(engine0, joint, [vs[0].pos])
    assert len({got[:, j].tobytes() for j in range(REPS)}) >= 2


def _made_joint(sizes, members, seed=5):
    """Joint barcodes without a BAM: per set `sizes[g]` texts and random (reads, alt0, single) per member, alt0 <= single <= reads."""
    rng = np.random.RandomState(seed)
    out = []
    for g, (n, m) in enumerate(zip(sizes, members)):
        reads = rng.randint(1, 6, (n, m))
        single = np.minimum(reads, rng.randint(0, 6, (n, m)))
        alt0 = np.minimum(single, rng.randint(0, 4, (n, m)))
        out.append((["S%dB%dACGT" % (g, b) for b in range(n)], np.stack([reads, alt0, single], axis=2).astype(np.uint32)))
    return out


def test_one_member_equals_the_depth_counts_columns(engine0):
    counters = TD._made_counters([300, 65])
    pos, seeds = [101, 202], PR.seeds(SEED, 3)
    thr, dthr = [PR.threshold(t) for t in TARGETS], [DS.frac_thr(f) for f in FRACS]
    depth = TD._device(engine0, counters, pos, seeds, thr, dthr)
    got = _device(engine0, [(names, c.reshape(-1, 1, 3)) for names, c in counters], pos, seeds, thr, dthr)
    assert np.array_equal(got, depth[..., [0, 1, 2, 4]]) and got.any()


def test_the_three_entries_on_the_same_made_covers(engine0):
    """Rows of 0, 1, 63, 64, 65 and 257 barcodes - the wavefront's and the workgroup's edges - through all three entries: the depth
    entry gives the five quantities of the restatement, the replicate entry its columns (S, READS, V1) at the fraction that keeps
    every barcode, the phase entry with one member the columns (N, V0, S, V1), and with three members the restatement's conjunction."""
    counters = TD._made_counters([0, 1, 63, 64, 65, 257])
    pos, seeds = [7, 11, 5000, 5001, 1 << 20, (1 << 32) - 1], PR.seeds(SEED, 3)
    thr, dthr = [PR.threshold(0.4), ONE], [ONE, 1 << 31]
    idents, cnts = [PR.idents(names) for names, _ in counters], [c for _, c in counters]
    five = DS.counts_from(counters, pos, thr, dthr, seeds)
    assert five.shape == (6, 3, 2, 2, 5) and not five[0].any() and all(five[v].any() for v in range(1, 6))
    depth = devplanes.spike_depth_counts(engine0, pos, idents, cnts, seeds, thr, dthr)
    assert np.array_equal(depth, five), np.argwhere(depth != five)[:5]
    reps = devplanes.spike_rep_counts(engine0, pos, idents, cnts, seeds, thr)
    assert reps.shape == (6, 3, 2, 3) and np.array_equal(reps, five[:, :, :, 0][..., [2, 3, 4]])
    one = _device(engine0, [(names, c.reshape(-1, 1, 3)) for names, c in counters], pos, seeds, thr, dthr)
    assert one.shape == (6, 3, 2, 2, 4) and np.array_equal(one, five[..., [0, 1, 2, 4]])
    # three members: a sure carrier, the made counters, and a carrier that every fourth barcode is only when hit
    sure, when_hit = np.array([3, 2, 3], np.uint32), np.array([4, 1, 3], np.uint32)
    joint = []
    for names, c in counters:
        cnt = np.stack([np.tile(sure, (len(c), 1)), c, np.tile(sure, (len(c), 1))], axis=1)
        cnt[1::4, 2] = when_hit
        joint.append((names, cnt))
    fails = np.concatenate([(2 * cnt[:, :, 1].astype(np.int64) <= cnt[:, :, 0]).sum(axis=1) for _, cnt in joint])
    assert (fails == 1).any() and (fails == 0).any() and (fails == 2).any()
    want = PH.counts_from(joint, pos, thr, dthr, seeds)
    got = _device(engine0, joint, pos, seeds, thr, dthr)
    assert got.shape == (6, 3, 2, 2, 4) and np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(got[..., [0, 2]], one[..., [0, 2]]) and (got[..., 1] <= one[..., 1]).all() and (got[..., 1] < one[..., 1]).any()


def test_eight_members_and_a_set_nobody_covers_between_two_that_are(engine0):
    joint = _made_joint([70, 0, 130], [8, 3, 2])                                          # (offsets 0, 70, 70, 200; rows of 24, 9 and 6 words)
    lead, seeds = [11, 5000, 1 << 20], PR.seeds(SEED, 2)
    thr, dthr = [PR.threshold(t) for t in (0.1, 0.5)], [DS.frac_thr(f) for f in (0.3, 1.0)]
    got = _device(engine0, joint, lead, seeds, thr, dthr)
    assert np.array_equal(got, PH.counts_from(joint, lead, thr, dthr, seeds))
    assert not got[1].any() and got[0].any() and got[2].any() and int(got[0, ..., 0].max()) <= 70 and int(got[2, ..., 0].max()) <= 130
    # with 8 members the conjunction bites: fewer carry all of them than carry the first
    c = joint[0][1].astype(np.int64)
    assert int(got[0, 0, 1, 1, 3]) < int((2 * np.where(True, c[:, 0, 2], 0) > c[:, 0, 0]).sum())


def test_thirty_two_cells_and_more_replicates_than_the_grid_is_deep(engine0):
    joint = _made_joint([300, 65], [2, 5])
    lead = [101, 202]
    thr = [PR.threshold(t) for t in (0.01, 0.05, 0.1, 0.2, 0.4, 0.6, 0.8, 1.0)]
    dthr = [DS.frac_thr(f) for f in (0.1, 0.25, 0.5, 1.0)]
    seeds = PR.seeds(PR.M64 - 3, 70)                                                    # (70 replicates > the 64 the entry launches; the seeds wrap)
    got = _device(engine0, joint, lead, seeds, thr, dthr)
    assert got.shape == (2, 70, 8, 4, 4)
    assert np.array_equal(got, PH.counts_from(joint, lead, thr, dthr, seeds))
    assert len({got[:, j].tobytes() for j in range(70)}) > 60
    assert np.array_equal(_device(engine0, joint, lead, seeds[:1], thr, dthr), got[:, :1])        # (R = 1)


def test_counts_refusals_launch_nothing(engine0):
    eng = engine0
    size = 8192
    out = DevBuf(eng, size).upload(np.full(size, 0x5A, np.uint8))
    src = DevBuf(eng, size).upload(np.zeros(size, np.uint8))
    half, above = np.full(40, 1 << 31, np.uint64), np.full(40, 1 << 31, np.uint64)
    above[1] = ONE + 1
    off, m = np.array([0, 3, 5], np.uint32), np.array([2, 8], np.uint32)

    def counts(off=off, m=m, n_sets=2, n_reps=2, thr=half, n_targets=2, dthr=half, n_fracs=2):
        return eng.L.smc_spike_phase_counts(eng.ctx, src.data_ptr(), src.data_ptr(), src.data_ptr(), off.ctypes.data, src.data_ptr(), m.ctypes.data,
                                            src.data_ptr(), src.data_ptr(), n_sets, src.data_ptr(), n_reps, thr.ctypes.data, n_targets,
                                            dthr.ctypes.data, n_fracs, out.data_ptr(), None)
    big_off = np.zeros(4097, np.uint32)
    for kw, msg in ((dict(m=np.array([2, 0], np.uint32)), "set 1 has 0 members, 1 .. 8 expected"), (dict(m=np.array([9, 1], np.uint32)), "set 0 has 9 members"),
                    (dict(off=np.array([0, 3, 2], np.uint32)), "offsets decrease at set 1"), (dict(n_targets=3, n_fracs=11), "3 targets x 11 fractions, at most 32 cells"),
                    (dict(n_targets=32, n_fracs=2), "at most 32 cells"), (dict(n_targets=33, n_fracs=1), "33 targets, at most 32"),
                    (dict(thr=above), "target 1: a threshold above 2^32"), (dict(dthr=above), "depth threshold 1 is above 2^32"),
                    (dict(n_reps=1001), "1001 replicates, at most 1000"), (dict(n_fracs=0), "0 fractions"),
                    (dict(n_sets=4097, off=big_off, m=np.ones(4097, np.uint32)), "at most 4096")):
        # (an output of 2^32 - 256 words: the entry checks it, and its own maxima - 4096 sets x 1000 replicates x 32 cells x 4 - stay below it)
        assert counts(**kw) == -4 and msg.encode() in eng.L.smc_last_error(), msg            # SMC_E_INPUT
    eng.L.smc_device_sync(eng.ctx)
    assert (out.download(np.uint8, size) == 0x5A).all()                                       # nothing zeroed, nothing launched
    out.free(); src.free()


# ---- the command line
def _lines(path):
    return [l.split("\t") for l in open(path).read().splitlines()]


def _tree(tmp_path, tag):
    """The files of the run with prefix `tag`, by suffix, with the prefix itself (a path in .cut.vcf, a name in the LOD summary) masked."""
    mask = lambda data: re.sub(b"(?m)^" + tag.encode() + b"(?=[.\t])", b"<prefix>", data.replace(str(tmp_path / tag).encode(), b"<prefix>"))
    return {f[len(tag):]: mask(open(str(tmp_path / f), "rb").read()) for f in sorted(os.listdir(str(tmp_path))) if f.startswith(tag + ".")}


def _pick(bam, fa, loci):
    """Two SNVs within 8 letters of each other - one MNV line - and one further away: the deepest loci of two windows."""
    pair = single = None
    for w in range(16 if len(loci) > 48 else 0, len(loci) - 7, 8):
        win = loci[w:w + 8]
        if win[-1][0] != win[0][0] or int(win[-1][1]) - int(win[0][1]) != 7:
            continue
        vs = SR.pick_positions(bam, fa, win, 2)
        if pair is None and len(vs) == 2:
            pair = vs
        elif pair is not None and vs:
            single = SR.pick_positions(bam, fa, win, 1)[0]
            break
    assert pair is not None and single is not None
    return pair + [single]


def _cli_contract(tmp_path, bam, fa, loci, P, targets, fracs, n_reps):
    variants = _pick(bam, fa, loci)
    sets = [(0, 1)]
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    a, b, s = variants
    ref = fasta.FastaFile(fa).fetch(a.chrom, a.pos - 1, b.pos).upper()
    vfile = str(tmp_path / "v.vcf")
    open(vfile, "w").write(PH.mnv_line(a.chrom, a.pos, ref, {0: a.alt, b.pos - a.pos: b.alt}) + PH.snv_line(s))
    loose = R.write_variants(str(tmp_path / "loose.vcf"), variants, vcf=True)
    T, F = len(targets), len(fracs)
    depth = ",".join("%g" % f for f in fracs)
    kw = dict(spikeAF=",".join("%g" % t for t in targets), dsSeed=SEED, spikeReps=n_reps, spikeDepth=depth)
    cells = [(t, f, max(1, int(py2_round(f * P.mtDepth))), ".spikeAF%g.dsMT%g" % (t, f)) for t in targets for f in fracs]
    # 1. no MNV line: with and without the flag the trees are identical
    TL._run_cli(tmp_path, "n0", bam, fa, bed, P, flags=["--lod"], spikeVariants=loose, **kw)
    TL._run_cli(tmp_path, "n1", bam, fa, bed, P, flags=["--lod", "--spikePhase"], spikeVariants=loose, **kw)
    assert _tree(tmp_path, "n0") == _tree(tmp_path, "n1") and ".spikeAF.detection.txt" in _tree(tmp_path, "n0")
    # 2. the phased run: every full-depth file unchanged; three pages added to the tree
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=["--lod", "--spikePhase"], spikeVariants=vfile, **kw)
    mine, unph = _tree(tmp_path, "o"), _tree(tmp_path, "n0")
    assert sorted(set(mine) - set(unph)) == [".spikeAF.phase.replicates.txt", ".spikeAF.phase.sensitivity.txt", ".spikeAF.phase.txt"]
    assert not set(unph) - set(mine)
    for sfx in SUFFIXES + TL.LOD_SUFFIXES:
        assert mine[sfx] == unph[sfx], sfx
    assert any(mine[".spikeAF%g%s" % (t, SUFFIXES[0])] != unph[".spikeAF%g%s" % (t, SUFFIXES[0])] for t in targets)      # (another draw at the second member)
    # 3. each target's files: a plain run on the tool's --phased BAM; each cell's: the two-step workflow on it
    for t in targets:
        out = str(tmp_path / ("sp%g.bam" % t))
        sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=SEED, refGenome=fa, phased=True))
        bamio.write_bai(out)
        ref_run = TL._run_cli(tmp_path, "w.spikeAF%g" % t, out, fa, bed, P, dsMT=depth, dsSampler="philox", dsSeed=SEED)
        theirs = [x.replace(ref_run.encode(), (got + ".spikeAF%g" % t).encode()) for x in TL._read(ref_run, SUFFIXES)]
        assert TL._read(got + ".spikeAF%g" % t, SUFFIXES) == theirs, "target %g" % t
        for f in fracs:
            sfx = ".spikeAF%g.dsMT%g" % (t, f)
            theirs = [x.replace((ref_run + ".dsMT%g" % f).encode(), (got + sfx).encode()) for x in TL._read(ref_run + ".dsMT%g" % f, SUFFIXES)]
            assert TL._read(got + sfx, SUFFIXES) == theirs, "cell %s" % sfx
    # 4. the phase page: the restatement's numbers and the outputs' own .cut.txt
    counts, _ = PH.restate_counts(bam, fa, variants, sets, targets, [1.0] + list(fracs), SEED, n_reps)
    page = _lines(got + ".spikeAF.phase.txt")
    assert page[0] == list(spike.PHASE_HEADER) and len(page) == 1 + 1 + T + T * F
    outs = [(None, None, P.mtDepth, got)] + [(t, None, P.mtDepth, got + ".spikeAF%g" % t) for t in targets] + \
           [(t, f, d, got + sfx) for t, f, d, sfx in cells]
    name = "%s:%d" % (a.chrom, a.pos)

    def want_line(o, c):
        _, cut = dsaf.read_output(o[3])
        called = int(all((v.chrom, "%d" % v.pos) in cut and cut[(v.chrom, "%d" % v.pos)][0] == v.ref and v.alt in cut[(v.chrom, "%d" % v.pos)][1]
                         for v in (a, b)))
        return [name, a.chrom, "%d,%d" % (a.pos, b.pos), a.ref + "," + b.ref, a.alt + "," + b.alt, "full" if o[0] is None else "%g" % o[0],
                "full" if o[1] is None else "%g" % o[1], "%d" % o[2]] + ["%d" % x for x in c] + \
               [dsaf.frac_text(int(c[3]) / int(c[0]) if int(c[0]) else 0.0), "%d" % called]
    for k, o in enumerate(outs):
        if o[0] is None:
            c = [counts[0, 0, 0, 0, 0], counts[0, 0, 0, 0, 1], 0, counts[0, 0, 0, 0, 1]]
        else:
            c = counts[0, 0, targets.index(o[0]), 0 if o[1] is None else 1 + fracs.index(o[1])]
        assert page[1 + k] == want_line(o, c), k
    # 5. the replicate lines: the phase page of a separate run with --dsSeed s_j; the sensitivity table what the replicate lines say
    reps = _lines(got + ".spikeAF.phase.replicates.txt")
    assert reps[0] == list(spike.PHASE_REPLICATES_HEADER) and len(reps) == 1 + (T + T * F) * n_reps
    for j, seed_j in enumerate(PR.seeds(SEED, n_reps)):
        one = TL._run_cli(tmp_path, "s%d" % j, bam, fa, bed, P, flags=["--spikePhase"], spikeVariants=vfile, spikeAF=kw["spikeAF"], spikeDepth=depth,
                          dsSeed=seed_j)
        single_page = _lines(one + ".spikeAF.phase.txt")
        for c in range(T + T * F):
            line = reps[1 + c * n_reps + j]
            assert line[8:10] == ["%d" % j, "%d" % seed_j] and line[:8] + line[10:] == single_page[2 + c], (c, j)
            t, f = (c, 0) if c < T else (divmod(c - T, F)[0], 1 + divmod(c - T, F)[1])
            assert line[10:14] == ["%d" % x for x in counts[0, j, t, f]]
        if j == 0:
            assert single_page == page
    sens = _lines(got + ".spikeAF.phase.sensitivity.txt")
    assert sens[0] == list(spike.PHASE_SENSITIVITY_HEADER) and len(sens) == 1 + T + T * F
    for c in range(T + T * F):
        per = reps[1 + c * n_reps:1 + (c + 1) * n_reps]
        called = sum(int(l[PH.R_CALLED]) for l in per)
        lo, hi = PR.wilson(called, n_reps)
        afs = [int(l[PH.R_V1]) / int(l[PH.R_N]) if int(l[PH.R_N]) else 0.0 for l in per]
        assert sens[1 + c] == per[0][:8] + ["%d" % n_reps, "%d" % called, dsaf.frac_text(called / n_reps), dsaf.frac_text(lo), dsaf.frac_text(hi),
                                            dsaf.frac_text(sum(afs) / n_reps), dsaf.frac_text(min(afs)), dsaf.frac_text(max(afs))]


def test_cli_on_the_synthetic_bam(tmp_path):
    bam, fa, loci, P = TS._synth(str(tmp_path))
    _cli_contract(tmp_path, bam, fa, loci[:64], P, (0.2, 0.05), (0.5, 0.25), 4)


def test_cli_on_bam_cigars(tmp_path):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    _cli_contract(tmp_path, bam, fa, loci, P, (0.3, 0.1), (0.5, 1.0), 4)
