"""--spikeIndelReps / --spikeIndelDepth on the GPU: smc_spike_indels_reps against smc_spike_indels copy by copy and field for field
(the bytes between the copies keep their pattern, a capacity one short stays one copy's affair, the entry's refusals); the four
counters of the pre-pass - smc_allele_carriers' on the run and on the copy spiked at 2^32, smc_spike_indel_touch - against the host
restatement (tests/spike_indel_reps_restate.py); smc_spike_indel_counts against the restatement and against what the copies hold; with
SNVs alone against smc_spike_rep_counts and smc_spike_depth_counts."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import abi, devplanes, fasta
from smcounter_amd.engine import DevBuf
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import spike_indel_reps_restate as QR  # noqa: E402
import spike_indel_restate as IR  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import test_gpu_spike_indels as TG  # noqa: E402  (its inputs and its decoded run in HBM)

pytestmark = pytest.mark.gpu
SEED = TG.SEED
POISON = 0x5A
THR = [1 << 31, 1 << 32, 0, 1 << 30, 1 << 31]           # per copy: copy 1 takes every barcode, copy 2 none


def _single(run, variants, thr, seed, caps=None):
    """smc_spike_indels with every variant at `thr` -> dict(aln, bq, cig (up to the copy's totals), nm, n_indel, stats, totals)."""
    A, n = run.A, len(run.A["aln"])
    var, ins, _ = devplanes.spike_indel_variants(variants, int(thr))
    out, stats, totals, nm, n_indel = devplanes.spike_indel_run(run.eng, run.up, A, var, ins, run.idents, seed, run.P.mismatchThr, run.nm, run.n_indel,
                                                               caps=caps)
    cap = caps or devplanes.spike_indel_caps(A, var)
    try:
        aln = out.aln.download(abi.DEV_ALN_DTYPE, n)
        # (what the copy holds: the run's own pools, then the relocated records' - all of them unless it is over capacity)
        used_p = max(len(A["bq"]) // 2, int((aln["seq_off"].astype(np.int64) + aln["l_seq"]).max()))
        used_c = max(len(A["cig"]), int((aln["cig_off"].astype(np.int64) + aln["n_cig"]).max()))
        assert int(totals[2]) or (used_p, used_c) == (int(totals[0]), int(totals[1]))
        return dict(aln=aln, bq=out.bq.download(np.uint8, 2 * cap[0]), cig=out.cig.download(np.uint32, cap[1]),
                    nm=nm, n_indel=n_indel, stats=stats, totals=totals, used=(used_p, used_c))
    finally:
        out.aln.free(); out.bq.free(); out.cig.free()


def _copies(run, variants, seeds, thr, caps=None):
    """smc_spike_indels_reps into buffers filled with POISON -> (per copy the same dict, the three whole buffers, strides, caps)."""
    A, n = run.A, len(run.A["aln"])
    var, ins, _ = devplanes.spike_indel_variants(variants, 0)
    got = devplanes.spike_indel_run_copies(run.eng, run.up, A, var, ins, run.idents, seeds, thr, run.P.mismatchThr, run.nm, run.n_indel, caps=caps,
                                           fill=POISON, mism=True)
    try:
        (sa, sb, sc), B = got["strides"], len(seeds)
        whole = [got[k].download(np.uint8, st * B) for k, st in zip(("aln", "bq", "cig"), (sa, sb, sc))]
    finally:
        for k in ("aln", "bq", "cig"):
            got[k].free()
    out = []
    for c in range(B):
        out.append(dict(aln=whole[0][c * sa:c * sa + 36 * n].view(abi.DEV_ALN_DTYPE), bq=whole[1][c * sb:(c + 1) * sb],
                        cig=whole[2][c * sc:(c + 1) * sc].view(np.uint32), nm=got["nm"][c], n_indel=got["n_indel"][c], stats=got["stats"][c],
                        totals=got["totals"][c]))
    # the run itself is only read
    assert run.up.aln.download(abi.DEV_ALN_DTYPE, n).tobytes() == A["aln"].tobytes()
    assert run.up.bq.download(np.uint8, len(A["bq"])).tobytes() == A["bq"].tobytes()
    assert run.up.cig.download(np.uint32, len(A["cig"])).tobytes() == A["cig"].tobytes()
    return out, whole, (sa, sb, sc), got["caps"]


def _assert_same_copy(got, want, A, strides, caps):
    """Copy `got` of the batched call is the single call's: records field for field, each record's pairs and words through its
    offsets, the pools up to what the copy uses, NM', n_indel', statistics and totals; behind that the pattern."""
    n = len(A["aln"])
    assert [int(x) for x in got["totals"]] == [int(x) for x in want["totals"]]
    for f in abi.DEV_ALN_DTYPE.names:
        assert np.array_equal(got["aln"][f], want["aln"][f]), f
    used_p, used_c = want["used"]
    for i in range(n):
        w = want["aln"][i]
        so, ls, co, nc = int(w["seq_off"]), int(w["l_seq"]), int(w["cig_off"]), int(w["n_cig"])
        assert got["bq"][2 * so:2 * (so + ls)].tobytes() == want["bq"][2 * so:2 * (so + ls)].tobytes(), i
        assert got["cig"][co:co + nc].tolist() == want["cig"][co:co + nc].tolist(), i
    assert got["bq"][:2 * used_p].tobytes() == want["bq"][:2 * used_p].tobytes() and got["cig"][:used_c].tobytes() == want["cig"][:used_c].tobytes()
    assert np.array_equal(got["nm"], want["nm"]) and np.array_equal(got["n_indel"], want["n_indel"]) and np.array_equal(got["stats"], want["stats"])
    # nothing beyond what the copy holds, nothing beyond its capacity
    assert (got["bq"][2 * used_p:] == POISON).all() and (got["cig"].view(np.uint8)[4 * used_c:] == POISON).all()
    assert used_p <= caps[0] and used_c <= caps[1]


@pytest.mark.parametrize("n_copies", (1, 5))
@pytest.mark.parametrize("name", ("case", "bam_cigars", "synth"))
def test_batched_copies_equal_single_calls(engine0, tmp_path, name, n_copies):
    bam_path, fa, loci, P, variants = TG._inputs(name, str(tmp_path))
    relocated = 0
    for chrom, lo, hi in ds_restate.stretches(loci):
        vs = [v for v in variants if v.chrom == chrom and lo < v.pos <= hi]
        if not vs:
            continue
        run = TG.Run(engine0, bam_path, chrom, lo, hi, P)
        try:
            A, n = run.A, len(run.A["aln"])
            seeds, thr = PR.seeds(SEED, n_copies), THR[:n_copies]
            got, whole, (sa, sb, sc), caps = _copies(run, vs, seeds, thr)
            for c in range(n_copies):
                want = _single(run, vs, thr[c], seeds[c])
                _assert_same_copy(got[c], want, A, (sa, sb, sc), caps)
                assert int(want["totals"][2]) == 0
                relocated += int((want["aln"]["seq_off"] != A["aln"]["seq_off"]).sum())
                # the bytes between a copy's records and the next stride
                assert (whole[0][c * sa + 36 * n:(c + 1) * sa] == POISON).all()
            if n_copies == 5 and name != "bam_cigars":
                assert not got[2]["stats"].any() and got[2]["aln"].tobytes() == A["aln"].tobytes()      # threshold 0: the run
                assert got[1]["stats"][:, 0].sum() > got[0]["stats"][:, 0].sum() > 0                        # 2^32: every barcode
                assert got[0]["aln"].tobytes() != got[4]["aln"].tobytes()                                   # one threshold, two seeds
            if name == "synth":
                assert n > 3 * 256 and len({int(i) // 256 for i in np.flatnonzero(got[0]["aln"]["seq_off"] != A["aln"]["seq_off"])}) >= 3
        finally:
            run.close()
    assert relocated > 0


def test_a_copy_over_capacity_is_its_own_affair(engine0, tmp_path):
    run, bam_path, fa, P, variants = TG._case_run(engine0, tmp_path)
    try:
        A = run.A
        seeds = PR.seeds(SEED, 5)
        need = _single(run, variants, THR[1], seeds[1])["totals"]
        caps = (int(need[0]) - 1, int(need[1]))                      # exactly what copy 1 needs, minus one pair
        got, whole, strides, _ = _copies(run, variants, seeds, THR, caps=caps)
        fits = 0
        for c in range(5):
            want = _single(run, variants, THR[c], seeds[c], caps=caps)
            _assert_same_copy(got[c], want, A, strides, caps)
            assert int(got[c]["totals"][2]) == (1 if c == 1 else 0)
            fits += c != 1 and int(got[c]["totals"][0]) > len(A["bq"]) // 2
        assert fits >= 2                                             # copies that relocate records and fit are exact
        # copy 1: the record that does not fit is the run's own, by smc_spike_indels' rule
        full = _single(run, variants, THR[1], seeds[1])
        short = np.flatnonzero(got[1]["aln"]["seq_off"] != full["aln"]["seq_off"]).tolist()
        assert len(short) == 1 and got[1]["aln"][short[0]]["seq_off"] == A["aln"][short[0]]["seq_off"]
        assert (got[1]["aln"]["seq_off"].astype(np.int64) + got[1]["aln"]["l_seq"]).max() <= caps[0]
    finally:
        run.close()


def test_refusals_launch_nothing(engine0):
    eng = engine0
    n = 8
    ok = np.zeros(3, abi.SPIKE_INDEL_VARIANT_DTYPE)
    ok["pos0"], ok["kind"], ok["ref"], ok["alt"], ok["len"] = [5, 9, 20], [0, 1, 2], ord("A"), [ord("G"), ord("A"), ord("A")], [0, 2, 3]
    bufs = [DevBuf(eng, 8192).upload(np.full(8192, POISON, np.uint8)) for _ in range(7)]   # aln, bq, cig, nm, n_indel, stats, totals
    src = DevBuf(eng, 4096).upload(np.zeros(4096, np.uint8))
    seeds = np.arange(70, dtype=np.uint64)

    def call(var=ok, n_copies=2, thr=(1 << 31, 1 << 32), caps=(100, 100), strides=(512, 256, 512), n_ins=2, shift=(0, 0, 0, 0, 0)):
        d_var = DevBuf(eng, var.nbytes + 256).upload(np.ascontiguousarray(var).view(np.uint8).reshape(-1))
        t = np.array(list(thr) + [0] * 70, np.uint64)
        b = [x.data_ptr() for x in bufs]
        rc = eng.L.smc_spike_indels_reps(eng.ctx, src.data_ptr(), n, src.data_ptr() + shift[0], 32, src.data_ptr() + shift[1], 64, d_var.data_ptr(),
                                         var.ctypes.data, len(var), src.data_ptr(), n_ins, src.data_ptr(), 4, seeds.ctypes.data, t.ctypes.data,
                                         n_copies, 6.0, src.data_ptr(), src.data_ptr(), caps[0], caps[1], b[0] + shift[2], strides[0],
                                         b[1] + shift[3], strides[1], b[2] + shift[4], strides[2], b[3], b[4], b[5], b[6], None)
        d_var.free()
        return rc

    def edit(**kw):
        v = ok.copy()
        for k, (i, x) in kw.items():
            v[k][i] = x
        return v
    for kw, msg in ((dict(n_copies=0), "0 copies"), (dict(n_copies=65), "65 copies"), (dict(n_copies=-1), "-1 copies"),
                    (dict(thr=(1 << 31, (1 << 32) + 1)), "copy 1: a threshold above 2^32"),
                    (dict(strides=(36 * n - 4, 256, 512)), "smaller than a copy"), (dict(strides=(512, 192, 512)), "smaller than a copy"),
                    (dict(strides=(512, 256, 384)), "smaller than a copy"),
                    (dict(strides=(514, 256, 512)), "multiple of 4"), (dict(strides=(512, 264, 512)), "of 16"), (dict(strides=(512, 256, 520)), "of 16"),
                    (dict(shift=(4, 0, 0, 0, 0)), "of 16"), (dict(shift=(0, 8, 0, 0, 0)), "of 16"), (dict(shift=(0, 0, 2, 0, 0)), "multiple of 4"),
                    (dict(shift=(0, 0, 0, 8, 0)), "of 16"), (dict(shift=(0, 0, 0, 0, 4)), "of 16"),
                    (dict(var=edit(pos0=(1, 5))), "not strictly ascending"), (dict(var=edit(pos0=(2, 10))), "footprint overlaps"),
                    (dict(var=edit(ref=(0, ord("N")))), "outside ACGT"), (dict(var=edit(kind=(1, 3))), "has kind 3"),
                    (dict(var=edit(len=(2, 256))), "a length of 256"), (dict(n_ins=1), "inserted letters"),
                    (dict(caps=(63, 100)), "capacities"), (dict(caps=(100, 31)), "capacities"), (dict(caps=(1 << 32, 100), strides=(512, 1 << 34, 512)), "capacities")):
        assert call(**kw) < 0 and msg.encode() in eng.L.smc_last_error(), msg
    # (the variants' own thresholds are not read: one above 2^32 is no refusal of this entry - it is of smc_spike_indel_touch's neither)
    d_out = DevBuf(eng, 4096).upload(np.full(4096, POISON, np.uint8))
    d_var = DevBuf(eng, 4096).upload(np.zeros(4096, np.uint8))
    for var, n_bc, msg in ((edit(pos0=(1, 5)), 4, "not strictly ascending"), (edit(pos0=(2, 10)), 4, "footprint overlaps"),
                           (edit(kind=(1, 3)), 4, "has kind 3"), (ok, 1 << 31, "run too large"), (ok, 0x7FFFFEFF, "too many counters")):
        rc = eng.L.smc_spike_indel_touch(eng.ctx, src.data_ptr(), n, src.data_ptr(), 32, 64, d_var.data_ptr(), var.ctypes.data, len(var), n_bc,
                                         d_out.data_ptr(), None)
        assert rc < 0 and msg.encode() in eng.L.smc_last_error(), msg
    eng.L.smc_device_sync(eng.ctx)
    for b in bufs:
        assert (b.download(np.uint8, 8192) == POISON).all()                              # nothing copied, nothing launched
    assert (d_out.download(np.uint8, 4096) == POISON).all()
    for b in bufs + [src, d_out, d_var]:
        b.free()


def _kept(eng, bam, fa, variants, P, targets=(0.5,), depth=None):
    """devplanes.spike_rules with the four counters -> (covers, counters) per variant; the kept runs are freed."""
    keep = {}
    more = dict(depth=depth) if depth is not None else {}
    try:
        devplanes.spike_rules(bam, fasta.FastaFile(fa), variants, list(targets), [P] * len(targets), SEED, eng, keep=keep, indel_counters=True, **more)
    finally:
        devplanes.free_af_runs(keep.get("runs"))
    return keep["covers"], keep["counters"]


@pytest.fixture(scope="module")
def restated(tmp_path_factory):
    """The inputs and their restated counters, made once: name -> (bam, fasta, loci, params, variants, counters, cases)."""
    out = {}
    for name in ("case", "bam_cigars"):
        tmp = tmp_path_factory.mktemp(name)
        bam, fa, loci, P, variants = TG._inputs(name, str(tmp))
        counters, cases = QR.host_counters(bam, variants, fa)
        out[name] = (bam, fa, loci, P, variants, counters, cases)
    return out


def test_the_inputs_hold_the_cases_three_counters_miss(restated):
    """On the CPU: a record whose anchor letter mismatches REF, one that shows the listed insertion already, one that ends inside a
    deletion's footprint."""
    total = {c: 0 for c in QR.CASES}
    for name, (_, _, _, _, variants, counters, cases) in restated.items():
        for v, c in zip(variants, cases):
            total["anchor_mismatch"] += c["anchor_mismatch"]
            total["shows_it_already"] += c["shows_it_already"] if v.kind == af.INS else 0
            total["ends_in_footprint"] += c["ends_in_footprint"] if v.kind == af.DEL else 0
    assert all(total[c] > 0 for c in QR.CASES), total
    # touch > alt1 - alt0 somewhere (another letter at the anchor), alt1 > touch somewhere (shows it already)
    both = [cnt.astype(np.int64) for _, _, _, _, vs, cs, _ in restated.values() for (_, cnt), v in zip(cs, vs) if v.kind != af.SNV]
    assert any((c[:, 2] < c[:, 3]).any() for c in both) and any((c[:, 2] > c[:, 3]).any() for c in both)


@pytest.mark.parametrize("name", ("case", "bam_cigars"))
def test_device_counters_equal_the_restatement(engine0, restated, name):
    bam, fa, loci, P, variants, counters, _ = restated[name]
    covers, got = _kept(engine0, bam, fa, variants, P)
    want_cov, want = QR.device_order(counters, PR.idents)
    for i, v in enumerate(variants):
        order = np.argsort(covers[i], kind="stable")
        assert np.array_equal(covers[i][order], want_cov[i]), i
        assert got[i].dtype == np.uint32 and got[i].shape == (len(covers[i]), 4)
        for k, what in enumerate(("reads", "alt0", "alt1", "touch")):
            assert np.array_equal(got[i][order][:, k], want[i][:, k]), (v.pos, what)


TARGETS, REPS, FRACS = (0.5, 0.25), 4, (1.0, 0.5)


@pytest.mark.parametrize("name", ("case", "bam_cigars"))
def test_stride_4_counts_equal_the_restatement(engine0, restated, name):
    bam, fa, loci, P, variants, counters, _ = restated[name]
    covers, cnt = QR.device_order(counters, PR.idents)
    pos, seeds, thr = [v.pos for v in variants], PR.seeds(SEED, REPS), [QR.threshold(t) for t in TARGETS]
    dthr = [QR.frac_thr(f) for f in FRACS]
    got = devplanes.spike_indel_counts(engine0, pos, covers, cnt, seeds, thr)
    assert got.shape == (len(variants), REPS, len(TARGETS), 3) and np.array_equal(got, QR.counts_from(counters, pos, thr, seeds))
    cells = devplanes.spike_indel_counts(engine0, pos, covers, cnt, seeds, thr, dthr)
    assert cells.shape == (len(variants), REPS, len(TARGETS), len(FRACS), 5) and np.array_equal(cells, QR.counts_from(counters, pos, thr, seeds, dthr))
    assert np.array_equal(cells[:, :, :, 0, 2:], got) and got.any() and (cells[:, :, :, 1, 0] < cells[:, :, :, 0, 0]).any()


def test_stride_4_counts_equal_what_the_copies_hold(engine0, restated):
    """READS from the copies' statistics, N and V1 from smc_allele_carriers on every copy - at fraction 0.5 through select_run."""
    bam, fa, loci, P, variants, counters, _ = restated["case"]
    (chrom, lo, hi), = ds_restate.stretches(loci)
    covers, cnt = QR.device_order(counters, PR.idents)
    pos, seeds, thr = [v.pos for v in variants], PR.seeds(SEED, REPS), [QR.threshold(t) for t in TARGETS]
    cells = devplanes.spike_indel_counts(engine0, pos, covers, cnt, seeds, thr, [QR.frac_thr(f) for f in FRACS])
    run = TG.Run(engine0, bam, chrom, lo, hi, P)
    try:
        A, n = run.A, len(run.A["aln"])
        var, ins, order = devplanes.spike_indel_variants(variants, 0)
        af_var, af_ins = devplanes.af_run_variants(variants, chrom, lo, fasta.FastaFile(fa))
        for t in range(len(TARGETS)):
            made = devplanes.spike_indel_run_copies(engine0, run.up, A, var, ins, run.idents, seeds, [thr[t]] * REPS, P.mismatchThr, run.nm, run.n_indel)
            try:
                sa, sb, sc = made["strides"]
                assert not made["totals"][:, 2].any()
                for j in range(REPS):
                    copy = devplanes.RunOnDevice(devplanes._BufView(made["aln"], j * sa), devplanes._BufView(made["cig"], j * sc),
                                                 devplanes._BufView(made["bq"], j * sb), run.up.loc, run.up.ref, n, run.up.loc_host)
                    reads = np.zeros(len(variants), np.int64)
                    reads[order] = made["stats"][j, :, 0]
                    assert reads.tolist() == cells[:, j, t, 0, 3].tolist(), (t, j)
                    cov, car, _ = devplanes.allele_carriers_run(engine0, copy, A, lo, af_var, af_ins)
                    assert cov.sum(axis=1).tolist() == cells[:, j, t, 0, 0].tolist() and car.sum(axis=1).tolist() == cells[:, j, t, 0, 4].tolist(), (t, j)
                    sel, sel_counts, d_orig = devplanes.select_run(engine0, copy, A, lo, idents=run.idents, frac=FRACS[1], seed=seeds[j])
                    try:
                        cov, car, _ = devplanes.allele_carriers_run(engine0, sel, sel_counts, lo, af_var, af_ins)
                    finally:
                        sel.free(shared=False); d_orig.free()
                    assert cov.sum(axis=1).tolist() == cells[:, j, t, 1, 0].tolist() and car.sum(axis=1).tolist() == cells[:, j, t, 1, 4].tolist(), (t, j)
            finally:
                for k in ("aln", "bq", "cig"):
                    made[k].free()
        assert cells[:, :, :, :, 2].any() and cells[:, :, :, :, 3].any()
    finally:
        run.close()


def test_snvs_only_equal_the_three_counter_entries(engine0):
    """alt1 = touch = single: the stride-4 entry returns what smc_spike_rep_counts and smc_spike_depth_counts return.  Variants of 0, 1,
    300 and 777 covering barcodes: none, one lane, more than one workgroup, no multiple of the tile."""
    rng = np.random.Generator(np.random.PCG64(5))
    covers, cnt3 = [], []
    for size in (0, 1, 300, 777):
        covers.append(rng.integers(1, 1 << 63, size=size, dtype=np.uint64))
        reads = rng.integers(1, 9, size=size)
        cnt3.append(np.stack([reads, rng.integers(0, 9, size=size) % (reads + 1), rng.integers(0, 9, size=size) % (reads + 1)], axis=1).astype(np.uint32))
    cnt4 = [np.concatenate([c, c[:, 2:3]], axis=1) for c in cnt3]
    pos, seeds = [101, 5, 70000, 1 << 31], PR.seeds(SEED, 5)
    thr, dthr = [QR.threshold(t) for t in (0.5, 0.05, 0.9)], [1 << 32, QR.frac_thr(0.5), QR.frac_thr(0.1)]
    want = devplanes.spike_rep_counts(engine0, pos, covers, cnt3, seeds, thr)
    assert np.array_equal(devplanes.spike_indel_counts(engine0, pos, covers, cnt4, seeds, thr), want) and want.any()
    want = devplanes.spike_depth_counts(engine0, pos, covers, cnt3, seeds, thr, dthr)
    assert np.array_equal(devplanes.spike_indel_counts(engine0, pos, covers, cnt4, seeds, thr, dthr), want) and want.any()
    with pytest.raises(ValueError, match="4 counters per covering barcode"):
        devplanes.spike_indel_counts(engine0, pos, covers, cnt3, seeds, thr)
