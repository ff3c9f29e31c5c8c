"""--spikeReps on the GPU: smc_spike_alleles_reps against single smc_spike_alleles calls and the restatement, byte for byte;
smc_spike_rep_counts against the restatement (tests/spike_reps_restate.py: spike_restate once per seed); the command line against
separate runs with --dsSeed s_j; a deep synthetic locus near the caller's limit, where the replicates disagree."""
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import abi, bamio, devplanes, dsaf, spike
from smcounter_amd.engine import DevBuf

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402
import test_gpu_ds_af_reps as TA  # noqa: E402  (its deep synthetic run)
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line)
import test_gpu_spike as TS  # noqa: E402  (its inputs, the single call, the restatement's bytes)

pytestmark = pytest.mark.gpu
SEED = 20240607
INPUTS = ("case", "bam_cigars", "synth")
COPY_SEEDS = (SEED, SEED + 1, 3, (1 << 63) + 5, PR.M64)
COPY_T = (0.0, 1.0, 0.5, 0.2, 0.05)                 # (thresholds 0 and 2^32 in the same call)
REPS, TARGETS = 5, (0.05, 0.3, 0.7)


def _variants(name, bam_path, fa, here, given):
    return given or (SR.pick_positions(bam_path, fa, here[120:136], 4) if name == "synth" else SR.pick_positions(bam_path, fa, here, 3))


def _svar(variants):
    var = np.zeros(len(variants), abi.SPIKE_VARIANT_DTYPE)
    for k, v in enumerate(sorted(variants, key=lambda v: v.pos)):
        var[k]["pos0"], var[k]["ref"], var[k]["alt"], var[k]["thr"] = v.pos - 1, ord(v.ref), ord(v.alt), 12345      # (thr: not read)
    return var


def _copies(eng, up, A, var, idents, seeds, thr, P, mism, strides):
    """One call -> (records bytes, pool bytes (the whole outputs, pre-filled with 0x5A), stats)."""
    d_aln, d_bq, (sa, sb), stats = devplanes.spike_run_copies(eng, up, A, var, idents, seeds, thr, P.mismatchThr, mism[0], mism[1],
                                                             strides=strides, fill=0x5A)
    try:
        return d_aln.download(np.uint8, sa * len(seeds)), d_bq.download(np.uint8, sb * len(seeds)), stats
    finally:
        d_aln.free(); d_bq.free()


@pytest.mark.parametrize("name", INPUTS)
def test_batched_rewrite_equals_single_calls_and_the_restatement(engine0, tmp_path, name):
    bam_path, fa, loci, P, given = TS._inputs(name, str(tmp_path))
    nat, py = bamio.NativeBam(bam_path), bamio.BamFile(bam_path)
    thr = [PR.threshold(t) for t in COPY_T]
    assert thr[0] == 0 and thr[1] == 1 << 32
    copies = rewritten = 0
    for chrom, lo, hi in ds_restate.stretches(loci):
        vs = _variants(name, bam_path, fa, [(chrom, p) for p in range(lo + 1, hi + 1)], given)
        if not vs:
            continue
        A = nat.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
        n, nb = len(A["aln"]), len(A["bq"])
        idents, mism = nat.barcode_idents(A["n_bc"]), nat.run_mismatches(n)
        sa, sb = devplanes.spike_copy_strides(n, nb // 2)
        strides = (sa + 260, sb + 528)                                  # (larger than a copy, and than the rounded copy)
        assert strides[0] > 36 * n and strides[1] > nb
        up = devplanes.upload_run(engine0, A, "A" * A["nl"])
        try:
            aln, bq, stats = _copies(engine0, up, A, _svar(vs), idents, COPY_SEEDS, thr, P, mism, strides)
            aln2, bq2, stats2 = _copies(engine0, up, A, _svar(vs), idents, COPY_SEEDS, thr, P, mism, strides)
            one = _copies(engine0, up, A, _svar(vs), idents, COPY_SEEDS[2:3], thr[2:3], P, mism, strides)
            assert up.aln.download(abi.DEV_ALN_DTYPE, n).tobytes() == A["aln"].tobytes()            # the run's arrays are only read
            assert up.bq.download(np.uint8, nb).tobytes() == A["bq"].tobytes()
        finally:
            up.free()
        assert aln2.tobytes() == aln.tobytes() and bq2.tobytes() == bq.tobytes() and np.array_equal(stats, stats2)
        recs = py.fetch(chrom, lo, hi)
        with PR.shared_pileups():
            for c, (s, t) in enumerate(zip(COPY_SEEDS, COPY_T)):
                mine_aln, mine_bq = aln[c * strides[0]:c * strides[0] + 36 * n], bq[c * strides[1]:c * strides[1] + nb]
                # the gaps still hold the fill
                assert (aln[c * strides[0] + 36 * n:(c + 1) * strides[0]] == 0x5A).all() and (bq[c * strides[1] + nb:(c + 1) * strides[1]] == 0x5A).all()
                # == smc_spike_alleles with that seed and threshold
                s_aln, s_bq, s_stats = TS._run_kernel(engine0, nat, A, chrom, vs, thr[c], s, P)
                assert mine_bq.tobytes() == s_bq.tobytes() and mine_aln.tobytes() == s_aln.tobytes() and np.array_equal(stats[c], s_stats)
                # == the restatement at that seed
                records, st = SR.restate(bam_path, fa, vs, t, s, P.mismatchThr)
                want_aln, want_bq = TS._expected(A, recs, records)
                assert mine_bq.tobytes() == want_bq.tobytes() and mine_aln.tobytes() == want_aln.tobytes()
                assert stats[c, :, 0].tolist() == [x["READS"] for x in st] and stats[c, :, 1].tolist() == [x["NMINC"] for x in st]
                copies += 1
        assert not stats[0].any() and aln[:36 * n].tobytes() == A["aln"].tobytes() and bq[:nb].tobytes() == A["bq"].tobytes()    # (threshold 0)
        assert len({bq[c * strides[1]:c * strides[1] + nb].tobytes() for c in range(5)}) >= 4
        rewritten += int(stats[:, :, 0].sum())
        # n_copies = 1: copy 2 of the call of five
        assert one[0][:36 * n].tobytes() == aln[2 * strides[0]:2 * strides[0] + 36 * n].tobytes()
        assert one[1][:nb].tobytes() == bq[2 * strides[1]:2 * strides[1] + nb].tobytes() and np.array_equal(one[2][0], stats[2])
        if name == "synth":
            assert n > 2000 and int(A["n_bc"]) > 64
    assert copies >= 5 and rewritten > 0
    nat.close(); py.close()


def _check_counts(eng, bam_path, fa, variants, P, seed=SEED, n_reps=REPS, targets=TARGETS):
    """smc_spike_rep_counts over the host-built counters == the restatement, for every (v, j, t) -> triples compared."""
    counters = PR.host_counters(bam_path, fa, variants)
    covers, cnts = [PR.idents(names) for names, _ in counters], [c for _, c in counters]
    thr = [PR.threshold(t) for t in targets]
    got = devplanes.spike_rep_counts(eng, [v.pos for v in variants], covers, cnts, PR.seeds(seed, n_reps), thr)
    assert got.shape == (len(variants), n_reps, len(targets), 3)
    want = PR.restate(bam_path, fa, variants, targets, seed, n_reps, P.mismatchThr)
    compared = 0
    for i in range(len(variants)):
        for j in range(n_reps):
            for t in range(len(targets)):
                st = want[j][t][1][i]
                assert got[i, j, t].tolist() == [st["S"], st["READS"], st["V1"]], (i, j, t)
                compared += 1
    # thresholds 0 and 2^32
    ends = devplanes.spike_rep_counts(eng, [v.pos for v in variants], covers, cnts, PR.seeds(seed, 2), [0, 1 << 32])
    for i, (names, c) in enumerate(counters):
        c = c.astype(np.int64)
        v0 = int((2 * c[:, 1] > c[:, 0]).sum())
        assert v0 == want[0][0][1][i]["V0"]
        for j in range(2):
            assert ends[i, j, 0].tolist() == [0, 0, v0]
            assert ends[i, j, 1].tolist() == [len(names), int(c[:, 2].sum()), int((2 * c[:, 2] > c[:, 0]).sum())]
    return compared, got


@pytest.mark.parametrize("name", INPUTS)
def test_counts_equal_the_restatement(engine0, tmp_path, name):
    bam_path, fa, loci, P, given = TS._inputs(name, str(tmp_path))
    total = 0
    for chrom, lo, hi in ds_restate.stretches(loci):
        vs = _variants(name, bam_path, fa, [(chrom, p) for p in range(lo + 1, hi + 1)], given)
        if vs:
            compared, got = _check_counts(engine0, bam_path, fa, vs, P)
            assert compared == len(vs) * REPS * len(TARGETS)
            total += compared
            assert len({got[:, j].tobytes() for j in range(REPS)}) >= 2                 # (the replicates draw different barcodes)
    assert total > 0


def test_counts_of_a_locus_wider_than_a_workgroup(engine0, tmp_path):
    cfg = dataclasses.replace(R.SYNTH_CFG, n_umi=300, rpb=2)
    bam, fa, loci, P, A = R.synth_bam(str(tmp_path), cfg, 24)
    vs = SR.pick_positions(bam, fa, loci[8:12], 2)
    n = [len(names) for names, _ in PR.host_counters(bam, fa, vs)]
    assert max(n) > 256 and any(x % 64 for x in n)
    compared, _ = _check_counts(engine0, bam, fa, vs, P)
    assert compared == len(vs) * REPS * len(TARGETS)


def test_device_draw_equals_the_restatements(engine0):
    """One covering barcode of one read per `variant`: S at the thresholds u and u + 1 is 0 and 1 exactly when the device drew u."""
    texts = ["ACGTACGTACGT", "TTTTGGGGCCCC", "A", "GATTACAGATTACA", "CCCCCCCCCCCCCCCC", "ACGTTGCAAC", "TGCATGCATGCA", "GGGTTTAAACCC"]
    ids = PR.idents(texts)
    pos = [1, 101, 4096, (1 << 31) - 1, 55555555, 7, 123456789, 1 << 20]
    one = np.array([[1, 0, 1]], np.uint32)
    for seed in (SEED, (1 << 32) + 5, PR.M64):
        u = [int(SR.draw([x], seed, p)[0]) for x, p in zip(texts, pos)]
        assert len(set(u)) == len(u)
        thr = sorted({x + d for x in u for d in (0, 1)})
        assert len(thr) <= 32
        got = devplanes.spike_rep_counts(engine0, pos, [ids[k:k + 1] for k in range(len(ids))], [one] * len(ids), [seed], thr)
        for k, x in enumerate(u):
            assert got[k, 0, :, 0].tolist() == [int(x < h) for h in thr], (seed, texts[k])
            assert got[k, 0, :, 2].tolist() == got[k, 0, :, 0].tolist() == got[k, 0, :, 1].tolist()


def test_refusals_launch_nothing(engine0):
    eng = engine0
    ok = np.zeros(2, abi.SPIKE_VARIANT_DTYPE)
    ok["pos0"], ok["ref"], ok["alt"], ok["thr"] = [5, 9], ord("A"), ord("G"), 1 << 31
    size = 8192
    bufs = [DevBuf(eng, size).upload(np.full(size, 0x5A, np.uint8)) for _ in range(3)]       # aln_out, bq_out, stats
    src = DevBuf(eng, size).upload(np.zeros(size, np.uint8))
    seeds = np.arange(70, dtype=np.uint64)
    half = np.full(70, 1 << 31, np.uint64)

    def rewrite(var=ok, n_copies=2, thr=half, sa=36 * 8, sb=128, n_var=None):
        d_var = DevBuf(eng, var.nbytes + 256).upload(np.ascontiguousarray(var).view(np.uint8).reshape(-1))
        rc = eng.L.smc_spike_alleles_reps(eng.ctx, src.data_ptr(), 8, src.data_ptr(), src.data_ptr(), 64, d_var.data_ptr(), var.ctypes.data,
                                          len(var) if n_var is None else n_var, src.data_ptr(), 4, seeds.ctypes.data, thr.ctypes.data, n_copies, 6.0,
                                          src.data_ptr(), src.data_ptr(), bufs[0].data_ptr(), sa, bufs[1].data_ptr(), sb, bufs[2].data_ptr(), None)
        d_var.free()
        return rc

    def edit(**kw):
        v = ok.copy()
        for k, (i, x) in kw.items():
            v[k][i] = x
        return v
    above = half.copy()
    above[1] = (1 << 32) + 1
    cases = [(dict(var=edit(pos0=(1, 5))), "not strictly ascending"), (dict(var=edit(ref=(0, ord("N")))), "outside ACGT"),
             (dict(var=edit(alt=(0, ord("A")))), "ref equals alt"), (dict(var=np.zeros(4097, abi.SPIKE_VARIANT_DTYPE)), "at most 4096"),
             (dict(n_copies=0), "0 copies"), (dict(n_copies=65), "65 copies"), (dict(thr=above), "above 2^32"),
             (dict(sa=36 * 8 - 4), "smaller than a copy"), (dict(sb=112), "smaller than a copy")]
    for kw, msg in cases:
        assert rewrite(**kw) == -4 and msg.encode() in eng.L.smc_last_error(), msg            # SMC_E_INPUT
    # (the variants' own thresholds are not read: one above 2^32 is no refusal - but this call would launch, so it is not made here)
    off = np.array([0, 3, 5], np.uint32)

    def counts(off=off, n_var=2, n_reps=2, thr=half, n_targets=2):
        return eng.L.smc_spike_rep_counts(eng.ctx, src.data_ptr(), src.data_ptr(), src.data_ptr(), off.ctypes.data, src.data_ptr(), n_var,
                                          src.data_ptr(), n_reps, thr.ctypes.data, n_targets, bufs[2].data_ptr(), None)
    for kw, msg in ((dict(n_targets=33), "33 targets, at most 32"), (dict(n_reps=1001), "1001 replicates, at most 1000"), (dict(thr=above), "above 2^32"),
                    (dict(off=np.array([0, 3, 2], np.uint32)), "offsets decrease"), (dict(n_var=4097), "at most 4096")):
        # (an output of 2^32 - 256 words: the entries check it, and their own maxima - 64 copies or 1000 x 32 cells of 4096 variants -
        # stay below it)
        assert counts(**kw) == -4 and msg.encode() in eng.L.smc_last_error(), msg
    eng.L.smc_device_sync(eng.ctx)
    for b in bufs:
        assert (b.download(np.uint8, size) == 0x5A).all()                                     # nothing copied, nothing launched
    for b in bufs + [src]:
        b.free()


def test_replicate_stage_builds_again_with_32_bit_words(engine0, tmp_path):
    """The hand-made BAM with one base quality of 70 under the first listed position: the 16-bit builder has no room for it, so the
    stage's first call answers NARROW, the engine goes over to 32-bit words and the call is made again - one rewrite more than a
    stage that starts at 32 bits, and the same rows."""
    from smcounter_amd import fasta
    from smcounter_amd.tools import ds_allele_fraction as af
    bam, fa, loci, P, variants = SR.make_case(str(tmp_path))
    variants = [af.Variant(v.chrom, v.pos, v.ref, v.alt, v.alt, af.SNV) for v in variants]
    recs = [dict(tid=0, pos=pos, qname=qname, flag=flag, mapq=60, cigar=list(cigar), seq=seq, qual=list(qual), nm=nm if has_nm else None)
            for qname, flag, pos, cigar, seq, qual, nm, has_nm in SR.file_records(bam)]
    first = next(r for r in recs if r["qname"].startswith("mfirst"))          # (P1 is its first aligned base)
    assert first["pos"] == SR.P1 - 1 and first["cigar"][0] == (SR.M, 30) and max(first["qual"]) <= 63
    first["qual"][0] = 70
    bam = str(tmp_path / "q70.bam")
    bamio.write_bam(bam, [(SR.CASE_CHROM, 400)], recs, block=8000)
    bamio.write_bai(bam)
    assert 0 <= P.minBQ <= 63

    def stage(bits):
        keep = {}
        devplanes.spike_rules(bam, fasta.FastaFile(fa), variants, [0.5], [P], SEED, engine0, keep=keep)
        engine0.word_bits = bits
        out = devplanes.spike_replicates(bam, fasta.FastaFile(fa), variants, [0.5], [P], SEED, 2, engine0, keep)
        return out, engine0.word_bits
    old = engine0.word_bits
    try:
        narrow, bits_after = stage(16)
        wide, _ = stage(32)
    finally:
        engine0.word_bits = old
    assert bits_after == 32
    assert len(narrow["rows"]) == len(variants) * 2 and narrow["rows"] == wide["rows"]
    assert narrow["times"]["rewrites"] == wide["times"]["rewrites"] + 1 == 2
    assert narrow["times"]["builds"] == wide["times"]["builds"] and narrow["times"]["batches"] == wide["times"]["batches"]


def _lines(path):
    return [l.split("\t") for l in open(path).read().splitlines()]


def _cli_contract(tmp_path, bam, fa, loci, P, variants, targets, n_reps, lod):
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = R.write_variants(str(tmp_path / "v.vcf"), variants, vcf=True)
    flags = ["--lod"] if lod else []
    kw = dict(spikeAF=",".join("%g" % t for t in targets), spikeVariants=vfile, dsSeed=SEED)
    before = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, **kw)
    names = sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("o."))
    old = {f: open(str(tmp_path / f), "rb").read() for f in names}
    assert len(names) >= 3 * (1 + len(targets)) + 1 and "o.spikeAF.detection.txt" in names
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, spikeReps=n_reps, **kw)
    assert got == before
    now = sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("o."))
    assert sorted(set(now) - set(names)) == ["o.spikeAF.curve.txt", "o.spikeAF.replicates.txt", "o.spikeAF.sensitivity.txt"]
    for f in names:
        assert open(str(tmp_path / f), "rb").read() == old[f], "%s changed with --spikeReps" % f
    reps = _lines(got + ".spikeAF.replicates.txt")
    assert reps[0] == list(spike.REPLICATES_HEADER) and len(reps) == 1 + len(variants) * len(targets) * n_reps
    T = len(targets)
    compared = 0
    for j, s in enumerate(PR.seeds(SEED, n_reps)):
        ref = TL._run_cli(tmp_path, "s%d" % j, bam, fa, bed, P, **dict(kw, dsSeed=s))
        det = _lines(ref + ".spikeAF.detection.txt")
        assert det[0] == list(spike.DETECTION_HEADER) and len(det) == 1 + len(variants) * (1 + T)
        for i in range(len(variants)):
            for t in range(T):
                mine = reps[1 + (i * T + t) * n_reps + j]
                assert mine[5:7] == ["%d" % j, "%d" % s]
                assert mine[:5] + mine[7:] == det[1 + i * (1 + T) + 1 + t], (i, t, j)
                compared += 1
    assert compared == len(variants) * T * n_reps
    sens, curve = _lines(got + ".spikeAF.sensitivity.txt"), _lines(got + ".spikeAF.curve.txt")
    assert sens[0] == list(spike.SENSITIVITY_HEADER) + (["LOD"] if lod else [])
    assert curve[0] == list(spike.curve_header(targets, lod))
    want = PR.sensitivity_from(reps[1:], variants, targets, n_reps, dsaf.frac_text)
    assert len(sens) == 1 + len(variants) * T == 1 + len(want) and [l[:19] for l in sens[1:]] == want
    want = PR.curve_from(reps[1:], variants, targets, n_reps, dsaf.frac_text)
    assert len(curve) == 1 + len(variants) and [l[:len(want[0])] for l in curve[1:]] == want
    if lod:
        det = _lines(got + ".spikeAF.detection.txt")
        top = max(range(T), key=lambda t: targets[t])
        n_lod = 0
        for i in range(len(variants)):
            for t in range(T):
                assert sens[1 + i * T + t][19] == det[1 + i * (1 + T) + 1 + t][17]
                n_lod += 1
            assert curve[1 + i][-1] == det[1 + i * (1 + T) + 1 + top][17]
        assert n_lod == len(variants) * T
    return reps, sens


def test_cli_replicates_equal_separate_runs_on_the_synthetic_bam(tmp_path):
    bam, fa, loci, P = TS._synth(str(tmp_path))
    variants = SR.pick_positions(bam, fa, loci[16:32], 3)
    _cli_contract(tmp_path, bam, fa, loci, P, variants, (0.2, 0.05), 4, lod=False)


def test_cli_replicates_equal_separate_runs_on_bam_cigars_with_lod(tmp_path):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    _cli_contract(tmp_path, bam, fa, loci, P, SR.pick_positions(bam, fa, loci, 3), (0.3, 0.1), 4, lod=True)


# (probed once over 0.01, 0.015, 0.02, 0.025, 0.03, 0.04, 0.05, 0.06, 0.08 with R = 16: called 1, 3, 6, 10, 12, 15 of 16 up to 0.04, 16 of
# 16 from 0.05; S ran from 1 .. 7 barcodes of 181 at 0.02 and from 2 .. 9 at 0.03)
WORTH_TARGETS = (0.02, 0.03)
WORTH_REPS = 16


def test_replicates_disagree_near_the_callers_limit(tmp_path):
    """What the flag is for: an SNV planted at a deep synthetic locus at a target near the caller's limit is found in some replicates
    and missed in others - one draw (--spikeAF alone) would have answered 0 or 1.  With R = 16, at least one target has
    0 < CALLED < R, and the replicates spike different numbers of barcodes (restated here on the CPU first)."""
    bam, fa, loci, P = TA._deep(tmp_path)
    variants = SR.pick_positions(bam, fa, loci, 1)
    assert len(variants) == 1
    v = variants[0]
    names, _ = PR.host_counters(bam, fa, variants)[0]
    for t in WORTH_TARGETS:
        s = [int((SR.draw(names, sd, v.pos) < np.uint64(PR.threshold(t))).sum()) for sd in PR.seeds(SEED, WORTH_REPS)]
        assert len(set(s)) >= 2, (t, s)                                     # (the binomial spread of S over the seeds)
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = R.write_variants(str(tmp_path / "v.txt"), variants)
    got = TL._run_cli(tmp_path, "w", bam, fa, bed, P, spikeAF=",".join("%g" % t for t in WORTH_TARGETS), spikeVariants=vfile, dsSeed=SEED,
                      spikeReps=WORTH_REPS)
    sens = _lines(got + ".spikeAF.sensitivity.txt")[1:]
    reps = _lines(got + ".spikeAF.replicates.txt")[1:]
    assert len(sens) == len(WORTH_TARGETS) and len(reps) == len(WORTH_TARGETS) * WORTH_REPS
    for l in sens:
        print("target %s: called %s of %s, rate %s [%s, %s], S %s .. %s, V1 %s .. %s" % (l[4], l[6], l[5], l[7], l[8], l[9], l[13], l[14], l[15], l[16]))
    assert any(0 < int(l[6]) < WORTH_REPS for l in sens)
    assert len({l[PR.S] for l in reps}) >= 2
