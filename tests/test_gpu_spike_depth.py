"""--spikeDepth on the GPU: smc_spike_depth_counts against the restatement (tests/spike_depth_restate.py) word for word, its edge
cases and refusals; the command line's cells against the two-step workflow (tools.spike_variants, then --dsMT --dsSampler philox),
its pages against the restatement, separate runs with --dsSeed s_j and what the test computes from the replicate lines."""
import argparse
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import bamio, devplanes, dsaf, spike
from smcounter_amd.engine import DevBuf
from smcounter_amd.py2compat import py2_round
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import spike_depth_restate as DS  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line)
import test_gpu_spike as TS  # noqa: E402  (its inputs)

pytestmark = pytest.mark.gpu
SEED = 20240607
REPS, TARGETS, FRACS = 3, (0.05, 0.3, 0.7), (0.2, 0.6, 1.0)
ONE = 1 << 32
SUFFIXES = TL.SUFFIXES


def _device(eng, counters, positions, seeds, thr, dthr):
    return devplanes.spike_depth_counts(eng, positions, [PR.idents(names) for names, _ in counters], [c for _, c in counters], seeds, thr, dthr)


def _check_counts(eng, bam_path, fa, variants):
    """The entry over the host-built counters == the restatement for every (v, j, t, f); two calls agree; thresholds 0 and 2^32 on both
    axes; R = 1; one fraction of 2^32 gives smc_spike_rep_counts' numbers -> words compared."""
    want, counters = DS.restate_counts(bam_path, fa, variants, TARGETS, FRACS, SEED, REPS)
    pos, seeds = [v.pos for v in variants], PR.seeds(SEED, REPS)
    thr, dthr = [PR.threshold(t) for t in TARGETS], [DS.frac_thr(f) for f in FRACS]
    assert dthr[-1] == ONE
    got = _device(eng, counters, pos, seeds, thr, dthr)
    assert got.shape == want.shape == (len(variants), REPS, len(TARGETS), len(FRACS), 5) and got.dtype == np.uint32
    assert np.array_equal(got, want), np.argwhere(got != want)[:5]
    assert np.array_equal(_device(eng, counters, pos, seeds, thr, dthr), got)
    ends = _device(eng, counters, pos, seeds[:1], [0, ONE], [0, ONE])                      # (R = 1)
    assert np.array_equal(ends, DS.counts_from(counters, pos, [0, ONE], [0, ONE], seeds[:1]))
    assert not ends[:, :, :, 0].any()
    for i, (names, c) in enumerate(counters):
        c = c.astype(np.int64)
        v0 = int((2 * c[:, 1] > c[:, 0]).sum())
        assert ends[i, 0, 0, 1].tolist() == [len(names), v0, 0, 0, v0]
        assert ends[i, 0, 1, 1].tolist() == [len(names), v0, len(names), int(c[:, 2].sum()), int((2 * c[:, 2] > c[:, 0]).sum())]
    plain = devplanes.spike_rep_counts(eng, pos, [PR.idents(names) for names, _ in counters], [c for _, c in counters], seeds, thr)
    assert np.array_equal(_device(eng, counters, pos, seeds, thr, [ONE])[:, :, :, 0, 2:], plain)
    assert np.array_equal(got[:, :, :, -1, 2:], plain)
    return got


@pytest.mark.parametrize("name", ("case", "bam_cigars"))
def test_counts_equal_the_restatement(engine0, tmp_path, name):
    bam_path, fa, loci, P, given = TS._inputs(name, str(tmp_path))
    total = 0
    for chrom, lo, hi in ds_restate.stretches(loci):
        vs = given or SR.pick_positions(bam_path, fa, [(chrom, p) for p in range(lo + 1, hi + 1)], 3)
        if vs:
            got = _check_counts(engine0, bam_path, fa, vs)
            total += got.size
            assert len({got[:, j].tobytes() for j in range(REPS)}) >= 2                   # (the replicates draw different barcodes)
            assert got[:, :, :, 0, 0].max() < got[:, :, :, 2, 0].max()                    # (the fractions keep different numbers)
    assert total > 0


def test_counts_of_a_locus_wider_than_a_workgroup(engine0, tmp_path):
    cfg = dataclasses.replace(R.SYNTH_CFG, n_umi=300, rpb=2)
    bam, fa, loci, P, A = R.synth_bam(str(tmp_path), cfg, 24)
    vs = SR.pick_positions(bam, fa, loci[8:12], 2)
    n = [len(names) for names, _ in PR.host_counters(bam, fa, vs)]
    assert max(n) > 256 and any(x % 64 for x in n) and any(x % 256 for x in n)
    _check_counts(engine0, bam, fa, vs)


def _made_counters(sizes, seed=5):
    """Counters without a BAM: per variant `sizes[v]` barcode texts and random (reads, alt0, single) with alt0, single <= reads."""
    rng = np.random.RandomState(seed)
    out = []
    for v, n in enumerate(sizes):
        reads = rng.randint(1, 6, n)
        single = np.minimum(reads, rng.randint(0, 6, n))
        alt0 = np.minimum(single, rng.randint(0, 3, n))
        out.append((["V%dB%dACGT" % (v, b) for b in range(n)], np.stack([reads, alt0, single], axis=1).astype(np.uint32)))
    return out


def test_a_variant_nobody_covers_between_two_that_are_covered(engine0):
    counters = _made_counters([70, 0, 130])                                              # (offsets 0, 70, 70, 200: not aligned to a wavefront)
    pos, seeds = [11, 5000, 1 << 20], PR.seeds(SEED, 2)
    thr, dthr = [PR.threshold(t) for t in (0.1, 0.5)], [DS.frac_thr(f) for f in (0.3, 0.8)]
    got = _device(engine0, counters, pos, seeds, thr, dthr)
    assert np.array_equal(got, DS.counts_from(counters, pos, thr, dthr, seeds))
    assert not got[1].any() and got[0].any() and got[2].any()
    assert int(got[0, :, :, :, 0].max()) <= 70 and int(got[2, :, :, :, 0].max()) <= 130


def test_thirty_two_cells_and_more_replicates_than_the_grid_is_deep(engine0):
    counters = _made_counters([300, 65])
    pos = [101, 202]
    thr = [PR.threshold(t) for t in (0.01, 0.05, 0.1, 0.2, 0.4, 0.6, 0.8, 1.0)]
    dthr = [DS.frac_thr(f) for f in (0.1, 0.25, 0.5, 1.0)]
    seeds = PR.seeds(PR.M64 - 3, 70)                                                    # (70 replicates > the 64 the entry launches; the seeds wrap)
    got = _device(engine0, counters, pos, seeds, thr, dthr)
    assert got.shape == (2, 70, 8, 4, 5)
    assert np.array_equal(got, DS.counts_from(counters, pos, thr, dthr, seeds))
    assert len({got[:, j].tobytes() for j in range(70)}) > 60


def test_refusals_launch_nothing(engine0):
    eng = engine0
    size = 8192
    out = DevBuf(eng, size).upload(np.full(size, 0x5A, np.uint8))
    src = DevBuf(eng, size).upload(np.zeros(size, np.uint8))
    half, above = np.full(40, 1 << 31, np.uint64), np.full(40, 1 << 31, np.uint64)
    above[1] = ONE + 1
    off = np.array([0, 3, 5], np.uint32)

    def counts(off=off, n_var=2, n_reps=2, thr=half, n_targets=2, dthr=half, n_fracs=2):
        return eng.L.smc_spike_depth_counts(eng.ctx, src.data_ptr(), src.data_ptr(), src.data_ptr(), off.ctypes.data, src.data_ptr(), n_var,
                                            src.data_ptr(), n_reps, thr.ctypes.data, n_targets, dthr.ctypes.data, n_fracs, out.data_ptr(), None)
    for kw, msg in ((dict(n_targets=33, n_fracs=1), "33 targets, at most 32"), (dict(n_reps=1001), "1001 replicates, at most 1000"),
                    (dict(thr=above), "target 1: a threshold above 2^32"), (dict(off=np.array([0, 3, 2], np.uint32)), "offsets decrease"),
                    (dict(n_var=4097), "at most 4096"), (dict(dthr=above), "depth threshold 1 is above 2^32"), (dict(n_fracs=0), "0 fractions"),
                    (dict(n_fracs=-1), "-1 fractions"), (dict(n_targets=3, n_fracs=11), "3 targets x 11 fractions, at most 32 cells"),
                    (dict(n_targets=32, n_fracs=2), "at most 32 cells")):
        # (an output of 2^32 - 256 words: the entry checks it, and its own maxima - 4096 variants x 1000 replicates x 32 cells x 5 - stay
        # below it)
        assert counts(**kw) == -4 and msg.encode() in eng.L.smc_last_error(), msg            # SMC_E_INPUT
    eng.L.smc_device_sync(eng.ctx)
    assert (out.download(np.uint8, size) == 0x5A).all()                                       # nothing zeroed, nothing launched
    out.free(); src.free()


def _lines(path):
    return [l.split("\t") for l in open(path).read().splitlines()]


def _files(tmp_path, tag):
    return sorted(f for f in os.listdir(str(tmp_path)) if f.startswith(tag + "."))


def _cli_contract(tmp_path, bam, fa, loci, P, variants, targets, fracs, n_reps, lod):
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = R.write_variants(str(tmp_path / "v.vcf"), variants, vcf=True)
    flags = ["--lod"] if lod else []
    T, F, V = len(targets), len(fracs), len(variants)
    kw = dict(spikeAF=",".join("%g" % t for t in targets), spikeVariants=vfile, dsSeed=SEED)
    depth = ",".join("%g" % f for f in fracs)
    cells = [(t, f, max(1, int(py2_round(f * P.mtDepth))), ".spikeAF%g.dsMT%g" % (t, f)) for t in targets for f in fracs]
    # 1. every file of a run without the flag is unchanged (the LOD summary keeps its lines and gets one per cell)
    TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, spikeReps=n_reps, **kw)
    names = _files(tmp_path, "o")
    old = {f: open(str(tmp_path / f), "rb").read() for f in names}
    assert {"o.spikeAF.detection.txt", "o.spikeAF.replicates.txt", "o.spikeAF.sensitivity.txt", "o.spikeAF.curve.txt"} <= set(names)
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, spikeReps=n_reps, spikeDepth=depth, **kw)
    added = sorted(set(_files(tmp_path, "o")) - set(names))
    assert added == sorted(["o" + c[3] + s for c in cells for s in SUFFIXES + (TL.LOD_SUFFIXES if lod else ())] +
                           ["o.spikeAF.depth.%s.txt" % x for x in ("detection", "replicates", "sensitivity", "curve")])
    for f in names:
        now = open(str(tmp_path / f), "rb").read()
        if f == "o.lod.summary.txt":
            assert now.startswith(old[f]) and len(now.splitlines()) == len(old[f].splitlines()) + len(cells)
            assert [l.split(b"\t")[:2] for l in now.splitlines()[-len(cells):]] == [[os.path.basename(got + c[3]).encode(), b"%d" % c[2]] for c in cells]
        else:
            assert now == old[f], "%s changed with --spikeDepth" % f
    mine = {c[3]: TL._read(got + c[3], SUFFIXES) for c in cells}
    if lod:
        for c in cells:
            assert TL._read(got + c[3], TL.LOD_SUFFIXES) == TL._tool_files(tmp_path, got + c[3] + SUFFIXES[0], "UMT", c[2]), c
    # 2. the detection page: the cells' counts are the restatement's, its lines the cells' own files
    det = _lines(got + ".spikeAF.depth.detection.txt")
    assert det[0] == list(spike.DEPTH_DETECTION_HEADER) + (["LOD"] if lod else []) and len(det) == 1 + V * T * F
    counts, _ = DS.restate_counts(bam, fa, variants, targets, fracs, SEED, n_reps)
    for i, v in enumerate(variants):
        for c, (t, f, d, suffix) in enumerate(cells):
            l = det[1 + i * T * F + c]
            assert l[:7] == [v.chrom, "%d" % v.pos, v.ref, v.alt, "%g" % t, "%g" % f, "%d" % d]
            assert l[7:12] == ["%d" % x for x in counts[i, 0, c // F, c % F]], (i, c)
            rows, cut = dsaf.read_output(got + suffix)
            r = dict(zip(DS.NAMES, (int(x) for x in l[7:12])))
            assert l[:5] + l[7:] == spike.detection_line(v, t, r, rows.get((v.chrom, "%d" % v.pos)), cut.get((v.chrom, "%d" % v.pos)),
                                                         float(l[19]) if lod else None).split("\t")
    # 3. every replicate line is the detection line of a separate run with --dsSeed s_j
    reps = _lines(got + ".spikeAF.depth.replicates.txt")
    assert reps[0] == list(spike.DEPTH_REPLICATES_HEADER) and len(reps) == 1 + V * T * F * n_reps
    compared = 0
    for j, s in enumerate(PR.seeds(SEED, n_reps)):
        ref = TL._run_cli(tmp_path, "s%d" % j, bam, fa, bed, P, spikeDepth=depth, **dict(kw, dsSeed=s))
        one = _lines(ref + ".spikeAF.depth.detection.txt")
        assert one[0] == list(spike.DEPTH_DETECTION_HEADER) and len(one) == 1 + V * T * F
        for i in range(V):
            for c in range(T * F):
                line = reps[1 + (i * T * F + c) * n_reps + j]
                assert line[7:9] == ["%d" % j, "%d" % s]
                assert line[:7] + line[9:] == one[1 + i * T * F + c], (i, c, j)
                assert line[9:14] == ["%d" % x for x in counts[i, j, c // F, c % F]]
                compared += 1
        if j == 0:
            assert [l[:19] for l in det[1:]] == one[1:]
    assert compared == V * T * F * n_reps
    # 4. the sensitivity table and the curve are what the replicate lines say
    sens = _lines(got + ".spikeAF.depth.sensitivity.txt")
    assert sens[0] == list(spike.DEPTH_SENSITIVITY_HEADER) + (["LOD"] if lod else [])
    want = DS.sensitivity_from(reps[1:], variants, [(c[0], c[1]) for c in cells], n_reps, dsaf.frac_text)
    assert len(sens) == 1 + V * T * F == 1 + len(want) and [l[:22] for l in sens[1:]] == want
    curve = _lines(got + ".spikeAF.depth.curve.txt")
    assert curve[0] == list(spike.depth_curve_header(targets, lod)) and len(curve) == 1 + V * (1 + F)
    plain = _lines(got + ".spikeAF.replicates.txt")[1:]
    want = DS.curve_from(plain, [P.mtDepth] * T, reps[1:], variants, targets, fracs, n_reps, dsaf.frac_text)
    assert [l[:8 + T] for l in curve[1:]] == want
    if lod:
        top = max(range(T), key=lambda t: targets[t])
        full_det = _lines(got + ".spikeAF.detection.txt")
        for i in range(V):
            for c in range(T * F):
                assert sens[1 + i * T * F + c][22] == det[1 + i * T * F + c][19]
            assert curve[1 + i * (1 + F)][8 + T] == full_det[1 + i * (1 + T) + 1 + top][17]
            for k in range(F):
                assert curve[1 + i * (1 + F) + 1 + k][8 + T] == det[1 + i * T * F + top * F + k][19]
    # 5. the specification: a cell is the .dsMT<f> output of --dsMT f --dsSampler philox on the BAM the tool writes for t.  The workflow
    # writes under a prefix of its own; the .cut.vcf names its prefix in the sample column, so that one word is mapped before comparing
    checked = 0
    for t in targets:
        out = str(tmp_path / ("sp%g.bam" % t))
        sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=SEED, refGenome=fa))
        if not os.path.exists(out + ".bai"):
            bamio.write_bai(out)
        ref = TL._run_cli(tmp_path, "w.spikeAF%g" % t, out, fa, bed, P, dsMT=depth, dsSampler="philox", dsSeed=SEED)
        for f in fracs:
            suffix = ".spikeAF%g.dsMT%g" % (t, f)
            theirs = [x.replace((ref + ".dsMT%g" % f).encode(), (got + suffix).encode()) for x in TL._read(ref + ".dsMT%g" % f, SUFFIXES)]
            assert TL._read(got + suffix, SUFFIXES) == mine[suffix]                          # (nothing wrote over the cell's files)
            for a, b, s in zip(mine[suffix], theirs, SUFFIXES):
                assert a == b, "cell %s: %s differs from the two-step workflow's" % (suffix, s)
            checked += 1
    assert checked == T * F


def test_cli_cells_equal_the_two_step_workflow_on_the_synthetic_bam(tmp_path):
    bam, fa, loci, P = TS._synth(str(tmp_path))
    variants = SR.pick_positions(bam, fa, loci[16:32], 3)
    _cli_contract(tmp_path, bam, fa, loci, P, variants, (0.2, 0.05), (0.5, 0.25), 4, lod=False)


def test_cli_cells_equal_the_two_step_workflow_on_bam_cigars_with_lod(tmp_path):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    _cli_contract(tmp_path, bam, fa, loci, P, SR.pick_positions(bam, fa, loci, 3), (0.3, 0.1), (0.5, 1.0), 4, lod=True)
