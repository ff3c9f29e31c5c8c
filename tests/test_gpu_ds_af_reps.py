"""--dsAFReps on the GPU: smc_af_rep_masks / smc_af_rep_counts against the restatement (tests/ds_af_reps_restate.py: titrate() once
per replicate), bit for bit; the device draw against tools.ds_allele_fraction.philox_word0; the command line against separate runs
with --dsSeed s_j; a deep synthetic locus near the caller's limit, where the replicates disagree."""
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, bamio, devplanes, dsaf, fasta, synth
from smcounter_amd.engine import DevBuf
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_reps_restate as RR  # noqa: E402
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line)

pytestmark = pytest.mark.gpu
FIXTURES = ("case", "bam_cigars", "bam_overcap", "bam_deep")
SEED = 7
REPS = 5
TARGETS = (0.02, 0.2, 0.9)              # (0.9 lies above every fraction met: k = 1, a threshold of exactly 2^32)
SUFFIXES = (".smCounter.all.txt", ".smCounter.cut.txt", ".smCounter.cut.vcf")


def _fixture(name, tmp):
    return ds_restate.make_case(tmp) if name == "case" else ds_restate.load_fixture(name, tmp)


def _device(eng, run_idents, covers, carries, targets, seed, n_reps, draws=False):
    """The two calls over one run's identities -> (masks uint32 [R, T, n_words], counts uint32 [V, R, T, 2], the table, draws)."""
    thr = RR.thresholds(covers, carries, targets)
    idents, table = dsaf.carrier_table(carries, thr)
    tab = devplanes.AfRepTable(eng, idents, table, dsaf.rep_seeds(seed, n_reps))
    n = len(run_idents)
    n_words = devplanes.mask_words(n)
    d_id = DevBuf(eng, 8 * max(1, n) + 256).upload(np.ascontiguousarray(run_idents, np.uint64) if n else np.zeros(1, np.uint64))
    d_m = DevBuf(eng, 4 * n_reps * len(targets) * n_words + 256)
    d_m.upload(np.full(n_reps * len(targets) * n_words, 0xA5A5A5A5, np.uint32))          # (every word must be written)
    d_u = DevBuf(eng, 4 * n_reps * max(1, n) + 256) if draws else None
    try:
        tab.masks(d_id.data_ptr(), n, d_m.data_ptr(), n_words, d_u.data_ptr() if draws else None)
        masks = d_m.download(np.uint32, n_reps * len(targets) * n_words).reshape(n_reps, len(targets), n_words)
        u = d_u.download(np.uint32, n_reps * n).reshape(n_reps, n) if draws else None
        counts = tab.counts(covers, carries)
    finally:
        for b in (d_id, d_m, d_u):
            if b is not None:
                b.free()
        tab.free()
    return masks, counts, (idents, table), u


def _check(eng, run_idents, covers, carries, targets=TARGETS, seed=SEED, n_reps=REPS):
    """masks and counts == the restatement, bit for bit -> (mask words compared, counters compared, table, distinct dropped sets)."""
    keep, want, dropped = RR.restate(run_idents, covers, carries, targets, seed, n_reps)
    masks, counts, (idents, table), _ = _device(eng, run_idents, covers, carries, targets, seed, n_reps)
    n_words = devplanes.mask_words(len(run_idents))
    assert masks.shape == (n_reps, len(targets), n_words)
    assert np.array_equal(masks, RR.pack(keep, n_words))
    assert counts.shape == want.shape == (len(covers), n_reps, len(targets), 2) and np.array_equal(counts, want)
    return masks.size, counts.size, (idents, table), len({d[t].tobytes() for d in dropped for t in range(len(targets))})


def _sets(bam_path, fa_path, variants):
    """(covers, carries) identities of the listed variants, by the tool's own file pass."""
    ids = af.unique_idents(bamio.placed_barcodes(bam_path), bam_path)
    vs = [af.Variant(v.chrom, v.pos, v.ref, v.alt, *af.allele_key(v.ref, v.alt)) for v in variants]
    counted = af.count_file(bam_path, vs, fasta.FastaFile(fa_path))
    arr = lambda texts: np.array([ids[t] for t in texts], np.uint64)
    return [arr(c) for c, _ in counted], [arr(sorted(k)) for _, k in counted]


def _check_all_tables(eng, run_idents, covers, carries):
    """The fixture's own table, then a table of one entry and of zero entries over the same run."""
    words, counters, (idents, table), distinct = _check(eng, run_idents, covers, carries)
    assert len(idents) == len(np.unique(np.concatenate(carries)))
    with_carriers = [v for v in range(len(carries)) if len(carries[v])]
    if with_carriers:
        assert bool((table == np.uint64(1 << 32)).any())                       # (the target above every fraction: k = 1)
        v = with_carriers[0]
        one = [np.asarray(c)[:1] if k == v else np.asarray(c)[:0] for k, c in enumerate(carries)]
        _, _, (i1, _), _ = _check(eng, run_idents, covers, one)
        assert len(i1) == 1
    _, _, (i0, t0), _ = _check(eng, run_idents, covers, [np.asarray(c)[:0] for c in carries])
    assert len(i0) == 0 and t0.shape == (0, len(TARGETS))
    return words, counters, len(idents), distinct


@pytest.mark.parametrize("name", FIXTURES)
def test_masks_and_counts_equal_the_restatement_on_the_fixtures(engine0, tmp_path, name):
    bam_path, fa, loci, P = _fixture(name, str(tmp_path))
    bam = bamio.NativeBam(bam_path)
    runs = carriers = 0
    try:
        for chrom, lo, hi in ds_restate.stretches(loci):
            here = [(chrom, p) for p in range(lo + 1, hi + 1)]
            variants = R.pick_variants(bam_path, fa, here)
            covers, carries = _sets(bam_path, fa, variants)
            A = bam.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
            run_idents = bam.barcode_idents(A["n_bc"])
            assert len(run_idents) == int(A["n_bc"])
            words, counters, n_car, _ = _check_all_tables(engine0, run_idents, covers, carries)
            assert words == REPS * len(TARGETS) * devplanes.mask_words(int(A["n_bc"])) and counters == len(variants) * REPS * len(TARGETS) * 2
            runs += 1
            carriers += n_car
    finally:
        bam.close()
    assert runs == len(ds_restate.stretches(loci)) and runs >= 1
    if name != "bam_overcap":
        assert carriers > 0


def _deep(tmp_path, alt_af=0.1):
    """C3's shape as tests/test_gpu_ds_af.py's deep run: 150 barcodes x 20 reads per locus -> (bam, fasta, loci, VcParams)."""
    cfg = dataclasses.replace(synth.CONFIGS["C3"], n_umi=150, rpb=20, alt_locus_frac=0.3, alt_af=alt_af)
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, 260, P)
    bam_path, fa = str(tmp_path / "deep.bam"), str(tmp_path / "deep.fa")
    chrom, p0, p1 = synth.alignments_to_bam(A, bam_path, 120, 126, fa)
    return bam_path, fa, [(chrom, p) for p in range(p0, p1 + 1)], P


def test_masks_and_counts_equal_the_restatement_on_a_deep_synthetic_run(engine0, tmp_path):
    bam_path, fa, here, P = _deep(tmp_path)
    variants = R.planted(bam_path, fa, here, limit=3) + R.pick_variants(bam_path, fa, here)
    seen = set()
    variants = [v for v in variants if not ((v.chrom, v.pos) in seen or seen.add((v.chrom, v.pos)))]      # (one variant per position)
    covers, carries = _sets(bam_path, fa, variants)
    bam = bamio.NativeBam(bam_path)
    try:
        A = bam.alignments_run(here[0][0], here[0][1] - 1, here[-1][1], ds_restate.BIG, P, 2)
        run_idents = bam.barcode_idents(A["n_bc"])
    finally:
        bam.close()
    assert int(A["n_bc"]) > 64 and devplanes.mask_words(int(A["n_bc"])) >= 3                    # (masks span several words)
    words, counters, n_car, distinct = _check_all_tables(engine0, run_idents, covers, carries)
    assert n_car > 1 and distinct > 2                                                           # (the replicates drop different sets)
    assert counters == len(variants) * REPS * len(TARGETS) * 2


def test_device_draw_equals_the_tool_draw(engine0):
    rng = np.random.RandomState(20240607)
    ids = np.unique(rng.randint(0, 1 << 62, 4200).astype(np.uint64) * np.uint64(3) + np.uint64(1))[:4096]
    assert len(ids) == 4096
    run = ids[rng.permutation(len(ids))]
    seeds = [7, (1 << 32) + 5, RR.M64]
    tab = devplanes.AfRepTable(engine0, ids, np.full((len(ids), 1), 1 << 32, np.uint64), np.array(seeds, np.uint64))
    d_id = DevBuf(engine0, 8 * len(run) + 256).upload(run)
    n_words = devplanes.mask_words(len(run))
    d_m, d_u = DevBuf(engine0, 4 * 3 * n_words + 256), DevBuf(engine0, 4 * 3 * len(run) + 256)
    try:
        tab.masks(d_id.data_ptr(), len(run), d_m.data_ptr(), n_words, d_u.data_ptr())
        u = d_u.download(np.uint32, 3 * len(run)).reshape(3, len(run))
        m = d_m.download(np.uint32, 3 * n_words).reshape(3, n_words)
    finally:
        for b in (d_id, d_m, d_u):
            b.free()
        tab.free()
    compared = 0
    for j, s in enumerate(seeds):
        want = af.philox_word0(run, s)
        assert np.array_equal(u[j].astype(np.uint64), want)
        compared += len(want)
    assert compared == 3 * 4096 and len({u[j].tobytes() for j in range(3)}) == 3
    assert np.array_equal(m, RR.pack(np.ones((3, len(run)), bool), n_words))                    # (thr 2^32: nobody goes)


def test_refusals_of_the_two_calls(engine0):
    ids = np.array([5, 9, 9, 12], np.uint64)
    thr = np.full((4, 1), 1 << 31, np.uint64)
    d = DevBuf(engine0, 4096)
    for bad_ids, bad_thr, msg in ((ids, thr, "not strictly ascending"), (ids[[0, 1, 3]], np.full((3, 1), (1 << 32) + 1, np.uint64), r"above 2\^32"),
                                  (ids[[0, 1, 3]], np.full((3, 33), 1, np.uint64), "at most 32")):
        tab = devplanes.AfRepTable(engine0, bad_ids, bad_thr, np.array([1, 2], np.uint64))
        try:
            with pytest.raises(_lib.SmcError, match=msg):
                tab.masks(d.data_ptr(), 4, d.data_ptr(), devplanes.mask_words(4))
            with pytest.raises(_lib.SmcError, match=msg):
                tab.counts([ids[:1]], [ids[:1]])
        finally:
            tab.free()
    tab = devplanes.AfRepTable(engine0, ids[[0, 1, 3]], thr[:3], np.array([1, 2], np.uint64))
    try:
        with pytest.raises(_lib.SmcError, match="words per mask"):
            tab.masks(d.data_ptr(), 100, d.data_ptr(), 2)
        with pytest.raises(_lib.SmcError, match="too many mask words"):
            tab.masks(d.data_ptr(), 64, d.data_ptr(), 1 << 31)
    finally:
        tab.free()
        d.free()


def _lines(path):
    return [l.split("\t") for l in open(path).read().splitlines()]


def _sensitivity_from(rep_lines, variants, targets, n_reps):
    """The sensitivity table's lines (without LOD) computed here from the replicate lines."""
    out = []
    for i, v in enumerate(variants):
        for t, target in enumerate(targets):
            per = rep_lines[(i * len(targets) + t) * n_reps:(i * len(targets) + t + 1) * n_reps]
            called = sum(int(l[16]) for l in per)
            lo, hi = RR.wilson(called, n_reps)
            afs = [int(l[8]) / int(l[7]) if int(l[7]) else 0.0 for l in per]
            vs = [int(l[8]) for l in per]
            pis = [float(l[14]) if l[14] else 0.0 for l in per]
            out.append([v.chrom, "%d" % v.pos, v.ref, v.alt, "%g" % target, "%d" % n_reps, "%d" % called, dsaf.frac_text(called / n_reps),
                        dsaf.frac_text(max(0.0, lo)), dsaf.frac_text(min(1.0, hi)), dsaf.frac_text(sum(afs) / n_reps), dsaf.frac_text(min(afs)),
                        dsaf.frac_text(max(afs)), "%d" % min(vs), "%d" % max(vs), dsaf.frac_text(sum(pis) / n_reps), dsaf.frac_text(min(pis))])
    return out


def _cli_contract(tmp_path, bam, fa, loci, P, variants, targets, n_reps, lod):
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = R.write_variants(str(tmp_path / "v.vcf"), variants, vcf=True)
    flags = ["--lod"] if lod else []
    kw = dict(dsAF=",".join("%g" % t for t in targets), dsAFVariants=vfile, dsSeed=SEED)
    before = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, **kw)
    names = sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("o."))
    old = {f: open(str(tmp_path / f), "rb").read() for f in names}
    assert len(names) >= 3 * (1 + len(targets)) + 1 and "o.dsAF.detection.txt" in names
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, dsAFReps=n_reps, **kw)
    assert got == before
    now = sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("o."))
    assert sorted(set(now) - set(names)) == ["o.dsAF.replicates.txt", "o.dsAF.sensitivity.txt"]
    same = 0
    for f in names:
        assert open(str(tmp_path / f), "rb").read() == old[f], "%s changed with --dsAFReps" % f
        same += 1
    assert same == len(names)
    reps = _lines(got + ".dsAF.replicates.txt")
    assert reps[0] == list(dsaf.REPLICATES_HEADER)
    assert len(reps) == 1 + len(variants) * len(targets) * n_reps
    compared = 0
    for j, s in enumerate(RR.seeds(SEED, n_reps)):
        ref = TL._run_cli(tmp_path, "s%d" % j, bam, fa, bed, P, **dict(kw, dsSeed=s))
        det = _lines(ref + ".dsAF.detection.txt")
        assert det[0] == list(dsaf.DETECTION_HEADER) and len(det) == 1 + len(variants) * (1 + len(targets))
        for i in range(len(variants)):
            for t in range(len(targets)):
                mine = reps[1 + (i * len(targets) + t) * n_reps + j]
                assert mine[5:7] == ["%d" % j, "%d" % s]
                assert mine[:5] + mine[7:] == det[1 + i * (1 + len(targets)) + 1 + t], (i, t, j)
                compared += 1
    assert compared == len(variants) * len(targets) * n_reps
    sens = _lines(got + ".dsAF.sensitivity.txt")
    assert sens[0] == list(dsaf.SENSITIVITY_HEADER) + (["LOD"] if lod else [])
    want = _sensitivity_from(reps[1:], variants, targets, n_reps)
    assert len(sens) == 1 + len(variants) * len(targets) == 1 + len(want)
    assert [l[:17] for l in sens[1:]] == want
    if lod:
        det = _lines(got + ".dsAF.detection.txt")
        n_lod = 0
        for i in range(len(variants)):
            for t in range(len(targets)):
                assert sens[1 + i * len(targets) + t][17] == det[1 + i * (1 + len(targets)) + 1 + t][15]
                n_lod += 1
        assert n_lod == len(variants) * len(targets)
    return reps, sens


def test_cli_replicates_equal_separate_runs_on_the_case_fixture(tmp_path):
    bam, fa, loci, P = ds_restate.make_case(str(tmp_path))
    variants = R.pick_variants(bam, fa, loci)
    assert variants
    _cli_contract(tmp_path, bam, fa, loci, P, variants, (0.05, 0.2), 4, lod=False)


def test_cli_replicates_equal_separate_runs_on_bam_cigars_with_lod(tmp_path):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    variants = R.pick_variants(bam, fa, loci)
    assert {"SNV", "INS", "DEL"} <= {"SNV" if len(v.key) == 1 else v.key[:3] for v in variants}
    _cli_contract(tmp_path, bam, fa, loci, P, variants, (0.05, 0.2), 4, lod=True)


WORTH_TARGETS = (0.02, 0.03)        # (probed once at 0.01 .. 0.08 with R = 16: called 1, 2, 6, 7, 11, 11, 13 of 16 up to 0.04, 16 of 16 from 0.05)
WORTH_REPS = 16


def test_replicates_disagree_near_the_callers_limit(tmp_path):
    """What the flag is for: a planted variant of a deep synthetic locus diluted to a target near the caller's limit is found in some
    replicates and missed in others - one draw (--dsAF alone) would have answered 0 or 1.  The inputs are fixed so that, with R = 16,
    at least one (variant, target) has 0 < CALLED < R and at least two replicates drop different barcodes (restated here on the CPU)."""
    bam, fa, loci, P = _deep(tmp_path)
    variants = R.planted(bam, fa, loci, min_frac=0.03, limit=1)         # (12 of the locus's 178 barcodes carry it)
    assert len(variants) == 1
    covers, carries = _sets(bam, fa, variants)
    _, _, dropped = RR.restate(np.zeros(0, np.uint64), covers, carries, WORTH_TARGETS, SEED, WORTH_REPS)
    assert len({d[0].tobytes() for d in dropped}) >= 2
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = R.write_variants(str(tmp_path / "v.txt"), variants)
    got = TL._run_cli(tmp_path, "w", bam, fa, bed, P, dsAF=",".join("%g" % t for t in WORTH_TARGETS), dsAFVariants=vfile, dsSeed=SEED,
                      dsAFReps=WORTH_REPS)
    sens = _lines(got + ".dsAF.sensitivity.txt")[1:]
    reps = _lines(got + ".dsAF.replicates.txt")[1:]
    assert len(sens) == len(WORTH_TARGETS) and len(reps) == len(WORTH_TARGETS) * WORTH_REPS
    for l in sens:
        print("target %s: called %s of %s, rate %s [%s, %s], V' %s .. %s" % (l[4], l[6], l[5], l[7], l[8], l[9], l[13], l[14]))
    assert any(0 < int(l[6]) < WORTH_REPS for l in sens)
    assert len({(l[7], l[8]) for l in reps}) >= 2                                   # (the achieved counts differ between replicates)
