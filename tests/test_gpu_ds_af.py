"""--dsAF on the GPU: smc_allele_carriers against the restatement from host-built pileups (tests/ds_af_restate.py), bit for bit; the
command line against the offline workflow - tools.ds_allele_fraction, then a plain run on the BAM it wrote; the detection file."""
import argparse
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import bamio, devplanes, dsaf, fasta, synth
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line, the LOD tool's files)

pytestmark = pytest.mark.gpu
FIXTURES = ("case", "bam_cigars", "bam_overcap", "bam_deep")
SEED = 7
SUFFIXES = (".smCounter.all.txt", ".smCounter.cut.txt", ".smCounter.cut.vcf")


def _fixture(name, tmp):
    return ds_restate.make_case(tmp) if name == "case" else ds_restate.load_fixture(name, tmp)


def _tool_variant(v):
    key, kind = af.allele_key(v.ref, v.alt)
    assert key == v.key
    return af.Variant(v.chrom, v.pos, v.ref, v.alt, key, kind)


def _check_run(eng, A, lo, chrom, variants, bam_path, fa_path, gid_of):
    """The kernel over run `A` for `variants` (the restatement's V, any number per locus) == the counts of the host-built pileups."""
    pb = R.pileups(bam_path, fa_path, [(v.chrom, v.pos) for v in variants])
    n_bc = int(A["n_bc"])
    want = np.zeros((len(variants), n_bc, 2), np.uint32)
    for l, v in enumerate(variants):
        names, reads, alt = R.counts(pb, l, v.key)
        g = np.array([gid_of(n) for n in names], np.int64)
        want[l, g, 0], want[l, g, 1] = reads, alt
        assert int(reads.sum()) == int(A["loc"]["n"][v.pos - 1 - lo])       # the reads the plane builder puts there
    var, ins = devplanes.af_run_variants([_tool_variant(v) for v in variants], chrom, lo, fasta.FastaFile(fa_path))
    up = devplanes.upload_run(eng, A, "A" * A["nl"])
    try:
        cov, car, cnt = devplanes.allele_carriers_run(eng, up, A, lo, var, ins, counts=True)
        cov2, car2, none = devplanes.allele_carriers_run(eng, up, A, lo, var, ins)         # (the counters in the library's scratch)
    finally:
        up.free()
    assert none is None and np.array_equal(cov, cov2) and np.array_equal(car, car2)
    assert np.array_equal(cnt, want)
    assert np.array_equal(cov, want[:, :, 0] > 0)
    assert np.array_equal(car, 2 * want[:, :, 1].astype(np.int64) > want[:, :, 0])
    return want


@pytest.mark.parametrize("name", FIXTURES)
def test_kernel_equals_the_restatement_on_the_fixtures(engine0, tmp_path, name):
    bam_path, fa, loci, P = _fixture(name, str(tmp_path))
    bam = bamio.NativeBam(bam_path)
    kinds = set()
    for chrom, lo, hi in ds_restate.stretches(loci):
        here = [(chrom, p) for p in range(lo + 1, hi + 1)]
        variants = R.pick_variants(bam_path, fa, here)
        # an allele nobody carries at a locus that has reads: a letter the pileup does not hold, or a long insertion
        variants.append(R.V(chrom, lo + 1, "A", "AGGGGGGGGGGGGGGGGGGGGGGGGG", "INS|A|AGGGGGGGGGGGGGGGGGGGGGGGGG"))
        A = bam.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
        assert A["nl"] == hi - lo
        names = {bam.barcode_name(g): g for g in range(int(A["n_bc"]))}
        want = _check_run(engine0, A, lo, chrom, variants, bam_path, fa, names.__getitem__)
        assert not want[-1, :, 1].any()
        kinds |= {"SNV" if len(v.key) == 1 else v.key[:3] for v, w in zip(variants[:-2], want) if w[:, 1].any()}
    bam.close()
    if name == "bam_cigars":
        assert kinds == {"SNV", "INS", "DEL"}
    elif name != "bam_overcap":
        assert "SNV" in kinds


def test_kernel_equals_the_restatement_on_a_deep_synthetic_run(engine0, tmp_path):
    """C3's shape - 3000 reads per locus, here 150 barcodes x 20 reads - so that a window takes several workgroups and a variant's
    masks several 64-bit words."""
    cfg = dataclasses.replace(synth.CONFIGS["C3"], n_umi=150, rpb=20, alt_locus_frac=0.3, alt_af=0.1)
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, 260, P)
    lo = int(A["start0"])
    l0, l1 = 120, 126
    assert int((A["loc"]["w1"][l0:l1] - A["loc"]["w0"][l0:l1]).min()) > 2048 and int(A["n_bc"]) > 64
    bam_path, fa = str(tmp_path / "deep.bam"), str(tmp_path / "deep.fa")
    chrom, p0, p1 = synth.alignments_to_bam(A, bam_path, l0, l1, fa)
    here = [(chrom, p) for p in range(p0, p1 + 1)]
    variants = R.planted(bam_path, fa, here, limit=3) + R.pick_variants(bam_path, fa, here)
    want = _check_run(engine0, A, lo, chrom, variants, bam_path, fa, lambda n: int(n[1:]))
    assert int((want[0, :, 0] > 0).sum()) > 64 and int((2 * want[0, :, 1].astype(np.int64) > want[0, :, 0]).sum()) > 0


def _assert_same(x, y, what):
    for a, b, s in zip(x, y, SUFFIXES):
        assert a == b, "%s: %s differs" % (what, s)


def _contract(tmp_path, bam, fa, loci, P, variants, targets, lod):
    """cli --dsAF == a plain cli run on the tool's BAM, per target; the full-depth files those of a run without --dsAF."""
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = R.write_variants(str(tmp_path / "v.vcf"), variants, vcf=True)
    flags = ["--lod"] if lod else []
    plain = TL._read(TL._run_cli(tmp_path, "o", bam, fa, bed, P), SUFFIXES)
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, dsAF=",".join("%g" % t for t in targets), dsAFVariants=vfile, dsSeed=SEED)
    _assert_same(TL._read(got, SUFFIXES), plain, "full depth")
    mine = {t: TL._read("%s.dsAF%g" % (got, t), SUFFIXES) for t in targets}
    detection = open(got + ".dsAF.detection.txt").read()
    if lod:
        for t in targets:
            p = "%s.dsAF%g" % (got, t)
            assert TL._read(p, TL.LOD_SUFFIXES) == TL._tool_files(tmp_path, p + SUFFIXES[0], "UMT", P.mtDepth), t
        assert len(open(got + ".lod.summary.txt").read().splitlines()) == 2 + len(targets)
    for t in targets:
        out = str(tmp_path / ("af%g.bam" % t))
        af.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=SEED, refGenome=fa))
        bamio.write_bai(out)
        ref = TL._run_cli(tmp_path, "o.dsAF%g" % t, out, fa, bed, P)
        _assert_same(mine[t], TL._read(ref, SUFFIXES), "target %g" % t)
    return got, detection


def test_cli_equals_the_tool_workflow_on_bam_cigars(tmp_path):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    variants = R.pick_variants(bam, fa, loci)
    assert len(variants) == 4
    _contract(tmp_path, bam, fa, loci, P, variants, (0.05, 0.2), lod=True)


def test_cli_equals_the_tool_workflow_and_the_detection_file_on_the_synthetic_bam(tmp_path):
    tmp = str(tmp_path)
    bam, fa, loci, P, _ = R.synth_bam(tmp)
    variants = R.planted(bam, fa, loci)
    targets = (0.05, 0.02)
    got, detection = _contract(tmp_path, bam, fa, loci, P, variants, targets, lod=True)
    _, want = R.restate(bam, fa, variants, targets, SEED)
    lines = [l.split("\t") for l in detection.splitlines()]
    assert lines[0] == list(dsaf.DETECTION_HEADER) + ["LOD"]
    assert len(lines) == 1 + len(variants) * (1 + len(targets))
    outs = [(None, got)] + [(t, "%s.dsAF%g" % (got, t)) for t in targets]
    called_full = 0
    for i, v in enumerate(variants):
        for j, (t, prefix) in enumerate(outs):
            f = lines[1 + i * len(outs) + j]
            rows, cut = dsaf.read_output(prefix)
            key = (v.chrom, "%d" % v.pos)
            assert f[:5] == [v.chrom, "%d" % v.pos, v.ref, v.alt, dsaf.target_text(t)]
            called = int(key in cut and cut[key][0] == v.ref and v.alt in cut[key][1])
            assert f[14] == "%d" % called
            r = want[max(j - 1, 0)]["rows"][i]
            n2, v2 = (r["N"], r["V"]) if t is None else (r["N2"], r["V2"])
            assert f[5:8] == ["%d" % n2, "%d" % v2, dsaf.frac_text(v2 / n2 if n2 else 0.0)]
            assert f[8] == dsaf.frac_text(1.0 if t is None else r["k"])
            lod_line = [l for l in open(prefix + ".lod.bedgraph").read().splitlines() if l.split("\t")[2] == "%d" % v.pos][0]
            assert f[15] == lod_line.split("\t")[3]
            called_full += called if t is None else 0
    # a planted variant is called at full depth - by a plain run of the same BAM (the full-depth files equal its files)
    assert called_full >= 1


def test_cli_refuses_a_variant_off_the_target_before_any_file(tmp_path):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = str(tmp_path / "v.txt")
    open(vfile, "w").write("%s\t%d\tA\tG\n" % (loci[0][0], max(p for _, p in loci) + 5000))
    with pytest.raises(SystemExit, match="is not a locus of --bedTarget"):
        TL._run_cli(tmp_path, "r", bam, fa, bed, P, dsAF="0.05", dsAFVariants=vfile)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("r.")]
