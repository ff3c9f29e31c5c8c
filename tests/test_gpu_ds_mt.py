"""--dsMT on the GPU: smc_select_alignments against its host restatement (tests/ds_restate.py), the builder on what it selects, and
the command line against the reference workflow - tools.ds_mt, then a plain run on the BAM it wrote."""
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import abi, bamio, cli, devplanes, synth
from smcounter_amd.py2compat import py2_round

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURES = ("case", "bam_cigars", "bam_overcap", "bam_deep")


def _fixture(name, tmp):
    return ds_restate.make_case(tmp) if name == "case" else ds_restate.load_fixture(name, tmp)


def _check_selection(eng, A, lo, P, mask=None, idents=None, frac=1.0, seed=0):
    """Device selection == host restatement, field for field; then the builder takes the selected run with status 0."""
    from smcounter_amd.engine import DevBuf
    if mask is None:
        mask = devplanes.philox_keep_host(eng.L, idents, frac, seed)
        use = dict(idents=idents, frac=frac, seed=seed)
    else:
        use = dict(mask=mask)
    want = ds_restate.select(A, mask, lo)
    run_ref = "A" * A["nl"]
    up = devplanes.upload_run(eng, A, run_ref)
    sel, counts, d_orig = devplanes.select_run(eng, up, A, lo, **use)
    k = sel.n_aln
    assert k == want["kept"] and counts["deepest"] == want["deepest"] and counts["n_slots"] == want["slots"]
    if k:
        got = sel.aln.download(abi.DEV_ALN_DTYPE, k)
        assert got.tobytes() == want["aln"].tobytes()
        assert np.array_equal(d_orig.download(np.uint32, k), want["orig_index"])
    loc = sel.loc.download(abi.DEV_LOCUS_DTYPE, A["nl"])
    assert loc.tobytes() == want["loc"].tobytes()
    # the builder on the selected run (32-bit words, every plane): the status word is 0 (build_run answers None otherwise)
    cap = want["slots"] + 64
    planes = [DevBuf(eng, 4 * cap) for _ in range(4)]
    words = DevBuf(eng, 4 * cap)
    words.word_bits = 32
    uaux = [DevBuf(eng, 4 * (cap + A["nl"] + 8192)) for _ in range(3)]
    done = devplanes.build_run(counts, eng.L, eng, abi.c_params(P), P, "chrQ", lo, synth.CyclicRef(), run_ref, [words] + planes, uaux,
                               0, 0, cap + A["nl"], eng.L.smc_build_max_depth(), lambda *a: "N", lambda g: "B%d" % g, uploaded=sel)
    assert done is not None and done != devplanes.NARROW
    assert np.array_equal(done[2]["n_reads"], want["loc"]["n"])
    sel.free(shared=False); d_orig.free(); up.free()
    for b in planes + [words] + uaux:
        b.free()
    return want


@pytest.mark.parametrize("name", FIXTURES)
def test_kernel_equals_host_restatement_on_the_fixtures(engine0, tmp_path, name):
    bam_path, _, loci, P = _fixture(name, str(tmp_path))
    bam = bamio.NativeBam(bam_path)
    rng = np.random.default_rng(3)
    for chrom, lo, hi in ds_restate.stretches(loci):
        A = bam.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
        nb = int(A["n_bc"])
        _check_selection(engine0, A, lo, P, mask=np.ones(nb, bool))
        w = _check_selection(engine0, A, lo, P, mask=np.zeros(nb, bool))
        assert w["kept"] == 0 and not w["loc"]["n"].any()
        _check_selection(engine0, A, lo, P, mask=rng.random(nb) < 0.4)
        _check_selection(engine0, A, lo, P, idents=bam.barcode_idents(nb), frac=0.5, seed=11)
    bam.close()


@pytest.mark.parametrize("n_loci", [260, 3000])
def test_kernel_equals_host_restatement_on_synthetic_runs(engine0, n_loci):
    cfg = synth.CONFIGS["C3"]
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, n_loci, P)
    lo, nb = int(A["start0"]), int(A["n_bc"])
    assert len(A["aln"]) > 4 * 1024                        # (several blocks of the kernel)
    w = _check_selection(engine0, A, lo, P, mask=np.ones(nb, bool))
    assert np.array_equal(w["loc"], A["loc"])
    _check_selection(engine0, A, lo, P, mask=np.zeros(nb, bool))
    _check_selection(engine0, A, lo, P, mask=np.random.default_rng(n_loci).random(nb) < 0.3)
    ids = devplanes.fnv64_array(["B%d" % g for g in range(nb)])
    for f in (0.25, 1.0):
        _check_selection(engine0, A, lo, P, idents=ids, frac=f, seed=5)


def _run_cli(tmp, tag, bam, fa, bed, P, **kw):
    prefix = str(tmp / tag)
    cli.main(dict(outPrefix=prefix, bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, hpLen=P.hpLen, minBQ=P.minBQ,
                  minMQ=P.minMQ, mismatchThr=P.mismatchThr, mtDrop=P.mtDrop, maxMT=P.maxMT, primerDist=P.primerDist, refGenome=fa, **kw))
    return prefix


def _files(prefix):
    return [open(prefix + s, "rb").read() for s in (".smCounter.all.txt", ".smCounter.cut.txt", ".smCounter.cut.vcf")]


def _assert_same(x_files, y_files, what):
    for x, y, suffix in zip(x_files, y_files, ("all.txt", "cut.txt", "cut.vcf")):
        if x != y:
            lx, ly = x.splitlines(), y.splitlines()
            k = next((i for i, (u, v) in enumerate(zip(lx, ly)) if u != v), min(len(lx), len(ly)))
            raise AssertionError("%s: %s differs (%d vs %d lines) at line %d:\n%r\n%r" % (what, suffix, len(lx), len(ly), k,
                                                                                        lx[k] if k < len(lx) else None, ly[k] if k < len(ly) else None))


@pytest.mark.parametrize("name", FIXTURES)
def test_cli_dsmt_equals_the_reference_workflow(tmp_path, name):
    """Every file, byte for byte - the VCF header names the output prefix, so each reference run writes under the same prefix as the
    file it is compared with (after that file has been read)."""
    bam_path, fa, loci, P = _fixture(name, str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    seed = 1234567
    plain = _files(_run_cli(tmp_path, "o", bam_path, fa, bed, P))
    got = _run_cli(tmp_path, "o", bam_path, fa, bed, P, dsMT="0.5,0.25")
    _assert_same(_files(got), plain, "full depth")         # the full-depth files do not change
    mine = {f: _files("%s.dsMT%g" % (got, f)) for f in (0.5, 0.25)}
    for f in (0.5, 0.25):
        d = max(1, int(py2_round(f * P.mtDepth)))
        ds_bam = ds_restate.write_ds_bam(bam_path, str(tmp_path / ("ds%g.bam" % f)), f, seed)
        ref = _run_cli(tmp_path, "o.dsMT%g" % f, ds_bam, fa, bed, dataclasses.replace(P, mtDepth=d))
        _assert_same(mine[f], _files(ref), "%s f=%g" % (name, f))


@pytest.mark.parametrize("name", ("case", "bam_cigars"))
def test_cli_dsmt_philox_equals_a_bam_of_its_kept_set(tmp_path, name):
    from smcounter_amd import _lib
    bam_path, fa, loci, P = _fixture(name, str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    got = _run_cli(tmp_path, "ph", bam_path, fa, bed, P, dsMT="0.5", dsSampler="philox", dsSeed=77, dsMtDepth=str(P.mtDepth))
    mine = _files(got + ".dsMT0.5")
    order = bamio.placed_barcodes(bam_path)
    keep = devplanes.philox_keep_host(_lib.load(), devplanes.fnv64_array(order), 0.5, 77)
    kept = {b for b, k in zip(order, keep) if k}
    assert 0 < len(kept) < len(order)
    ref = _run_cli(tmp_path, "ph.dsMT0.5", ds_restate.write_kept_bam(bam_path, str(tmp_path / "ph.bam"), kept), fa, bed, P)
    _assert_same(mine, _files(ref), "philox " + name)
