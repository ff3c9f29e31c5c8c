"""--dsRpb on the GPU: the read-level rule of smc_select_alignments_keyed against its host restatement (tests/ds_rpb_restate.py), the
builder on what it selects, the renumbering of the kept ids (the decoder's ids and rows back from a run whose ids were scrambled), and
the command line against the reference workflow - tools.ds_reads_within_mt, then a plain run with --rpb r on the BAM it wrote."""
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import abi, bamio, cli, devplanes, fasta, synth, vc
from smcounter_amd.py2compat import py2_round

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import ds_rpb_restate  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURES = ("case", "bam_cigars", "bam_overcap", "bam_deep")
SEED = 1234567


def _fixture(name, tmp):
    return ds_restate.make_case(tmp) if name == "case" else ds_restate.load_fixture(name, tmp)


def _check_selection(eng, A, lo, P, mask):
    """Device selection (read level) == host restatement, field for field; then the builder takes the selected run with status 0."""
    from smcounter_amd.engine import DevBuf
    want = ds_rpb_restate.select(A, mask, lo)
    run_ref = "A" * A["nl"]
    up = devplanes.upload_run(eng, A, run_ref)
    sel, counts, d_orig = devplanes.select_run(eng, up, A, lo, mask=mask, level="read")
    k = sel.n_aln
    assert k == want["kept"] and counts["deepest"] == want["deepest"] and counts["n_slots"] == want["slots"]
    if k:
        got = sel.aln.download(abi.DEV_ALN_DTYPE, k)
        assert got.tobytes() == want["aln"].tobytes()
        assert np.array_equal(d_orig.download(np.uint32, k), want["orig_index"])
    loc = sel.loc.download(abi.DEV_LOCUS_DTYPE, A["nl"])
    assert loc.tobytes() == want["loc"].tobytes()
    cap = want["slots"] + 64
    planes = [DevBuf(eng, 4 * cap) for _ in range(4)]
    words = DevBuf(eng, 4 * cap)
    words.word_bits = 32
    uaux = [DevBuf(eng, 4 * (cap + A["nl"] + 8192)) for _ in range(3)]
    done = devplanes.build_run(counts, eng.L, eng, abi.c_params(P), P, "chrQ", lo, synth.CyclicRef(), run_ref, [words] + planes, uaux,
                               0, 0, cap + A["nl"], eng.L.smc_build_max_depth(), lambda *a: "N", lambda g: "B%d" % g, uploaded=sel)
    assert done is not None and done != devplanes.NARROW          # (None: the builder's status word was not 0)
    assert np.array_equal(done[2]["n_reads"], want["loc"]["n"])
    sel.free(shared=False); d_orig.free(); up.free()
    for b in planes + [words] + uaux:
        b.free()
    return want


@pytest.mark.parametrize("name", FIXTURES)
def test_read_level_kernel_equals_host_restatement_on_the_fixtures(engine0, tmp_path, name):
    bam_path, _, loci, P = _fixture(name, str(tmp_path))
    rules = devplanes.reference_read_rules(bam_path, (1.5, 2.5), [P, P], SEED)
    bam = bamio.NativeBam(bam_path)
    rng = np.random.default_rng(3)
    partial = 0
    for chrom, lo, hi in ds_restate.stretches(loci):
        A = bam.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
        npr = int(A["n_pair"])
        w = _check_selection(engine0, A, lo, P, np.ones(npr, bool))
        assert w["kept"] == len(A["aln"]) and np.array_equal(w["loc"], A["loc"])
        w = _check_selection(engine0, A, lo, P, np.zeros(npr, bool))
        assert w["kept"] == 0 and not w["loc"]["n"].any()
        _check_selection(engine0, A, lo, P, rng.random(npr) < 0.5)
        for rule in rules:
            w = _check_selection(engine0, A, lo, P, ds_rpb_restate.pair_mask(bam, npr, rule.kept))
            partial += 0 < w["kept"] < len(A["aln"])
    bam.close()
    assert partial >= 1


@pytest.mark.parametrize("n_loci", [260, 3000])
def test_read_level_kernel_equals_host_restatement_on_synthetic_runs(engine0, n_loci):
    cfg = synth.CONFIGS["C3"]
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, n_loci, P)
    lo, npr = int(A["start0"]), int(A["n_pair"])
    assert len(A["aln"]) > 4 * 1024                        # (several blocks of the kernel)
    w = _check_selection(engine0, A, lo, P, np.ones(npr, bool))
    assert np.array_equal(w["loc"], A["loc"])
    _check_selection(engine0, A, lo, P, np.zeros(npr, bool))
    rng = np.random.default_rng(n_loci)
    for p in (0.2, 0.7):
        _check_selection(engine0, A, lo, P, rng.random(npr) < p)


def _rows(eng, A, P, chrom, lo, ref, run_ref, allele_key, barcode_name, uploaded=None):
    """The called rows (abi.ROW_DTYPE bytes) and allele tables of one run built by smc_build_planes (32-bit read words)."""
    from smcounter_amd.engine import DevBuf
    nl, ns = A["nl"], A["n_slots"]
    cap = ns + 64
    uaux = [DevBuf(eng, 4 * (cap + nl + 8192)) for _ in range(3)]
    words = DevBuf(eng, 4 * cap, walk_output=True)
    words.word_bits = 32
    done = devplanes.build_run(A, eng.L, eng, abi.c_params(P), P, chrom, lo, ref, run_ref, [words, None, None, None, None], uaux, 0, 0,
                               cap + nl, eng.L.smc_build_max_depth(), allele_key, barcode_name, uploaded=uploaded)
    assert done is not None and done != devplanes.NARROW
    nl, ns, lc, tb = done
    uaux[1].free(); uaux[2].free()
    rb = devplanes.ResidentBatch(planes=[None] * 4 + [uaux[0]], words=words, n_slots=ns, n_ustart=ns + nl + 1, loci=lc,
                                 chrom=[chrom] * nl, pos=np.arange(lo + 1, lo + 1 + nl, dtype=np.int64), ref=list(run_ref), alleles=tb,
                                 n_device_runs=1)
    rows = vc.vc_resident_rows(rb, P, eng)
    words.free(); uaux[0].free()
    return rows.tobytes(), tb


def _renumbered(A, rng):
    """A copy of run A with bc_gid and pair_gid put through random bijections."""
    aln = A["aln"].copy()
    pb, pp = rng.permutation(int(A["n_bc"])), rng.permutation(int(A["n_pair"]))
    aln["bc_gid"] = pb[aln["bc_gid"]]
    aln["pair_gid"] = pp[aln["pair_gid"]]
    return dict(A, aln=aln)


def _check_renumbering(eng, A, P, chrom, lo, ref, run_ref, allele_key, barcode_name, rng):
    """Run A's rows; then A with its ids through random bijections, selected at the read level keeping every name: the kernel hands back
    the decoder's records (ids renumbered by first kept appearance) and the rows built from them are A's, byte for byte.  -> whether
    the bijections changed the run's ids (not in an empty run or one of a single barcode and read name)."""
    want = _rows(eng, A, P, chrom, lo, ref, run_ref, allele_key, barcode_name)
    B = _renumbered(A, rng)
    scrambled = not (np.array_equal(B["aln"]["bc_gid"], A["aln"]["bc_gid"]) and np.array_equal(B["aln"]["pair_gid"], A["aln"]["pair_gid"]))
    up = devplanes.upload_run(eng, B, run_ref)
    sel, counts, d_orig = devplanes.select_run(eng, up, B, lo, mask=np.ones(int(B["n_pair"]), bool), level="read")
    assert sel.aln.download(abi.DEV_ALN_DTYPE, sel.n_aln).tobytes() == A["aln"].tobytes()
    got = _rows(eng, counts, P, chrom, lo, ref, run_ref, allele_key, barcode_name, uploaded=sel)
    assert got[0] == want[0] and got[1] == want[1]
    sel.free(shared=False); d_orig.free(); up.free()
    return scrambled


@pytest.mark.parametrize("name", FIXTURES)
def test_read_level_selection_renumbers_the_ids_as_the_decoder(engine0, tmp_path, name):
    """Dropping reads can move a barcode's first appearance, so the selected run's ids need not be in the order the down-sampled BAM's
    decoder numbers them, and the builder's rows are not independent of that order (built once with a run's ids and once with both
    ids through a random bijection, the rows of `case` and `bam_cigars` differed: profiles/ds_rpb_id_bijection.txt).  So the read
    level renumbers the kept ids by first kept appearance; this pins that it restores the decoder's ids and rows exactly."""
    bam_path, fa, loci, P = _fixture(name, str(tmp_path))
    ref = fasta.FastaFile(fa)
    bam = bamio.NativeBam(bam_path)
    rng = np.random.default_rng(17)
    scrambled = 0
    for chrom, lo, hi in ds_restate.stretches(loci):
        A = bam.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
        run_ref = ref.fetch(chrom, lo, lo + A["nl"]).upper()
        names = [bam.barcode_name(g) for g in range(int(A["n_bc"]))]
        scrambled += _check_renumbering(engine0, A, P, chrom, lo, ref, run_ref, bam.allele_key, lambda g: names[g], rng)
    bam.close()
    assert scrambled >= 1


def test_read_level_selection_renumbers_the_ids_as_the_decoder_synthetic(engine0):
    cfg = synth.CONFIGS["C3"]
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, 1000, P)
    lo = int(A["start0"])
    assert _check_renumbering(engine0, A, P, synth.ALN_CHROM, lo, synth.CyclicRef(), synth.aln_ref_fetch(lo, lo + A["nl"]),
                              devplanes.synth_allele_key(A), lambda g: "B%d" % g, np.random.default_rng(5))


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


def _reference_rpb(tmp, bam_path, fa, bed, P, r, tag):
    ds_bam = ds_rpb_restate.write_rpb_bam(bam_path, str(tmp / ("rpb%g.bam" % r)), r, SEED)
    return _files(_run_cli(tmp, tag, ds_bam, fa, bed, dataclasses.replace(P, rpb=r)))


TARGETS = {"case": "1.5,2,9", "bam_cigars": "1.5,2.5", "bam_overcap": "1.5,2.5", "bam_deep": "2,4"}


@pytest.mark.parametrize("name", FIXTURES)
def test_cli_dsrpb_equals_the_reference_workflow(tmp_path, name):
    """Every file, byte for byte - the VCF header names the output prefix, so each reference run writes under the same prefix as the
    file it is compared with (after that file has been read)."""
    bam_path, fa, loci, P = _fixture(name, str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    plain = _files(_run_cli(tmp_path, "o", bam_path, fa, bed, P))
    got = _run_cli(tmp_path, "o", bam_path, fa, bed, P, dsRpb=TARGETS[name])
    _assert_same(_files(got), plain, "full depth")         # the full-depth files do not change
    targets = [float(x) for x in TARGETS[name].split(",")]
    assert len(targets) >= 2
    mine = {r: _files("%s.dsRpb%g" % (got, r)) for r in targets}
    for r in targets:
        _assert_same(mine[r], _reference_rpb(tmp_path, bam_path, fa, bed, P, r, "o.dsRpb%g" % r), "%s r=%g" % (name, r))


@pytest.mark.parametrize("name", ("case", "bam_deep"))
def test_cli_dsmt_and_dsrpb_in_one_run(tmp_path, name):
    bam_path, fa, loci, P = _fixture(name, str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    plain = _files(_run_cli(tmp_path, "o", bam_path, fa, bed, P))
    got = _run_cli(tmp_path, "o", bam_path, fa, bed, P, dsMT="0.5", dsRpb="2", dsSeed=SEED)
    _assert_same(_files(got), plain, "full depth")
    mt, rpb = _files(got + ".dsMT0.5"), _files(got + ".dsRpb2")
    d = max(1, int(py2_round(0.5 * P.mtDepth)))
    ds_bam = ds_restate.write_ds_bam(bam_path, str(tmp_path / "ds0.5.bam"), 0.5, SEED)
    _assert_same(mt, _files(_run_cli(tmp_path, "o.dsMT0.5", ds_bam, fa, bed, dataclasses.replace(P, mtDepth=d))), "dsMT 0.5")
    _assert_same(rpb, _reference_rpb(tmp_path, bam_path, fa, bed, P, 2.0, "o.dsRpb2"), "dsRpb 2")


def test_cli_dsrpb_over_the_barcode_cap_equals_the_reference_workflow(tmp_path):
    """bam_deep with --maxMT 40: every locus is over the barcode cap (the reference's sample over the barcode texts), and in every run
    the kept barcodes come out of first-appearance order - the renumbered ids must reach the sampler's texts through the old ids."""
    bam_path, fa, loci, P = _fixture("bam_deep", str(tmp_path))
    P = dataclasses.replace(P, maxMT=40)
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    got = _run_cli(tmp_path, "o", bam_path, fa, bed, P, dsRpb="2,4")
    mine = {r: _files("%s.dsRpb%g" % (got, r)) for r in (2.0, 4.0)}
    for r in (2.0, 4.0):
        _assert_same(mine[r], _reference_rpb(tmp_path, bam_path, fa, bed, P, r, "o.dsRpb%g" % r), "bam_deep maxMT 40 r=%g" % r)
