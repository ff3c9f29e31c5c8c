"""--spikeAF on the GPU: smc_spike_alleles against the restatement from host-built pileups (tests/spike_restate.py), byte for byte;
the command line against the offline workflow - tools.spike_variants, then a plain run on the BAM it wrote; the detection file."""
import argparse
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, bamio, devplanes, dsaf, fasta, spike, synth
from smcounter_amd.engine import DevBuf
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import spike_restate as SR  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line, the LOD tool's files)

pytestmark = pytest.mark.gpu
SEED = 20240607
T = 0.5
MMOK = 16
SUFFIXES = TL.SUFFIXES


def _synth(tmp):
    """About 300 reads per locus, 100 barcodes at a locus, 900 loci: a few thousand alignments (several workgroups), several hundred
    run-wide barcodes."""
    cfg = dataclasses.replace(R.SYNTH_CFG, n_umi=100, rpb=3)
    bam, fa, loci, P, A = R.synth_bam(tmp, cfg, 900)
    return bam, fa, loci, P


def _inputs(name, tmp):
    if name == "case":
        return SR.make_case(tmp)
    bam, fa, loci, P = _synth(tmp) if name == "synth" else ds_restate.load_fixture(name, tmp)
    return bam, fa, loci, P, None


def _svar(variants, thr):
    """The variants as the entries take them, sorted by position; thr: one threshold for all, or one per variant in that order."""
    var = np.zeros(len(variants), abi.SPIKE_VARIANT_DTYPE)
    for k, v in enumerate(sorted(variants, key=lambda v: v.pos)):
        var[k]["pos0"], var[k]["ref"], var[k]["alt"] = v.pos - 1, ord(v.ref), ord(v.alt)
        var[k]["thr"] = thr if isinstance(thr, int) else thr[k]
    return var


def _run_kernel(eng, nat, A, chrom, variants, thr, seed, P):
    """smc_spike_alleles over run `A` for `variants` (all on `chrom`) at one threshold, or one per variant -> (aln_out, bq_out, stats);
    the run's own arrays in HBM must come back as they went up."""
    var = _svar(variants, thr)
    idents = nat.barcode_idents(A["n_bc"])
    nm, n_indel = nat.run_mismatches(len(A["aln"]))
    up = devplanes.upload_run(eng, A, "A" * A["nl"])
    try:
        out, stats = devplanes.spike_run(eng, up, A, var, idents, seed, P.mismatchThr, nm, n_indel)
        try:
            aln = out.aln.download(abi.DEV_ALN_DTYPE, len(A["aln"]))
            bq = out.bq.download(np.uint8, len(A["bq"]))
        finally:
            out.aln.free(); out.bq.free()
        assert up.aln.download(abi.DEV_ALN_DTYPE, len(A["aln"])).tobytes() == A["aln"].tobytes()
        assert up.bq.download(np.uint8, len(A["bq"])).tobytes() == A["bq"].tobytes()
    finally:
        up.free()
    return aln, bq, stats


def _expected(A, recs, records):
    """The run's records and pool as the restatement rewrites them; `recs`: the readable decoder's records of the run, in its order."""
    aln, bq = A["aln"].copy(), A["bq"].copy()
    assert len(recs) == len(aln) and [a.pos for a in recs] == aln["pos"].tolist()
    for i, a in enumerate(recs):
        r = records.get(SR.rec_key(a))
        if r is None:
            continue
        for q, letter in r["edits"].items():
            at = 2 * (int(aln["seq_off"][i]) + q)
            assert chr(bq[at]) == r["old"][q]
            bq[at] = ord(letter)
        aln["oflag"][i] = (int(aln["oflag"][i]) & (0xFF ^ MMOK)) | (MMOK if r["mmok"] else 0)
    return aln, bq


def _check_run(eng, nat, py, chrom, lo, hi, P, variants, bam_path, fa, t=T):
    A = nat.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
    assert A["nl"] == hi - lo
    records, stats = SR.restate(bam_path, fa, variants, t, SEED, P.mismatchThr)
    aln, bq, got = _run_kernel(eng, nat, A, chrom, variants, sv.threshold(t), SEED, P)
    want_aln, want_bq = _expected(A, py.fetch(chrom, lo, hi), records)
    assert bq.tobytes() == want_bq.tobytes()
    assert aln.tobytes() == want_aln.tobytes()
    return A, records, stats, got, (aln, bq)


@pytest.mark.parametrize("name", ("case", "bam_cigars", "bam_deep", "synth"))
def test_kernel_equals_the_restatement(engine0, tmp_path, name):
    bam_path, fa, loci, P, variants = _inputs(name, str(tmp_path))
    nat, py = bamio.NativeBam(bam_path), bamio.BamFile(bam_path)
    rewritten = 0
    for chrom, lo, hi in ds_restate.stretches(loci):
        here = [(chrom, p) for p in range(lo + 1, hi + 1)]
        # (the synthetic run: four positions out of sixteen loci in its middle - the readable decoder builds only those pileups)
        vs = variants or (SR.pick_positions(bam_path, fa, here[120:136], 4) if name == "synth" else SR.pick_positions(bam_path, fa, here, 3))
        if not vs:
            continue
        A, records, stats, got, (aln, bq) = _check_run(engine0, nat, py, chrom, lo, hi, P, vs, bam_path, fa)
        # every listed position is a locus of the run: every record that spans it is in the run, the statistics are the file's
        assert got[:, 0].tolist() == [s["READS"] for s in stats] and got[:, 1].tolist() == [s["NMINC"] for s in stats]
        rewritten += int(got[:, 0].sum())
        if name == "synth":
            assert len(A["aln"]) > 2000 and int(A["n_bc"]) > 64
        if name == "case":
            assert int(((aln["oflag"] ^ A["aln"]["oflag"]) & MMOK != 0).sum()) > 0        # an increment flipped incCond
        # two calls give identical bytes
        aln2, bq2, got2 = _run_kernel(engine0, nat, A, chrom, vs, sv.threshold(T), SEED, P)
        assert aln2.tobytes() == aln.tobytes() and bq2.tobytes() == bq.tobytes() and np.array_equal(got, got2)
    assert rewritten > 0
    nat.close(); py.close()


def test_thresholds_zero_and_all(engine0, tmp_path):
    bam_path, fa, loci, P, variants = SR.make_case(str(tmp_path))
    nat, py = bamio.NativeBam(bam_path), bamio.BamFile(bam_path)
    (chrom, lo, hi), = ds_restate.stretches(loci)
    A = nat.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
    aln, bq, st = _run_kernel(engine0, nat, A, chrom, variants, 0, SEED, P)
    assert aln.tobytes() == A["aln"].tobytes() and bq.tobytes() == A["bq"].tobytes() and not st.any()
    aln, bq, st = _run_kernel(engine0, nat, A, chrom, variants, 1 << 32, SEED, P)
    # every eligible record: the pileup's reads whose key is a single letter, counted from the host-built pileups
    pb = R.pileups(bam_path, fa, [(v.chrom, v.pos) for v in variants])
    for l, v in enumerate(variants):
        sl = pb.locus_slice(l)
        assert int(st[l, 0]) == sum(len(pb.alleles[l][int(a)]) == 1 for a in pb.allele[sl]) > 0
    recs = py.fetch(chrom, lo, hi)
    for v in variants:
        for i, a in enumerate(recs):
            q = sv.base_at(a, v.pos) if a.pos < v.pos <= a.end else None
            if q is not None:
                assert chr(bq[2 * (int(A["aln"]["seq_off"][i]) + q)]) == v.alt
    nat.close(); py.close()


def test_own_thresholds_are_per_variant_and_the_copies_ignore_them(engine0, tmp_path):
    """P1 at threshold 0 and P2 - the `first` reads cover both - at 2^32 in ONE smc_spike_alleles call: P2 alone is written.  The same
    array through smc_spike_alleles_reps: the copy's threshold holds for both variants, the array's own are not read."""
    bam_path, fa, loci, P, variants = SR.make_case(str(tmp_path))
    vs, own = variants[:2], [0, 1 << 32]
    nat, py = bamio.NativeBam(bam_path), bamio.BamFile(bam_path)
    (chrom, lo, hi), = ds_restate.stretches(loci)
    A = nat.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
    recs = py.fetch(chrom, lo, hi)
    assert any(a.pos < vs[0].pos and vs[1].pos <= a.end for a in recs)
    n, nb = len(A["aln"]), len(A["bq"])
    # the single call: the restatement of P2 alone at t = 1
    records, stats = SR.restate(bam_path, fa, vs[1:], 1.0, SEED, P.mismatchThr)
    want_aln, want_bq = _expected(A, recs, records)
    aln, bq, st = _run_kernel(engine0, nat, A, chrom, vs, own, SEED, P)
    assert st.tolist() == [[0, 0], [stats[0]["READS"], stats[0]["NMINC"]]] and stats[0]["READS"] > 0
    assert bq.tobytes() == want_bq.tobytes() and aln.tobytes() == want_aln.tobytes()
    column = {2 * (int(A["aln"]["seq_off"][i]) + sv.base_at(a, vs[1].pos)) for i, a in enumerate(recs)
              if a.pos < vs[1].pos <= a.end and sv.base_at(a, vs[1].pos) is not None}
    changed = np.flatnonzero(bq != A["bq"]).tolist()
    assert changed and set(changed) <= column
    # one copy at 2^32: both variants, the restatement of both at t = 1; one copy at 0: the input
    records, stats = SR.restate(bam_path, fa, vs, 1.0, SEED, P.mismatchThr)
    both_aln, both_bq = _expected(A, recs, records)
    assert all(x["READS"] > 0 for x in stats)
    idents, (nm, n_indel) = nat.barcode_idents(A["n_bc"]), nat.run_mismatches(n)
    up = devplanes.upload_run(engine0, A, "A" * A["nl"])
    try:
        for thr, w_aln, w_bq, w_st in ((1 << 32, both_aln, both_bq, [[x["READS"], x["NMINC"]] for x in stats]),
                                       (0, A["aln"], A["bq"], [[0, 0], [0, 0]])):
            d_aln, d_bq, _, got = devplanes.spike_run_copies(engine0, up, A, _svar(vs, own), idents, [SEED], [thr], P.mismatchThr, nm, n_indel)
            try:
                c_aln, c_bq = d_aln.download(np.uint8, 36 * n), d_bq.download(np.uint8, nb)
            finally:
                d_aln.free(); d_bq.free()
            assert got.tolist() == [w_st]
            assert c_bq.tobytes() == w_bq.tobytes() and c_aln.tobytes() == w_aln.tobytes()
    finally:
        up.free()
    nat.close(); py.close()


def test_a_listed_position_outside_the_runs_loci(engine0, tmp_path):
    """The run holds three loci in front of P1; P1 is listed and is none of them - the records that span it are rewritten all the
    same, and their mismatch bit moves at every locus they cover."""
    bam_path, fa, loci, P, variants = SR.make_case(str(tmp_path))
    nat, py = bamio.NativeBam(bam_path), bamio.BamFile(bam_path)
    lo, hi = SR.P1 - 5, SR.P1 - 2
    A, records, stats, got, (aln, bq) = _check_run(engine0, nat, py, SR.CASE_CHROM, lo, hi, P, variants[:1], bam_path, fa)
    assert 0 < int(got[0, 0]) <= stats[0]["READS"]
    assert int(((aln["oflag"] ^ A["aln"]["oflag"]) & MMOK != 0).sum()) > 0
    nat.close(); py.close()


def test_refusals_launch_nothing(engine0, tmp_path):
    eng = engine0
    n = 8
    ok = np.zeros(2, abi.SPIKE_VARIANT_DTYPE)
    ok["pos0"], ok["ref"], ok["alt"], ok["thr"] = [5, 9], ord("A"), ord("G"), 1 << 31
    bufs = [DevBuf(eng, 4096).upload(np.full(4096, 0x5A, np.uint8)) for _ in range(3)]      # aln_out, bq_out, stats
    src = DevBuf(eng, 4096).upload(np.zeros(4096, np.uint8))

    def call(var, n_var=None):
        d_var = DevBuf(eng, var.nbytes + 256).upload(np.ascontiguousarray(var).view(np.uint8).reshape(-1)) if len(var) else src
        rc = eng.L.smc_spike_alleles(eng.ctx, src.data_ptr(), n, src.data_ptr(), src.data_ptr(), 64, d_var.data_ptr(), var.ctypes.data,
                                     len(var) if n_var is None else n_var, src.data_ptr(), 4, 7, 6.0, src.data_ptr(), src.data_ptr(),
                                     bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), None)
        if d_var is not src:
            d_var.free()
        return rc

    def edit(**kw):
        v = ok.copy()
        for k, (i, x) in kw.items():
            v[k][i] = x
        return v
    for var, msg in ((edit(pos0=(1, 5)), "not strictly ascending"), (edit(pos0=(1, 4)), "not strictly ascending"),
                     (edit(ref=(0, ord("N"))), "outside ACGT"), (edit(alt=(1, ord("a"))), "outside ACGT"), (edit(alt=(0, ord("A"))), "ref equals alt"),
                     (edit(thr=(1, (1 << 32) + 1)), "above 2^32")):
        assert call(var) < 0 and msg.encode() in eng.L.smc_last_error()
    big = np.zeros(4097, abi.SPIKE_VARIANT_DTYPE)
    assert call(big) < 0 and b"at most 4096" in eng.L.smc_last_error()
    eng.L.smc_device_sync(eng.ctx)
    for b in bufs:
        assert (b.download(np.uint8, 4096) == 0x5A).all()                              # nothing copied, nothing launched
    for b in bufs + [src]:
        b.free()


def _assert_same(x, y, what):
    for a, b, s in zip(x, y, SUFFIXES):
        assert a == b, "%s: %s differs" % (what, s)


def _contract(engine0, tmp_path, bam, fa, loci, P, variants, targets):
    """cli --spikeAF --lod == a plain cli run on the tool's BAM, per target; the full-depth files those of a run without the flags;
    the LOD files the tool's; the detection file the outputs' own rows and the restatement's numbers."""
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = R.write_variants(str(tmp_path / "v.vcf"), variants, vcf=True)
    plain = TL._read(TL._run_cli(tmp_path, "o", bam, fa, bed, P), SUFFIXES)
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=["--lod"], spikeAF=",".join("%g" % t for t in targets), spikeVariants=vfile,
                      dsSeed=SEED)
    _assert_same(TL._read(got, SUFFIXES), plain, "full depth")
    assert len(open(got + ".lod.summary.txt").read().splitlines()) == 2 + len(targets)
    lines = [l.split("\t") for l in open(got + ".spikeAF.detection.txt").read().splitlines()]
    assert lines[0] == list(spike.DETECTION_HEADER) + ["LOD"] and len(lines) == 1 + len(variants) * (1 + len(targets))
    outs = [(None, got)] + [(t, "%s.spikeAF%g" % (got, t)) for t in targets]
    stats = {t: SR.restate(bam, fa, variants, t, SEED, P.mismatchThr)[1] for t in targets}
    called = 0
    for j, (t, prefix) in enumerate(outs):
        if t is not None:
            assert TL._read(prefix, TL.LOD_SUFFIXES) == TL._tool_files(tmp_path, prefix + SUFFIXES[0], "UMT", P.mtDepth), t
            out = str(tmp_path / ("spike%g.bam" % t))
            sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=SEED, refGenome=fa))
            bamio.write_bai(out)
            ref = TL._run_cli(tmp_path, "o.spikeAF%g" % t, out, fa, bed, P)
            _assert_same(TL._read(prefix, SUFFIXES), TL._read(ref, SUFFIXES), "target %g" % t)
            # V1: smc_allele_carriers over the spiked file
            tool_vs = [af.Variant(v.chrom, v.pos, v.ref, v.alt, v.alt, af.SNV) for v in variants]
            _, carries = devplanes.ds_af_sets(out, fasta.FastaFile(fa), tool_vs, P, engine0)
        rows, cut = dsaf.read_output(prefix)
        for i, v in enumerate(variants):
            f = lines[1 + i * len(outs) + j]
            key = (v.chrom, "%d" % v.pos)
            s = stats[t if t is not None else targets[0]][i]
            want = [s["N"], s["V0"], 0, 0, s["V0"]] if t is None else [s["N"], s["V0"], s["S"], s["READS"], s["V1"]]
            assert f[:5] == [v.chrom, "%d" % v.pos, v.ref, v.alt, dsaf.target_text(t)]
            assert f[5:11] == ["%d" % x for x in want] + [dsaf.frac_text(want[4] / want[0] if want[0] else 0.0)]
            assert f[11:16] == [rows[key][dsaf._COL[c]] for c in ("UMT", "VMT", "VMF", "PI", "FILTER")]
            is_called = int(key in cut and cut[key][0] == v.ref and v.alt in cut[key][1])
            assert f[16] == "%d" % is_called
            lod_line = [l for l in open(prefix + ".lod.bedgraph").read().splitlines() if l.split("\t")[2] == "%d" % v.pos][0]
            assert f[17] == lod_line.split("\t")[3]
            if t is not None:
                assert len(carries[i]) == s["V1"]
                called += is_called
    return called


def test_cli_equals_the_tool_workflow_on_the_synthetic_bam(engine0, tmp_path):
    bam, fa, loci, P = _synth(str(tmp_path))
    variants = SR.pick_positions(bam, fa, loci[16:32], 3)
    assert _contract(engine0, tmp_path, bam, fa, loci, P, variants, (0.2, 0.05)) >= 1


def test_cli_equals_the_tool_workflow_on_bam_cigars(engine0, tmp_path):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    _contract(engine0, tmp_path, bam, fa, loci, P, SR.pick_positions(bam, fa, loci, 3), (0.3, 0.1))
