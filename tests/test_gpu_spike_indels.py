"""--spikeIndels on the GPU: smc_spike_indels against the restatement over the file's records (tests/spike_indel_restate.py) - records
field for field, every record's pairs and CIGAR words through its offsets, the offsets themselves, NM', n_indel', statistics and
totals; thresholds 0 and 2^32, a capacity one short, the entry's refusals, SNVs only against smc_spike_alleles, the plane builder on
the copy."""
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import abi, bamio, devplanes
from smcounter_amd.engine import DevBuf
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import spike_indel_restate as IR  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 20240607
T = 0.5


def _synth(tmp):
    """About 300 reads per locus, 100 barcodes at a locus, 900 loci: a few thousand alignments - a dozen workgroups, so the scan crosses
    the workgroups' sums."""
    cfg = dataclasses.replace(R.SYNTH_CFG, n_umi=100, rpb=3)
    bam, fa, loci, P, A = R.synth_bam(tmp, cfg, 900)
    return bam, fa, loci, P


def _inputs(name, tmp):
    """-> (bam, fasta, loci, VcParams, variants)."""
    if name == "case":
        return IR.make_case(tmp)
    if name == "synth":
        bam, fa, loci, P = _synth(tmp)
        return bam, fa, loci, P, IR.pick_variants(bam, fa, loci[100:260], 4)
    bam, fa, loci, P = ds_restate.load_fixture(name, tmp)
    return bam, fa, loci, P, IR.pick_variants(bam, fa, loci, 4, gap=8)


class Run(object):
    """A decoded run in HBM with what smc_spike_indels takes beside it."""

    def __init__(self, eng, bam_path, chrom, lo, hi, P):
        self.eng, self.P = eng, P
        self.nat, self.py = bamio.NativeBam(bam_path), bamio.BamFile(bam_path)
        self.A = self.nat.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
        assert self.A["nl"] == hi - lo
        self.recs = self.py.fetch(chrom, lo, hi)
        self.idents = self.nat.barcode_idents(self.A["n_bc"])
        self.nm, self.n_indel = self.nat.run_mismatches(len(self.A["aln"]))
        self.up = devplanes.upload_run(eng, self.A, "A" * self.A["nl"])

    def spike(self, variants, thr, caps=None, keep=False):
        """-> dict(aln, bq, cig (the copies, whole capacity), nm, n_indel, stats (in the order of `variants`), totals, caps)."""
        A, n = self.A, len(self.A["aln"])
        var, ins, order = devplanes.spike_indel_variants(variants, thr)
        cap = caps or devplanes.spike_indel_caps(A, var)
        out, stats, totals, nm, n_indel = devplanes.spike_indel_run(self.eng, self.up, A, var, ins, self.idents, SEED, self.P.mismatchThr, self.nm,
                                                                    self.n_indel, caps=caps)
        try:
            got = dict(aln=out.aln.download(abi.DEV_ALN_DTYPE, n), bq=out.bq.download(np.uint8, 2 * cap[0] + 64),
                       cig=out.cig.download(np.uint32, cap[1] + 16), nm=nm, n_indel=n_indel, totals=totals, caps=cap)
        finally:
            if not keep:
                out.aln.free(); out.bq.free(); out.cig.free()
        if keep:
            got["dev"] = out
        st = np.zeros_like(stats)
        st[order] = stats
        got["stats"] = st
        # the run itself is only read
        assert self.up.aln.download(abi.DEV_ALN_DTYPE, n).tobytes() == A["aln"].tobytes()
        assert self.up.bq.download(np.uint8, len(A["bq"])).tobytes() == A["bq"].tobytes()
        assert self.up.cig.download(np.uint32, len(A["cig"])).tobytes() == A["cig"].tobytes()
        return got

    def close(self):
        self.up.free()
        self.nat.close(); self.py.close()


def _assert_copy(got, want, A):
    """The copy is the restated one: records field for field, each record's pairs and words through its offsets, the pools whole."""
    n_pairs, n_cw = want["totals"]
    assert [int(x) for x in got["totals"]] == [n_pairs, n_cw, 0]
    for f in abi.DEV_ALN_DTYPE.names:
        assert np.array_equal(got["aln"][f], want["aln"][f]), f
    for i in range(len(want["aln"])):
        g, w = got["aln"][i], want["aln"][i]
        so, ls, co, nc = int(w["seq_off"]), int(w["l_seq"]), int(w["cig_off"]), int(w["n_cig"])
        assert got["bq"][2 * so:2 * (so + ls)].tobytes() == want["bq"][2 * so:2 * (so + ls)].tobytes(), i
        assert got["cig"][co:co + nc].tolist() == want["cig"][co:co + nc].tolist(), i
    assert got["bq"][:2 * n_pairs].tobytes() == want["bq"].tobytes() and got["cig"][:n_cw].tobytes() == want["cig"].tobytes()
    assert np.array_equal(got["nm"], want["nm"]) and np.array_equal(got["n_indel"], want["n_indel"])
    # the relocated records stand behind the run's own, in alignment order, densely
    at_p, at_c = len(A["bq"]) // 2, len(A["cig"])
    for i in want["relocated"]:
        assert (int(got["aln"]["seq_off"][i]), int(got["aln"]["cig_off"][i])) == (at_p, at_c)
        at_p, at_c = at_p + int(got["aln"]["l_seq"][i]), at_c + int(got["aln"]["n_cig"][i])
    assert (at_p, at_c) == (n_pairs, n_cw)
    moved = np.flatnonzero((got["aln"]["seq_off"] != A["aln"]["seq_off"]) | (got["aln"]["cig_off"] != A["aln"]["cig_off"])).tolist()
    assert moved == want["relocated"]


@pytest.mark.parametrize("name", ("case", "bam_cigars", "synth"))
def test_kernel_equals_the_restatement(engine0, tmp_path, name):
    bam_path, fa, loci, P, variants = _inputs(name, str(tmp_path))
    relocated = 0
    for chrom, lo, hi in ds_restate.stretches(loci):
        vs = [v for v in variants if v.chrom == chrom and lo < v.pos <= hi]
        if not vs:
            continue
        run = Run(engine0, bam_path, chrom, lo, hi, P)
        try:
            thr = sv.threshold(T)
            records, stats = IR.restate(bam_path, vs, thr, SEED, P.mismatchThr, fa)
            want = IR.expected_run(run.A, run.recs, records, run.nm, run.n_indel)
            got = run.spike(vs, thr)
            _assert_copy(got, want, run.A)
            # every listed position is a locus of the run: every record that spans it is in the run, the statistics are the file's
            assert got["stats"][:, 0].tolist() == [s["READS"] for s in stats] and got["stats"][:, 1].tolist() == [s["NMINC"] for s in stats]
            assert got["totals"][0] <= got["caps"][0] and got["totals"][1] <= got["caps"][1]
            relocated += len(want["relocated"])
            if name == "synth":
                assert len(run.A["aln"]) > 3 * 256 and len(want["relocated"]) > 50
                blocks = {i // 256 for i in want["relocated"]}
                assert len(blocks) >= 3                              # offsets that start from a workgroup's scanned, non-zero sum
            if name == "case":
                assert {af.SNV, af.INS, af.DEL} == {v.kind for v in vs}
                assert int(((got["aln"]["oflag"] ^ run.A["aln"]["oflag"]) & IR.MMOK != 0).sum()) > 0       # the shorter l_seq flipped the bit
            # two calls give identical results
            again = run.spike(vs, thr)
            for k in ("aln", "bq", "cig", "nm", "n_indel", "stats", "totals"):
                assert np.asarray(again[k]).tobytes() == np.asarray(got[k]).tobytes(), k
        finally:
            run.close()
    assert relocated > 0


def _case_run(engine0, tmp_path):
    bam_path, fa, loci, P, variants = IR.make_case(str(tmp_path))
    (chrom, lo, hi), = ds_restate.stretches(loci)
    return Run(engine0, bam_path, chrom, lo, hi, P), bam_path, fa, P, variants


def test_thresholds_zero_and_all(engine0, tmp_path):
    run, bam_path, fa, P, variants = _case_run(engine0, tmp_path)
    try:
        A = run.A
        got = run.spike(variants, 0)
        assert got["aln"].tobytes() == A["aln"].tobytes() and not got["stats"].any()
        assert [int(x) for x in got["totals"]] == [len(A["bq"]) // 2, len(A["cig"]), 0]
        assert got["bq"][:len(A["bq"])].tobytes() == A["bq"].tobytes() and got["cig"][:len(A["cig"])].tobytes() == A["cig"].tobytes()
        assert np.array_equal(got["nm"], run.nm) and np.array_equal(got["n_indel"], run.n_indel)
        records, stats = IR.restate(bam_path, variants, 1 << 32, SEED, P.mismatchThr, fa)
        assert all(s["S"] == s["N"] for s in stats)
        got = run.spike(variants, 1 << 32)
        _assert_copy(got, IR.expected_run(A, run.recs, records, run.nm, run.n_indel), A)
        assert got["stats"][:, 0].tolist() == [s["READS"] for s in stats] and all(s["READS"] > 0 for s in stats)
    finally:
        run.close()


def test_a_capacity_one_short_sets_the_status_bit_and_nothing_is_written_past_it(engine0, tmp_path):
    run, bam_path, fa, P, variants = _case_run(engine0, tmp_path)
    try:
        thr = sv.threshold(T)
        full = run.spike(variants, thr)
        need_p, need_c = int(full["totals"][0]), int(full["totals"][1])
        assert need_p > len(run.A["bq"]) // 2 and need_c > len(run.A["cig"])
        exact = run.spike(variants, thr, caps=(need_p, need_c))
        assert int(exact["totals"][2]) == 0 and exact["aln"].tobytes() == full["aln"].tobytes()
        for caps in ((need_p - 1, need_c), (need_p, need_c - 1)):
            got = run.spike(variants, thr, caps=caps)
            assert [int(x) for x in got["totals"]] == [need_p, need_c, 1]
            assert (got["aln"]["seq_off"].astype(np.int64) + got["aln"]["l_seq"]).max() <= caps[0]
            assert (got["aln"]["cig_off"].astype(np.int64) + got["aln"]["n_cig"]).max() <= caps[1]
            # what fits is the full copy's; the record that does not is the run's own
            short = np.flatnonzero(got["aln"]["seq_off"] != full["aln"]["seq_off"]).tolist()
            assert len(short) == 1 and got["aln"][short[0]]["seq_off"] == run.A["aln"][short[0]]["seq_off"]
            assert got["bq"][:2 * int(full["aln"]["seq_off"][short[0]])].tobytes() == full["bq"][:2 * int(full["aln"]["seq_off"][short[0]])].tobytes()
    finally:
        run.close()


def test_nothing_is_stored_beyond_the_capacities(engine0, tmp_path):
    """The pools handed over are filled with a pattern beyond the capacity; the call with capacities one short leaves it there."""
    import ctypes
    from smcounter_amd import _lib
    run, bam_path, fa, P, variants = _case_run(engine0, tmp_path)
    eng = engine0
    try:
        thr = sv.threshold(T)
        full = run.spike(variants, thr)
        need_p, need_c = int(full["totals"][0]), int(full["totals"][1])
        A, n = run.A, len(run.A["aln"])
        var, ins, _ = devplanes.spike_indel_variants(variants, thr)
        up8 = lambda a: DevBuf(eng, a.nbytes + 256).upload(a.view(np.uint8).reshape(-1))
        bufs = [up8(var), up8(run.idents[:int(A["n_bc"])]), up8(np.ascontiguousarray(run.nm, np.int32)), up8(np.ascontiguousarray(run.n_indel, np.int32)),
                up8(ins)]
        for cap_p, cap_c in ((need_p - 1, need_c), (need_p, need_c - 1), (need_p, need_c)):
            outs = [DevBuf(eng, 36 * n + 256), DevBuf(eng, 2 * need_p + 512), DevBuf(eng, 4 * need_c + 512), DevBuf(eng, 4 * n + 256),
                    DevBuf(eng, 4 * n + 256), DevBuf(eng, 8 * len(var) + 256), DevBuf(eng, 256)]
            outs[1].upload(np.full(2 * need_p + 512, 0x5A, np.uint8)); outs[2].upload(np.full(4 * need_c + 512, 0x5A, np.uint8))
            _lib.check(eng.L.smc_spike_indels(eng.ctx, run.up.aln.data_ptr(), n, run.up.cig.data_ptr(), len(A["cig"]), run.up.bq.data_ptr(),
                                              len(A["bq"]) // 2, bufs[0].data_ptr(), var.ctypes.data, len(var), bufs[4].data_ptr(), len(ins),
                                              bufs[1].data_ptr(), int(A["n_bc"]), ctypes.c_uint64(SEED), float(P.mismatchThr), bufs[2].data_ptr(),
                                              bufs[3].data_ptr(), cap_p, cap_c, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                              outs[3].data_ptr(), outs[4].data_ptr(), outs[5].data_ptr(), outs[6].data_ptr(), None), "smc_spike_indels")
            bq, cig = outs[1].download(np.uint8, 2 * need_p + 512), outs[2].download(np.uint8, 4 * need_c + 512)
            totals = outs[6].download(np.uint64, 3)
            assert int(totals[2]) == (0 if (cap_p, cap_c) == (need_p, need_c) else 1)
            assert (bq[2 * cap_p:] == 0x5A).all() and (cig[4 * cap_c:] == 0x5A).all()
            for b in outs:
                b.free()
        for b in bufs:
            b.free()
    finally:
        run.close()


def test_snvs_only_equal_smc_spike_alleles_byte_for_byte(engine0, tmp_path):
    run, bam_path, fa, P, variants = _case_run(engine0, tmp_path)
    try:
        A = run.A
        snvs = [IR.variant(v.chrom, v.pos, v.ref[0], "ACGT"[("ACGT".index(v.ref[0]) + 1) % 4]) for v in variants]
        thr = sv.threshold(T)
        got = run.spike(snvs, thr)
        svar = np.zeros(len(snvs), abi.SPIKE_VARIANT_DTYPE)
        for k, v in enumerate(snvs):
            svar[k]["pos0"], svar[k]["ref"], svar[k]["alt"], svar[k]["thr"] = v.pos - 1, ord(v.ref), ord(v.alt), thr
        out, stats = devplanes.spike_run(engine0, run.up, A, svar, run.idents, SEED, P.mismatchThr, run.nm, run.n_indel)
        try:
            aln, bq = out.aln.download(abi.DEV_ALN_DTYPE, len(A["aln"])), out.bq.download(np.uint8, len(A["bq"]))
        finally:
            out.aln.free(); out.bq.free()
        assert got["aln"].tobytes() == aln.tobytes() and got["bq"][:len(A["bq"])].tobytes() == bq.tobytes() and stats.any()
        assert np.array_equal(got["stats"], stats) and [int(x) for x in got["totals"]] == [len(A["bq"]) // 2, len(A["cig"]), 0]
        assert got["cig"][:len(A["cig"])].tobytes() == A["cig"].tobytes()
    finally:
        run.close()


def test_refusals_launch_nothing(engine0):
    eng = engine0
    n = 8
    ok = np.zeros(3, abi.SPIKE_INDEL_VARIANT_DTYPE)
    ok["pos0"], ok["kind"], ok["ref"], ok["alt"], ok["len"], ok["thr"] = [5, 9, 20], [0, 1, 2], ord("A"), [ord("G"), ord("A"), ord("A")], [0, 2, 3], 1 << 31
    bufs = [DevBuf(eng, 4096).upload(np.full(4096, 0x5A, np.uint8)) for _ in range(7)]   # aln, bq, cig, nm, n_indel, stats, totals
    src = DevBuf(eng, 4096).upload(np.zeros(4096, np.uint8))

    def call(var, n_ins=2, caps=(100, 100)):
        d_var = DevBuf(eng, var.nbytes + 256).upload(np.ascontiguousarray(var).view(np.uint8).reshape(-1))
        rc = eng.L.smc_spike_indels(eng.ctx, src.data_ptr(), n, src.data_ptr(), 32, src.data_ptr(), 64, d_var.data_ptr(), var.ctypes.data, len(var),
                                    src.data_ptr(), n_ins, src.data_ptr(), 4, 7, 6.0, src.data_ptr(), src.data_ptr(), caps[0], caps[1],
                                    *([b.data_ptr() for b in bufs] + [None]))
        d_var.free()
        return rc

    def edit(**kw):
        v = ok.copy()
        for k, (i, x) in kw.items():
            v[k][i] = x
        return v
    for var, kw, msg in ((edit(pos0=(1, 5)), {}, "not strictly ascending"), (edit(ref=(0, ord("N"))), {}, "outside ACGT"),
                         (edit(alt=(0, ord("A"))), {}, "ref equals alt"), (edit(alt=(1, ord("C"))), {}, "anchor"),
                         (edit(thr=(2, (1 << 32) + 1)), {}, "above 2^32"), (edit(kind=(1, 3)), {}, "has kind 3"),
                         (edit(len=(1, 0)), {}, "a length of 0"), (edit(len=(2, 256)), {}, "a length of 256"), (edit(len=(0, 1)), {}, "a length of 1"),
                         (ok, dict(n_ins=1), "inserted letters"), (edit(ins_off=(1, 1)), {}, "inserted letters"),
                         (edit(pos0=(2, 10)), {}, "footprint overlaps"),            # the deletion's anchor in the insertion's footprint [9, 10]
                         (edit(pos0=(0, 6), kind=(0, 2), alt=(0, ord("A")), len=(0, 2)), {}, "footprint overlaps"),   # [6, 9] holds the anchor 9
                         (ok, dict(caps=(63, 100)), "capacities"), (ok, dict(caps=(100, 31)), "capacities"), (ok, dict(caps=(1 << 32, 100)), "capacities")):
        assert call(var, **kw) < 0 and msg.encode() in eng.L.smc_last_error(), msg
    big = np.zeros(4097, abi.SPIKE_INDEL_VARIANT_DTYPE)
    assert call(big) < 0 and b"at most 4096" in eng.L.smc_last_error()
    eng.L.smc_device_sync(eng.ctx)
    for b in bufs:
        assert (b.download(np.uint8, 4096) == 0x5A).all()                              # nothing copied, nothing launched
    for b in bufs + [src]:
        b.free()


def test_build_planes_on_the_copy_equals_the_builder_on_the_tools_bam(engine0, tmp_path):
    """The copy through smc_build_planes, called: the rows of the listed loci are those of the run decoded from the BAM the tool wrote
    (whose arrays the test above shows to be the restated ones)."""
    import argparse
    from smcounter_amd import fasta
    bam, fa, loci, P, variants = IR.make_case(str(tmp_path))
    vfile = R.write_variants(str(tmp_path / "v.txt"), variants)
    out = str(tmp_path / "tool.bam")
    sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % T, seed=SEED, refGenome=fa, indels=True))
    bamio.write_bai(out)
    (chrom, lo, hi), = ds_restate.stretches(loci)
    genome = fasta.FastaFile(fa)
    run = Run(engine0, bam, chrom, lo, hi, P)
    nat1 = bamio.NativeBam(out)
    try:
        got = run.spike(variants, sv.threshold(T), keep=True)
        copy = got["dev"]
        try:
            key = devplanes.copy_allele_key(copy, run.A, run.nat.allele_key)
            mine = _build(engine0, run.A, copy, P, chrom, lo, genome, key, run.nat.barcode_name)
        finally:
            devplanes.free_spiked(copy, run.up)
        A1 = nat1.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
        up1 = devplanes.upload_run(engine0, A1, "A" * A1["nl"])
        try:
            want = _build(engine0, A1, up1, P, chrom, lo, genome, nat1.allele_key, nat1.barcode_name)
        finally:
            up1.free()
        assert mine[0].tobytes() == want[0].tobytes() and mine[1] == want[1] and mine[2].tobytes() == want[2].tobytes()
        assert any(len(t) > 6 and any(k.startswith("INS|") for k in t) for t in mine[1])
        assert any(any(k.startswith("DEL|") for k in t) for t in mine[1])
    finally:
        nat1.close()
        run.close()


def _build(eng, A, up, P, chrom, lo, genome, allele_key, barcode_name):
    """smc_build_planes over the arrays `up` of run `A` -> (read words of the run, allele tables, locus descriptors)."""
    nl, ns = A["nl"], A["n_slots"]
    cap = ns + 64
    words = DevBuf(eng, 4 * cap)
    uaux = [DevBuf(eng, 4 * (cap + nl + 8192)) for _ in range(3)]
    run_ref = genome.fetch(chrom, lo, lo + nl).upper()
    d_ref = DevBuf(eng, nl + 256).upload(np.frombuffer(run_ref.encode().ljust(nl, b"\0"), np.uint8).copy())
    with_ref = devplanes.RunOnDevice(up.aln, up.cig, up.bq, up.loc, d_ref, up.n_aln, up.loc_host)
    try:
        done = devplanes.build_run(A, eng.L, eng, abi.c_params(P), P, chrom, lo, genome, run_ref, [words, None, None, None, None], uaux, 0, 0,
                                   cap + nl, eng.L.smc_build_max_depth(), allele_key, barcode_name, uploaded=with_ref)
        assert done is not None and done != devplanes.NARROW
        return words.download(np.uint32, ns), done[3], done[2]
    finally:
        for b in [words, d_ref] + uaux:
            b.free()


@pytest.mark.parametrize("name", ("case", "bam_cigars"))
def test_the_spiked_batches_equal_the_host_builder_on_the_tools_bam(engine0, tmp_path, name):
    """The main pass's spiked batch - smc_spike_indels, then smc_build_planes on the copy, its allele texts from the copy - against
    the HOST builder (smc_bam_planes) on the BAM the tool wrote: descriptors, barcodes, fragments, reads, marks and allele tables by
    planecheck's fingerprint, and the read words against the raw-field planes (test_gpu_devplanes._same_batch)."""
    import argparse
    from smcounter_amd import fasta
    import test_gpu_devplanes as TD
    bam, fa, loci, P, variants = _inputs(name, str(tmp_path))
    vfile = R.write_variants(str(tmp_path / "v.txt"), variants)
    out = str(tmp_path / "tool.bam")
    sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % T, seed=SEED, refGenome=fa, indels=True))
    bamio.write_bai(out)
    genome = fasta.FastaFile(fa)
    text_loci = [(c, "%d" % p) for c, p in loci]
    rule = devplanes.DsRule(1.0, P, seed=SEED, af=T, spike=devplanes.SpikeSet(variants))
    host = list(bamio.iter_device_batches_native(out, genome, text_loci, P))
    plain = list(bamio.iter_device_batches_native(bam, genome, text_loci, P))
    dev = list(devplanes.iter_resident_batches(bam, genome, text_loci, P, engine0, ds_rules=[rule]))
    assert len(host) == len(dev) == len(plain) >= 1
    keys = set()
    for (f1, hb), (f2, (full, spiked)), (_, pb) in zip(host, dev, plain):
        assert f1 == f2
        TD._same_batch(full, pb)                                     # (the full-depth batch beside it is the input's)
        TD._same_batch(spiked, hb)
        assert spiked.n_device_runs >= 1
        keys |= {k for t in hb.alleles for k in t}
    for v in variants:
        if v.kind != af.SNV:
            assert v.key in keys                                     # (the planted alleles went through the extras list of the copy)


def _contract(engine0, tmp_path, bam, fa, loci, P, variants, targets):
    """cli --spikeAF --spikeIndels --lod == a plain cli run on the BAM tools.spike_variants --indels writes, per target; the full-depth
    files those of a run without the flags; the detection page the outputs' own rows and the restatement's numbers; V1 from
    smc_allele_carriers over the tool's BAM."""
    import argparse
    from smcounter_amd import dsaf, fasta, spike
    import test_gpu_lod as TL
    SUFFIXES = TL.SUFFIXES
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = R.write_variants(str(tmp_path / "v.vcf"), variants, vcf=True)
    plain = TL._read(TL._run_cli(tmp_path, "o", bam, fa, bed, P), SUFFIXES)
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=["--lod", "--spikeIndels"], spikeAF=",".join("%g" % t for t in targets),
                      spikeVariants=vfile, dsSeed=SEED)
    assert TL._read(got, SUFFIXES) == plain
    lines = [l.split("\t") for l in open(got + ".spikeAF.detection.txt").read().splitlines()]
    assert lines[0] == list(spike.DETECTION_HEADER) + ["LOD"] and len(lines) == 1 + len(variants) * (1 + len(targets))
    outs = [(None, got)] + [(t, "%s.spikeAF%g" % (got, t)) for t in targets]
    stats = {}
    for t in targets:
        stats[t] = [None] * len(variants)
        for chrom in sorted({v.chrom for v in variants}):
            idx = [k for k, v in enumerate(variants) if v.chrom == chrom]
            for k, s in zip(idx, IR.restate(bam, [variants[k] for k in idx], sv.threshold(t), SEED, P.mismatchThr, fa)[1]):
                stats[t][k] = s
    relocated = 0
    for j, (t, prefix) in enumerate(outs):
        if t is not None:
            out = str(tmp_path / ("spike%g.bam" % t))
            rows_tool = sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=SEED, refGenome=fa, indels=True))
            bamio.write_bai(out)
            ref = TL._run_cli(tmp_path, "o.spikeAF%g" % t, out, fa, bed, P)
            for a, b, s in zip(TL._read(prefix, SUFFIXES), TL._read(ref, SUFFIXES), SUFFIXES):
                assert a == b, "target %g: %s differs" % (t, s)
            _, carries = devplanes.ds_af_sets(out, fasta.FastaFile(fa), variants, P, engine0)
            relocated += sum(r["READS"] for r, v in zip(rows_tool, variants) if v.kind != af.SNV)
        rows, cut = dsaf.read_output(prefix)
        for i, v in enumerate(variants):
            f = lines[1 + i * len(outs) + j]
            key = (v.chrom, "%d" % v.pos)
            s = stats[t if t is not None else targets[0]][i]
            want = [s["N"], s["V0"], 0, 0, s["V0"]] if t is None else [s["N"], s["V0"], s["S"], s["READS"], s["V1"]]
            assert f[:5] == [v.chrom, "%d" % v.pos, v.ref, v.alt, dsaf.target_text(t)]
            assert f[5:11] == ["%d" % x for x in want] + [dsaf.frac_text(want[4] / want[0] if want[0] else 0.0)]
            assert f[11:16] == [rows[key][dsaf._COL[c]] for c in ("UMT", "VMT", "VMF", "PI", "FILTER")]
            assert f[16] == "%d" % int(key in cut and cut[key][0] == v.ref and v.alt in cut[key][1])
            if t is not None:
                assert len(carries[i]) == s["V1"]
    assert relocated > 0


def test_cli_equals_the_tool_workflow_on_the_hand_made_bam(engine0, tmp_path):
    bam, fa, loci, P, variants = IR.make_case(str(tmp_path))
    _contract(engine0, tmp_path, bam, fa, loci, P, variants, (0.5, 0.2))


def test_cli_equals_the_tool_workflow_on_bam_cigars(engine0, tmp_path):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    _contract(engine0, tmp_path, bam, fa, loci, P, IR.pick_variants(bam, fa, loci, 4, gap=8), (0.3, 0.1))
