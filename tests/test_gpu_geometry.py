"""The device plane builders against the reference, read by read: the comparison of tests/test_geometry_ref.py - per parameter set,
locus and allele key what the reference's vc() had tallied (tests/golden/geometry/*.npz) against what the built read words say - for
    smc_build_planes with the raw-field planes (the walk's exact path at every position; the `dist` plane against the reference's
    end-distance lists),
    the words alone in 32 bits and in 16 bits (the walk's byte-lane path on plain rows and on the linearised general CIGARs: the
    end-distance tests from the per-row constants - what the command line runs),
    smc_build_listed over the long run, a tile's first and last loci and the anchors of the boundary indels among the listed,
and, for each, that the device builder took every run itself (nothing fell back to the host builder), in the word width asked for.
The shallow run holds alignments flagged neither READ1 nor READ2: the listed builder declines it by contract - asserted as such."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import bamio, devplanes

sys.path.insert(0, os.path.join(ROOT, "tests"))
import geometry_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = [(name, s) for name in gc.FIXTURES for s in range(len(gc.fixture_sets(name)))]
IDS = ["%s-%s" % (name, gc.set_id(gc.fixture_sets(name)[s])) for name, s in CASES]


@pytest.fixture(scope="module")
def unpacked(tmp_path_factory):
    return {name: gc.load_fixture(name, tmp_path_factory.mktemp(name)) for name in gc.FIXTURES}


def built_and_compared(what, unpacked, name, s, eng, all_planes, bits):
    """The fixture's loci through iter_resident_batches -> the word widths used.  Every batch is compared with the reference and has
    been built by the device builder alone."""
    bam, fa, loci, meta = unpacked[name]
    t = tuple(meta["sets"][s]["params"])
    seen, widths, n = set(), set(), 0
    eng.word_bits = bits
    try:
        for first, rb in devplanes.iter_resident_batches(bam, fa, loci, gc.params_of(t), eng, max_reads=20_000, nthreads=2, all_planes=all_planes):
            assert rb.n_device_runs >= 1 and rb.n_host_runs == 0, "%s: a run went to the host builder" % what
            wb = rb.words.word_bits
            words = rb.words.download(np.uint16 if wb == 16 else np.uint32, rb.n_slots)
            if wb == 16:
                words = devplanes.words32_from_16(words)
            us = rb.planes[4].download(np.uint32, rb.n_ustart)
            m = d = None
            if all_planes:
                db = rb.to_host()
                m, d = db.meta, db.dist
                assert np.array_equal(words, devplanes.pack_words_host(db.meta, db.frag, db.loci))
            gc.assert_equal(gc.compare_batch(what, meta, s, first, rb.loci, words, us, rb.alleles, m, d))
            seen |= gc.classes_seen(words)
            widths.add(wb)
            n += rb.n_loci
    finally:
        eng.word_bits = 16
    assert n == len(loci)
    assert seen == set(range(22)) - set(meta["sets"][s]["unreachable"])
    return widths


@pytest.mark.parametrize("name,s", CASES, ids=IDS)
def test_exact_path_with_all_planes(name, s, unpacked, engine0):
    assert built_and_compared("smc_build_planes, all planes", unpacked, name, s, engine0, True, 16) == {32}


@pytest.mark.parametrize("name,s", CASES, ids=IDS)
def test_words_only_in_32_bits(name, s, unpacked, engine0):
    assert built_and_compared("smc_build_planes, words only, 32 bits", unpacked, name, s, engine0, False, 32) == {32}


@pytest.mark.parametrize("name,s", CASES, ids=IDS)
def test_words_only_in_16_bits(name, s, unpacked, engine0):
    """The product's path.  Every locus stays below 16 allele ids and every quality at or below 63, so no run is built again in 32
    bits; smc_build_planes_w16 wants minBQ in 0 .. 63 (include/smcounter_hip.h), so the sets with minBQ 64 are built in 32 bits."""
    min_bq = unpacked[name][3]["sets"][s]["params"][1]
    widths = built_and_compared("smc_build_planes_w16", unpacked, name, s, engine0, False, 16)
    assert widths == ({16} if min_bq <= 63 else {32})


@pytest.mark.parametrize("name,s", CASES, ids=IDS)
def test_listed_builder(name, s, unpacked, engine0):
    """smc_build_listed over every locus of the long run, 64 listed loci a call (a tile's first and last locus, the insertion behind a
    tile's last locus and the deletion across a tile boundary are among them in every call that covers a tile), in 16-bit words
    where minBQ allows and in 32-bit ones; the shallow run, which holds unflagged alignments, is declined with its status bit."""
    import test_gpu_build_listed as tl
    bam_path, fa, loci, meta = unpacked[name]
    t = tuple(meta["sets"][s]["params"])
    P = gc.params_of(t)
    bam = bamio.NativeBam(bam_path)
    try:
        for (lo, hi), declined in ((gc.RUN_A, False), (gc.RUN_B, True)):
            first = loci.index((gc.CHROM, str(lo + 1)))
            A = bam.alignments_run(gc.CHROM, lo, hi, 1_000_000, P, 2)
            nl = A["nl"]
            assert nl == hi - lo and bool(A["status"] & 1) == declined
            up = devplanes.upload_run(engine0, A, fa.fetch(gc.CHROM, lo, hi).upper())
            try:
                for bits in ((16, 32) if t[1] <= 63 else (32,)):
                    for g0 in range(0, nl, devplanes.LISTED_MAX_LOCI):
                        offsets = list(range(g0, min(nl, g0 + devplanes.LISTED_MAX_LOCI)))
                        caps = [tl.align4(A["loc"]["n"][a]) for a in offsets]
                        Lb = tl.Listed(engine0, [(up, tl.counts_of(A))], up.ref, lo, nl, offsets, caps, P, bits, 0, xcap=1024)
                        status = int(Lb.counters[0, 1])
                        if declined:
                            assert status & tl.ST_UNFLAGGED, "the listed builder took a run with unflagged alignments (status %d)" % status
                            continue
                        assert status == 0 and int(Lb.counters[0, 0]) <= Lb.xcap
                        xl = Lb.x[0, :int(Lb.counters[0, 0])]
                        tables = [devplanes.extras_table(xl, a, bam.allele_key, gc.CHROM, lo, fa) for a in offsets]
                        words = devplanes.words32_from_16(Lb.words) if bits == 16 else Lb.words
                        gc.assert_equal(gc.compare_batch("smc_build_listed, %d bits" % bits, meta, s, first + g0, Lb.loci[:len(offsets)], words, Lb.us, tables))
            finally:
                up.free()
    finally:
        bam.close()
