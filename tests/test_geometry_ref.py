"""The host plane builders against the reference, read by read (tests/golden/geometry/*.npz, made by make_geometry_golden.py in the
build container): the bytes of a BAM of constructed records (tests/geometry_cases.py) and, for every parameter set and target locus,
what the REFERENCE ITSELF had tallied per allele key when vc() returned - alleleCnt, r1Cnt, r2Cnt, forwardCnt, reverseCnt, lowQReads,
bqSum, the three end-distance lists, the barcodes and fragments of allBcDict, cvg.  A builder's read words say the same through the
read class (tests/geometry_tallies.py restates them from the class table of include/smcounter_hip.h), its `dist` plane holds the
distances themselves:
    the readable Python decoder -> features.extract_features;
    the native decoder -> smc_bam_planes.
Every key, count and distance has to be equal - a read on the wrong side of `<= 20`, of `<= primerDist`, of minBQ, minMQ or
mismatchThr, or with the wrong leftSP, changes one.  The device builders: tests/test_gpu_geometry.py."""
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import bamio, devplanes, features, pileup

sys.path.insert(0, os.path.join(ROOT, "tests"))
import geometry_cases as gc  # noqa: E402

CASES = [(name, s) for name in gc.FIXTURES for s in range(len(gc.fixture_sets(name)))]
IDS = ["%s-%s" % (name, gc.set_id(gc.fixture_sets(name)[s])) for name, s in CASES]


@pytest.fixture(scope="module")
def unpacked(tmp_path_factory):
    """name -> (bam, fasta, loci, meta, the Python decoder's pileup of all loci)"""
    out = {}
    for name in gc.FIXTURES:
        bam, fa, loci, meta = gc.load_fixture(name, tmp_path_factory.mktemp(name))
        pb = pileup.concat([b for _, b in bamio.iter_pileup_batches(bamio.BamFile(bam), fa, loci)])
        out[name] = (bam, fa, loci, meta, pb)
    return out


@pytest.mark.parametrize("name", gc.FIXTURES)
def test_fixture_states_its_coverage(name, unpacked):
    """The stored fixture is the one the cases describe, and says what it covers: the parameter sets, every value of the issue's
    lists at least twice; per set the classes that occur (the 22 minus the ones the set cannot reach), the barcode-end distances
    19, 20, 21 per (mate, strand) and the primer-end distances around primerDist for read 2."""
    bam, fa, loci, meta, pb = unpacked[name]
    sets = [tuple(s["params"]) for s in meta["sets"]]
    assert sets == list(gc.PARAM_SETS) and len(sets) >= 8 and loci == gc.loci()
    for col, values in enumerate(((0, 1, 2, 19, 20, 21, 60, 200, 100000), (0, 1, 20, 41, 63, 64), (0, 30, 60, 61, 255), (6.0, 100.0))):
        for v in values:
            assert sum(t[col] == v for t in sets) >= 2, (col, v)
    assert os.path.getsize(os.path.join(gc.GOLDEN, name + ".npz")) < 256 * 1024
    assert int(pb.bq.max()) <= 63 and max(len(t) for t in pb.alleles) <= 16
    assert max(c["cvg"] for c in meta["captures"][0]) > 256 and meta["shape"]["deepest_tile_rows"] > 256
    lo, hi = gc.RUN_A
    assert hi - lo >= 200 and gc.RUN_B[1] - gc.RUN_B[0] < 64
    for t, s, cov in zip(sets, meta["sets"], meta["coverage"]):
        assert s["unreachable"] == gc.unreachable_classes(t) == cov["unreachable"]
        assert sorted(cov["classes"] + cov["unreachable"]) == list(range(22))
        if t[1] <= 63:
            assert sorted(cov["bc_end"]) == ["R1fwd", "R1rev", "R2fwd", "R2rev"] and all(v == [19, 20, 21] for v in cov["bc_end"].values())
            for name_, first in (("R2fwd", 0), ("R2rev", 1)):
                assert cov["primer_end"][name_] == [d for d in (t[0] - 1, t[0], t[0] + 1) if first <= d <= 150 + first]
        else:
            assert cov["bc_end"] == {} and cov["primer_end"] == {}      # (minBQ 64: no base is included)


@pytest.mark.parametrize("name,s", CASES, ids=IDS)
def test_python_decoder_and_extract_features_tally_what_the_reference_tallies(name, s, unpacked):
    bam, fa, loci, meta, pb = unpacked[name]
    t = tuple(meta["sets"][s]["params"])
    db = features.extract_features(pb, gc.params_of(t))
    words = devplanes.pack_words_host(db.meta, db.frag, db.loci)
    gc.assert_equal(gc.compare_batch("bamio (Python) -> extract_features", meta, s, 0, db.loci, words, db.umi_start, db.alleles, db.meta, db.dist))
    assert gc.classes_seen(words) == set(range(22)) - set(meta["sets"][s]["unreachable"])


@pytest.mark.parametrize("name,s", CASES, ids=IDS)
def test_native_decoder_and_host_builder_tally_what_the_reference_tallies(name, s, unpacked):
    bam, fa, loci, meta, pb = unpacked[name]
    t = tuple(meta["sets"][s]["params"])
    seen, n = set(), 0
    for first, db in bamio.iter_device_batches_native(bam, fa, loci, gc.params_of(t), max_reads=20_000, nthreads=2):
        words = devplanes.pack_words_host(db.meta, db.frag, db.loci)
        gc.assert_equal(gc.compare_batch("native decoder -> smc_bam_planes", meta, s, first, db.loci, words, db.umi_start, db.alleles, db.meta, db.dist))
        seen |= gc.classes_seen(words)
        n += db.n_loci
    assert n == len(loci)
    assert seen == set(range(22)) - set(meta["sets"][s]["unreachable"])
