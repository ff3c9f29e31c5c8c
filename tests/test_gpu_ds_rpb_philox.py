"""--dsRpbSampler philox on the GPU: the file-wide read-name table (smc_read_groups_*) against the host restatement
(tests/ds_rpb_philox_restate.py) - counters, first names, kept names per target, per-run masks -, its collision reports, and the
command line against a plain run with --rpb r on a BAM that holds exactly the restated kept names."""
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import bamio, cli, devplanes

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import ds_rpb_philox_restate as rp  # noqa: E402

pytestmark = pytest.mark.gpu
FIXTURES = ("case", "bam_cigars", "bam_overcap", "bam_deep")
SEED = 1234567


def _fixture(name, tmp):
    return ds_restate.make_case(tmp) if name == "case" else ds_restate.load_fixture(name, tmp)


def _unpack(words, n_ids, n_masks):
    w = words.reshape(n_masks, -1)
    return [np.unpackbits(w[t].view(np.uint8), bitorder="little")[:n_ids].astype(bool) for t in range(n_masks)]


def _masks(eng, groups, idents, seed, thr):
    from smcounter_amd.engine import DevBuf
    n = len(idents)
    n_words = (n + 31) // 32
    d_id = DevBuf(eng, 8 * max(1, n) + 256).upload(np.ascontiguousarray(idents, np.uint64) if n else np.zeros(1, np.uint64))
    d_m = DevBuf(eng, 4 * max(1, n_words * len(thr)) + 256)
    groups.masks(d_id.data_ptr(), n, seed, thr, d_m.data_ptr())
    words = d_m.download(np.uint32, n_words * len(thr))
    d_id.free(); d_m.free()
    return _unpack(words, n, len(thr))


def _check_table(eng, path, qn, chunk, targets):
    """The table built from the file pass in chunks of `chunk` records == the restatement: counters, first names (a mask at thr 0),
    the kept names of every target (masks and kept counts)."""
    g = rp.restate(qn, targets, SEED)
    groups = devplanes.ReadGroups(eng)
    try:
        bam = bamio.NativeBam(path)
        n_chunks = 0
        for first, keys in bam.name_keys(chunk, 4):
            groups.add(keys, first)
            n_chunks += 1
        bam.close()
        assert n_chunks == (len(qn) + chunk - 1) // chunk
        c = groups.finish()
        assert groups.status() == 0
        assert c == g["counts"], (c, g["counts"])
        thr = [0] + g["thr"] + [1 << 32]
        m = _masks(eng, groups, g["ident"], SEED, thr)
        assert np.array_equal(m[0], g["first"])
        for k in range(len(targets)):
            assert np.array_equal(m[k + 1], g["keep"][k]), targets[k]
        assert m[-1].all() and groups.status() == 0
        assert groups.kept(SEED, g["thr"]) == [int(k.sum()) for k in g["keep"]]
    finally:
        groups.close()
    return g


@pytest.mark.parametrize("name", FIXTURES)
def test_table_equals_the_restatement_on_the_fixtures(engine0, tmp_path, name):
    path = _fixture(name, str(tmp_path))[0]
    qn = ds_restate.placed_qnames(path)
    for chunk in (1 << 20, 7):
        g = _check_table(engine0, path, qn, chunk, (1.0, 1.5, 2.0, 4.0, 50.0))
    assert any(0 < k.sum() - g["first"].sum() < len(k) - g["first"].sum() for k in g["keep"])      # (some target draws)


def test_table_equals_the_restatement_on_a_million_records(engine0, tmp_path):
    path = str(tmp_path / "names.bam")
    qn = rp.write_names_bam(path, 1_050_000)
    g1 = _check_table(engine0, path, qn, 1 << 22, (1.5, 2.0, 3.0))
    g2 = _check_table(engine0, path, qn, 100_003, (1.5, 2.0, 3.0))
    assert g1["counts"]["records"] >= 1_000_000 and g1["counts"] == g2["counts"]


def _keys(rows):
    """[(name id, barcode id, name check, barcode check)] -> smc_read_key rows."""
    return np.array([(n, b, nc | bc << 32) for n, b, nc, bc in rows], np.uint64)


def test_collisions_and_misses_set_the_status(engine0):
    eng = engine0

    def status(rows, look=None):
        groups = devplanes.ReadGroups(eng)
        try:
            groups.add(_keys(rows), 0)
            groups.finish()
            if look is not None:
                _masks(eng, groups, np.array(look, np.uint64), SEED, [1 << 31])
            return groups.status()
        finally:
            groups.close()
    ok = [(11, 100, 1, 7), (12, 100, 2, 7), (13, 101, 3, 8), (11, 100, 1, 7)]
    assert status(ok) == 0
    assert status(ok, look=[11, 12, 13]) == 0
    # one name identity, two check words: two names behind one identity
    assert status(ok + [(12, 100, 9, 7)]) == devplanes.RG_NAME_COLLISION
    # one name identity and check word with two barcodes: the same
    assert status(ok + [(13, 100, 3, 7)]) == devplanes.RG_NAME_COLLISION
    # one barcode identity, two check words
    assert status(ok + [(14, 101, 4, 5)]) == devplanes.RG_BARCODE_COLLISION
    # an identity the table does not hold, in a run's lookup
    assert status(ok, look=[11, 99]) == devplanes.RG_MISS
    # identity 0 marks an empty slot
    assert status(ok + [(0, 100, 4, 7)]) & devplanes.RG_RESERVED


@pytest.mark.parametrize("name", FIXTURES)
def test_run_masks_are_the_restated_kept_names(engine0, tmp_path, name):
    bam_path, _, loci, P = _fixture(name, str(tmp_path))
    targets = (1.5, 2.0, 4.0)
    rules = devplanes.philox_read_rules(bam_path, targets, [P] * len(targets), SEED, engine0, chunk=13)
    try:
        g = rp.restate(ds_restate.placed_qnames(bam_path), targets, SEED)
        assert [r.prob_keep for r in rules] == g["probs"] and [r.thr for r in rules] == g["thr"]
        assert [r.n_kept for r in rules] == [len(k) for k in g["kept"]] and all(r.groups is rules[0].groups for r in rules)
        assert [r.sampler for r in rules] == ["philox"] * 3 and rules[0].n_names == g["counts"]["names"]
        bam = bamio.NativeBam(bam_path)
        for chrom, lo, hi in ds_restate.stretches(loci):
            A = bam.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
            idents, shared = bam.pair_idents(A["n_pair"])
            assert not shared
            buf, n_words, index = devplanes._run_read_masks(engine0, rules[0].groups, rules, idents, chrom, lo, A["nl"])
            m = _unpack(buf.download(np.uint32, n_words * len(rules)), len(idents), len(rules))
            buf.free()
            names = [bam.pair_name(k) for k in range(int(A["n_pair"]))]
            for rule, kept in zip(rules, g["kept"]):
                assert np.array_equal(m[index[id(rule)]], np.array([q in kept for q in names], bool)), rule.target
        bam.close()
    finally:
        devplanes.close_rules(rules)


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


def write_names_kept_bam(src, dst, kept):
    """The placed records of `src` whose full read name is in `kept` -> dst, indexed."""
    header, recs = bamio.iter_raw_records(src)
    bamio.write_raw(dst, header, (raw for tid, q, raw in recs if tid >= 0 and q in kept))
    bamio.write_bai(dst)
    return dst


def _reference(tmp, bam_path, fa, bed, P, r, kept, tag):
    ds_bam = write_names_kept_bam(bam_path, str(tmp / ("kept%g.bam" % r)), kept)
    return _files(_run_cli(tmp, tag, ds_bam, fa, bed, dataclasses.replace(P, rpb=r)))


CASES = [(n, None) for n in FIXTURES] + [("bam_deep", 40)]


@pytest.mark.parametrize("name,max_mt", CASES)
def test_cli_philox_equals_a_run_on_the_kept_names(tmp_path, name, max_mt):
    """Every file byte for byte against a plain run with --rpb r on a BAM of the restated kept names; the same with runs cut small
    (--batchReads); the full-depth files unchanged.  (bam_deep at --maxMT 40: every locus over the barcode cap - the renumbered ids
    reach the cap sampler's texts through the old ids.)  Each reference run writes under the prefix of the file it is compared with
    (the VCF header names it), after that file has been read."""
    bam_path, fa, loci, P = _fixture(name, str(tmp_path))
    if max_mt:
        P = dataclasses.replace(P, maxMT=max_mt)
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    targets = (2.0, 4.0)
    g = rp.restate(ds_restate.placed_qnames(bam_path), targets, SEED)
    plain = _files(_run_cli(tmp_path, "o", bam_path, fa, bed, P))
    got = _run_cli(tmp_path, "o", bam_path, fa, bed, P, dsRpb="2,4", dsRpbSampler="philox", dsSeed=SEED)
    _assert_same(_files(got), plain, "full depth")
    mine = {r: _files("%s.dsRpb%g" % (got, r)) for r in targets}
    cut = _run_cli(tmp_path, "c", bam_path, fa, bed, P, dsRpb="2,4", dsRpbSampler="philox", dsSeed=SEED, batchReads=20)
    cut_files = {r: _files("%s.dsRpb%g" % (cut, r)) for r in targets}
    _assert_same(_files(cut)[:2], plain[:2], "full depth, --batchReads 20")      # (the VCF header names the prefix)
    for r, kept in zip(targets, g["kept"]):
        _assert_same(mine[r], _reference(tmp_path, bam_path, fa, bed, P, r, kept, "o.dsRpb%g" % r), "%s r=%g" % (name, r))
        ref_cut = _reference(tmp_path, bam_path, fa, bed, P, r, kept, "c.dsRpb%g" % r)
        _assert_same(cut_files[r], ref_cut, "%s r=%g --batchReads 20" % (name, r))


def test_cli_dsmt_and_philox_dsrpb_in_one_run(tmp_path):
    from smcounter_amd.py2compat import py2_round
    bam_path, fa, loci, P = _fixture("bam_deep", str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    plain = _files(_run_cli(tmp_path, "o", bam_path, fa, bed, P))
    got = _run_cli(tmp_path, "o", bam_path, fa, bed, P, dsMT="0.5", dsRpb="2", dsRpbSampler="philox", dsSeed=SEED)
    _assert_same(_files(got), plain, "full depth")
    mt, rpb = _files(got + ".dsMT0.5"), _files(got + ".dsRpb2")
    d = max(1, int(py2_round(0.5 * P.mtDepth)))
    ds_bam = ds_restate.write_ds_bam(bam_path, str(tmp_path / "ds0.5.bam"), 0.5, SEED)
    _assert_same(mt, _files(_run_cli(tmp_path, "o.dsMT0.5", ds_bam, fa, bed, dataclasses.replace(P, mtDepth=d))), "dsMT 0.5")
    kept = rp.restate(ds_restate.placed_qnames(bam_path), (2.0,), SEED)["kept"][0]
    _assert_same(rpb, _reference(tmp_path, bam_path, fa, bed, P, 2.0, kept, "o.dsRpb2"), "dsRpb 2 philox")


def test_cli_philox_refuses_a_file_without_a_multi_name_barcode(tmp_path):
    import ds_rpb_restate
    import bam_fixture
    case = bam_fixture.make_case(str(tmp_path))
    one = ds_rpb_restate.write_one_name_per_barcode(case["bam"], str(tmp_path / "one.bam"))
    with pytest.raises(SystemExit, match=r"--dsRpb 2: .*one\.bam has no barcode with more than one read name"):
        cli.main(dict(outPrefix=str(tmp_path / "o"), bamFile=one, bedTarget=case["bed"], mtDepth=12, rpb=3.0, hpLen=8,
                      refGenome=case["fasta"], dsRpb="2", dsRpbSampler="philox"))
    assert not os.path.exists(str(tmp_path / "o.smCounter.all.txt"))
