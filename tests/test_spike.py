"""--spikeAF without a GPU: tools.spike_variants against the restatement from host-built pileups (tests/spike_restate.py) record
for record, the properties of the draw, a planted variant called by the CPU restatement of the caller, parsing and every refusal
before any file, the detection file's format, the header, and the decoder's accessor."""
import argparse
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, bamio, cli, fasta, features, spike, vc, writers
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import spike_restate as SR  # noqa: E402

SEED = 20240607
T = 0.5
INPUTS = ("case", "bam_cigars", "bam_deep")


def _inputs(name, tmp):
    """-> (bam, fasta path, loci, VcParams, listed variants)."""
    if name == "case":
        return SR.make_case(tmp)
    if name == "synth":
        bam, fa, loci, P, _ = R.synth_bam(tmp)
        return bam, fa, loci, P, SR.pick_positions(bam, fa, loci[20:44], 4)
    bam, fa, loci, P = ds_restate.load_fixture(name, tmp)
    return bam, fa, loci, P, SR.pick_positions(bam, fa, loci, 3)


def _tool(bam, fa, variants, t, seed, tmp, tag="out"):
    vfile = R.write_variants(os.path.join(tmp, "v_%s.txt" % tag), variants)
    out = os.path.join(tmp, "%s.bam" % tag)
    rows = sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=seed, refGenome=fa))
    return out, rows


@pytest.mark.parametrize("name", INPUTS)
def test_tool_equals_the_restatement_record_for_record(tmp_path, name):
    tmp = str(tmp_path)
    bam, fa, loci, P, variants = _inputs(name, tmp)
    records, stats = SR.restate(bam, fa, variants, T, SEED, P.mismatchThr)
    out, rows = _tool(bam, fa, variants, T, SEED, tmp)
    got, want = SR.file_records(out), SR.expected_records(bam, records)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    for row, s in zip(rows, stats):
        assert row == {k: s[k] for k in ("N", "V0", "S", "READS", "V1")}
    assert sum(s["READS"] for s in stats) > 0
    if name == "case":
        # every case of the rewrite rule is in the hand-made file, and the draw at this seed reaches each of them
        notes = set().union(*(r["notes"] for r in records.values()))
        assert not set(SR.CASES) - notes, set(SR.CASES) - notes
        by = lambda note: [r for r in records.values() if note in r["notes"]]
        assert all(not r["edits"] for r in by("in_deletion") if r["notes"] <= {"in_deletion"})
        assert any(r["edits"] and r["inc"] == 0 for r in by("already_alt")) and any(r["edits"] and r["inc"] == 0 for r in by("third_letter"))
        assert any(len(r["edits"]) == 2 and r["inc"] == 2 for r in by("two_positions"))
        assert any(r["mmok0"] and not r["mmok"] for r in by("flips_inccond"))
        # a record untouched at P1 because of its CIGAR keeps every letter there (it may be rewritten at P2)
        for note in ("in_deletion", "ins_behind", "del_behind"):
            assert by(note)


def test_spiked_sets_are_nested_and_unspiked_barcodes_keep_their_records(tmp_path):
    tmp = str(tmp_path)
    bam, fa, loci, P, variants = _inputs("case", tmp)
    before = SR.file_records(bam)
    last = None
    for t in (0.05, 0.2, 0.5, 0.9):
        _, stats = SR.restate(bam, fa, variants, t, SEED, P.mismatchThr)
        out, _ = _tool(bam, fa, variants, t, SEED, tmp, "t%g" % t)
        sets = [s["spiked"] for s in stats]
        if last is not None:
            assert all(a <= b for a, b in zip(last, sets))
        last = sets
        every = set().union(*sets)
        n_same = 0
        for b, a in zip(before, SR.file_records(out)):
            if af.barcode_of(b[0]) not in every:
                assert a == b
                n_same += 1
            else:
                assert a[:4] == b[:4] and a[5] == b[5]          # name, flag, position, CIGAR and qualities stay in every record
        assert n_same > 0
    assert any(last)


@pytest.mark.parametrize("name", ("case", "synth"))
def test_spiked_count_within_the_binomial_width(tmp_path, name):
    """|S - t N| <= 4 sqrt(N t (1 - t)): the width of binomial(N, t), not a tuned tolerance.  The seed is fixed; it is one for which
    the RESTATEMENT holds the bound (asserted first) - then the tool must."""
    tmp = str(tmp_path)
    bam, fa, loci, P, variants = _inputs(name, tmp)
    for t in (0.1, 0.5):
        _, stats = SR.restate(bam, fa, variants, t, SEED, P.mismatchThr)
        rows = sv.spike_file(bam, None, [_tool_variant(v) for v in variants], t, SEED)
        for res in (stats, rows):
            for v, s in zip(variants, res):
                print(name, v.pos, t, s["N"], s["S"], 4 * math.sqrt(s["N"] * t * (1 - t)))
                assert s["N"] > 10
                assert abs(s["S"] - t * s["N"]) <= 4 * math.sqrt(s["N"] * t * (1 - t))


def _tool_variant(v):
    return af.Variant(v.chrom, v.pos, v.ref, v.alt, v.alt, af.SNV)


def test_a_planted_variant_absent_at_full_depth_is_called(tmp_path):
    """On the synthetic BAM: a position where nobody carries the ALT is spiked at 0.2 - far above the limit of detection at 150
    barcodes - and the caller (its CPU restatement, from host-built pileups of the tool's BAM) cuts it."""
    import oracle_lib
    tmp = str(tmp_path)
    bam, fa, loci, P, _ = R.synth_bam(tmp)
    pb = R.pileups(bam, fa, loci[20:44])
    pick = None
    for l in range(len(pb.pos)):
        sl = pb.locus_slice(l)
        keys = {pb.alleles[l][int(a)] for a in pb.allele[sl]}
        if pb.ref[l] in "ACGT" and keys <= {pb.ref[l]} and sl.stop - sl.start > 300:
            alt = "ACGT"[("ACGT".index(pb.ref[l]) + 2) % 4]
            pick = SR.V(pb.chrom[l], int(pb.pos[l]), pb.ref[l], alt, alt)
            break
    assert pick is not None
    out, rows = _tool(bam, fa, [pick], 0.2, SEED, tmp)
    assert rows[0]["V0"] == 0 and rows[0]["V1"] == rows[0]["S"] > 10
    bamio.write_bai(out)
    ref = fasta.FastaFile(fa)
    threshold = writers.pi_threshold(P.mtDepth, 0)
    called = []
    for path in (bam, out):
        db = features.extract_features(R.pileups(path, fa, [(pick.chrom, pick.pos)]), P)
        text = vc._strings(oracle_lib.call_batch(db, abi.c_params(P), abi.ROW_DTYPE), db, P, ref)
        hit = writers.cut_row(text[0], threshold)
        called.append(hit is not None and hit[1]["REF"] == pick.ref and pick.alt in hit[1]["ALT"].split(","))
    assert called == [False, True]


def test_variant_file_parsing(tmp_path):
    p = str(tmp_path / "v.vcf")
    open(p, "w").write("#CHROM\tPOS\tID\tREF\tALT\nchr1\t100\t.\ta\tg\t50\tPASS\tx\nchr1\t200\tC\tT\n")
    assert [(v.chrom, v.pos, v.ref, v.alt) for v in sv.parse_variants(p)] == [("chr1", 100, "A", "G"), ("chr1", 200, "C", "T")]
    for text, msg in (("chr1\t9\tA\tACG\n", "only one-letter substitutions"), ("chr1\t9\tGTT\tG\n", "only one-letter substitutions"),
                      ("chr1\t9\tN\tG\n", "must be one of A, C, G, T"), ("chr1\t9\tA\tR\n", "must be one of A, C, G, T"),
                      ("chr1\t9\tA\tG\nchr1\t9\tA\tT\n", "listed twice"), ("chr1\t9\tA\tA\n", "neither a substitution")):
        open(p, "w").write(text)
        with pytest.raises(ValueError, match=re.escape(msg)):
            sv.parse_variants(p)
    assert sv.threshold(0.5) == 1 << 31 and sv.threshold(0.005) == int(math.floor(0.005 * 4294967296.0))


def _args(tmp, **kw):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp))
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    vfile = str(tmp / "v.txt")
    c, p = loci[0]
    letter = fasta.FastaFile(fa).fetch(c, p - 1, p).upper()
    open(vfile, "w").write("%s\t%d\t%s\t%s\n" % (c, p, letter, "ACGT"[("ACGT".index(letter) + 1) % 4]))
    d = dict(outPrefix=str(tmp / "o"), bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, refGenome=fa, spikeAF="0.05", spikeVariants=vfile)
    d.update(kw)
    return {k: v for k, v in d.items() if v is not None}, loci, letter


@pytest.mark.parametrize("kw,msg", [
    (dict(spikeVariants=None), "it needs --spikeVariants"),
    (dict(spikeAF=None), "it needs --spikeAF"),
    (dict(spikeAF=None, spikeVariants=None, spikeMtDepth="5"), "it needs --spikeAF"),
    (dict(spikeAF="0.5,1"), "must lie in (0, 1)"),
    (dict(spikeAF="0"), "must lie in (0, 1)"),
    (dict(spikeAF="0.1,0.10"), "listed twice"),
    (dict(spikeAF=",".join("%g" % (0.01 * k) for k in range(1, 34))), "at most 32"),
    (dict(spikeMtDepth="10,20"), "2 depths for 1 --spikeAF targets"),
    (dict(dsMT="0.5"), "cannot be combined with --dsMT"),
    (dict(dsRpb="2"), "cannot be combined with --dsRpb"),
    (dict(dsAF="0.1", dsAFVariants="x"), "cannot be combined with --dsAF"),
])
def test_cli_refusals_before_any_file(tmp_path, kw, msg):
    args, _, _ = _args(tmp_path, **kw)
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(args)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_cli_refuses_more_processes_host_planes_and_bad_variant_files(tmp_path, monkeypatch):
    args, loci, letter = _args(tmp_path)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--spikeAF runs in one process only"):
        cli.main(args)
    monkeypatch.setenv("WORLD_SIZE", "1")
    for env, val in (("SMC_PLANES", "host"), ("SMC_BAM_DECODER", "python")):
        monkeypatch.setenv(env, val)
        with pytest.raises(SystemExit, match="--spikeAF needs the device builder"):
            cli.main(args)
        monkeypatch.delenv(env)
    ns = argparse.Namespace(**args)
    loc_list = [(c, str(p)) for c, p in loci]
    ref = fasta.FastaFile(ns.refGenome)
    assert len(spike.variants(ns, loc_list, ref)) == 1
    c, p = loci[0]
    alt = "ACGT"[("ACGT".index(letter) + 1) % 4]
    for text, msg in (("%s\t%d\t%s\t%s\n" % (c, max(q for _, q in loci) + 1000, letter, alt), None),
                      ("%s\t%d\t%s\t%sGG\n" % (c, p, letter, letter), "only one-letter substitutions"),
                      ("%s\t%d\t%sT\t%s\n" % (c, p, letter, letter), "only one-letter substitutions"),
                      ("%s\t%d\t%s\t%s\n" % (c, p, alt, letter), "the reference genome has"),
                      ("%s\t%d\t%s\t%s\n%s\t%d\t%s\t%s\n" % (c, p, letter, alt, c, p, letter, alt), "listed twice")):
        open(ns.spikeVariants, "w").write(text)
        with pytest.raises(SystemExit, match=re.escape(msg) if msg else "is not a locus of --bedTarget|the reference genome has"):
            spike.variants(ns, loc_list, ref)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_an_identity_collision_is_refused():
    with pytest.raises(ValueError, match="share a 64-bit identity"):
        import unittest.mock as mock
        with mock.patch.object(af, "fnv64", lambda text: 7):
            af.unique_idents(["AAA", "CCC"], "x.bam")


def test_detection_file_format(tmp_path):
    from smcounter_amd.rows import HEADER_ALL
    v = af.Variant("chr1", 100, "A", "G", "G", af.SNV)
    row = [""] * len(HEADER_ALL)
    for name, val in (("CHROM", "chr1"), ("POS", "100"), ("REF", "A"), ("ALT", "G"), ("UMT", "3500"), ("VMT", "17"), ("VMF", "0.0049"),
                      ("PI", "31.25"), ("FILTER", "PASS")):
        row[HEADER_ALL.index(name)] = val
    r = dict(N=3600, V0=2, S=20, READS=171, V1=21)
    assert spike.detection_line(v, None, r, row, None) == "chr1\t100\tA\tG\tfull\t3600\t2\t0\t0\t2\t0.000556\t3500\t17\t0.0049\t31.25\tPASS\t0"
    assert spike.detection_line(v, 0.005, r, row, ("A", ["T", "G"]), lod=0.0021) == \
        "chr1\t100\tA\tG\t0.005\t3600\t2\t20\t171\t21\t0.005833\t3500\t17\t0.0049\t31.25\tPASS\t1\t0.0021"
    for prefix in ("o", "o.spikeAF0.005"):
        open(str(tmp_path / prefix) + ".smCounter.all.txt", "w").write("\t".join(HEADER_ALL) + "\n" + "\t".join(row) + "\n")
        open(str(tmp_path / prefix) + ".smCounter.cut.txt", "w").write("CHROM\tPOS\tREF\tALT\n" + ("" if prefix == "o" else "chr1\t100\tA\tG\n"))
    spike.write_detection(str(tmp_path / "o"), [v], [(None, str(tmp_path / "o"), None, None), (0.005, str(tmp_path / "o.spikeAF0.005"), [r], None)])
    lines = open(str(tmp_path / "o.spikeAF.detection.txt")).read().splitlines()
    assert lines[0].split("\t") == list(spike.DETECTION_HEADER)
    assert [l.split("\t")[4:11] + [l.split("\t")[-1]] for l in lines[1:]] == [["full", "3600", "2", "0", "0", "2", "0.000556", "0"],
                                                                             ["0.005", "3600", "2", "20", "171", "21", "0.005833", "1"]]


def test_header_symbol_and_abi():
    h = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"\bint smc_spike_alleles\(smc_ctx\* ctx,", h) and "typedef struct smc_spike_variant" in h
    assert re.search(r"#define SMC_ABI_VERSION 11\b", h)
    assert "smc_spike_alleles" in _lib.SYMBOLS and abi.SPIKE_VARIANT_DTYPE.itemsize == 16
    L = _lib.load()
    assert L.smc_abi_version() == 11 and hasattr(L, "smc_spike_alleles")
    assert "smc_bam_run_mismatches" in open(os.path.join(ROOT, "include", "smcounter_host.h")).read()


@pytest.mark.parametrize("name", INPUTS)
def test_decoder_accessor_equals_bamio(tmp_path, name):
    bam, fa, loci, P, _ = _inputs(name, str(tmp_path))
    nat, py = bamio.NativeBam(bam), bamio.BamFile(bam)
    n = 0
    for chrom, lo, hi in ds_restate.stretches(loci):
        A = nat.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
        nm, n_indel = nat.run_mismatches(len(A["aln"]))
        recs = py.fetch(chrom, lo, hi)
        assert len(recs) == len(A["aln"]) == len(nm) == len(n_indel)
        assert [a.pos for a in recs] == A["aln"]["pos"].tolist()
        assert nm.tolist() == [a.nm for a in recs]
        assert n_indel.tolist() == [sum(l for op, l in a.cigar if op in (1, 2)) for a in recs]
        n += len(recs)
    assert n > 0
    if name == "case":
        assert any(not a.has_nm for a in recs) and n_indel.max() > 0
    nat.close(); py.close()
