"""--spikeIndels without a GPU: tools.spike_variants --indels against the restatement (tests/spike_indel_restate.py) record for record,
the decoder on the tool's BAM, the properties of the draw, a planted deletion called by the CPU restatement of the caller, parsing and
every refusal before any file, and the header."""
import argparse
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, bamio, cli, fasta, features, vc, writers
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import spike_indel_restate as IR  # noqa: E402

SEED = 20240607
T = 0.5


def _inputs(name, tmp):
    if name == "case":
        return IR.make_case(tmp)
    if name == "synth":
        bam, fa, loci, P, _ = R.synth_bam(tmp)
        return bam, fa, loci, P, IR.pick_variants(bam, fa, loci[8:56], 4, gap=10)
    bam, fa, loci, P = ds_restate.load_fixture(name, tmp)
    return bam, fa, loci, P, IR.pick_variants(bam, fa, loci, 4, gap=8)


def _tool(bam, fa, variants, t, seed, tmp, tag="out", indels=True):
    vfile = R.write_variants(os.path.join(tmp, "v_%s.txt" % tag), variants)
    out = os.path.join(tmp, "%s.bam" % tag)
    rows = sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=seed, refGenome=fa, indels=indels))
    return out, rows


@pytest.mark.parametrize("name", ("case", "bam_cigars"))
def test_tool_equals_the_restatement_record_for_record(tmp_path, name):
    tmp = str(tmp_path)
    bam, fa, loci, P, variants = _inputs(name, tmp)
    out, rows = _tool(bam, fa, variants, T, SEED, tmp)
    got = IR.file_records(out)
    want, stats = [], [None] * len(variants)
    for chrom in sorted({v.chrom for v in variants}):                # (the restatement takes one chromosome's variants at a time)
        idx = [k for k, v in enumerate(variants) if v.chrom == chrom]
        records, st = IR.restate(bam, [variants[k] for k in idx], sv.threshold(T), SEED, P.mismatchThr, fa)
        for k, s in zip(idx, st):
            stats[k] = s
        want.append(records)
    merged = {}
    for r in want:
        merged.update(r)
    exp = IR.expected_records(bam, merged)
    assert len(got) == len(exp)
    for g, w in zip(got, exp):
        assert g == w                                                # name, flag, position, CIGAR, SEQ, QUAL, NM
    for row, s in zip(rows, stats):
        assert row == {k: s[k] for k in ("N", "V0", "S", "READS", "V1")}
    assert sum(r["relocated"] for r in merged.values()) > 0
    if name == "case":
        # every case of the rule is in the hand-made file, and the draw at this seed reaches each of them
        notes = set().union(*(r["notes"] for r in merged.values()))
        assert not set(IR.CASES) - notes, set(IR.CASES) - notes
        by = lambda note: [r for r in merged.values() if note in r["notes"]]
        # (these read shapes lie around the insertion: it is not applied to them, whatever the other variants do)
        for note in ("across_operations", "anchor_in_deletion", "own_insertion_behind", "shows_it_already"):
            assert by(note) and all(not any(variants[k].kind == af.INS for k in r["applied"]) for r in by(note)), note
        assert any(r["mmok0"] and not r["mmok"] for r in by("flips_mmok_by_length"))
        assert any((7, 5) == r["cigar"][0] and (1, 3) == r["cigar"][1] and r["cigar"][2][0] == 7 for r in by("splits_eq_or_x"))
        assert any(len(r["applied"]) == 3 for r in by("insertion_and_deletion"))


def test_the_decoder_on_the_tools_bam_gives_the_restated_records(tmp_path):
    tmp = str(tmp_path)
    bam, fa, loci, P, variants = IR.make_case(tmp)
    out, _ = _tool(bam, fa, variants, T, SEED, tmp)
    bamio.write_bai(out)
    records, _ = IR.restate(bam, variants, sv.threshold(T), SEED, P.mismatchThr, fa)
    (chrom, lo, hi), = ds_restate.stretches(loci)
    nat0, nat1, py = bamio.NativeBam(bam), bamio.NativeBam(out), bamio.BamFile(bam)
    A0, A1 = (n.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2) for n in (nat0, nat1))
    want = IR.expected_run(A0, py.fetch(chrom, lo, hi), records, *nat0.run_mismatches(len(A0["aln"])))
    nm1, ni1 = nat1.run_mismatches(len(A1["aln"]))
    assert np.array_equal(nm1, want["nm"]) and np.array_equal(ni1, want["n_indel"]) and want["relocated"]
    for f in ("pos", "end", "n_cig", "oflag", "mapq", "left_sp", "qalen", "l_seq", "bc_gid", "pair_gid"):
        assert np.array_equal(A1["aln"][f], want["aln"][f]), f
    for g, w in zip(A1["aln"], want["aln"]):
        assert A1["bq"][2 * int(g["seq_off"]):2 * (int(g["seq_off"]) + int(g["l_seq"]))].tobytes() == \
            want["bq"][2 * int(w["seq_off"]):2 * (int(w["seq_off"]) + int(w["l_seq"]))].tobytes()
        assert A1["cig"][int(g["cig_off"]):int(g["cig_off"]) + int(g["n_cig"])].tolist() == \
            want["cig"][int(w["cig_off"]):int(w["cig_off"]) + int(w["n_cig"])].tolist()
    for n in (nat0, nat1, py):
        n.close()


def test_spiked_sets_are_nested_and_unspiked_barcodes_keep_their_records(tmp_path):
    tmp = str(tmp_path)
    bam, fa, loci, P, variants = IR.make_case(tmp)
    before = IR.file_records(bam)
    last = None
    for t in (0.05, 0.2, 0.5, 0.9):
        _, stats = IR.restate(bam, variants, sv.threshold(t), SEED, P.mismatchThr, fa)
        out, _ = _tool(bam, fa, variants, t, SEED, tmp, "t%g" % t)
        sets = [s["spiked"] for s in stats]
        if last is not None:
            assert all(a <= b for a, b in zip(last, sets))
        last = sets
        every = set().union(*sets)
        n_same = 0
        for b, a in zip(before, IR.file_records(out)):
            if af.barcode_of(b[0]) not in every:
                assert a == b
                n_same += 1
            else:
                assert a[:3] == b[:3]                               # name, flag and position stay in every record
        assert n_same > 0
    assert any(last)


@pytest.mark.parametrize("name", ("case", "synth"))
def test_spiked_count_within_the_binomial_width(tmp_path, name):
    """|S - t N| <= 4 sqrt(N t (1 - t)): the width of binomial(N, t), the bound of tests/test_spike.py - asserted on the RESTATEMENT
    first, then on the tool."""
    tmp = str(tmp_path)
    bam, fa, loci, P, variants = _inputs(name, tmp)
    genome = fasta.FastaFile(fa)
    for t in (0.1, 0.5):
        _, stats = IR.restate(bam, variants, sv.threshold(t), SEED, P.mismatchThr, fa)
        rows = sv.spike_file(bam, None, variants, t, SEED, genome)
        for res in (stats, rows):
            for v, s in zip(variants, res):
                assert abs(s["S"] - t * s["N"]) <= 4 * math.sqrt(s["N"] * t * (1 - t))
        assert [r["S"] for r in rows] == [s["S"] for s in stats] and max(s["N"] for s in stats) > 10


def test_a_planted_deletion_absent_at_full_depth_is_called_as_an_indel(tmp_path):
    """On the synthetic BAM: a 3-base deletion nobody carries is spiked at 0.2 - far above the limit of detection at 150 barcodes - and
    the caller (its CPU restatement, from host-built pileups of the tool's BAM) writes it to .cut.vcf as an INDEL with REF / ALT."""
    import oracle_lib
    tmp = str(tmp_path)
    bam, fa, loci, P, _ = R.synth_bam(tmp)
    genome = fasta.FastaFile(fa)
    pb = R.pileups(bam, fa, loci[20:44])
    pick = None
    for l in range(len(pb.pos)):
        clean = all(len(pb.alleles[l][int(a)]) == 1 for a in pb.allele[pb.locus_slice(l)])       # (no read shows an indel there)
        letters = genome.fetch(pb.chrom[l], int(pb.pos[l]) - 1, int(pb.pos[l]) + 3).upper()
        sl = pb.locus_slice(l)
        # (a deletion that does not shift: the letter behind the deleted ones differs from the first of them)
        if clean and sl.stop - sl.start > 300 and all(c in "ACGT" for c in letters) and len(set(letters)) > 2:
            pick = IR.variant(pb.chrom[l], int(pb.pos[l]), letters, letters[0])
            break
    assert pick is not None and pick.kind == af.DEL
    out, rows = _tool(bam, fa, [pick], 0.2, SEED, tmp)
    assert rows[0]["V0"] == 0 and rows[0]["V1"] > 10 and rows[0]["S"] >= rows[0]["V1"]
    bamio.write_bai(out)
    threshold = writers.pi_threshold(P.mtDepth, 0)
    called = []
    for tag, path in (("full", bam), ("spiked", out)):
        db = features.extract_features(R.pileups(path, fa, [(pick.chrom, pick.pos)]), P)
        text = vc._strings(oracle_lib.call_batch(db, abi.c_params(P), abi.ROW_DTYPE), db, P, genome)
        prefix = os.path.join(tmp, tag)
        writers.write_outputs(prefix, text, threshold)
        lines = [l.split("\t") for l in open(prefix + ".smCounter.cut.vcf").read().splitlines() if not l.startswith("#")]
        called.append([(l[3], l[4], [x for x in l[7].split(";") if x.startswith("TYPE=")][0]) for l in lines if l[1] == "%d" % pick.pos])
    assert called == [[], [(pick.ref, pick.alt, "TYPE=INDEL")]]


def test_variant_file_parsing(tmp_path):
    p = str(tmp_path / "v.txt")
    open(p, "w").write("chr1\t100\ta\tagt\nchr1\t110\tCTT\tC\nchr1\t120\tA\tG\n")
    got = sv.parse_variants(p, indels=True)
    assert [(v.pos, v.ref, v.alt, v.kind) for v in got] == [(100, "A", "AGT", af.INS), (110, "CTT", "C", af.DEL), (120, "A", "G", af.SNV)]
    assert [sv.footprint(v) for v in got] == [(100, 101), (110, 113), (120, 120)]
    with pytest.raises(ValueError, match="only one-letter substitutions"):
        sv.parse_variants(p)                                         # without the flag an indel line is refused as ever
    for text, msg in (("chr1\t9\tA\tANG\n", "made of A, C, G, T"), ("chr1\t9\tGNT\tG\n", "made of A, C, G, T"),
                      ("chr1\t9\tA\tA%s\n" % ("C" * 256), "at most 255"), ("chr1\t9\tA%s\tA\n" % ("C" * 256), "at most 255"),
                      ("chr1\t9\tAC\tGT\n", "neither a substitution"), ("chr1\t9\tAC\tGTT\n", "neither a substitution"),
                      ("chr1\t9\tA\tAC\nchr1\t10\tG\tT\n", "line 2: chr1:10 G>T lies in the footprint 9-10"),
                      ("chr1\t13\tG\tT\nchr1\t9\tACGT\tA\n", "line 1: chr1:13 G>T lies in the footprint 9-13"),
                      ("chr1\t9\tA\tG\nchr1\t9\tA\tAT\n", "listed twice")):
        open(p, "w").write(text)
        with pytest.raises(ValueError, match=re.escape(msg)):
            sv.parse_variants(p, indels=True)
    open(p, "w").write("chr1\t9\tA\tAC\nchr1\t11\tG\tT\nchr2\t10\tG\tT\nchr1\t12\tACGT\tA\nchr1\t17\tC\tCA\n")   # 9-10, 11, 12-16, 17-18
    assert len(sv.parse_variants(p, indels=True)) == 5              # footprints that touch nothing


def _args(tmp, lines=None, **kw):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp))
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    vfile = str(tmp / "v.txt")
    c, p = loci[0]
    letters = fasta.FastaFile(fa).fetch(c, p - 1, p + 3).upper()
    open(vfile, "w").write(lines(c, p, letters) if lines else "%s\t%d\t%s\t%sGA\n" % (c, p, letters[0], letters[0]))
    d = dict(outPrefix=str(tmp / "o"), bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, refGenome=fa, spikeAF="0.05", spikeVariants=vfile)
    d.update(kw)
    ns = cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in d.items() if v is not None and v is not True] +
                                       ["--" + k for k, v in d.items() if v is True])
    return ns


@pytest.mark.parametrize("kw,lines,msg", [
    (dict(spikeIndels=True, spikeAF=None, spikeVariants=None), None, "it needs --spikeAF"),
    (dict(spikeIndels=True, spikeReps="3"), None, "cannot be combined with --spikeReps"),
    (dict(spikeIndels=True, spikeDepth="0.5"), None, "cannot be combined with --spikeDepth"),
    (dict(spikeIndels=True, spikePhase=True), None, "cannot be combined with --spikePhase"),
    (dict(spikeIndels=True, dsMT="0.5"), None, "cannot be combined with --dsMT"),
    (dict(), None, "only one-letter substitutions"),
    (dict(spikeIndels=True), lambda c, p, s: "%s\t%d\t%sC\t%sGG\n" % (c, p, s[0], s[0]), "neither a substitution"),
    (dict(spikeIndels=True), lambda c, p, s: "%s\t%d\t%s\t%sG\n%s\t%d\t%s\t%s\n" % (c, p, s[0], s[0], c, p + 1, s[1], "ACGT"[("ACGT".index(s[1]) + 1) % 4]),
     "lies in the footprint"),
    (dict(spikeIndels=True), lambda c, p, s: "%s\t%d\t%s%s\t%s\n" % (c, p, s[0], "ACGT"[("ACGT".index(s[1]) + 1) % 4] + s[2], s[0]),
     "the reference genome has"),
    (dict(spikeIndels=True), lambda c, p, s: "%s\t%d\t%s\t%sG\n" % (c, p + 100000, s[0], s[0]), "is not a locus of --bedTarget|the reference genome has"),
])
def test_cli_refusals_before_any_file(tmp_path, kw, lines, msg):
    ns = _args(tmp_path, lines, **kw)
    with pytest.raises(SystemExit, match=msg if "|" in msg else re.escape(msg)):
        cli.main(ns)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_the_tool_with_snvs_only_writes_the_same_file_with_and_without_the_flag(tmp_path):
    import spike_restate as SR
    tmp = str(tmp_path)
    bam, fa, loci, P, variants = SR.make_case(tmp)
    a, rows_a = _tool(bam, fa, variants, T, SEED, tmp, "a", indels=False)
    b, rows_b = _tool(bam, fa, variants, T, SEED, tmp, "b", indels=True)
    assert open(a, "rb").read() == open(b, "rb").read() and rows_a == rows_b


def test_header_symbol_and_abi():
    h = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"\bint smc_spike_indels\(smc_ctx\* ctx,", h) and "typedef struct smc_spike_indel_variant" in h
    assert re.search(r"#define SMC_ABI_VERSION 11\b", h)
    assert "smc_spike_indels" in _lib.SYMBOLS and abi.SPIKE_INDEL_VARIANT_DTYPE.itemsize == 24 and abi.SPIKE_VARIANT_DTYPE.itemsize == 16
    L = _lib.load()
    assert L.smc_abi_version() == 11 and hasattr(L, "smc_spike_indels")
