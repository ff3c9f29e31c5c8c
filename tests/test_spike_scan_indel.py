"""--spikeScanIndel without a GPU: every refusal before any file, the SNV scan's messages unchanged without the flag, the pass lists
of tools.spike_scan_lists --indel on a hand-made BED and FASTA (texts, skipped loci, the smallest stride), every list under
spike_variants.parse_variants(indels=True), the page writers with indel texts against spike.sensitivity_line / spike.curve_line, and
the header."""
import argparse
import os
import re
import sys

import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, bedops, cli, dsaf, fasta, spike
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_scan_lists as lists
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402


def _args(tmp, **kw):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp))
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    d = dict(outPrefix=str(tmp / "o"), bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, refGenome=fa, spikeScan="0.3,0.7",
             spikeScanReps="4", spikeScanIndel="del1")
    d.update(kw)
    return {k: v for k, v in d.items() if v is not None}


@pytest.mark.parametrize("kw,msg", [
    (dict(spikeScan=None, spikeScanReps=None), "--spikeScanIndel belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScanAlt="transition"), "--spikeScanIndel cannot be combined with --spikeScanAlt"),
    (dict(spikeScanIndel="ins2"), "--spikeScanIndel: del<d> or dup<s> with a length in 1 .. 255 expected, got 'ins2'"),
    (dict(spikeScanIndel="del"), "--spikeScanIndel: del<d> or dup<s> with a length in 1 .. 255 expected, got 'del'"),
    (dict(spikeScanIndel="del-1"), "--spikeScanIndel: del<d> or dup<s> with a length in 1 .. 255 expected, got 'del-1'"),
    (dict(spikeScanIndel="dup1.5"), "--spikeScanIndel: del<d> or dup<s> with a length in 1 .. 255 expected, got 'dup1.5'"),
    (dict(spikeScanIndel="del0"), "--spikeScanIndel: del<d> or dup<s> with a length in 1 .. 255 expected, got 'del0'"),
    (dict(spikeScanIndel="dup256"), "--spikeScanIndel: del<d> or dup<s> with a length in 1 .. 255 expected, got 'dup256'"),
    (dict(spikeScanIndel="del3", spikeScanStride="4"),
     "--spikeScanStride: a stride of 4 with del3: the footprints of a pass would overlap, the smallest stride allowed is 5"),
    (dict(spikeScanIndel="dup7", spikeScanStride="1"),
     "--spikeScanStride: a stride of 1 with dup7: the footprints of a pass would overlap, the smallest stride allowed is 2"),
    # what --spikeScan refuses stays refused, with its text
    (dict(spikeScanReps=None), "it needs --spikeScanReps"),
    (dict(spikeIndelReps="4"), "--spikeScan cannot be combined with --spikeIndelReps"),
    (dict(dsMT="0.5"), "--spikeScan cannot be combined with --dsMT"),
    (dict(spikeScanStride="0"), "--spikeScanStride: an integer >= 1 expected, got 0"),
])
def test_cli_refusals_before_any_file(tmp_path, kw, msg):
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(_args(tmp_path, **kw))
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_cli_refuses_a_pass_beyond_the_rewrites_limit(tmp_path, monkeypatch):
    args = _args(tmp_path, spikeScanStride="3")
    open(args["bedTarget"], "w").write("chrA\t100\t%d\n" % (100 + 3 * (cli.SCAN_MAX_PASS_VARIANTS + 1)))
    monkeypatch.setattr(cli, "_EarlyEngine", lambda device: None)
    monkeypatch.setattr(lists, "scan_indels", lambda loc_list, fa, rule: (
        [af.Variant(c, int(p), "AC", "A", "DEL|AC|A", af.DEL) for c, p in loc_list], []))
    with pytest.raises(SystemExit, match=re.escape("--spikeScan: pass 0 holds 4097 loci of chrA, at most 4096")):
        cli.main(args)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


@pytest.mark.parametrize("kw,msg", [
    (dict(spikeScanAlt="transversal"), "--spikeScanAlt: one of complement, transition, transversion expected, got 'transversal'"),
    (dict(spikeScan=None, spikeScanReps=None, spikeScanAlt="transition"), "--spikeScanAlt belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScan="0.1,0.10"), "--spikeScan: a target is listed twice"),
    (dict(spikeReps="4"), "--spikeScan cannot be combined with --spikeReps in one run: the scan plants its own SNV at every locus of "
                          "--bedTarget (a pass of it is the --spikeAF --spikeReps run of tools/spike_scan_lists.py's list)"),
])
def test_the_snv_scans_messages_are_unchanged_without_the_flag(tmp_path, kw, msg):
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(_args(tmp_path, spikeScanIndel=None, **kw))
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_scan_reads_the_flag():
    ns = argparse.Namespace(spikeScan="0.7,0.3", spikeScanReps="32")
    assert spike.scan(ns) == dict(targets=[0.7, 0.3], reps=32, stride=256, alt="transition")          # (no key without the flag)
    ns = argparse.Namespace(spikeScan="0.005", spikeScanReps=2, spikeScanStride=5, spikeScanIndel="del3")
    assert spike.scan(ns) == dict(targets=[0.005], reps=2, stride=5, alt="transition", indel=("del", 3))
    ns = argparse.Namespace(spikeScan="0.005", spikeScanReps=2, spikeScanStride=2, spikeScanIndel="dup255")
    assert spike.scan(ns)["indel"] == ("dup", 255)
    assert lists.parse_indel_rule(" dup2 ") == ("dup", 2) and lists.indel_min_stride(("del", 255)) == 257
    src = __import__("inspect").getsource(cli._make_rules)
    assert "lists.scan_indels(" in src and "lists.scan_passes(" in src


# ---- the lists
FA = ("chrA", "ACGTNacgtRACGTACGTACG", "chrB", "TTTTGGGG")         # (a lower-case stretch, an N and an R; chrB's run of T, then of G)
SPANS = (("chrA", ((0, 12), (14, 21))), ("chrB", ((2, 8),)))       # (both chromosomes to their last letter)


def _fasta(tmp):
    path = str(tmp / "g.fa")
    with open(path, "w") as fh:
        for name, seq in zip(FA[::2], FA[1::2]):
            fh.write(">%s\n%s\n" % (name, seq))
    off, fai = 0, []
    for name, seq in zip(FA[::2], FA[1::2]):
        off += len(name) + 2
        fai.append("%s\t%d\t%d\t%d\t%d\n" % (name, len(seq), off, len(seq), len(seq) + 1))
        off += len(seq) + 1
    open(path + ".fai", "w").write("".join(fai))
    return path


def _bed(tmp):
    path = str(tmp / "t.bed")
    open(path, "w").write("".join("%s\t%d\t%d\n" % (c, a, b) for c, spans in SPANS for a, b in spans))
    return path


def _expected(kind, n):
    """The rule restated letter by letter -> ([(chrom, pos, REF, ALT)], skipped for a letter, skipped for the chromosome's end)."""
    seqs = dict(zip(FA[::2], FA[1::2]))
    out, bad_letter, past_end = [], [], []
    for chrom, spans in SPANS:
        seq = seqs[chrom].upper()
        for a, b in spans:
            for p in range(a, b):
                if p + n >= len(seq):
                    past_end.append((chrom, p + 1))
                elif any(c not in "ACGT" for c in seq[p:p + n + 1]):
                    bad_letter.append((chrom, p + 1))
                elif kind == "del":
                    out.append((chrom, p + 1, seq[p:p + n + 1], seq[p]))
                else:
                    out.append((chrom, p + 1, seq[p], seq[p:p + n + 1]))
    return out, bad_letter, past_end


def test_the_texts_of_del1_del3_and_dup2(tmp_path):
    fa = fasta.FastaFile(_fasta(tmp_path))
    loc_list = bedops.expand_loci(_bed(tmp_path))
    text = lambda vs: {(v.chrom, v.pos): (v.ref, v.alt, v.key, v.kind) for v in vs}
    d1, s1 = lists.scan_indels(loc_list, fa, ("del", 1))
    assert text(d1)[("chrA", 1)] == ("AC", "A", "DEL|AC|A", af.DEL) and text(d1)[("chrA", 8)] == ("GT", "G", "DEL|GT|G", af.DEL)
    # an N behind the anchor, the N itself, the R and the letter in front of it; each chromosome's last letter
    assert s1 == [("chrA", 4), ("chrA", 5), ("chrA", 9), ("chrA", 10), ("chrA", 21), ("chrB", 8)]
    d3, s3 = lists.scan_indels(loc_list, fa, ("del", 3))
    assert text(d3)[("chrA", 1)] == ("ACGT", "A", "DEL|ACGT|A", af.DEL) and text(d3)[("chrB", 3)] == ("TTGG", "T", "DEL|TTGG|T", af.DEL)
    assert ("chrA", 2) in s3 and ("chrA", 6) not in s3 and ("chrA", 7) in s3          # (the N at 5 lies inside 2 .. 5; 6 .. 9 is acgt; 7 .. 10 ends on the R)
    assert s3[-3:] == [("chrB", 6), ("chrB", 7), ("chrB", 8)] and ("chrB", 5) not in s3
    u2, t2 = lists.scan_indels(loc_list, fa, ("dup", 2))
    assert text(u2)[("chrA", 1)] == ("A", "ACG", "INS|A|ACG", af.INS)
    assert text(u2)[("chrB", 5)] == ("G", "GGG", "INS|G|GGG", af.INS)                 # (a homopolymer grows inside its run)
    assert text(u2)[("chrB", 4)] == ("T", "TGG", "INS|T|TGG", af.INS)
    assert ("chrA", 3) in t2 and ("chrA", 20) in t2 and ("chrA", 19) not in t2
    for kind, n, got, skipped in (("del", 1, d1, s1), ("del", 3, d3, s3), ("dup", 2, u2, t2)):
        want, bad_letter, past_end = _expected(kind, n)
        assert [(v.chrom, v.pos, v.ref, v.alt) for v in got] == want
        assert bad_letter and past_end and sorted(skipped) == sorted(bad_letter + past_end)
        assert all(sv.footprint(v) == (v.pos, v.pos + (n + 1 if kind == "del" else 1)) for v in got)
    again, _ = lists.scan_indels(loc_list + loc_list[:3], fa, ("del", 1))           # (a locus listed twice counts once)
    assert again == d1


@pytest.mark.parametrize("rule,stride", [("del1", 3), ("del1", 7), ("del3", 5), ("del3", 1000), ("dup2", 2), ("dup2", 4)])
def test_pass_lists_parse_as_spike_indel_variants(tmp_path, rule, stride, capsys):
    fa, bed = _fasta(tmp_path), _bed(tmp_path)
    prefix = str(tmp_path / "scan")
    names = lists.main(argparse.Namespace(runPath=None, bedTarget=bed, refGenome=fa, stride=stride, alt="transition", indel=rule,
                                          outPrefix=prefix))
    kind, n = lists.parse_indel_rule(rule)
    assert stride >= lists.indel_min_stride((kind, n))
    want, bad_letter, past_end = _expected(kind, n)
    by_k = {}
    for w in want:
        by_k.setdefault(w[1] % stride, []).append(w)
    assert names == ["%s.pass%d.txt" % (prefix, k) for k in sorted(by_k)]
    for k, name in zip(sorted(by_k), names):
        got = [tuple(l.split("\t")) for l in open(name).read().splitlines()]
        assert got == [(c, "%d" % p, r, a) for c, p, r, a in by_k[k]]
        parsed = sv.parse_variants(name, "--spikeVariants", indels=True)          # (the footprints of a pass do not overlap)
        sv.check_reference(parsed, fasta.FastaFile(fa), "--spikeVariants")
        assert [(v.chrom, v.pos, v.ref, v.alt) for v in parsed] == by_k[k]
        assert all(v.kind == (af.DEL if kind == "del" else af.INS) for v in parsed)
    table = open(prefix + ".passes.txt").read().splitlines()
    assert table[-1] == "#skipped\t%d" % len(bad_letter + past_end)
    assert "(%s), %d skipped for a letter inside the footprint" % (rule, len(bad_letter + past_end)) in capsys.readouterr().out


def test_the_smallest_stride_is_accepted_and_one_below_is_refused(tmp_path):
    fa, bed = _fasta(tmp_path), _bed(tmp_path)
    ns = lambda rule, stride: argparse.Namespace(runPath=None, bedTarget=bed, refGenome=fa, stride=stride, alt="transition", indel=rule,
                                                 outPrefix=str(tmp_path / "s"))
    for rule, d in (("del1", 1), ("del3", 3), ("del255", 255)):
        with pytest.raises(SystemExit, match=re.escape("--stride: a stride of %d with %s: the footprints of a pass would overlap, the "
                                                       "smallest stride allowed is %d" % (d + 1, rule, d + 2))):
            lists.main(ns(rule, d + 1))
        assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("s.")]
    for rule, d in (("del1", 1), ("del3", 3), ("del255", 255)):
        lists.main(ns(rule, d + 2))
    with pytest.raises(SystemExit, match="the smallest stride allowed is 2"):
        lists.main(ns("dup9", 1))
    lists.main(ns("dup9", 2))
    with pytest.raises(SystemExit, match=re.escape("--indel: del<d> or dup<s> with a length in 1 .. 255 expected, got 'ins3'")):
        lists.main(ns("ins3", 8))
    # S = d + 1 IS an overlap under the parser's own rule: the list of one pass at that stride is refused by line
    variants, _ = lists.scan_indels([("chrA", p) for p in (13, 15)], fasta.FastaFile(fa), ("del", 1))
    lists.write_lists(str(tmp_path / "bad"), variants, [(1, [0, 1])], 0)
    with pytest.raises(ValueError, match=re.escape("chrA:15 AC>A lies in the footprint 13-15 of chrA:13 GT>G")):
        sv.parse_variants(str(tmp_path / "bad.pass1.txt"), "--spikeVariants", indels=True)


# ---- the pages
@pytest.mark.parametrize("with_lod", (False, True))
def test_page_writers_with_indel_texts(tmp_path, with_lod):
    variants = [af.Variant("chrA", 3, "GT", "G", "DEL|GT|G", af.DEL), af.Variant("chrA", 7, "C", "CGT", "INS|C|CGT", af.INS),
                af.Variant("chrB", 4, "TGGG", "T", "DEL|TGGG|T", af.DEL), af.Variant("chrB", 6, "G", "GG", "INS|G|GG", af.INS)]
    loci = [("chrA", 3, 0), ("chrA", 5, None), ("chrA", 7, 1), ("chrB", 4, 2), ("chrB", 6, 3)]
    targets, R = [0.7, 0.3], 4
    entries, full = {}, {}
    for i, v in enumerate(variants):
        for t in range(len(targets)):
            n_called = R if (i == 3 and t == 0) else (i + 2 * t) % (R + 1)
            per, per_full = [], []
            for j in range(R):
                r = dict(N=100 + i, V0=i % 3, S=10 * t + j, READS=20 * t + 2 * j + i, V1=i % 3 + 10 * t + j)
                per.append(spike.scan_entry(v, r, j < n_called))
                row = [""] * (dsaf._COL["PI"] + 1)
                row[dsaf._COL["PI"]] = "%.2f" % (30.0 + j if j < n_called else 3.0)
                per_full.append((r, row, (v.ref, [v.alt]) if j < n_called else None))
            entries[(i, t)], full[(i, t)] = per, per_full
    lods = [0.0123, 1.0, 0.5, 0.004] if with_lod else None
    prefix = str(tmp_path / "o")
    spike.write_scan(prefix, loci, variants, targets, entries, lods)
    sens = open(prefix + ".spikeScan.sensitivity.txt").read().splitlines()
    assert sens[0].split("\t") == list(spike.SCAN_SENSITIVITY_HEADER) + (["LOD"] if with_lod else [])
    want = []
    for i, v in enumerate(variants):
        for t, target in enumerate(targets):
            f = spike.sensitivity_line(v, target, full[(i, t)]).split("\t")
            assert f[2:4] == [v.ref, v.alt]
            want.append("\t".join(f[:17] + (["%.15g" % lods[i]] if with_lod else [])))
    assert sens[1:] == want
    curve = open(prefix + ".spikeScan.curve.txt").read().splitlines()
    assert curve[1:] == [spike.curve_line(v, 100 + i, targets, [full[(i, t)] for t in range(2)], lods[i] if with_lod else None)
                         for i, v in enumerate(variants)]
    # the bedgraph position is the anchor
    for t, target in enumerate(targets):
        got = open("%s.spikeScan%g.rate.bedgraph" % (prefix, target)).read().splitlines()
        assert got == ["%s\t%d\t%d\t%s" % (v.chrom, v.pos - 1, v.pos, want[i * 2 + t].split("\t")[7]) for i, v in enumerate(variants)]
    t95 = open(prefix + ".spikeScan.t95.bedgraph").read().splitlines()
    assert [l.split("\t")[:3] for l in t95] == [[c, "%d" % (p - 1), "%d" % p] for c, p, _ in loci]
    assert t95[1] == "chrA\t4\t5\t1" and t95[-1].split("\t")[3] != "1"


def test_header_defines_the_entry_and_the_abi_number_stays():
    text = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"^int smc_scan_detect_keys\(", text, re.M) and re.search(r"^int smc_scan_detect\(", text, re.M)
    assert re.search(r"^#define SMC_ABI_VERSION 11$", text, re.M)
    assert "smc_scan_detect_keys" in _lib.SYMBOLS
    assert re.search(r"^#define SMC_SCAN_ID_NONE 0xFFFFFFFFu$", text, re.M) and abi.SCAN_ID_NONE == 0xFFFFFFFF
    assert re.search(r"^#define SMC_SCAN_ID_HOST 0xFFFFFFFEu$", text, re.M) and abi.SCAN_ID_HOST == 0xFFFFFFFE
    L = _lib.load()
    assert len(L.smc_scan_detect_keys.argtypes) == 28
