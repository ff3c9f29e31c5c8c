"""--spikeScan without a GPU: every refusal before any file, the messages of the neighbouring flags unchanged, the pass lists of
tools.spike_scan_lists on a hand-made BED and FASTA, the page writers against spike.sensitivity_line / spike.curve_line, and the
header."""
import argparse
import os
import re
import sys

import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, cli, dsaf, fasta, spike
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_scan_lists as lists
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402


def _args(tmp, **kw):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp))
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    d = dict(outPrefix=str(tmp / "o"), bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, refGenome=fa, spikeScan="0.3,0.7",
             spikeScanReps="4")
    d.update(kw)
    return {k: v for k, v in d.items() if v is not None}


@pytest.mark.parametrize("kw,msg", [
    (dict(spikeAF="0.1", spikeVariants="v.txt"), "--spikeScan cannot be combined with --spikeAF"),
    (dict(spikeVariants="v.txt"), "--spikeScan cannot be combined with --spikeVariants"),
    (dict(spikeMtDepth="5"), "--spikeScan cannot be combined with --spikeMtDepth"),
    (dict(spikeReps="4"), "--spikeScan cannot be combined with --spikeReps"),
    (dict(spikeDepth="0.5"), "--spikeScan cannot be combined with --spikeDepth"),
    (dict(spikeRpb="2"), "--spikeScan cannot be combined with --spikeRpb"),
    (dict(spikeIndelReps="4"), "--spikeScan cannot be combined with --spikeIndelReps"),
    (dict(spikeIndelDepth="0.5"), "--spikeScan cannot be combined with --spikeIndelDepth"),
    (dict(spikeIndelRpb="2"), "--spikeScan cannot be combined with --spikeIndelRpb"),
    (dict(spikePhaseRpb="2"), "--spikeScan cannot be combined with --spikePhaseRpb"),
    (dict(dsMT="0.5"), "--spikeScan cannot be combined with --dsMT"),
    (dict(dsRpb="2"), "--spikeScan cannot be combined with --dsRpb"),
    (dict(dsAF="0.1", dsAFVariants="x"), "--spikeScan cannot be combined with --dsAF"),
    (dict(dsAFVariants="x"), "--spikeScan cannot be combined with --dsAFVariants"),
    (dict(dsAFReps="4"), "--spikeScan cannot be combined with --dsAFReps"),
    (dict(dsAFDepth="0.5"), "--spikeScan cannot be combined with --dsAFDepth"),
    (dict(dsMtDepth="5"), "--spikeScan cannot be combined with --dsMtDepth"),
    (dict(spikeScanReps=None), "it needs --spikeScanReps"),
    (dict(spikeScan=None), "--spikeScanReps belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScan=None, spikeScanReps=None, spikeScanStride="8"), "--spikeScanStride belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScan=None, spikeScanReps=None, spikeScanAlt="transition"), "--spikeScanAlt belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScan="0.5,1"), "--spikeScan: every target allele fraction must lie in (0, 1)"),
    (dict(spikeScan="0"), "--spikeScan: every target allele fraction must lie in (0, 1)"),
    (dict(spikeScan="x"), "--spikeScan: comma-separated allele fractions in (0, 1) expected"),
    (dict(spikeScan="0.1,0.10"), "--spikeScan: a target is listed twice"),
    (dict(spikeScan=",".join("%g" % (0.01 * k) for k in range(1, spike.MAX_TARGETS + 2))), "--spikeScan: 33 targets, at most 32"),
    (dict(spikeScanReps="1"), "--spikeScanReps: an integer in 2 .. 1000 expected, got 1"),
    (dict(spikeScanReps="1001"), "--spikeScanReps: an integer in 2 .. 1000 expected, got 1001"),
    (dict(spikeScanReps="2.5"), "--spikeScanReps: an integer in 2 .. 1000 expected, got '2.5'"),
    (dict(spikeScanReps="four"), "--spikeScanReps: an integer in 2 .. 1000 expected, got 'four'"),
    (dict(spikeScanStride="0"), "--spikeScanStride: an integer >= 1 expected, got 0"),
    (dict(spikeScanStride="-3"), "--spikeScanStride: an integer >= 1 expected, got -3"),
    (dict(spikeScanStride="1.5"), "--spikeScanStride: an integer >= 1 expected, got '1.5'"),
    (dict(spikeScanAlt="transversal"), "--spikeScanAlt: one of complement, transition, transversion expected, got 'transversal'"),
])
def test_cli_refusals_before_any_file(tmp_path, kw, msg):
    assert (spike.REPS_MIN, spike.REPS_MAX, spike.MAX_TARGETS) == (2, 1000, 32)
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(_args(tmp_path, **kw))
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


@pytest.mark.parametrize("flag", ("spikePhase", "spikeIndels", "spikeIndelPhase"))
def test_cli_refuses_the_switches_of_the_spike_family(tmp_path, flag):
    args = _args(tmp_path)
    ns = cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in args.items()] + ["--" + flag])
    with pytest.raises(SystemExit, match=re.escape("--spikeScan cannot be combined with --%s" % flag)):
        cli.main(ns)
    with pytest.raises(SystemExit, match=re.escape("--spikeScan cannot be combined with --dsGrid")):
        cli.main(cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in args.items()] + ["--dsGrid"]))
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_cli_refuses_more_processes_host_planes_the_python_decoder_and_an_identity_collision(tmp_path, monkeypatch):
    args = _args(tmp_path)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--spikeScan runs in one process only"):
        cli.main(args)
    monkeypatch.setenv("WORLD_SIZE", "1")
    for env, val in (("SMC_PLANES", "host"), ("SMC_BAM_DECODER", "python")):
        monkeypatch.setenv(env, val)
        with pytest.raises(SystemExit, match="--spikeScan needs the device builder"):
            cli.main(args)
        monkeypatch.delenv(env)
    # (the existing check, with its text: two barcode texts of the file with one identity)
    monkeypatch.setattr(af, "fnv64", lambda text: 7)
    monkeypatch.setattr(cli, "_EarlyEngine", lambda device: None)
    with pytest.raises(SystemExit, match="share a 64-bit identity"):
        cli.main(args)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_cli_refuses_a_pass_beyond_the_rewrites_limit(tmp_path, monkeypatch):
    args = _args(tmp_path, spikeScanStride="1")
    open(args["bedTarget"], "w").write("chrA\t100\t%d\n" % (100 + cli.SCAN_MAX_PASS_VARIANTS + 1))
    monkeypatch.setattr(cli, "_EarlyEngine", lambda device: None)
    with pytest.raises(SystemExit, match=re.escape("--spikeScan: pass 0 holds 4097 loci of chrA, at most 4096")):
        cli.main(args)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


@pytest.mark.parametrize("kw,msg", [
    (dict(spikeAF="0.05"), "--spikeAF plants listed variants: it needs --spikeVariants"),
    (dict(spikeVariants="v.txt"), "--spikeVariants lists the variants --spikeAF plants: it needs --spikeAF"),
    (dict(spikeMtDepth="5"), "--spikeMtDepth gives the mtDepth of each --spikeAF target: it needs --spikeAF"),
    (dict(spikeReps="4"), "--spikeReps replicates the spike-ins of --spikeAF: it needs --spikeAF"),
    (dict(spikeAF="0.05", spikeVariants="v.txt", dsMT="0.5"),
     "--spikeAF cannot be combined with --dsMT in one run (spike-ins on a down-sampled file are not built)"),
    (dict(spikeAF="0.1,0.10", spikeVariants="v.txt"), "--spikeAF: a target is listed twice"),
])
def test_the_neighbours_messages_are_unchanged_without_the_flag(tmp_path, kw, msg):
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(_args(tmp_path, spikeScan=None, spikeScanReps=None, **kw))
    assert spike.scan(argparse.Namespace()) is None


def test_scan_reads_its_flags():
    ns = argparse.Namespace(spikeScan="0.7,0.3", spikeScanReps="32")
    assert spike.scan(ns) == dict(targets=[0.7, 0.3], reps=32, stride=256, alt="transition")
    ns = argparse.Namespace(spikeScan="0.005", spikeScanReps=2, spikeScanStride=16, spikeScanAlt="complement")
    assert spike.scan(ns) == dict(targets=[0.005], reps=2, stride=16, alt="complement")


# ---- the lists
FA = ("chrA", "ACGTNacgtRACGTACGTACG", "chrB", "TTTTGGGG")         # (a lower-case stretch, an N and an R)


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
    open(path, "w").write("chrA\t0\t12\nchrA\t14\t21\nchrB\t2\t6\n")
    return path


def _expected(alt):
    out, skipped = [], 0
    for chrom, seq, spans in (("chrA", FA[1], ((0, 12), (14, 21))), ("chrB", FA[3], ((2, 6),))):
        for a, b in spans:
            for p in range(a, b):
                letter = seq[p].upper()
                if letter not in "ACGT":
                    skipped += 1
                    continue
                out.append((chrom, p + 1, letter, lists.ALT_RULES[alt][letter]))
    return out, skipped


def test_the_three_alt_rules():
    assert lists.ALT_RULES["transition"] == {"A": "G", "G": "A", "C": "T", "T": "C"}
    assert lists.ALT_RULES["transversion"] == {"A": "C", "C": "A", "G": "T", "T": "G"}
    assert lists.ALT_RULES["complement"] == {"A": "T", "T": "A", "C": "G", "G": "C"}
    assert (lists.DEFAULT_STRIDE, lists.DEFAULT_ALT) == (256, "transition")


@pytest.mark.parametrize("alt", ("transition", "transversion", "complement"))
@pytest.mark.parametrize("stride", (1, 4, 5, 1000))
def test_pass_lists_on_a_hand_made_target(tmp_path, alt, stride):
    fa, bed = _fasta(tmp_path), _bed(tmp_path)
    prefix = str(tmp_path / "scan")
    names = lists.main(argparse.Namespace(runPath=None, bedTarget=bed, refGenome=fa, stride=stride, alt=alt, outPrefix=prefix))
    want, skipped = _expected(alt)
    assert skipped == 2
    by_k = {}
    for chrom, pos, ref, alt_letter in want:
        by_k.setdefault(pos % stride, []).append((chrom, pos, ref, alt_letter))
    assert names == ["%s.pass%d.txt" % (prefix, k) for k in sorted(by_k)]
    # (S = 1: one pass with every locus; S beyond the span: a pass per distinct position, those two chromosomes share joined)
    assert len(by_k) == (1 if stride == 1 else len({p for _, p, _, _ in want}) if stride == 1000 else stride)
    seen = []
    for k, name in zip(sorted(by_k), names):
        got = [tuple(l.split("\t")) for l in open(name).read().splitlines()]
        assert got == [(c, "%d" % p, r, a) for c, p, r, a in by_k[k]]
        assert all(int(p) % stride == k for _, p, _, _ in got)
        by_chrom = {}
        for c, p, _, _ in got:
            by_chrom.setdefault(c, []).append(int(p))
        assert all(b - a >= stride for ps in by_chrom.values() for a, b in zip(ps, ps[1:]))
        # (the lists are --spikeVariants files: the parser of the flags that exist takes them, and REF is the genome's letter)
        parsed = sv.parse_variants(name, "--spikeVariants")
        sv.check_reference(parsed, fasta.FastaFile(fa), "--spikeVariants")
        assert [(v.chrom, v.pos, v.ref, v.alt) for v in parsed] == by_k[k]
        seen += by_k[k]
    assert sorted(seen) == sorted(want)
    table = open(prefix + ".passes.txt").read().splitlines()
    assert table[0] == "#k\tvariants\tfile" and table[-1] == "#skipped\t2"
    assert table[1:-1] == ["%d\t%d\t%s" % (k, len(by_k[k]), n) for k, n in zip(sorted(by_k), names)]
    assert not os.path.exists("%s.pass%d.txt" % (prefix, stride))


def test_the_command_line_uses_the_tools_functions(tmp_path):
    fa, bed = _fasta(tmp_path), _bed(tmp_path)
    from smcounter_amd import bedops
    loc_list = bedops.expand_loci(bed)
    variants, skipped = lists.scan_variants(loc_list + loc_list[:3], fasta.FastaFile(fa), "transition")       # (a locus listed twice counts once)
    assert [(v.chrom, v.pos, v.ref, v.alt) for v in variants] == _expected("transition")[0]
    assert skipped == [("chrA", 5), ("chrA", 10)]
    assert all(v.kind == af.SNV and v.key == v.alt for v in variants)
    passes = lists.scan_passes(variants, 4)
    assert [k for k, _ in passes] == [0, 1, 2, 3] and sorted(i for _, m in passes for i in m) == list(range(len(variants)))
    with pytest.raises(ValueError, match="--spikeScanAlt"):
        lists.scan_variants(loc_list, fasta.FastaFile(fa), "none")
    with pytest.raises(ValueError, match="--spikeScanStride"):
        lists.scan_passes(variants, 0)
    import inspect
    src = inspect.getsource(cli._make_rules)
    assert "lists.scan_variants(" in src and "lists.scan_passes(" in src


# ---- the pages
def _entries(variants, targets, R):
    """Hand-made replicates: variant i is called in the first (i + 2 t) mod (R + 1) replicates of target t."""
    entries, full = {}, {}
    for i, v in enumerate(variants):
        for t in range(len(targets)):
            n_called = (i + 2 * t) % (R + 1)
            per, per_full = [], []
            for j in range(R):
                r = dict(N=100 + i, V0=i % 3, S=10 * t + j, READS=20 * t + 2 * j + i, V1=i % 3 + 10 * t + j)
                called = j < n_called
                per.append(spike.scan_entry(v, r, called))
                # (what --spikeReps holds for the same replicate: the row's fields and its cut)
                row = [""] * (dsaf._COL["PI"] + 1)
                row[dsaf._COL["PI"]] = "%.2f" % (30.0 + j if called else 3.0)
                per_full.append((r, row, (v.ref, [v.alt]) if called else None))
            entries[(i, t)], full[(i, t)] = per, per_full
    return entries, full


@pytest.mark.parametrize("with_lod", (False, True))
def test_page_writers_against_the_lines_of_spike_reps(tmp_path, with_lod):
    variants = [af.Variant("chrA", 3, "G", "A", "A", af.SNV), af.Variant("chrA", 7, "C", "T", "T", af.SNV),
                af.Variant("chrB", 4, "T", "C", "C", af.SNV), af.Variant("chrB", 5, "G", "A", "A", af.SNV),
                af.Variant("chrB", 6, "G", "A", "A", af.SNV)]          # (the last one is called in every replicate at 0.7: a T95)
    loci = [("chrA", 3, 0), ("chrA", 5, None), ("chrA", 7, 1), ("chrB", 4, 2), ("chrB", 5, 3), ("chrB", 6, 4)]
    targets, R = [0.7, 0.3], 4
    entries, full = _entries(variants, targets, R)
    lods = [0.0123, 1.0, 0.5, 0.25, 0.004] if with_lod else None
    prefix = str(tmp_path / "o")
    spike.write_scan(prefix, loci, variants, targets, entries, lods)
    drop = [spike.SENSITIVITY_HEADER.index(c) for c in ("PI_MEAN", "PI_MIN")]
    assert drop == [17, 18] and spike.SCAN_SENSITIVITY_HEADER == spike.SENSITIVITY_HEADER[:17]
    sens = open(prefix + ".spikeScan.sensitivity.txt").read().splitlines()
    assert sens[0].split("\t") == list(spike.SCAN_SENSITIVITY_HEADER) + (["LOD"] if with_lod else [])
    want = []
    for i, v in enumerate(variants):
        for t, target in enumerate(targets):
            f = spike.sensitivity_line(v, target, full[(i, t)]).split("\t")
            assert len(f) == 19
            want.append("\t".join(f[:17] + (["%.15g" % lods[i]] if with_lod else [])))
    assert sens[1:] == want
    curve = open(prefix + ".spikeScan.curve.txt").read().splitlines()
    assert curve[0].split("\t") == list(spike.curve_header(targets, with_lod))
    assert curve[1:] == [spike.curve_line(v, 100 + i, targets, [full[(i, t)] for t in range(2)], lods[i] if with_lod else None)
                         for i, v in enumerate(variants)]
    # the bedgraphs follow from the pages
    for t, target in enumerate(targets):
        got = open("%s.spikeScan%g.rate.bedgraph" % (prefix, target)).read().splitlines()
        assert got == ["%s\t%d\t%d\t%s" % (v.chrom, v.pos - 1, v.pos, want[i * 2 + t].split("\t")[7]) for i, v in enumerate(variants)]
    t95 = open(prefix + ".spikeScan.t95.bedgraph").read().splitlines()
    col = {(l.split("\t")[0], int(l.split("\t")[1])): l.split("\t")[curve[0].split("\t").index("T95")] for l in curve[1:]}
    assert set(col.values()) - {"NA"}, "no locus with a T95: the bedgraph's other branch is not exercised"
    assert t95 == ["%s\t%d\t%d\t%s" % (c, p - 1, p, "1" if i is None or col[(c, p)] == "NA" else col[(c, p)]) for c, p, i in loci]
    assert any(l.endswith("\t1") for l in t95) and "chrA\t4\t5\t1" in t95


def test_header_defines_the_entry_and_the_abi_number_stays():
    text = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"^int smc_scan_detect\(", text, re.M)
    assert re.search(r"^#define SMC_ABI_VERSION 11$", text, re.M)
    assert "smc_scan_detect" in _lib.SYMBOLS
    assert abi.SCAN_VERDICT_DTYPE.itemsize == 16 and abi.SCAN_LOCUS_DTYPE.itemsize == 8
    for name, value in (("NOT", abi.SCAN_NOT), ("CALLED", abi.SCAN_CALLED), ("HOST", abi.SCAN_HOST)):
        assert re.search(r"^#define SMC_SCAN_%s %du$" % (name, value), text, re.M)
    assert re.search(r"^#define SMC_SCAN_MT_MASK 0x3FFFFFFFu$", text, re.M) and abi.SCAN_MT_MASK == 0x3FFFFFFF
