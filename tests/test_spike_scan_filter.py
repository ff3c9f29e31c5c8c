"""--spikeScanFilter without a GPU: the refusal before any file, the neighbours' messages, the header entry; the two words per listed
variant on a hand-made FASTA and hand-made repeat BEDs; the host twin of the kernel against the FILTER column rows.format_row and
postfilter.apply_repeat_filters print for the same rows; a printed FILTER column as a word; the page writers and the bedgraphs on
hand-made replicates (scan_filter_pages restates them from the FILTER and CALLED columns)."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, cli, fasta, postfilter, rows, spike
from smcounter_amd.params import VcParams
from smcounter_amd.pileup import BASE_ALLELES
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import scan_filter_pages as pages  # noqa: E402

HOST = abi.SCAN_FLT_HOST


# ---- the command line
def _argv(tmp, **kw):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp))
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    d = dict(outPrefix=str(tmp / "o"), bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, refGenome=fa)
    d.update(kw)
    return ["--%s=%s" % (k, v) for k, v in d.items() if v is not None]


def test_the_switch_is_refused_without_the_scan_before_any_file(tmp_path):
    for more in ({}, dict(spikeScanReps="4")):
        with pytest.raises(SystemExit, match=re.escape("--spikeScanFilter belongs to --spikeScan: it needs --spikeScan")
                           if not more else "belongs to --spikeScan: it needs --spikeScan"):
            cli.main(cli.build_parser().parse_args(_argv(tmp_path, **more) + ["--spikeScanFilter"]))
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]
    # (with the scan it still needs the replicates)
    with pytest.raises(SystemExit, match="it needs --spikeScanReps"):
        cli.main(cli.build_parser().parse_args(_argv(tmp_path, spikeScan="0.3") + ["--spikeScanFilter"]))
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_scan_reads_the_switch_beside_every_axis():
    base = dict(targets=[0.3], reps=4, stride=256, alt="transition")
    ns = dict(spikeScan="0.3", spikeScanReps="4")
    assert spike.scan(argparse.Namespace(**ns)) == base
    assert spike.scan(argparse.Namespace(spikeScanFilter=False, **ns)) == base
    assert spike.scan(argparse.Namespace(spikeScanFilter=True, **ns)) == dict(base, filter=True)
    assert spike.scan(argparse.Namespace(spikeScanFilter=True, spikeScanAlt="complement", **ns)) == dict(base, alt="complement", filter=True)
    assert spike.scan(argparse.Namespace(spikeScanFilter=True, spikeScanIndel="del1", **ns)) == dict(base, indel=("del", 1), filter=True)
    assert spike.scan(argparse.Namespace(spikeScanFilter=True, spikeScanDepth="0.5", **ns)) == dict(base, fracs=[0.5], filter=True)
    assert spike.scan(argparse.Namespace(spikeScanFilter=True, spikeScanRpb="4", **ns)) == dict(base, rpbs=[4.0], filter=True)
    assert spike.scan(argparse.Namespace(spikeScanFilter=False)) is None
    assert "--spikeScanFilter" in cli.build_parser().format_help()


@pytest.mark.parametrize("kw,msg", [
    (dict(spikeScanReps="4"), "--spikeScanReps belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScanStride="8"), "--spikeScanStride belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScanAlt="transition"), "--spikeScanAlt belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScanIndel="del1"), "--spikeScanIndel belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScanDepth="0.5"), "--spikeScanDepth belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScanRpb="4"), "--spikeScanRpb belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScan="0.3", spikeScanReps="4", spikeReps="4"), "--spikeScan cannot be combined with --spikeReps"),
    (dict(spikeScan="0.3", spikeScanReps="4", spikeScanRpb="4", spikeScanDepth="0.5"),
     "--spikeScanRpb cannot be combined with --spikeScanDepth in one run"),
    (dict(spikeReps="4"), "--spikeReps replicates the spike-ins of --spikeAF: it needs --spikeAF"),
])
def test_the_neighbours_messages_are_unchanged_without_the_flag(tmp_path, kw, msg):
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(cli.build_parser().parse_args(_argv(tmp_path, **kw)))
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_header_defines_the_entry_and_the_abi_number_stays():
    text = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"^int smc_scan_filter\(", text, re.M)
    assert re.search(r"^#define SMC_ABI_VERSION 11$", text, re.M)
    assert "smc_scan_filter" in _lib.SYMBOLS
    for name, value in (("SMC_F_REPT", abi.F_REPT), ("SMC_F_REPS", abi.F_REPS), ("SMC_F_SL", abi.F_SL), ("SMC_F_OTHER_REPEAT", abi.F_OTHER_REPEAT),
                        ("SMC_SCAN_FLT_HOST", abi.SCAN_FLT_HOST)):
        assert re.search(r"^#define %s 0x0*%Xu\b" % (name, value), text, re.M), name
    assert [abi.F_REPT, abi.F_REPS, abi.F_SL, abi.F_OTHER_REPEAT] == [1 << 10, 1 << 11, 1 << 12, 1 << 13] and abi.SCAN_FLT_HOST == 1 << 31
    # the 14 names in the issue's order, bit k the k-th name
    assert tuple(n for _, n in abi.SCAN_FILTER_NAMES) == pages.NAMES == spike.SCAN_FILTER_NAMES
    assert [b for b, _ in abi.SCAN_FILTER_NAMES] == [1 << k for k in range(14)]
    assert spike.SCAN_FILTER_HEADER == pages.HEADER


# ---- the two words per listed variant
HP_LEN = 4
BG = "ACGTCAGTGCATGACTCGAT"                      # no run of 4, no window of 8 with two letters
# 1 .. 20 background, 21 .. 24 a homopolymer of hpLen, 25 .. 44 background, 45 .. 56 (AT)6: low complexity, 57 .. 76 background
SEQ = BG + "AAAA" + "CGTCAGTGCATGACTCGATC" + "ATATATATATAT" + "CGTCAGTGCATGACTCGATC"
TRF = "chrA\t29\t33\n"
# (RepeatMasker codes of all four kinds with a gap between them - touching intervals would merge -, and two codes on one interval)
RM = ("chrA\t57\t59\tSimple_repeat\nchrA\t60\t62\tLow_complexity\nchrA\t63\t65\tSatellite\nchrA\t66\t68\tLINE\n"
      "chrA\t69\t72\tSimple_repeat\nchrA\t69\t72\tSatellite\n")


def _genome(tmp):
    path = str(tmp / "g.fa")
    open(path, "w").write(">chrA\n%s\n" % SEQ)
    open(path + ".fai", "w").write("chrA\t%d\t6\t%d\t%d\n" % (len(SEQ), len(SEQ), len(SEQ) + 1))
    for name, text in (("t.bed", "chrA\t0\t%d\n" % len(SEQ)), ("trf.bed", TRF), ("rm.bed", RM)):
        open(str(tmp / name), "w").write(text)
    trf, rm = postfilter.load_repeat_regions(str(tmp / "t.bed"), str(tmp / "trf.bed"), str(tmp / "rm.bed"))
    return fasta.FastaFile(path), trf, rm


def _snv(pos, alt=None):
    ref = SEQ[pos - 1]
    alt = alt or ("G" if ref != "G" else "A")
    return af.Variant("chrA", pos, ref, alt, alt, af.SNV)


def test_the_words_on_a_hand_made_genome_and_hand_made_repeats(tmp_path):
    fa, trf, rm = _genome(tmp_path)
    HP, LOWC, T, S, SL, O = abi.F_HP, abi.F_LOWC, abi.F_REPT, abi.F_REPS, abi.F_SL, abi.F_OTHER_REPEAT
    want = {
        22: (HP, 0),            # inside the homopolymer
        25: (HP, 0),            # next to it: the window of hpLen letters to the left is the run
        19: (0, 0),             # just outside on the left: three of the run's letters in reach
        26: (0, 0),             # just outside on the right
        50: (LOWC, 0),          # inside (AT)6: a window of 2 x hpLen letters with two kinds
        40: (0, 0),
        29: (0, 0),             # the interval's start is open: chrA 29 33 covers 30 .. 33
        30: (0, T), 33: (0, T),
        34: (0, 0),             # ... and its end closed
        57: (LOWC, 0), 58: (0, S), 59: (0, S), 60: (0, 0),
        61: (0, LOWC), 62: (0, LOWC),                       # RepeatMasker's Low_complexity is LowC, not gated
        64: (0, SL), 67: (0, O), 68: (0, O), 69: (0, 0),
        70: (0, S | SL), 72: (0, S | SL), 73: (0, 0),       # two codes on one interval
    }
    variants = [_snv(p) for p in sorted(want)]
    gate, always = spike.scan_filter_words(variants, HP_LEN, fa, trf, rm)
    assert gate.dtype == always.dtype == np.uint32
    got = {v.pos: (int(g), int(a)) for v, g, a in zip(variants, gate, always)}
    assert got == want
    # (an ALT that makes the run: chrA:20 T>A gives AAAAA)
    g, _ = spike.scan_filter_words([_snv(26, "A"), _snv(27, "A")], HP_LEN, fa, trf, rm)
    assert g.tolist() == [0, 0]
    g, _ = spike.scan_filter_words([af.Variant("chrA", 17, "CGAT", "C", "DEL|CGAT|C", af.DEL)], HP_LEN, fa, trf, rm)
    assert g.tolist() == [HP]                                # the deletion joins nothing new, but its right flank is the run
    # no repeat files: no always bits
    nothing = postfilter.load_repeat_regions(str(tmp_path / "t.bed"), None, None)
    assert spike.scan_filter_words(variants, HP_LEN, fa, *nothing)[1].tolist() == [0] * len(variants)


# ---- the host twin against the printed FILTER column
EDGE = 4.995
LO, HI = EDGE - 1e-6, EDGE + 1e-6
ALL_DEVICE = abi.F_LM | abi.F_LSM | abi.F_DP | abi.F_SB | abi.F_LOWQ | abi.F_R1CP | abi.F_R2CP | abi.F_PRIMERCP


def _row(alt_letter, pi, applied, flt, below, bi=0, status=0):
    r = np.zeros(1, abi.ROW_DTYPE)
    r["cvg"], r["all_frag"], r["all_mt"], r["used_frag"], r["used_mt"] = 400, 400, 120, 380, 100
    r["dp"], r["umt"], r["vsm"], r["pi"] = 100, 25, 20, 1.5
    c = r["cand"]
    c["allele"][0, 0], c["allele"][0, 1] = BASE_ALLELES.index(alt_letter), -1
    c["vdp"], c["vmt"], c["vsm"], c["pi"] = 40, 12, 9, 0.0
    c["pi"][0, 0], c["flt_applied"][0, 0], c["flt"][0, 0], c["vmf_lt_099"][0, 0] = pi, applied, flt, below
    r["biallelic"], r["status"] = bi, status
    if bi:
        c["allele"][0, 1], c["pi"][0, 1] = (BASE_ALLELES.index(alt_letter) + 1) % 4, 45.0
    return r[0]


def _printed_filter(row, v, P, fa, trf, rm):
    text = rows.format_row(row, v.chrom, v.pos, v.ref, list(BASE_ALLELES), P, fa)
    return list(postfilter.apply_repeat_filters([text], trf, rm))[0].split("\t")[-1]


def test_the_host_twin_equals_the_printed_filter_column(tmp_path):
    fa, trf, rm = _genome(tmp_path)
    P = VcParams(mtDepth=250, rpb=3.0, hpLen=HP_LEN)
    variants = [_snv(p) for p in (22, 40, 50, 31, 58, 61, 64, 67, 70)]
    gate, always = spike.scan_filter_words(variants, HP_LEN, fa, trf, rm)
    above, below_edge = float(np.nextafter(HI, np.inf)), float(np.nextafter(LO, -np.inf))
    seen = set()
    for v, g, a in zip(variants, gate.tolist(), always.tolist()):
        for flt in [0, ALL_DEVICE] + [b for b, n in abi.FILTER_NAMES if b not in (abi.F_HP, abi.F_LOWC)]:
            for below in (0, 1):
                for pi, applied in ((40.0, 1), (5.0, 1), (above, 0), (4.9951, 0), (4.9949, 0), (below_edge, 0), (3.0, 0), (40.0, 0)):
                    row = _row(v.alt, pi, applied, flt if applied else 0xFFFFFFFF, below)
                    w = spike.scan_filter_host(row, g, a)
                    assert not w & HOST and not w & ~abi.SCAN_FLT_NAMES_MASK
                    text = _printed_filter(row, v, P, fa, trf, rm)
                    assert w == spike.scan_filter_of_text(text), (v, flt, below, pi, applied, text, hex(w))
                    if not applied:
                        assert not w & abi.SCAN_FLT_DEVICE_MASK & ~a           # garbage in flt does not show
                    seen.add(text)
    print("%d different FILTER columns" % len(seen))
    assert "PASS" in seen and len(seen) > 40
    for name in pages.NAMES:
        assert any(name in s.split(";") for s in seen), name
    # what the kernel leaves to the host, with the reason
    v, g, a = variants[3], int(gate[3]), int(always[3])
    for row in (_row(v.alt, EDGE, 0, 0, 1), _row(v.alt, LO, 0, 0, 1), _row(v.alt, HI, 0, 0, 1), _row(v.alt, float("nan"), 0, 0, 1),
                _row(v.alt, 40.0, 1, 0, 1, bi=1), _row(v.alt, 40.0, 1, 0, 1, status=abi.ST_ZERO_COVERAGE), _row(v.alt, 40.0, 2, 0, 1),
                _row(v.alt, 40.0, -1, 0, 1)):
        assert spike.scan_filter_host(row, g, a) & HOST
    # (inside the band py2's round decides: the two sides of 4.995 print differently, which is why the kernel does not)
    assert _printed_filter(_row(v.alt, 4.9951, 0, 0, 1), v, P, fa, trf, rm) == "RepT"
    assert _printed_filter(_row(v.alt, 4.9949, 0, 0, 1), v, P, fa, trf, rm) == "PASS"


def test_a_printed_filter_column_as_a_word():
    assert spike.scan_filter_of_text("PASS") == 0
    for k, name in enumerate(pages.NAMES):
        assert spike.scan_filter_of_text(name) == 1 << k
    assert spike.scan_filter_of_text(";".join(pages.NAMES)) == abi.SCAN_FLT_NAMES_MASK
    assert spike.scan_filter_of_text("HP;LowC;RepT;LowC") == abi.F_HP | abi.F_LOWC | abi.F_REPT          # a name counts once
    for bad in ("Zero_Coverage", "", ";", "HP;", "PASS;HP"):
        with pytest.raises(ValueError):
            spike.scan_filter_of_text(bad)


# ---- the pages
FILTERS = ("PASS", "HP", "RepT", "HP;LowC;RepT;LowC", "SB;R1CP", "PASS", "LM;LSM;DP;LowQ;R2CP;PrimerCP", "RepS;SL", "Other_Repeat", "PASS")


def _replicates(i, t, R):
    """Hand-made: variant i at target t is called in the first (2 i + 3 t) mod (R + 1) replicates; FILTER walks through FILTERS - but
    variant 4 passes wherever it is called, and is called everywhere at the larger target."""
    n_called = (R if t == 0 else 2) if i == 4 else (2 * i + 3 * t) % (R + 1)
    return [("PASS" if i == 4 else FILTERS[(i + 3 * t + j) % len(FILTERS)], 1 if j < n_called else 0) for j in range(R)]


def _arrays(V, T, R, extra=()):
    shape = (V, T) + tuple(extra) + (R,)
    called, words = np.zeros(shape, bool), np.zeros(shape, np.uint32)
    per = {}
    for idx in np.ndindex(*shape[:-1]):
        reps = _replicates(idx[0], idx[1] + sum(idx[2:]), R)
        per[idx] = reps
        for j, (f, c) in enumerate(reps):
            called[idx + (j,)] = bool(c)
            # (a word means something only where the replicate is called: garbage elsewhere must not count)
            words[idx + (j,)] = spike.scan_filter_of_text(f) if c else 0x3FFF
    return called, words, per


def test_page_writers_and_bedgraphs_on_hand_made_replicates(tmp_path):
    variants = [_snv(p) for p in (3, 7, 22, 50, 60)]
    loci = [("chrA", 3, 0), ("chrA", 5, None), ("chrA", 7, 1), ("chrA", 22, 2), ("chrA", 50, 3), ("chrA", 60, 4)]
    targets, R = [0.7, 0.3], 5
    ns = [100 + i for i in range(5)]
    called, words, per = _arrays(5, 2, R)
    prefix = str(tmp_path / "o")
    spike.write_scan_filter(prefix, loci, variants, targets, ns, called, words)
    page = [l.split("\t") for l in open(prefix + ".spikeScan.filter.txt").read().splitlines()]
    assert page[0] == list(pages.HEADER)
    want = [pages.line([v.chrom, "%d" % v.pos, v.ref, v.alt, "%g" % t], per[(i, k)]) for i, v in enumerate(variants) for k, t in enumerate(targets)]
    assert page[1:] == want
    i_c, i_p = pages.HEADER.index("CALLED"), pages.HEADER.index("PASS")
    assert any(int(f[i_p]) < int(f[i_c]) for f in want) and any(int(f[i_p]) == int(f[i_c]) > 0 for f in want)
    assert all(sum(int(f[pages.HEADER.index(n)]) for f in want) > 0 for n in pages.NAMES), "a name no hand-made replicate holds"
    curve = [l.split("\t") for l in open(prefix + ".spikeScan.filter.curve.txt").read().splitlines()]
    assert curve[0] == ["CHROM", "POS", "REF", "ALT", "N", "RATE_PASS@0.3", "RATE_PASS@0.7", "T95_PASS"]
    assert curve[1:] == [pages.curve_line([v.chrom, "%d" % v.pos, v.ref, v.alt], ns[i], targets, [per[(i, 0)], per[(i, 1)]])
                         for i, v in enumerate(variants)]
    t95 = pages.check_bedgraphs(prefix, targets, [(c, p) for c, p, _ in loci], page, curve)
    assert "chrA\t4\t5\t1" in t95 and "chrA\t59\t60\t0.7" in t95          # a skipped locus; a T95_PASS
    assert sum(1 for l in t95 if l.endswith("\t1")) == 5
    # the cells' pages: the same line with the axis column and MTDEPTH behind TARGET
    for axis, infix, name, values, mts in ((spike.DEPTH_AXIS, "depth", "FRACTION", [0.5, 0.25], [125, 62]),
                                           (spike.RPB_AXIS, "rpb", "RPB", [4.0, 2.5], [250, 250])):
        called, words, per = _arrays(5, 2, R, (2,))
        spike.write_scan_filter_cells(prefix, variants, targets, values, mts, called, words, axis)
        got = [l.split("\t") for l in open("%s.spikeScan.%s.filter.txt" % (prefix, infix)).read().splitlines()]
        assert got[0] == list(pages.HEADER[:5]) + [name, "MTDEPTH"] + list(pages.HEADER[5:])
        assert got[1:] == [pages.line([v.chrom, "%d" % v.pos, v.ref, v.alt, "%g" % t], per[(i, k, f)], ["%g" % values[f], "%d" % mts[f]])
                           for i, v in enumerate(variants) for k, t in enumerate(targets) for f in range(2)]
