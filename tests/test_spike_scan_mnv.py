"""--spikeScanMnv without a GPU: the MNV lists of tools.spike_scan_lists on a hand-made BED and FASTA and what parse_variants(phased=True)
reads from them, the skips, mnv_min_stride, every refusal before any file, the rule that no set is split over two decoded runs, the
page writers from hand-made entries, the entry's declaration and binding, and the joint rule in numpy."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, bedops, cli, devplanes, dsaf, fasta, spike
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_scan_lists as lists
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402

# chrA: an N at 5 and an R at 10 (1-based); chrB ends inside the BED's last interval's reach
FA = ("chrA", "ACGTNacgtRACGTACGTACG", "chrB", "TTTTGGGG")
# (unordered intervals, an interval that runs to the chromosome's end, and chrA 15-17 listed twice)
BED = "chrA\t14\t21\nchrA\t0\t12\nchrB\t2\t8\nchrA\t14\t17\n"


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
    open(path, "w").write(BED)
    return path


def _expected(L, alt):
    """The MNVs by the issue's words: in the BED's order, each locus once; skipped when a position of P .. P+L-1 is no locus of the
    target or its letter is not A, C, G or T."""
    seq = dict(zip(FA[::2], FA[1::2]))
    order, seen = [], set()
    for line in BED.splitlines():
        c, a, b = line.split("\t")
        for p in range(int(a) + 1, int(b) + 1):
            if (c, p) not in seen:
                seen.add((c, p))
                order.append((c, p))
    out, skipped = [], []
    for c, p in order:
        ok = all((c, q) in seen and q <= len(seq[c]) and seq[c][q - 1].upper() in "ACGT" for q in range(p, p + L))
        if not ok:
            skipped.append((c, p))
            continue
        ref = seq[c][p - 1:p - 1 + L].upper()
        out.append((c, p, ref, "".join(lists.ALT_RULES[alt][x] for x in ref)))
    return out, skipped


@pytest.mark.parametrize("alt", ("transition", "complement"))
@pytest.mark.parametrize("L,stride", ((2, 2), (2, 5), (3, 3), (3, 4)))
def test_mnv_lists_parse_into_sets_of_L_members_named_by_their_leader(tmp_path, L, stride, alt):
    fa, bed = _fasta(tmp_path), _bed(tmp_path)
    prefix = str(tmp_path / "scan")
    names = lists.main(argparse.Namespace(runPath=None, bedTarget=bed, refGenome=fa, stride=stride, alt=alt, mnv=L, outPrefix=prefix))
    want, skipped = _expected(L, alt)
    by_k = {}
    for c, p, ref, a in want:
        by_k.setdefault(p % stride, []).append((c, p, ref, a))
    assert names == ["%s.pass%d.txt" % (prefix, k) for k in sorted(by_k)]
    for k, name in zip(sorted(by_k), names):
        got = [tuple(l.split("\t")) for l in open(name).read().splitlines()]
        assert got == [(c, "%d" % p, r, a) for c, p, r, a in by_k[k]]
        parsed = sv.parse_variants(name, "--spikeVariants", phased=True)
        sv.check_reference(parsed, fasta.FastaFile(fa), "--spikeVariants")
        assert len(parsed.sets) == len(by_k[k]) and len(parsed) == L * len(by_k[k])
        for ps, (c, p, ref, a) in zip(parsed.sets, by_k[k]):
            assert ps.name == "%s:%d" % (c, p) and ps.chrom == c and len(ps.members) == L
            assert [(parsed[m].pos, parsed[m].ref, parsed[m].alt) for m in ps.members] == [(p + x, ref[x], a[x]) for x in range(L)]
            assert parsed[ps.members[0]].pos == p                    # the leader first
        assert sv.leaders(parsed) == [p for _, p, _, _ in by_k[k] for _ in range(L)]
    table = open(prefix + ".passes.txt").read().splitlines()
    assert table[-1] == "#skipped\t%d" % len(skipped)
    assert table[1:-1] == ["%d\t%d\t%s" % (k, len(by_k[k]), n) for k, n in zip(sorted(by_k), names)]


def test_scan_mnvs_skips_and_the_command_line_uses_the_tools_functions(tmp_path):
    fa, bed = _fasta(tmp_path), _bed(tmp_path)
    loc_list = bedops.expand_loci(bed)
    for L in (2, 3, 8):
        mnvs, leaders, skipped = lists.scan_mnvs(loc_list, fasta.FastaFile(fa), L, "transition")
        want, want_skipped = _expected(L, "transition")
        assert leaders == [(c, p) for c, p, _, _ in want] and skipped == want_skipped
        assert isinstance(mnvs, sv.PhasedVariants) and len(mnvs) == L * len(want) and len(mnvs.sets) == len(want)
        for i, (ps, (c, p, ref, alt)) in enumerate(zip(mnvs.sets, want)):
            assert ps == sv.PhaseSet("%s:%d" % (c, p), c, tuple(range(i * L, i * L + L)))
            assert [(mnvs[m].chrom, mnvs[m].pos, mnvs[m].ref, mnvs[m].alt, mnvs[m].kind) for m in ps.members] == \
                [(c, p + x, ref[x], alt[x], af.SNV) for x in range(L)]
        assert len(set(leaders) | set(skipped)) == len(leaders) + len(skipped) == len(set(loc_list))
    mnvs, leaders, skipped = lists.scan_mnvs(loc_list, fasta.FastaFile(fa), 2, "transition")
    # an N or an R anywhere in P .. P+1; the last locus of a BED interval; the chromosome's end; a locus listed twice counts once
    for cp in (("chrA", 4), ("chrA", 5), ("chrA", 9), ("chrA", 10), ("chrA", 12), ("chrA", 21), ("chrB", 8)):
        assert cp in skipped, cp
    assert leaders.count(("chrA", 15)) == 1 and leaders[0] == ("chrA", 15)          # (the BED's order: unordered intervals)
    passes = lists.mnv_passes(mnvs, 4)
    assert sorted(i for _, m in passes for i in m) == list(range(len(leaders)))
    assert all(leaders[i][1] % 4 == k for k, m in passes for i in m)
    one = lists.mnv_pass_variants(mnvs, passes[0][1])
    assert [s.name for s in one.sets] == ["%s:%d" % leaders[i] for i in passes[0][1]]
    assert [s.members for s in one.sets] == [(2 * r, 2 * r + 1) for r in range(len(one.sets))]
    with pytest.raises(ValueError, match="--spikeScanAlt"):
        lists.scan_mnvs(loc_list, fasta.FastaFile(fa), 2, "none")
    import inspect
    src = inspect.getsource(cli._make_rules)
    assert "lists.scan_mnvs(" in src and "lists.mnv_passes(" in src


def test_mnv_min_stride():
    assert [lists.mnv_min_stride(L) for L in range(2, 9)] == list(range(2, 9))
    lists.check_mnv_stride(3, 3)
    with pytest.raises(ValueError, match=re.escape("the smallest stride allowed is 3")):
        lists.check_mnv_stride(3, 2)
    for bad in (1, 9, 0, "x", "2.5", None):
        with pytest.raises(ValueError, match=re.escape("an integer in 2 .. 8 expected")):
            lists.parse_mnv(bad)
    assert lists.parse_mnv("4") == 4 and lists.parse_mnv(8) == 8


# ---- the refusals
def _args(tmp, **kw):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp))
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    d = dict(outPrefix=str(tmp / "o"), bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, refGenome=fa, spikeScan="0.3,0.7",
             spikeScanReps="4", spikeScanStride="8", spikeScanMnv="2")
    d.update(kw)
    return {k: v for k, v in d.items() if v is not None}


@pytest.mark.parametrize("kw,msg", [
    (dict(spikeScan=None, spikeScanReps=None, spikeScanStride=None), "--spikeScanMnv belongs to --spikeScan: it needs --spikeScan"),
    (dict(spikeScanMnv="1"), "--spikeScanMnv: an integer in 2 .. 8 expected"),
    (dict(spikeScanMnv="9"), "--spikeScanMnv: an integer in 2 .. 8 expected"),
    (dict(spikeScanMnv="2.5"), "--spikeScanMnv: an integer in 2 .. 8 expected"),
    (dict(spikeScanMnv="two"), "--spikeScanMnv: an integer in 2 .. 8 expected"),
    (dict(spikeScanMnv="3", spikeScanStride="2"), "the smallest stride allowed is 3"),
    (dict(spikeScanMnv="8", spikeScanStride="7"), "the smallest stride allowed is 8"),
    (dict(spikeScanIndel="del1", spikeScanStride="8"), "--spikeScanMnv cannot be combined with --spikeScanIndel"),
    (dict(spikeScanDepth="0.5"), "--spikeScanMnv cannot be combined with --spikeScanDepth: the depth axis of an MNV scan is not built"),
    (dict(spikeScanRpb="2"), "--spikeScanMnv cannot be combined with --spikeScanRpb: the reads-per-barcode axis of an MNV scan is not built"),
    (dict(spikeScanFilter=True), "--spikeScanMnv cannot be combined with --spikeScanFilter: the filter axis of an MNV scan is not built"),
    # everything --spikeScan refuses
    (dict(spikeScanReps=None), "it needs --spikeScanReps"),
    (dict(spikeReps="4"), "--spikeScan cannot be combined with --spikeReps"),
    (dict(dsMT="0.5"), "--spikeScan cannot be combined with --dsMT"),
    (dict(spikeScanAlt="transversal"), "--spikeScanAlt: one of complement, transition, transversion expected"),
    (dict(spikeScanBuild="some"), "--spikeScanBuild: whole or listed expected"),
])
def test_cli_refusals_before_any_file(tmp_path, kw, msg):
    args = _args(tmp_path, **kw)
    if args.pop("spikeScanFilter", False):       # (a switch)
        args = cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in args.items()] + ["--spikeScanFilter"])
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(args)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_more_processes_are_refused_and_the_flags_are_read(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--spikeScan runs in one process only"):
        cli.main(_args(tmp_path))
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]
    ns = argparse.Namespace(spikeScan="0.7,0.3", spikeScanReps="32", spikeScanMnv="3", spikeScanStride=3, spikeScanBuild="listed")
    assert spike.scan(ns) == dict(targets=[0.7, 0.3], reps=32, stride=3, alt="transition", mnv=3, build="listed")
    # without the flag the dict is the scan's own
    assert spike.scan(argparse.Namespace(spikeScan="0.7,0.3", spikeScanReps="32")) == dict(targets=[0.7, 0.3], reps=32, stride=256, alt="transition")
    with pytest.raises(ValueError, match="not built"):
        devplanes.spike_scan("x.bam", None, sv.PhasedVariants(), [], [0.5], None, 1, 2, None, 5, None, mnv=2, flt=True)


# ---- no set is split over two decoded runs
def _mnvs(leaders, L):
    members, sets = [], []
    for c, p in leaders:
        sets.append(sv.PhaseSet("%s:%d" % (c, p), c, tuple(range(len(members), len(members) + L))))
        members += [af.Variant(c, p + x, "A", "G", "G", af.SNV) for x in range(L)]
    return sv.PhasedVariants(members, sets)


def _walk(mnvs, order, nl_of):
    """The stage's loop over _set_spans: nl_of(lo, hi) is what the decoded run gives back -> per run (chrom, lo, the sets taken)."""
    runs = []
    spans = devplanes._set_spans(mnvs, mnvs.sets, order)
    for chrom, lo, hi, span in spans:
        taken = devplanes.sets_inside(mnvs, mnvs.sets, span, lo, nl_of(lo, hi))
        assert taken and taken == span[:len(taken)]
        runs.append((chrom, lo, hi, taken))
        spans.send(len(taken))
    return runs


def test_a_set_is_never_split_over_two_decoded_runs():
    assert devplanes.AF_RUN_LOCI == 512
    L = 3
    # leaders 1000 .. 1000 + 509 fit the window with their last member; 1510 (last member 1512) does not: deferred whole
    leaders = [("chrA", 1000 + 10 * x) for x in range(0, 52)] + [("chrB", 7), ("chrB", 600)]
    mnvs = _mnvs(leaders, L)
    order = list(range(len(leaders)))
    runs = _walk(mnvs, order, lambda lo, hi: hi - lo)
    assert [(c, lo, hi) for c, lo, hi, _ in runs] == [("chrA", 999, 1502), ("chrA", 1509, 1512), ("chrB", 6, 9), ("chrB", 599, 602)]
    assert runs[0][3] == list(range(51)) and runs[1][3] == [51]
    # the set at 1510 straddles the 512-position window of the run that starts at 1000 (1510, 1511 inside, 1512 not): deferred whole
    leaders = [("chrA", 1000), ("chrA", 1510), ("chrA", 1520)]
    runs = _walk(_mnvs(leaders, L), [0, 1, 2], lambda lo, hi: hi - lo)
    assert [(lo, hi, taken) for _, lo, hi, taken in runs] == [(999, 1002, [0]), (1509, 1522, [1, 2])]
    # a decoded run that comes back shorter than asked: the set it cuts is deferred whole and starts the next run
    leaders = [("chrA", 100 + 4 * x) for x in range(20)]
    mnvs = _mnvs(leaders, L)
    short = lambda lo, hi: min(hi - lo, 42)                      # 42 loci: sets at +0 .. +36 whole, the one at +40 is cut
    runs = _walk(mnvs, list(range(20)), short)
    assert runs[0][3] == list(range(10)) and runs[1][1] == 139 and runs[1][3] == list(range(10, 20))
    for _, lo, hi, taken in runs:
        nl = short(lo, hi)
        for i in taken:
            assert all(0 <= mnvs[k].pos - 1 - lo < nl for k in mnvs.sets[i].members)
    # every leader is handed out exactly once, whatever the run gives back
    rng = np.random.default_rng(3)
    leaders = sorted({("chrA", int(p)) for p in rng.integers(1, 5000, 300)}) + sorted({("chrB", int(p)) for p in rng.integers(1, 900, 60)})
    mnvs = _mnvs(leaders, 8)
    for nl_of in (lambda lo, hi: hi - lo, lambda lo, hi: max(8, (hi - lo) // 2), lambda lo, hi: max(8, hi - lo - 3)):
        runs = _walk(mnvs, list(range(len(leaders))), nl_of)
        assert [i for r in runs for i in r[3]] == list(range(len(leaders)))
        for c, lo, hi, taken in runs:
            assert all(mnvs.sets[i].chrom == c and lo <= mnvs[k].pos - 1 < lo + nl_of(lo, hi) for i in taken for k in mnvs.sets[i].members)
            assert hi - lo <= devplanes.AF_RUN_LOCI


# ---- the pages
def test_page_writers_from_hand_made_entries(tmp_path):
    leaders = [("chrA", 3), ("chrA", 7), ("chrB", 4), ("chrB", 6)]
    mnvs = _mnvs(leaders, 2)
    loci = [("chrA", 3, 0), ("chrA", 5, None), ("chrA", 7, 1), ("chrB", 4, 2), ("chrB", 5, None), ("chrB", 6, 3)]
    targets, R, mt_depth = [0.7, 0.3], 4, 250
    entries = {}
    for i in range(len(leaders)):
        for t in range(len(targets)):
            n_called = R if (i == 3 and t == 0) else (i + 2 * t) % (R + 1)          # (the last set is called in every replicate at 0.7: a T95)
            entries[(i, t)] = [(dict(N_ALL=90 + i, V0_ALL=i % 2, S_ALL=10 * t + j, V1_ALL=i % 2 + 10 * t + j), int(j < n_called))
                               for j in range(R)]
    prefix = str(tmp_path / "o")
    spike.write_scan_mnv(prefix, loci, mnvs, mnvs.sets, targets, mt_depth, entries)
    sens = open(prefix + ".spikeScan.mnv.sensitivity.txt").read().splitlines()
    assert sens[0].split("\t") == list(spike.PHASE_SENSITIVITY_HEADER)
    want = [spike.phase_sensitivity_line(ps, mnvs, target, None, mt_depth, entries[(i, t)])
            for i, ps in enumerate(mnvs.sets) for t, target in enumerate(targets)]
    assert sens[1:] == want
    f = sens[1].split("\t")
    assert f[:8] == ["chrA:3", "chrA", "3,4", "A,A", "G,G", "0.7", "full", "250"]
    curve = [l.split("\t") for l in open(prefix + ".spikeScan.mnv.curve.txt").read().splitlines()]
    assert curve[0] == ["CHROM", "POS", "REF", "ALT", "N_ALL", "RATE@0.3", "RATE@0.7", "T95"]
    i_rate, i_called = spike.PHASE_SENSITIVITY_HEADER.index("RATE"), spike.PHASE_SENSITIVITY_HEADER.index("CALLED_ALL")
    for i, (c, p) in enumerate(leaders):
        rates = [sum(called for _, called in entries[(i, t)]) / float(R) for t in range(2)]
        best = dsaf.t95(targets, rates)
        assert curve[1 + i] == [c, "%d" % p, "AA", "GG", "%d" % (90 + i), dsaf.frac_text(rates[1]), dsaf.frac_text(rates[0]),
                                dsaf.NA if best is None else "%g" % best]
        # (the curve recomputed from the sensitivity page: RATE is the page's text)
        assert [curve[1 + i][6], curve[1 + i][5]] == [want[2 * i + t].split("\t")[i_rate] for t in range(2)]
        assert [int(want[2 * i + t].split("\t")[i_called]) for t in range(2)] == [int(round(r * R)) for r in rates]
    # the bedgraphs follow from the pages
    for t, target in enumerate(targets):
        got = open("%s.spikeScan%g.mnv.rate.bedgraph" % (prefix, target)).read().splitlines()
        assert got == ["%s\t%d\t%d\t%s" % (c, p - 1, p, want[2 * i + t].split("\t")[i_rate]) for i, (c, p) in enumerate(leaders)]
    t95 = open(prefix + ".spikeScan.mnv.t95.bedgraph").read().splitlines()
    col = {(f[0], int(f[1])): f[7] for f in curve[1:]}
    assert set(col.values()) - {"NA"} and "NA" in col.values()
    assert t95 == ["%s\t%d\t%d\t%s" % (c, p - 1, p, "1" if i is None or col[(c, p)] == "NA" else col[(c, p)]) for c, p, i in loci]
    assert "chrA\t4\t5\t1" in t95
    assert sorted(f for f in os.listdir(str(tmp_path))) == sorted(["o.spikeScan.mnv.sensitivity.txt", "o.spikeScan.mnv.curve.txt",
                                                                    "o.spikeScan0.7.mnv.rate.bedgraph", "o.spikeScan0.3.mnv.rate.bedgraph",
                                                                    "o.spikeScan.mnv.t95.bedgraph"])


# ---- the entry
def test_the_entry_is_declared_and_bound_and_the_abi_number_stays():
    text = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"^int smc_scan_detect_sets\(", text, re.M) and re.search(r"^int smc_scan_detect\(", text, re.M)
    assert re.search(r"^#define SMC_ABI_VERSION 11$", text, re.M) and re.search(r"^#define SMC_SPIKE_PHASE_MAX_MEMBERS 8$", text, re.M)
    assert "smc_scan_detect_sets" in _lib.SYMBOLS
    host = open(os.path.join(ROOT, "smcounter_amd", "csrc", "host_abi.inc")).read()
    kern = open(os.path.join(ROOT, "smcounter_amd", "csrc", "k_scan_detect.inc")).read()
    assert re.search(r"^int smc_scan_detect_sets\(", host, re.M) and "k_scan_detect_sets" in host
    # one shared device function for the member rule
    assert kern.count("scd_member(rows, n_loci, c, listed[g], lo, hi, rec)") == 2 and kern.count("__device__ __forceinline__ uint32_t scd_member(") == 1
    L = _lib.load()
    assert L.smc_abi_version() == 11 and hasattr(L, "smc_scan_detect_sets")
    assert len(L.smc_scan_detect_sets.argtypes) == 16
    assert callable(devplanes.scan_detect_sets)


def test_the_joint_rule_in_numpy():
    N, C, H = abi.SCAN_NOT, abi.SCAN_CALLED, abi.SCAN_HOST
    verdicts = np.array([[C, C, C, H, C, N, H, C],
                         [N, H, C, C, H, H, H, H]])
    off = [0, 1, 3, 6, 8]
    words, listed = abi.scan_joint_rule(verdicts, off)
    assert words.dtype == np.uint32 and listed.dtype == np.uint32
    assert words.tolist() == [[(C << 30) | 0x1, (C << 30) | 0x3, (N << 30) | 0x2 | (0x1 << 8) | (0x4 << 16), (H << 30) | 0x2 | (0x1 << 8)],
                              [(N << 30) | (0x1 << 16), (H << 30) | 0x2 | (0x1 << 8), (H << 30) | 0x1 | (0x6 << 8), (H << 30) | (0x3 << 8)]]
    # a HOST member beside a NOT member (copy 0, record 3) decides nothing and is not listed
    assert listed.tolist() == [6, 8 + 1, 8 + 4, 8 + 5, 8 + 6, 8 + 7]
    assert np.array_equal(devplanes.scan_joint_members(words, off), verdicts)
    words, listed = abi.scan_joint_rule(np.zeros((3, 0), np.int64), [0])
    assert words.shape == (3, 0) and len(listed) == 0
