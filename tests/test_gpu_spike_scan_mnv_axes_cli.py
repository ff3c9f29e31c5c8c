"""--spikeScanMnvFilter and --spikeScanMnvDepth on the GPU, through the command line: the small synthetic input of test_gpu_spike with L = 2, S = 4, R = 4 and
the targets 0.5 and 0.3, and a --bedTandemRepeats file over the lower half of the scanned positions - its interval ends between the two
members of one scanned MNV, so that member is RepT and its neighbour is not.  Every line of the new pages is restated from the member
SNVs' FILTER and CALLED columns in .spikeAF.replicates.txt of the passes' own --spikeAF --spikeVariants pass<k>.txt --spikeReps R
--spikePhase runs: CALLED_ALL_j = every member CALLED, PASS_ALL_j = CALLED_ALL_j and every member's FILTER exactly PASS, a name
tallied once per replicate with CALLED_ALL_j in which a member holds it.  Every file of the MNV scan without the switch stays byte for
byte; --spikeScanBuild whole and listed give equal files; the run log's closing line carries the new counts; with --lod the LOD files
are unchanged and the new pages have no LOD column.
With --spikeScanMnvDepth 0.5 - alone and beside the switch - every line of the depth pages is restated from the same passes run with
--spikeDepth 0.5 beside --spikeReps --spikePhase: the sensitivity lines byte for byte the set's cell lines of
.spikeAF.phase.sensitivity.txt, the curve, need page and bedgraphs from them and from N_ALL of .spikeAF.phase.replicates.txt, and
.spikeScan.mnv.depth.filter.txt from the members' lines of .spikeAF.depth.replicates.txt.
(The input is called at --rpb 2.9: at its own 3 every called record holds LSM - test_gpu_spike_scan_filter_cli.py measured it - and no
set could be PASS.)"""
import argparse
import dataclasses
import os
import re
import sys

import pytest

from conftest import ROOT
from smcounter_amd import devplanes, dsaf, spike
from smcounter_amd.tools import spike_scan_lists as lists

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import scan_filter_pages as pages  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line)
import test_gpu_spike as TS  # noqa: E402  (the small inputs)
import test_gpu_spike_scan_filter_cli as TF  # noqa: E402  (the repeat track over the lower half, the files of a prefix)

pytestmark = pytest.mark.gpu
SEED = 20240607
L, STRIDE, REPS, TARGETS = 2, 4, 4, (0.5, 0.3)
FRAC = 0.5
HEADER = list(spike.SCAN_MNV_FILTER_HEADER)
PHASE = list(spike.PHASE_SENSITIVITY_HEADER)
DEPTH_FILES = ["o.spikeScan.mnv.depth.sensitivity.txt", "o.spikeScan.mnv.depth.curve.txt", "o.spikeScan.mnv.depth.need.txt"] + \
    ["o.spikeScan%g.dsMT%g.mnv.rate.bedgraph" % (t, 0.5) for t in (0.5, 0.3)] + ["o.spikeScan.dsMT0.5.mnv.t95.bedgraph"] + \
    ["o.spikeScan%g.mnv.f95.bedgraph" % t for t in (0.5, 0.3)]
FILTER_FILES = ["o.spikeScan.mnv.filter.txt", "o.spikeScan.mnv.filter.curve.txt", "o.spikeScan.mnv.t95pass.bedgraph"] + \
    ["o.spikeScan%g.mnv.passrate.bedgraph" % t for t in (0.5, 0.3)]
I_CALLED, I_PASS = HEADER.index("CALLED_ALL"), HEADER.index("PASS_ALL")
CLOSING = (r"^--spikeScanMnv (\d+): (\d+) sets scanned, (\d+) loci skipped, (\d+) of (\d+) joint verdicts decided by the host; "
           r"--spikeScanMnvFilter: (\d+) of (\d+) called sets PASS, the FILTER of (\d+) decided by the host; (.*)$")
_lines, _files = TF._lines, TF._files


def _joint(members):
    """members: per member SNV its replicates (FILTER, CALLED) -> the set's replicates as scan_filter_pages takes them: CALLED_ALL_j, and
    where it is 1 the union of the members' names (PASS when every member's column is exactly PASS)."""
    out = []
    for reps in zip(*members):
        called = all(int(c) == 1 for _, c in reps)
        names = [n for n in pages.NAMES if any(n in f.split(";") for f, _ in reps)]
        assert (not names) == all(f == "PASS" for f, _ in reps) or not called
        out.append((";".join(names) or "PASS", "1" if called else "0"))
    return out


@pytest.fixture(scope="module")
def scanned(tmp_path_factory):
    """The inputs, the scan without the switch, and the passes as runs of their own -> dict."""
    tmp = tmp_path_factory.mktemp("mnv_axes")
    bam, fa, loci, P, _ = TS._inputs("synth", str(tmp))
    loci, P = loci[:32], dataclasses.replace(P, rpb=2.9)
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    trf = TF._half_bed(str(tmp / "trf.bed"), loci)
    text = ",".join("%g" % t for t in TARGETS)
    more = dict(spikeScan=text, spikeScanReps=REPS, spikeScanStride=STRIDE, spikeScanMnv=L, dsSeed=SEED, bedTandemRepeats=trf)
    TL._run_cli(tmp, "o", bam, fa, bed, P, **more)
    without = _files(tmp, "o")
    assert without and not [f for f in without if "filter" in f or "pass" in f]
    names = lists.main(argparse.Namespace(runPath=None, bedTarget=bed, refGenome=fa, stride=STRIDE, alt="transition", mnv=L,
                                          outPrefix=str(tmp / "scan")))
    # (pass, chrom, pos, ref, alt, target) -> the member's replicates - a position is the second member of one pass's set and the leader
    # of the next pass's; the scanned MNVs
    member, sets = {}, []
    cell_member, phase_sens, n_all = {}, {}, {}  # the cells' member replicates; the phase sensitivity lines and N_ALL by (set, target, fraction)
    for name in names:
        k = int(re.search(r"\.pass(\d+)\.txt$", name).group(1))
        ref = TL._run_cli(tmp, "p%d" % k, bam, fa, bed, P, flags=["--spikePhase"], spikeAF=text, spikeVariants=name, spikeReps=REPS, dsSeed=SEED,
                          bedTandemRepeats=trf, spikeDepth="%g" % FRAC)
        for f in _lines(ref + ".spikeAF.depth.replicates.txt")[1:]:
            cell_member.setdefault((k,) + tuple(f[:7]), []).append((f[-2], f[-1]))
        sens = open(ref + ".spikeAF.phase.sensitivity.txt").read().splitlines()
        assert sens[0].split("\t") == PHASE
        for line in sens[1:]:
            f = line.split("\t")
            phase_sens[(f[0], f[5], f[6])] = line
        for f in _lines(ref + ".spikeAF.phase.replicates.txt")[1:]:
            n_all.setdefault((f[0], f[5], f[6]), []).append(int(f[10]))
        page = _lines(ref + ".spikeAF.replicates.txt")
        assert page[0] == list(spike.REPLICATES_HEADER) and page[0][5] == "REP" and page[0][-2:] == ["FILTER", "CALLED"]
        for f in page[1:]:
            assert int(f[5]) == len(member.setdefault((k,) + tuple(f[:5]), []))    # (replicates ascending)
            member[(k,) + tuple(f[:5])].append((f[-2], f[-1]))
    curve = _lines(str(tmp / "o") + ".spikeScan.mnv.curve.txt")
    joint = {}
    for f in curve[1:]:
        c, p, ref, alt = f[0], int(f[1]), f[2], f[3]
        assert len(ref) == len(alt) == L
        sets.append((c, p, ref, alt))
        for t in TARGETS:
            joint[(c, f[1], ref, alt, "%g" % t)] = _joint([member[(p % STRIDE, c, "%d" % (p + m), ref[m], alt[m], "%g" % t)] for m in range(L)])
    assert all(len(r) == REPS for r in joint.values()) and len(member) == len(sets) * L * len(TARGETS)
    cell_joint = {}
    mt = spike.scan_depth_mt(P.mtDepth, FRAC)
    for c, p, ref, alt in sets:
        for t in TARGETS:
            cell_joint[(c, "%d" % p, ref, alt, "%g" % t)] = _joint(
                [cell_member[(p % STRIDE, c, "%d" % (p + m), ref[m], alt[m], "%g" % t, "%g" % FRAC, "%d" % mt)] for m in range(L)])
    assert all(len(r) == REPS for r in cell_joint.values())
    return dict(tmp=tmp, inputs=(bam, fa, bed, P), loci=loci, more=more, without=without, member=member, joint=joint, sets=sets, curve=curve,
                n_passes=len(names), cell_joint=cell_joint, phase_sens=phase_sens, n_all=n_all, mt=(P.mtDepth, mt))


def _with_flag(S, capsys, monkeypatch, flags=("--spikeScanMnvFilter",), **kw):
    """The scan with the switch under the prefix of the run without -> (its files, its log, the smc_scan_filter_sets calls)."""
    calls, real = [], devplanes.scan_filter_sets

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append(out[0].shape)
        return out
    monkeypatch.setattr(devplanes, "scan_filter_sets", spy)
    capsys.readouterr()
    TL._run_cli(S["tmp"], "o", *S["inputs"], flags=list(flags), **dict(S["more"], **kw))
    log = capsys.readouterr().out
    monkeypatch.setattr(devplanes, "scan_filter_sets", real)
    return _files(S["tmp"], "o"), log, calls


def test_the_fixture_makes_the_joint_rule_matter(scanned):
    """On the passes' own runs: a set that is PASS in some replicate, a set that is called more often than it is PASS, and a called
    replicate whose members' FILTER columns differ."""
    S = scanned
    tallies = {k: pages.counts(r) for k, r in S["joint"].items()}
    print("(CALLED_ALL, PASS_ALL) per set and target:", sorted((k[1], k[4], v[1], v[2]) for k, v in tallies.items()))
    assert any(v[2] > 0 for v in tallies.values()), "no (set, target) with PASS_ALL > 0"
    assert any(v[1] > v[2] for v in tallies.values()), "no (set, target) with CALLED_ALL > PASS_ALL"
    differ = 0
    for (c, p, ref, alt) in S["sets"]:
        for t in TARGETS:
            mem = [S["member"][(p % STRIDE, c, "%d" % (p + m), ref[m], alt[m], "%g" % t)] for m in range(L)]
            differ += sum(1 for reps in zip(*mem) if all(int(x) == 1 for _, x in reps) and len({f for f, _ in reps}) > 1)
    print("called replicates whose members' FILTER columns differ: %d" % differ)
    assert differ > 0


def test_the_filter_pages_equal_the_passes_whole_and_listed(scanned, capsys, monkeypatch):
    S = scanned
    got = str(S["tmp"] / "o")
    with_flag, log, calls = _with_flag(S, capsys, monkeypatch)
    # every file of the MNV scan without the switch - the full-depth files among them - byte for byte; the new files are the filter's
    for name, data in S["without"].items():
        assert with_flag[name] == data, "%s changed with --spikeScanMnvFilter" % name
    new = ["o.spikeScan.mnv.filter.txt", "o.spikeScan.mnv.filter.curve.txt", "o.spikeScan.mnv.t95pass.bedgraph"] + \
        ["o.spikeScan%g.mnv.passrate.bedgraph" % t for t in TARGETS]
    assert sorted(set(with_flag) - set(S["without"])) == sorted(new)
    assert calls and all(shape[1] > 0 for shape in calls), "smc_scan_filter_sets was not called"
    # the page: every line from the members' FILTER and CALLED columns of the passes' own runs, in the sensitivity page's order
    sens = _lines(got + ".spikeScan.mnv.sensitivity.txt")
    page = _lines(got + ".spikeScan.mnv.filter.txt")
    assert page[0] == HEADER and HEADER[:5] == list(pages.HEADER[:5]) and HEADER[8:] == list(pages.HEADER[8:]) and "LOD" not in HEADER
    order = [(c, "%d" % p, ref, alt, "%g" % t) for c, p, ref, alt in S["sets"] for t in TARGETS]
    assert [tuple(f[:5]) for f in page[1:]] == order and len(page) - 1 == len(S["joint"])
    for f in page[1:]:
        assert f == pages.line(f[:5], S["joint"][tuple(f[:5])]), (f, S["joint"][tuple(f[:5])])
    i_sens = list(spike.PHASE_SENSITIVITY_HEADER).index("CALLED_ALL")
    assert [f[I_CALLED] for f in page[1:]] == [f[i_sens] for f in sens[1:]]            # (the phase page's CALLED_ALL)
    # the curve and the bedgraphs follow from the page
    curve = _lines(got + ".spikeScan.mnv.filter.curve.txt")
    assert curve[0] == ["CHROM", "POS", "REF", "ALT", "N_ALL"] + ["RATE_PASS@%g" % t for t in sorted(TARGETS)] + ["T95_PASS"]
    assert [f[:5] for f in curve[1:]] == [f[:5] for f in S["curve"][1:]]
    for f in curve[1:]:
        assert f == pages.curve_line(f[:4], int(f[4]), TARGETS, [S["joint"][tuple(f[:4]) + ("%g" % t,)] for t in TARGETS])
    i_rate = HEADER.index("RATE_PASS")
    for t in TARGETS:
        bg = open("%s.spikeScan%g.mnv.passrate.bedgraph" % (got, t)).read().splitlines()
        mine = [f for f in page[1:] if f[4] == "%g" % t]
        assert bg == ["%s\t%d\t%d\t%s" % (f[0], int(f[1]) - 1, int(f[1]), f[i_rate]) for f in mine] and len(mine) == len(S["sets"])
    t95 = {(f[0], int(f[1])): f[-1] for f in curve[1:]}
    bg = open(got + ".spikeScan.mnv.t95pass.bedgraph").read().splitlines()
    assert bg == ["%s\t%d\t%d\t%s" % (c, p - 1, p, "1" if t95.get((c, p), "NA") == "NA" else t95[(c, p)]) for c, p in S["loci"]]
    assert len(S["sets"]) < len(S["loci"]), "no skipped locus"
    # the run log: the pass lines keep their shape, the closing line carries the new counts
    assert len(re.findall(r"^--spikeScan pass \d+: \d+ variants, \d+ copies, \d+ builds, \d+ verdicts decided by the host, [0-9.]+ s$", log,
                          re.M)) == S["n_passes"]
    last = re.findall(CLOSING, log, re.M)
    assert len(last) == 1
    n_pass, n_called, n_host, tail = last[0][5:]
    totals = [sum(int(f[HEADER.index(n)]) for f in page[1:]) for n in pages.NAMES]
    assert tail == ", ".join("%s %d" % (n, x) for n, x in zip(pages.NAMES, totals))
    assert int(n_called) == sum(int(f[I_CALLED]) for f in page[1:]) and int(n_pass) == sum(int(f[I_PASS]) for f in page[1:])
    assert 0 <= int(n_host) <= int(n_called) and [int(x) for x in last[0][:2]] == [L, len(S["sets"])]
    print("FILTER decided by the host for %s of %s called sets; totals: %s" % (n_host, n_called, tail))
    assert dict(zip(pages.NAMES, totals))["RepT"] > 0 and int(n_pass) > 0
    # --spikeScanBuild listed: every file byte for byte
    listed, log, calls = _with_flag(S, capsys, monkeypatch, spikeScanBuild="listed")
    assert sorted(listed) == sorted(with_flag) and calls
    for name in with_flag:
        assert listed[name] == with_flag[name], name
    closing = re.findall(r"^--spikeScanBuild listed: (\d+) listed builds, (\d+) whole fallbacks, (\d+) replicate-0 row checks$", log, re.M)
    assert len(closing) == 1 and int(closing[0][0]) > 0 and int(closing[0][1]) == 0
    assert len(re.findall(CLOSING, log, re.M)) == 1


def test_with_lod_the_lod_files_stay_and_the_new_pages_carry_no_lod(tmp_path, capsys):
    bam, fa, loci, P = ds_restate.load_fixture("bam_deep", str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    suffixes = TL.SUFFIXES + TL.LOD_SUFFIXES
    plain = TL._read(TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=["--lod"]), suffixes)
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=["--lod", "--spikeScanMnvFilter"], spikeScan="0.2", spikeScanReps=2,
                      spikeScanStride=8, spikeScanMnv=2, dsSeed=SEED)
    assert TL._read(got, suffixes) == plain
    page = _lines(got + ".spikeScan.mnv.filter.txt")
    curve = _lines(got + ".spikeScan.mnv.filter.curve.txt")
    assert page[0] == HEADER and curve[0] == list(spike.scan_filter_curve_header([0.2], spike.SCAN_MNV_CURVE_HEADER))
    assert "LOD" not in page[0] + curve[0] and len(page) > 1
    assert all(len(f) == len(HEADER) for f in page) and all(len(f) == len(curve[0]) for f in curve)


def _depth_pages(S, got):
    """Every line of the depth pages under the prefix `got`, restated from the passes' own --spikeDepth runs."""
    mt_full, mt = S["mt"]
    mean = lambda xs: sum(float(x) for x in xs) / len(xs)
    i_rate, i_called = PHASE.index("RATE"), PHASE.index("CALLED_ALL")
    sens = open(got + ".spikeScan.mnv.depth.sensitivity.txt").read().splitlines()
    assert sens[0].split("\t") == PHASE and "LOD" not in PHASE
    names = ["%s:%d" % (c, p) for c, p, _, _ in S["sets"]]
    assert [tuple(l.split("\t")[i] for i in (0, 5, 6)) for l in sens[1:]] == [(n, "%g" % t, "%g" % FRAC) for n in names for t in TARGETS]
    for line in sens[1:]:                                           # byte for byte the set's cell line in the pass's own run
        f = line.split("\t")
        assert line == S["phase_sens"][(f[0], f[5], f[6])] and f[7] == "%d" % mt
    rate = lambda n, t, d: float(int(S["phase_sens"][(n, "%g" % t, d)].split("\t")[i_called])) / REPS
    text = lambda n, t, d: S["phase_sens"][(n, "%g" % t, d)].split("\t")[i_rate]
    order = sorted(TARGETS)
    curve = _lines(got + ".spikeScan.mnv.depth.curve.txt")
    assert curve[0] == list(spike.depth_curve_header(TARGETS)) and len(curve) - 1 == 2 * len(S["sets"])
    need = _lines(got + ".spikeScan.mnv.depth.need.txt")
    assert need[0] == ["CHROM", "POS", "REF", "ALT", "TARGET", "N_ALL", "F95", "MTDEPTH95", "N95"]
    assert len(need) - 1 == len(S["sets"]) * len(TARGETS)
    f95 = {}
    for k, ((c, p, ref, alt), n) in enumerate(zip(S["sets"], names)):
        for row, d, m in ((curve[1 + 2 * k], "full", mt_full), (curve[2 + 2 * k], "%g" % FRAC, mt)):
            best = dsaf.t95(list(TARGETS), [rate(n, t, d) for t in TARGETS])
            assert row == [c, "%d" % p, ref, alt, d, "%d" % m, dsaf.frac_text(mean([mean(S["n_all"][(n, "%g" % t, d)]) for t in TARGETS]))] + \
                [text(n, t, d) for t in order] + [dsaf.NA if best is None else "%g" % best], row
        for ti, t in enumerate(TARGETS):
            # F95: the smallest depth of (0.5, 1 = full) whose rate is at least 0.95 together with every larger depth's
            ok_full, ok_cell = rate(n, t, "full") >= 0.95, rate(n, t, "%g" % FRAC) >= 0.95
            at = None if not ok_full else ("%g" % FRAC, mt) if ok_cell else ("full", mt_full)
            head = [c, "%d" % p, ref, alt, "%g" % t, "%d" % S["n_all"][(n, "%g" % t, "full")][0]]
            want = head + (["NA"] * 3 if at is None else ["%g" % (FRAC if at[0] != "full" else 1.0), "%d" % at[1],
                                                           dsaf.frac_text(mean(S["n_all"][(n, "%g" % t, at[0])]))])
            assert need[1 + k * len(TARGETS) + ti] == want, (need[1 + k * len(TARGETS) + ti], want)
            f95[(c, p, t)] = want[6]
    # the bedgraphs follow from the pages
    for t in TARGETS:
        bg = open("%s.spikeScan%g.dsMT%g.mnv.rate.bedgraph" % (got, t, FRAC)).read().splitlines()
        assert bg == ["%s\t%d\t%d\t%s" % (c, p - 1, p, text(n, t, "%g" % FRAC)) for (c, p, _, _), n in zip(S["sets"], names)]
        bg = open("%s.spikeScan%g.mnv.f95.bedgraph" % (got, t)).read().splitlines()
        assert bg == ["%s\t%d\t%d\t%s" % (c, p - 1, p, "2" if f95.get((c, p, t), "NA") == "NA" else f95[(c, p, t)]) for c, p in S["loci"]]
    t95 = {(row[0], int(row[1])): row[-1] for row in curve[1:] if row[4] != "full"}
    bg = open("%s.spikeScan.dsMT%g.mnv.t95.bedgraph" % (got, FRAC)).read().splitlines()
    assert bg == ["%s\t%d\t%d\t%s" % (c, p - 1, p, "1" if t95.get((c, p), "NA") == "NA" else t95[(c, p)]) for c, p in S["loci"]]
    return f95


def test_the_depth_pages_equal_the_passes_alone_and_beside_the_switch(scanned, capsys, monkeypatch):
    S = scanned
    got = str(S["tmp"] / "o")
    for n in [n for n in _files(S["tmp"], "o") if n not in S["without"]]:
        os.remove(str(S["tmp"] / n))
    # the depth flag alone
    alone, log, calls = _with_flag(S, capsys, monkeypatch, flags=(), spikeScanMnvDepth="%g" % FRAC)
    assert not calls
    for name, data in S["without"].items():
        assert alone[name] == data, "%s changed with --spikeScanMnvDepth" % name
    assert sorted(set(alone) - set(S["without"])) == sorted(DEPTH_FILES)
    f95 = _depth_pages(S, got)
    print("F95 per (set, target):", sorted(set(f95.values())))
    last = re.findall(r"^--spikeScanMnv 2: .* joint verdicts decided by the host; --spikeScanMnvDepth: fractions 0.5: 2 cells per pass, (\d+) builds "
                      r"\(S x R x T x \(1 \+ F\)\), (\d+) select_copies calls$", log, re.M)
    assert len(last) == 1 and int(last[0][0]) == S["n_passes"] * REPS * len(TARGETS) * 2 and int(last[0][1]) > 0
    # both flags, whole and listed
    both, log, calls = _with_flag(S, capsys, monkeypatch, spikeScanMnvDepth="%g" % FRAC)
    assert calls
    for name, data in alone.items():
        assert both[name] == data, "%s changed with --spikeScanMnvFilter beside --spikeScanMnvDepth" % name
    assert sorted(set(both) - set(alone)) == sorted(FILTER_FILES + ["o.spikeScan.mnv.depth.filter.txt"])
    page = _lines(got + ".spikeScan.mnv.depth.filter.txt")
    assert page[0] == HEADER[:5] + ["FRACTION", "MTDEPTH"] + HEADER[5:]
    cell = ["%g" % FRAC, "%d" % S["mt"][1]]
    assert [tuple(f[:5]) for f in page[1:]] == [(c, "%d" % p, ref, alt, "%g" % t) for c, p, ref, alt in S["sets"] for t in TARGETS]
    for f in page[1:]:
        assert f == pages.line(f[:5], S["cell_joint"][tuple(f[:5])], cell), (f, S["cell_joint"][tuple(f[:5])])
    full = _lines(got + ".spikeScan.mnv.filter.txt")
    for f in full[1:]:
        assert f == pages.line(f[:5], S["joint"][tuple(f[:5])])
    last = re.findall(CLOSING[:-1] + r"; --spikeScanMnvDepth: fractions 0.5: .*$", log, re.M)
    assert len(last) == 1
    lines = full[1:] + [f[:5] + f[7:] for f in page[1:]]
    totals = [sum(int(f[HEADER.index(n)]) for f in lines) for n in pages.NAMES]
    assert last[0][8] == ", ".join("%s %d" % (n, x) for n, x in zip(pages.NAMES, totals))
    assert int(last[0][6]) == sum(int(f[I_CALLED]) for f in lines) and int(last[0][5]) == sum(int(f[I_PASS]) for f in lines)
    listed, log, calls = _with_flag(S, capsys, monkeypatch, spikeScanMnvDepth="%g" % FRAC, spikeScanBuild="listed")
    assert sorted(listed) == sorted(both) and calls
    for name in both:
        assert listed[name] == both[name], name
