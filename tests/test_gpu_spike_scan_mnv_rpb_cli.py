"""--spikeScanMnvRpb on the GPU, through the command line: the fixture of test_gpu_spike_scan_mnv_axes_cli.py - the small synthetic
input of test_gpu_spike, 32 loci, --rpb 2.9, a --bedTandemRepeats file over the lower half, L = 2, S = 4, R = 4, targets 0.5 and 0.3 -
with --spikeScanMnvRpb 2,1.5.  THE DEFINITION is the passes' own runs --spikeAF <targets> --spikeVariants pass<k>.txt --spikeIndelReps 4
--spikePhaseRpb 2,1.5 --dsSeed s: every sensitivity line is byte for byte the set's cell line of that run's
.spikeAF.rpb.phase.sensitivity.txt; the curve, the need page and the bedgraphs are restated from those lines and from N_ALL' of
.spikeAF.rpb.phase.replicates.txt (full depth: .spikeAF.phase.*); beside --spikeScanMnvFilter .spikeScan.mnv.rpb.filter.txt is restated
from the members' FILTER and CALLED columns of .spikeAF.rpb.replicates.txt.  --spikeScanBuild whole and listed give equal files; every
file of the scan without the flag stays byte for byte; with --lod the LOD files are unchanged and the new pages have no LOD column; the
closing line's builds are S x R x T x (1 + Rr), summed from the pass lines."""
import argparse
import dataclasses
import os
import re
import sys

import pytest

from conftest import ROOT
from smcounter_amd import cli, devplanes, dsaf, spike
from smcounter_amd.tools import spike_scan_lists as lists

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import ds_rpb_restate  # noqa: E402
import scan_filter_pages as pages  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line)
import test_gpu_spike as TS  # noqa: E402  (the small inputs)
import test_gpu_spike_scan_filter_cli as TF  # noqa: E402  (the repeat track over the lower half, the files of a prefix)
from test_gpu_spike_scan_mnv_axes_cli import _joint  # noqa: E402  (the joint rule on the members' (FILTER, CALLED) columns)

pytestmark = pytest.mark.gpu
SEED = 20240607
L, STRIDE, REPS, TARGETS = 2, 4, 4, (0.5, 0.3)
RPBS, RPB_TEXT, RUN_RPB = (2.0, 1.5), "2,1.5", 2.9
PHASE = list(spike.phase_sensitivity_header(spike.RPB_AXIS))
HEADER = list(spike.SCAN_MNV_FILTER_HEADER)
RPB_FILES = ["o.spikeScan.mnv.rpb.sensitivity.txt", "o.spikeScan.mnv.rpb.curve.txt", "o.spikeScan.mnv.rpb.need.txt"] + \
    ["o.spikeScan%g.dsRpb%g.mnv.rate.bedgraph" % (t, r) for t in TARGETS for r in RPBS] + \
    ["o.spikeScan.dsRpb%g.mnv.t95.bedgraph" % r for r in RPBS] + ["o.spikeScan%g.mnv.r95.bedgraph" % t for t in TARGETS]
FILTER_FILES = ["o.spikeScan.mnv.filter.txt", "o.spikeScan.mnv.filter.curve.txt", "o.spikeScan.mnv.t95pass.bedgraph"] + \
    ["o.spikeScan%g.mnv.passrate.bedgraph" % t for t in TARGETS]
PASS_LINE = r"^--spikeScan pass \d+: \d+ variants, (\d+) copies, (\d+) builds, (?:\d+ of them whole, )?\d+ verdicts decided by the host, [0-9.]+ s$"
CLOSING = (r"; --spikeScanMnvRpb: reads-per-barcode targets 2,1\.5: 4 cells per pass, (\d+) builds \(S x R x T x \(1 \+ Rr\)\), "
           r"(\d+) select_copies_reads calls$")
_lines, _files = TF._lines, TF._files
mean = lambda xs: sum(float(x) for x in xs) / len(xs)


@pytest.fixture(scope="module")
def scanned(tmp_path_factory):
    """The inputs, the scan without the flag, and the passes as --spikePhaseRpb runs of their own -> dict."""
    tmp = tmp_path_factory.mktemp("mnv_rpb")
    bam, fa, loci, P, _ = TS._inputs("synth", str(tmp))
    loci, P = loci[:32], dataclasses.replace(P, rpb=RUN_RPB)
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    trf = TF._half_bed(str(tmp / "trf.bed"), loci)
    text = ",".join("%g" % t for t in TARGETS)
    more = dict(spikeScan=text, spikeScanReps=REPS, spikeScanStride=STRIDE, spikeScanMnv=L, dsSeed=SEED, bedTandemRepeats=trf)
    TL._run_cli(tmp, "o", bam, fa, bed, P, **more)
    without = _files(tmp, "o")
    assert without and not [f for f in without if "rpb" in f or "dsRpb" in f or "r95" in f]
    names = lists.main(argparse.Namespace(runPath=None, bedTarget=bed, refGenome=fa, stride=STRIDE, alt="transition", mnv=L,
                                          outPrefix=str(tmp / "scan")))
    sens, n_all, member = {}, {}, {}            # by (set, target, r or "full"): the sensitivity line, N_ALL' per replicate; the members' columns
    for name in names:
        k = int(re.search(r"\.pass(\d+)\.txt$", name).group(1))
        ref = TL._run_cli(tmp, "p%d" % k, bam, fa, bed, P, spikeAF=text, spikeVariants=name, spikeIndelReps=REPS, spikePhaseRpb=RPB_TEXT,
                          dsSeed=SEED, bedTandemRepeats=trf)
        for page, head in ((".spikeAF.rpb.phase.sensitivity.txt", PHASE), (".spikeAF.phase.sensitivity.txt", list(spike.PHASE_SENSITIVITY_HEADER))):
            text_lines = open(ref + page).read().splitlines()
            assert text_lines[0].split("\t") == head
            for line in text_lines[1:]:
                f = line.split("\t")
                if page.startswith(".spikeAF.rpb") or f[6] == "full":
                    sens[(f[0], f[5], f[6])] = line
        for page in (".spikeAF.rpb.phase.replicates.txt", ".spikeAF.phase.replicates.txt"):
            rows = _lines(ref + page)
            assert rows[0][8:11] == ["REP", "SEED", "N_ALL"]
            for f in rows[1:]:
                if page.startswith(".spikeAF.rpb") or f[6] == "full":
                    n_all.setdefault((f[0], f[5], f[6]), []).append(int(f[10]))
        rows = _lines(ref + ".spikeAF.rpb.replicates.txt")
        assert rows[0] == list(spike.cell_replicates_header(spike.RPB_AXIS)) and rows[0][5:8] == ["RPB", "MTDEPTH", "REP"] and \
            rows[0][-2:] == ["FILTER", "CALLED"]
        for f in rows[1:]:
            assert int(f[7]) == len(member.setdefault((k,) + tuple(f[:7]), []))      # (replicates ascending)
            member[(k,) + tuple(f[:7])].append((f[-2], f[-1]))
    curve = _lines(str(tmp / "o") + ".spikeScan.mnv.curve.txt")
    sets = [(f[0], int(f[1]), f[2], f[3]) for f in curve[1:]]
    cell_joint = {}
    for c, p, ref, alt in sets:
        for t in TARGETS:
            for r in RPBS:
                cell_joint[(c, "%d" % p, ref, alt, "%g" % t, "%g" % r)] = _joint(
                    [member[(p % STRIDE, c, "%d" % (p + m), ref[m], alt[m], "%g" % t, "%g" % r, "%d" % P.mtDepth)] for m in range(L)])
    assert all(len(v) == REPS for v in cell_joint.values()) and all(len(v) == REPS for v in n_all.values())
    assert len(sens) >= len(sets) * len(TARGETS) * (1 + len(RPBS))
    return dict(tmp=tmp, inputs=(bam, fa, bed, P), loci=loci, more=more, without=without, sets=sets, sens=sens, n_all=n_all,
                cell_joint=cell_joint, n_passes=len(names), mt=P.mtDepth)


def _with_flag(S, capsys, flags=(), **kw):
    """The scan with the flag under the prefix of the run without -> (its files, its log)."""
    capsys.readouterr()
    TL._run_cli(S["tmp"], "o", *S["inputs"], flags=list(flags), **dict(S["more"], spikeScanMnvRpb=RPB_TEXT, **kw))
    return _files(S["tmp"], "o"), capsys.readouterr().out


def test_the_fixture_shows_thinning_biting(scanned):
    """On the passes' own runs: at some set, target and r the mean N_ALL' is below N_ALL, and some joint CALLED_ALL differs between full
    depth and a cell."""
    S = scanned
    i_called = PHASE.index("CALLED_ALL")
    assert list(spike.PHASE_SENSITIVITY_HEADER).index("CALLED_ALL") == i_called
    fewer, differ = [], []
    for c, p, _, _ in S["sets"]:
        n = "%s:%d" % (c, p)
        for t in TARGETS:
            for r in RPBS:
                key, full = (n, "%g" % t, "%g" % r), (n, "%g" % t, "full")
                if mean(S["n_all"][key]) < S["n_all"][full][0]:
                    fewer.append((key, mean(S["n_all"][key]), S["n_all"][full][0]))
                if S["sens"][key].split("\t")[i_called] != S["sens"][full].split("\t")[i_called]:
                    differ.append((key, S["sens"][full].split("\t")[i_called], S["sens"][key].split("\t")[i_called]))
    print("cells with a mean N_ALL' below N_ALL: %d of %d, e.g. %r" % (len(fewer), len(S["sets"]) * len(TARGETS) * len(RPBS), fewer[:3]))
    print("cells whose CALLED_ALL is not full depth's: %d, e.g. %r" % (len(differ), differ[:3]))
    assert fewer, "thinning takes no barcode out of a joint pileup"
    assert differ, "no joint CALLED_ALL differs between full depth and a cell"


def _rpb_pages(S, got):
    """Every line of the read-axis pages under the prefix `got`, restated from the passes' own --spikePhaseRpb runs."""
    i_rate, i_called = PHASE.index("RATE"), PHASE.index("CALLED_ALL")
    names = ["%s:%d" % (c, p) for c, p, _, _ in S["sets"]]
    sens = open(got + ".spikeScan.mnv.rpb.sensitivity.txt").read().splitlines()
    assert sens[0].split("\t") == PHASE and "LOD" not in PHASE
    assert [tuple(l.split("\t")[i] for i in (0, 5, 6)) for l in sens[1:]] == [(n, "%g" % t, "%g" % r) for n in names for t in TARGETS for r in RPBS]
    for line in sens[1:]:                                           # byte for byte the set's cell line in the pass's own run
        f = line.split("\t")
        assert line == S["sens"][(f[0], f[5], f[6])] and f[7] == "%d" % S["mt"]
    rate = lambda n, t, d: float(int(S["sens"][(n, "%g" % t, d)].split("\t")[i_called])) / REPS
    text = lambda n, t, d: S["sens"][(n, "%g" % t, d)].split("\t")[i_rate]
    axis = ["full"] + ["%g" % r for r in RPBS]
    curve = _lines(got + ".spikeScan.mnv.rpb.curve.txt")
    assert curve[0] == list(spike.depth_curve_header(TARGETS, False, spike.RPB_AXIS)) and len(curve) - 1 == len(axis) * len(S["sets"])
    need = _lines(got + ".spikeScan.mnv.rpb.need.txt")
    assert need[0] == ["CHROM", "POS", "REF", "ALT", "TARGET", "N_ALL", "R95", "N95"] and len(need) - 1 == len(S["sets"]) * len(TARGETS)
    r95, t95 = {}, {}
    for k, ((c, p, ref, alt), n) in enumerate(zip(S["sets"], names)):
        for a, d in enumerate(axis):
            row = curve[1 + len(axis) * k + a]
            best = dsaf.t95(list(TARGETS), [rate(n, t, d) for t in TARGETS])
            assert row == [c, "%d" % p, ref, alt, d, "%d" % S["mt"], dsaf.frac_text(mean([mean(S["n_all"][(n, "%g" % t, d)]) for t in TARGETS]))] + \
                [text(n, t, d) for t in sorted(TARGETS)] + [dsaf.NA if best is None else "%g" % best], row
            t95[(c, p, d)] = row[-1]
        for ti, t in enumerate(TARGETS):
            # R95: the smallest of (the targets ascending, full on top) whose rate is at least 0.95 together with every larger entry's
            at = None
            if rate(n, t, "full") >= 0.95:
                at = "full"
                for r in sorted(RPBS, reverse=True):
                    if rate(n, t, "%g" % r) < 0.95:
                        break
                    at = "%g" % r
            want = [c, "%d" % p, ref, alt, "%g" % t, "%d" % S["n_all"][(n, "%g" % t, "full")][0]] + \
                (["NA", "NA"] if at is None else [at, dsaf.frac_text(mean(S["n_all"][(n, "%g" % t, at)]))])
            assert need[1 + k * len(TARGETS) + ti] == want, (need[1 + k * len(TARGETS) + ti], want)
            r95[(c, p, t)] = want[6]
    above = "%g" % (2.0 * max((RUN_RPB,) + RPBS))
    for t in TARGETS:
        for r in RPBS:
            bg = open("%s.spikeScan%g.dsRpb%g.mnv.rate.bedgraph" % (got, t, r)).read().splitlines()
            assert bg == ["%s\t%d\t%d\t%s" % (c, p - 1, p, text(n, t, "%g" % r)) for (c, p, _, _), n in zip(S["sets"], names)]
        bg = open("%s.spikeScan%g.mnv.r95.bedgraph" % (got, t)).read().splitlines()
        fill = lambda x: above if x == "NA" else "%g" % RUN_RPB if x == "full" else x
        assert bg == ["%s\t%d\t%d\t%s" % (c, p - 1, p, fill(r95.get((c, p, t), "NA"))) for c, p in S["loci"]]
    for r in RPBS:
        bg = open("%s.spikeScan.dsRpb%g.mnv.t95.bedgraph" % (got, r)).read().splitlines()
        assert bg == ["%s\t%d\t%d\t%s" % (c, p - 1, p, "1" if t95.get((c, p, "%g" % r), "NA") == "NA" else t95[(c, p, "%g" % r)])
                      for c, p in S["loci"]]
    assert len(S["sets"]) < len(S["loci"]), "no skipped locus"
    return r95


def _builds(S, log):
    """The closing line's builds against S x R x T x (1 + Rr), summed from the pass lines; the per-r lines of the log."""
    per_pass = re.findall(PASS_LINE, log, re.M)
    assert len(per_pass) == S["n_passes"]
    last = re.findall(r"^--spikeScanMnv 2: .* joint verdicts decided by the host.*" + CLOSING, log, re.M)
    assert len(last) == 1, log[-2000:]
    assert int(last[0][0]) == sum(int(b) for _, b in per_pass) == S["n_passes"] * REPS * len(TARGETS) * (1 + len(RPBS))
    assert all(int(b) == int(c) * (1 + len(RPBS)) for c, b in per_pass) and int(last[0][1]) > 0
    for r in RPBS:
        assert len(re.findall(r"^--spikeScanMnvRpb %g: sampler philox, seed %d, probKeep [0-9.e+-]+, threshold \d+, \d+ of \d+ read names kept "
                              r"\(mtDepth %d\)$" % (r, SEED, S["mt"]), log, re.M)) == 1


def test_the_pages_equal_the_passes_whole_and_listed(scanned, capsys, monkeypatch):
    S = scanned
    got = str(S["tmp"] / "o")
    calls, real = [], devplanes.scan_phase_rpb_counts

    def spy(*a, **k):
        out = real(*a, **k)
        calls.append(out.shape)
        return out
    monkeypatch.setattr(devplanes, "scan_phase_rpb_counts", spy)
    alone, log = _with_flag(S, capsys)
    # every file of the MNV scan without the flag byte for byte; the new files are the read axis'
    for name, data in S["without"].items():
        assert alone[name] == data, "%s changed with --spikeScanMnvRpb" % name
    assert sorted(set(alone) - set(S["without"])) == sorted(RPB_FILES)
    # ONE counts call per pass and run (one chunk here): its rows are the pass's sets, then every member as a row of one
    assert len(calls) == S["n_passes"] and sum(n for n, _, _, _, _ in calls) == len(S["sets"]) * (1 + L)
    assert all(shape[1:3] == (REPS, len(TARGETS)) and shape[4] == 4 for shape in calls)
    r95 = _rpb_pages(S, got)
    print("R95 per (set, target):", sorted(set(r95.values())))
    _builds(S, log)
    # a byte budget that holds one set's bit rows only: a call per set, the chunks' outputs concatenated - every file byte for byte
    del calls[:]
    monkeypatch.setattr(devplanes, "SCAN_BITS_BUDGET", 1)
    chunked, _ = _with_flag(S, capsys)
    monkeypatch.undo()
    assert len(calls) == len(S["sets"]) and all(shape[0] == 1 + L for shape in calls)
    assert sorted(chunked) == sorted(alone)
    for name in alone:
        assert chunked[name] == alone[name], name
    # --spikeScanBuild listed: every file byte for byte
    listed, log = _with_flag(S, capsys, spikeScanBuild="listed")
    assert sorted(listed) == sorted(alone)
    for name in alone:
        assert listed[name] == alone[name], name
    closing = re.findall(r"^--spikeScanBuild listed: (\d+) listed builds, (\d+) whole fallbacks, (\d+) replicate-0 row checks$", log, re.M)
    assert len(closing) == 1 and int(closing[0][0]) > 0 and int(closing[0][1]) == 0
    _builds(S, log)
    # beside --spikeScanMnvFilter, whole and listed
    both, log = _with_flag(S, capsys, flags=["--spikeScanMnvFilter"])
    for name, data in alone.items():
        assert both[name] == data, "%s changed with --spikeScanMnvFilter beside --spikeScanMnvRpb" % name
    assert sorted(set(both) - set(alone)) == sorted(FILTER_FILES + ["o.spikeScan.mnv.rpb.filter.txt"])
    page = _lines(got + ".spikeScan.mnv.rpb.filter.txt")
    assert page[0] == HEADER[:5] + ["RPB", "MTDEPTH"] + HEADER[5:] and "CALLED_ALL" in page[0] and "PASS_ALL" in page[0]
    assert [tuple(f[:6]) for f in page[1:]] == [(c, "%d" % p, ref, alt, "%g" % t, "%g" % r) for c, p, ref, alt in S["sets"] for t in TARGETS
                                                for r in RPBS]
    for f in page[1:]:
        assert f == pages.line(f[:5], S["cell_joint"][tuple(f[:6])], [f[5], "%d" % S["mt"]]), (f, S["cell_joint"][tuple(f[:6])])
    assert sum(int(f[page[0].index("CALLED_ALL")]) for f in page[1:]) > 0
    assert len(re.findall(r"; --spikeScanMnvFilter: \d+ of \d+ called sets PASS.*" + CLOSING, log, re.M)) == 1
    listed, log = _with_flag(S, capsys, flags=["--spikeScanMnvFilter"], spikeScanBuild="listed")
    assert sorted(listed) == sorted(both)
    for name in both:
        assert listed[name] == both[name], name


def test_with_lod_the_lod_files_stay_and_the_new_pages_carry_no_lod(tmp_path, capsys):
    bam, fa, loci, P = ds_restate.load_fixture("bam_deep", str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    suffixes = TL.SUFFIXES + TL.LOD_SUFFIXES
    plain = TL._read(TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=["--lod"]), suffixes)
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=["--lod"], spikeScan="0.2", spikeScanReps=2, spikeScanStride=8, spikeScanMnv=2,
                      spikeScanMnvRpb="2", dsSeed=SEED)
    assert TL._read(got, suffixes) == plain
    sens, curve, need = (_lines(got + ".spikeScan.mnv.rpb.%s.txt" % x) for x in ("sensitivity", "curve", "need"))
    assert sens[0] == PHASE and curve[0] == list(spike.depth_curve_header([0.2], False, spike.RPB_AXIS)) and \
        need[0] == list(spike.SCAN_MNV_RPB_NEED_HEADER)
    assert "LOD" not in sens[0] + curve[0] + need[0] and len(sens) > 1
    assert all(len(f) == len(sens[0]) for f in sens) and all(len(f) == len(curve[0]) for f in curve) and all(len(f) == len(need[0]) for f in need)


def test_a_file_without_a_multi_name_barcode_is_refused_under_the_flag(tmp_path):
    """--dsRpbSampler philox's refusal, named after this flag, and no file written."""
    bam, fa, loci, P = ds_restate.make_case(str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci[:8])
    one = ds_rpb_restate.write_one_name_per_barcode(bam, str(tmp_path / "one.bam"))
    with pytest.raises(SystemExit, match=r"--spikeScanMnvRpb 1\.5: .*one\.bam has no barcode with more than one read name"):
        cli.main(dict(outPrefix=str(tmp_path / "bad"), bamFile=one, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, hpLen=P.hpLen, refGenome=fa,
                      spikeScan="0.3", spikeScanReps=2, spikeScanMnv=2, spikeScanStride=4, spikeScanMnvRpb="1.5,3", dsSeed=SEED))
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("bad.")]
