"""--spikeScanMnv on the GPU, through the command line: every line of the sensitivity page against the line the same set and target
have in .spikeAF.phase.sensitivity.txt of the pass's own --spikeAF --spikeVariants pass<k>.txt --spikeReps R --spikePhase run
(tools.spike_scan_lists --mnv writes the lists); the curve from the sensitivity page; the bedgraphs from the pages; the full-depth files
those of a run without the flags; the run log's pass lines and closing lines, the count of host-decided joint verdicts against the
joint words of smc_scan_detect_sets."""
import argparse
import os
import re
import sys

import pytest

from conftest import ROOT
from smcounter_amd import abi, devplanes, dsaf, spike
from smcounter_amd.tools import spike_scan_lists as lists

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line)
import test_gpu_spike as TS  # noqa: E402  (the small inputs)

pytestmark = pytest.mark.gpu
SEED = 20240607
SUFFIXES = TL.SUFFIXES
HEAD = list(spike.PHASE_SENSITIVITY_HEADER)
PAGES = (".spikeScan.mnv.sensitivity.txt", ".spikeScan.mnv.curve.txt", ".spikeScan.mnv.t95.bedgraph")


def _scan(tmp_path, capsys, monkeypatch, tag, bam, fa, bed, P, stride, n_reps, targets, L, flags=(), **kw):
    """One run with the flag -> (prefix, its log, the joint verdicts smc_scan_detect_sets left to the host by its words, the calls of
    devplanes.scan_detect: there must be none)."""
    joint_host, plain_calls = [], []
    real, real_snv = devplanes.scan_detect_sets, devplanes.scan_detect

    def spy(*a, **k):
        words, todo, rec = real(*a, **k)
        joint_host.append(int(((words >> 30) == abi.SCAN_HOST).sum()))
        assert (joint_host[-1] > 0) == (len(todo) > 0)
        return words, todo, rec
    monkeypatch.setattr(devplanes, "scan_detect_sets", spy)
    monkeypatch.setattr(devplanes, "scan_detect", lambda *a, **k: plain_calls.append(1) or real_snv(*a, **k))
    capsys.readouterr()
    text = ",".join("%g" % t for t in targets)
    got = TL._run_cli(tmp_path, tag, bam, fa, bed, P, flags=flags, spikeScan=text, spikeScanReps=n_reps, spikeScanStride=stride,
                      spikeScanMnv=L, dsSeed=SEED, **kw)
    log = capsys.readouterr().out
    monkeypatch.setattr(devplanes, "scan_detect_sets", real)
    monkeypatch.setattr(devplanes, "scan_detect", real_snv)
    assert not plain_calls
    return got, log, sum(joint_host)


def _contract(tmp_path, capsys, monkeypatch, bam, fa, loci, P, stride, n_reps, targets, L, alt="transition"):
    """-> (the sensitivity page's lines as fields, the joint verdicts decided by the host by the words, that number by the run log,
    the prefix)."""
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    plain = TL._read(TL._run_cli(tmp_path, "o", bam, fa, bed, P), SUFFIXES)
    got, log, by_words = _scan(tmp_path, capsys, monkeypatch, "o", bam, fa, bed, P, stride, n_reps, targets, L,
                               **(dict(spikeScanAlt=alt) if alt != "transition" else {}))
    assert TL._read(got, SUFFIXES) == plain, "the full-depth files changed with --spikeScanMnv"
    assert not [f for f in os.listdir(str(tmp_path)) if ".spikeAF" in f]
    assert not os.path.exists(got + ".spikeScan.sensitivity.txt") and not os.path.exists(got + ".spikeScan.curve.txt")
    # the passes as runs of their own
    text = ",".join("%g" % t for t in targets)
    names = lists.main(argparse.Namespace(runPath=None, bedTarget=bed, refGenome=fa, stride=stride, alt=alt, mnv=L,
                                          outPrefix=str(tmp_path / "scan")))
    want_sens, ks = {}, []
    for name in names:
        k = int(re.search(r"\.pass(\d+)\.txt$", name).group(1))
        ks.append(k)
        ref = TL._run_cli(tmp_path, "p%d" % k, bam, fa, bed, P, flags=["--spikePhase"], spikeAF=text, spikeVariants=name, spikeReps=n_reps,
                          dsSeed=SEED)
        sens = open(ref + ".spikeAF.phase.sensitivity.txt").read().splitlines()
        assert sens[0].split("\t") == HEAD
        for line in sens[1:]:
            f = line.split("\t")
            assert f[HEAD.index("FRACTION")] == "full" and int(f[0].split(":")[1]) % stride == k
            want_sens[(f[0], f[HEAD.index("TARGET")])] = line
    capsys.readouterr()
    scanned = [(l.split("\t")[0], int(l.split("\t")[1])) for name in names for l in open(name).read().splitlines()]
    in_order = [(c, p) for c, p in loci if (c, p) in set(scanned)]
    assert len(scanned) == len(set(scanned)) == len(in_order)
    lines = open(got + ".spikeScan.mnv.sensitivity.txt").read().splitlines()
    assert lines[0].split("\t") == HEAD
    sens = [l.split("\t") for l in lines[1:]]
    assert [f[0] for f in sens] == ["%s:%d" % cp for cp in in_order for _ in targets]
    for line in lines[1:]:                                          # byte for byte the set's line in the pass's own run
        f = line.split("\t")
        assert line == want_sens[(f[0], f[HEAD.index("TARGET")])], (line, want_sens[(f[0], f[HEAD.index("TARGET")])])
        assert len(f[2].split(",")) == len(f[3].split(",")) == len(f[4].split(",")) == L
    assert len(sens) == len(want_sens) == len(scanned) * len(targets)
    # the curve page recomputed from the sensitivity page
    curve = [l.split("\t") for l in open(got + ".spikeScan.mnv.curve.txt").read().splitlines()]
    assert curve[0] == list(spike.scan_mnv_curve_header(targets)) and "LOD" not in curve[0] and "LOD" not in HEAD
    assert [(f[0], int(f[1])) for f in curve[1:]] == in_order
    i_rate, i_called, i_reps = HEAD.index("RATE"), HEAD.index("CALLED_ALL"), HEAD.index("REPS")
    by_set = {}
    for f in sens:
        by_set.setdefault(f[0], {})[f[HEAD.index("TARGET")]] = f
    for f in curve[1:]:
        mine = by_set["%s:%d" % (f[0], int(f[1]))]
        one = next(iter(mine.values()))
        assert f[2] == one[3].replace(",", "") and f[3] == one[4].replace(",", "") and len(f[2]) == L
        rates = [float(int(mine["%g" % t][i_called])) / int(mine["%g" % t][i_reps]) for t in targets]
        best = dsaf.t95(list(targets), rates)
        assert f[5:] == [mine["%g" % t][i_rate] for t in sorted(targets)] + [dsaf.NA if best is None else "%g" % best]
    # (N_ALL: the joint barcodes at full depth - the pass's own phase page has it)
    for name in names:
        k = int(re.search(r"\.pass(\d+)\.txt$", name).group(1))
        page = [l.split("\t") for l in open(str(tmp_path / ("p%d" % k)) + ".spikeAF.phase.txt").read().splitlines()]
        n_all = {f[0]: f[page[0].index("N_ALL")] for f in page[1:]}
        for f in curve[1:]:
            if int(f[1]) % stride == k:
                assert f[4] == n_all["%s:%d" % (f[0], int(f[1]))]
    # the bedgraphs follow from the pages
    for t in targets:
        bg = open("%s.spikeScan%g.mnv.rate.bedgraph" % (got, t)).read().splitlines()
        mine = [f for f in sens if f[HEAD.index("TARGET")] == "%g" % t]
        assert bg == ["%s\t%d\t%d\t%s" % (f[1], int(f[0].split(":")[1]) - 1, int(f[0].split(":")[1]), f[i_rate]) for f in mine]
        assert len(mine) == len(scanned)
    t95 = {(f[0], int(f[1])): f[-1] for f in curve[1:]}
    bg = open(got + ".spikeScan.mnv.t95.bedgraph").read().splitlines()
    assert bg == ["%s\t%d\t%d\t%s" % (c, p - 1, p, "1" if t95.get((c, p), "NA") == "NA" else t95[(c, p)]) for c, p in loci]
    # the run log: the pass lines keep their shape (`variants` counts member SNVs), and the closing lines
    per_pass = [m for m in (spike.scan_pass_line(l) for l in log.splitlines()) if m is not None]
    assert [m["k"] for m in per_pass] == sorted(ks)
    assert sum(m["variants"] for m in per_pass) == len(scanned) * L
    closing = re.findall(r"^--spikeScanMnv (\d+): (\d+) sets scanned, (\d+) loci skipped, (\d+) of (\d+) joint verdicts decided by the host$",
                         log, re.M)
    assert len(closing) == 1
    assert [int(x) for x in closing[0][:3]] == [L, len(scanned), len(set(loci)) - len(scanned)]
    assert int(closing[0][4]) == len(scanned) * len(targets) * n_reps
    return sens, by_words, int(closing[0][3]), got


def test_mnv_scan_equals_its_passes_on_the_synthetic_bam(tmp_path, capsys, monkeypatch):
    """(a) The file's first 32 loci, S = 8, R = 4, targets 0.3 and 0.7, L = 2.  Both joint verdicts must occur."""
    bam, fa, loci, P, _ = TS._inputs("synth", str(tmp_path))
    n_reps = 4
    sens, by_words, by_log, _ = _contract(tmp_path, capsys, monkeypatch, bam, fa, loci[:32], P, 8, n_reps, (0.3, 0.7), 2)
    called = [int(f[HEAD.index("CALLED_ALL")]) for f in sens]
    print("CALLED_ALL per line:", called)
    assert any(c > 0 for c in called) and any(c < n_reps for c in called), called
    assert by_words == by_log


def test_mnv_scan_equals_its_passes_next_to_indels_and_clips(tmp_path, capsys, monkeypatch):
    """(b) bam_cigars, S = 4, R = 3, target 0.4, L = 2: bi-allelic and indel-candidate rows; at least one joint verdict is decided by
    the host, and the count by the joint words is the run log's."""
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    sens, by_words, by_log, _ = _contract(tmp_path, capsys, monkeypatch, bam, fa, loci, P, 4, 3, (0.4,), 2)
    print("joint verdicts decided by the host: %d by the words, %d by the log" % (by_words, by_log))
    print("CALLED_ALL per line:", [int(f[HEAD.index("CALLED_ALL")]) for f in sens])
    assert by_words == by_log and by_words > 0, "no joint verdict reached the host path"


def test_whole_and_listed_builds_give_the_same_files(tmp_path, capsys, monkeypatch):
    """(c) Case (a) with L = 3 under --spikeScanBuild whole and listed: every file byte for byte, no whole fallback."""
    bam, fa, loci, P, _ = TS._inputs("synth", str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci[:32])
    targets = (0.3, 0.7)
    # (the same prefix for both runs: the .cut.vcf names it)
    def files():
        return {n: open(str(tmp_path / n), "rb").read() for n in sorted(os.listdir(str(tmp_path))) if n.startswith("o.")}
    _scan(tmp_path, capsys, monkeypatch, "o", bam, fa, bed, P, 8, 4, targets, 3, spikeScanBuild="whole")
    whole = files()
    for n in whole:
        os.remove(str(tmp_path / n))
    _, log, _ = _scan(tmp_path, capsys, monkeypatch, "o", bam, fa, bed, P, 8, 4, targets, 3, spikeScanBuild="listed")
    listed = files()
    assert sorted(whole) == sorted(listed) and all("o" + s in whole for s in PAGES + SUFFIXES)
    assert all("o.spikeScan%g.mnv.rate.bedgraph" % t in whole for t in targets)
    for n in whole:
        assert whole[n] == listed[n], n
    closing = re.findall(r"^--spikeScanBuild listed: (\d+) listed builds, (\d+) whole fallbacks, (\d+) replicate-0 row checks$", log, re.M)
    assert len(closing) == 1 and int(closing[0][0]) > 0 and int(closing[0][1]) == 0 and int(closing[0][2]) > 0
    per_pass = [m for m in (spike.scan_pass_line(l) for l in log.splitlines()) if m is not None]
    assert per_pass and all(m["whole"] == 0 for m in per_pass)


def test_mnv_scan_with_lod_keeps_the_lod_files_and_its_pages_carry_no_lod(tmp_path, capsys, monkeypatch):
    """(d) bam_deep with --lod and the transversion rule: the LOD files are those of the run without the scan; no LOD column."""
    bam, fa, loci, P = ds_restate.load_fixture("bam_deep", str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    plain = TL._read(TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=["--lod"]), SUFFIXES + TL.LOD_SUFFIXES)
    got, _, _ = _scan(tmp_path, capsys, monkeypatch, "o", bam, fa, bed, P, 8, 2, (0.2,), 2, flags=["--lod"], spikeScanAlt="transversion")
    assert TL._read(got, SUFFIXES + TL.LOD_SUFFIXES) == plain
    assert len(open(got + ".lod.summary.txt").read().splitlines()) == 2
    sens = [l.split("\t") for l in open(got + ".spikeScan.mnv.sensitivity.txt").read().splitlines()]
    curve = [l.split("\t") for l in open(got + ".spikeScan.mnv.curve.txt").read().splitlines()]
    assert sens[0] == HEAD and curve[0] == list(spike.scan_mnv_curve_header([0.2])) and "LOD" not in sens[0] + curve[0]
    assert len(sens) > 1 and all(len(f) == len(HEAD) for f in sens) and all(len(f) == len(curve[0]) for f in curve)
    rule = lists.ALT_RULES["transversion"]
    for f in curve[1:]:
        assert len(f[2]) == 2 and f[3] == "".join(rule[x] for x in f[2])
