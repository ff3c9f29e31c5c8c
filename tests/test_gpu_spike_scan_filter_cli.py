"""--spikeScanFilter on the GPU, through the command line, with a --bedTandemRepeats file over the first half of the scanned positions:
every line of .spikeScan.filter.txt (and of the cells' pages) recomputed from the FILTER and CALLED columns of the replicate pages the
passes write as runs of their own (--spikeAF --spikeVariants pass<k>.txt --spikeReps R, tools.spike_scan_lists writes the lists); the
curve and the bedgraphs from the page; every file of the same scan without the switch byte for byte; the run log's new line."""
import argparse
import dataclasses
import os
import re
import sys

import pytest

from conftest import ROOT
from smcounter_amd import devplanes, spike
from smcounter_amd.tools import spike_scan_lists as lists

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import scan_filter_pages as pages  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line)
import test_gpu_spike as TS  # noqa: E402  (the small inputs)

pytestmark = pytest.mark.gpu
SEED = 20240607
I_CALLED, I_PASS = pages.HEADER.index("CALLED"), pages.HEADER.index("PASS")


def _lines(path):
    return [l.split("\t") for l in open(path).read().splitlines()]


def _half_bed(path, loci):
    """A tandem-repeat track over the lower half of every chromosome's scanned positions (start open, end closed)."""
    by = {}
    for c, p in loci:
        by.setdefault(c, []).append(int(p))
    with open(path, "w") as fh:
        for c in sorted(by):
            ps = sorted(by[c])
            fh.write("%s\t%d\t%d\n" % (c, ps[0] - 1, ps[(len(ps) - 1) // 2]))
    return path


def _files(tmp, tag):
    return {f: open(os.path.join(str(tmp), f), "rb").read() for f in sorted(os.listdir(str(tmp))) if f.startswith(tag + ".")}


def _contract(tmp_path, capsys, monkeypatch, bam, fa, loci, P, stride, n_reps, targets, rule=None, fracs=None, rpbs=None):
    """-> (the lines of every filter page of the run as fields, the called records whose FILTER the host decided, the name totals)."""
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    trf = _half_bed(str(tmp_path / "trf.bed"), loci)
    text = ",".join("%g" % t for t in targets)
    axis = None
    if fracs:
        axis = ("depth", "FRACTION", fracs, "spikeScanDepth", "spikeIndelDepth" if rule else "spikeDepth")
    if rpbs:
        axis = ("rpb", "RPB", rpbs, "spikeScanRpb", "spikeIndelRpb" if rule else "spikeRpb")
    atext = ",".join("%g" % x for x in axis[2]) if axis else None
    more = dict(spikeScan=text, spikeScanReps=n_reps, spikeScanStride=stride, dsSeed=SEED, bedTandemRepeats=trf)
    if rule:
        more["spikeScanIndel"] = rule
    if axis:
        more[axis[3]] = atext
    TL._run_cli(tmp_path, "o", bam, fa, bed, P, **more)
    without = _files(tmp_path, "o")
    assert without and not [f for f in without if "filter" in f or "pass" in f]
    calls = []
    real = devplanes.scan_filter

    def spy(*a, **kw):
        out = real(*a, **kw)
        calls.append(out.shape)
        return out
    monkeypatch.setattr(devplanes, "scan_filter", spy)
    capsys.readouterr()
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=["--spikeScanFilter"], **more)
    log = capsys.readouterr().out
    monkeypatch.setattr(devplanes, "scan_filter", real)
    with_flag = _files(tmp_path, "o")
    # every file of the scan without the switch - the full-depth files among them - byte for byte; the new files are the filter's
    for name, data in without.items():
        assert with_flag[name] == data, "%s changed with --spikeScanFilter" % name
    new = ["o.spikeScan.filter.txt", "o.spikeScan.filter.curve.txt", "o.spikeScan.t95pass.bedgraph"] + \
        ["o.spikeScan%g.passrate.bedgraph" % t for t in targets] + (["o.spikeScan.%s.filter.txt" % axis[0]] if axis else [])
    assert sorted(set(with_flag) - set(without)) == sorted(new)
    assert calls, "smc_scan_filter was not called"
    # the passes as runs of their own
    names = lists.main(argparse.Namespace(runPath=None, bedTarget=bed, refGenome=fa, stride=stride, alt="transition", outPrefix=str(tmp_path / "scan"),
                                          **(dict(indel=rule) if rule else {})))
    reps = {"spikeIndelReps" if rule else "spikeReps": n_reps}
    if axis:
        reps[axis[4]] = atext
    full, cells = {}, {}
    for name in names:
        k = int(re.search(r"\.pass(\d+)\.txt$", name).group(1))
        ref = TL._run_cli(tmp_path, "p%d" % k, bam, fa, bed, P, spikeAF=text, spikeVariants=name, dsSeed=SEED, bedTandemRepeats=trf, **reps)
        page = _lines(ref + ".spikeAF.replicates.txt")
        assert page[0] == list(spike.REPLICATES_HEADER) and page[0][5] == "REP" and page[0][-2:] == ["FILTER", "CALLED"]
        for f in page[1:]:
            assert int(f[5]) == len(full.setdefault(tuple(f[:5]), []))             # (replicates ascending)
            full[tuple(f[:5])].append((f[-2], f[-1]))
        if axis:
            page = _lines("%s.spikeAF.%s.replicates.txt" % (ref, axis[0]))
            assert page[0][:9] == list(spike.REPLICATES_HEADER[:5]) + [axis[1], "MTDEPTH", "REP", "SEED"] and page[0][-2:] == ["FILTER", "CALLED"]
            for f in page[1:]:
                cells.setdefault(tuple(f[:7]), []).append((f[-2], f[-1]))
    capsys.readouterr()
    assert all(len(r) == n_reps for r in list(full.values()) + list(cells.values()))
    # the page: every line from the passes' FILTER and CALLED columns, in the sensitivity page's order
    sens = _lines(got + ".spikeScan.sensitivity.txt")[1:]
    page = _lines(got + ".spikeScan.filter.txt")
    assert page[0] == list(pages.HEADER)
    assert [f[:5] for f in page[1:]] == [f[:5] for f in sens] and len(page) - 1 == len(full)
    for f in page[1:]:
        assert f == pages.line(f[:5], full[tuple(f[:5])]), (f, full[tuple(f[:5])])
    i_sens_called = spike.SCAN_SENSITIVITY_HEADER.index("CALLED")
    assert [f[I_CALLED] for f in page[1:]] == [f[i_sens_called] for f in sens]
    # the curve and the bedgraphs follow from the page
    scan_curve = _lines(got + ".spikeScan.curve.txt")
    curve = _lines(got + ".spikeScan.filter.curve.txt")
    assert curve[0] == ["CHROM", "POS", "REF", "ALT", "N"] + ["RATE_PASS@%g" % t for t in sorted(targets)] + ["T95_PASS"]
    assert [f[:5] for f in curve[1:]] == [f[:5] for f in scan_curve[1:]]
    for f in curve[1:]:
        assert f == pages.curve_line(f[:4], int(f[4]), targets, [full[tuple(f[:4]) + ("%g" % t,)] for t in targets])
    pages.check_bedgraphs(got, targets, [(c, int(p)) for c, p in loci], page, curve)
    all_lines = list(page[1:])
    if axis:
        cell_sens = _lines("%s.spikeScan.%s.sensitivity.txt" % (got, axis[0]))[1:]
        cpage = _lines("%s.spikeScan.%s.filter.txt" % (got, axis[0]))
        assert cpage[0] == list(pages.HEADER[:5]) + [axis[1], "MTDEPTH"] + list(pages.HEADER[5:])
        assert [f[:7] for f in cpage[1:]] == [f[:7] for f in cell_sens] and len(cpage) - 1 == len(cells)
        for f in cpage[1:]:
            assert f == pages.line(f[:5], cells[tuple(f[:7])], f[5:7]), (f, cells[tuple(f[:7])])
        all_lines += [f[:5] + f[7:] for f in cpage[1:]]
    # the run log: the scan's own lines keep their text, one line more
    assert re.search(r"^--spikeScan: \d+ loci x \d+ targets x \d+ replicates in \d+ passes: .* \d+ of \d+ verdicts decided by the host, "
                     r"stage [0-9.]+ s$", log, re.M)
    assert len(re.findall(r"^--spikeScan pass \d+: \d+ variants, \d+ copies, \d+ builds, \d+ verdicts decided by the host, [0-9.]+ s$", log,
                          re.M)) == len(names)
    last = re.findall(r"^--spikeScanFilter: (\d+) of (\d+) called records PASS, the FILTER of (\d+) decided by the host; (.*)$", log, re.M)
    assert len(last) == 1
    n_pass, n_called, n_host, tail = last[0]
    totals = [sum(int(f[pages.HEADER.index(n)]) for f in all_lines) for n in pages.NAMES]
    assert tail == ", ".join("%s %d" % (n, x) for n, x in zip(pages.NAMES, totals))
    assert int(n_called) == sum(int(f[I_CALLED]) for f in all_lines) and int(n_pass) == sum(int(f[I_PASS]) for f in all_lines)
    assert 0 <= int(n_host) <= int(n_called)
    print("FILTER decided by the host for %s of %s called records; totals: %s" % (n_host, n_called, tail))
    return all_lines, int(n_host), dict(zip(pages.NAMES, totals))


def test_filter_pages_equal_the_passes_on_the_synthetic_bam_and_next_to_indels_and_clips(tmp_path, capsys, monkeypatch):
    """The inputs of test_gpu_spike_scan_cli.py.  The synthetic file's first 32 loci, S = 8, R = 4, targets 0.3 and 0.7: the called
    replicates in the lower half of the window are RepT, those above it are not, and no called record's FILTER is left to the host.
    bam_cigars, S = 4, R = 3, target 0.4: bi-allelic and indel-candidate rows next to the planted SNV - the host-decided share may be
    anything there.
    The feature must decide something: a line that loses called replicates to a flag, and a line that keeps all of them.  No repeat
    file can give the second on these two inputs as they stand: at their --rpb of 3 the strong-barcode threshold is 4
    (VcParams.smt), the planted allele has fewer than two strong barcodes, and every called record of the passes' own runs holds LSM
    (255 of 255 on the synthetic file, 284 of 284 on bam_cigars - measured on an MI355X).  So the synthetic input is scanned a second
    time at --rpb 2.9 (threshold 3: no LSM there; 127 of 255 called records RepT, 128 PASS), and the two conditions are asserted over
    the three scans."""
    for name in ("synth", "cigars", "synth29"):
        (tmp_path / name).mkdir()
    bam, fa, loci, P, _ = TS._inputs("synth", str(tmp_path / "synth"))
    half = sorted(p for _, p in loci[:32])[15]
    i_rept = pages.HEADER.index("RepT")
    lines = []
    for name, Q in (("synth", P), ("synth29", dataclasses.replace(P, rpb=2.9))):
        mine, n_host, totals = _contract(tmp_path / name, capsys, monkeypatch, bam, fa, loci[:32], Q, 8, 4, (0.3, 0.7))
        assert n_host == 0
        # RepT holds exactly for the called replicates of the covered half
        for f in mine:
            assert int(f[i_rept]) == (int(f[I_CALLED]) if int(f[1]) <= half else 0), f
        assert totals["RepT"] > 0
        lines += mine
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path / "cigars"))
    lines += _contract(tmp_path / "cigars", capsys, monkeypatch, bam, fa, loci, P, 4, 3, (0.4,))[0]
    pairs = [(int(f[I_CALLED]), int(f[I_PASS])) for f in lines]
    print("(CALLED, PASS) per line:", pairs)
    assert any(p < c for c, p in pairs), "no line with PASS < CALLED"
    assert any(p == c > 0 for c, p in pairs), "no line with PASS == CALLED > 0"


def test_indel_filter_pages_equal_the_passes(tmp_path, capsys, monkeypatch):
    """--spikeScanIndel del1 on the synthetic file's first 16 loci, S = 4, R = 3: the words of a deletion (REF and ALT its texts)."""
    bam, fa, loci, P, _ = TS._inputs("synth", str(tmp_path))
    lines, n_host, totals = _contract(tmp_path, capsys, monkeypatch, bam, fa, loci[:16], P, 4, 3, (0.3, 0.7), rule="del1")
    assert any(int(f[I_CALLED]) > 0 for f in lines)


def test_depth_filter_page_equals_the_passes(tmp_path, capsys, monkeypatch):
    """--spikeScanDepth 0.5 on the synthetic file's first 16 loci, S = 4, R = 3."""
    bam, fa, loci, P, _ = TS._inputs("synth", str(tmp_path))
    lines, n_host, totals = _contract(tmp_path, capsys, monkeypatch, bam, fa, loci[:16], P, 4, 3, (0.3, 0.7), fracs=(0.5,))
    assert any(int(f[I_CALLED]) > 0 for f in lines) and n_host == 0


def test_rpb_filter_page_equals_the_passes(tmp_path, capsys, monkeypatch):
    """--spikeScanRpb 4 on the synthetic file's first 16 loci, S = 4, R = 3."""
    bam, fa, loci, P, _ = TS._inputs("synth", str(tmp_path))
    lines, n_host, totals = _contract(tmp_path, capsys, monkeypatch, bam, fa, loci[:16], P, 4, 3, (0.3, 0.7), rpbs=(4,))
    assert any(int(f[I_CALLED]) > 0 for f in lines) and n_host == 0
