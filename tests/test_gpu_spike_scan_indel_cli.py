"""--spikeScanIndel on the GPU, through the command line: every line of the scan's two pages against the line the same variant and
target have in the pass's own --spikeAF --spikeVariants pass<k>.txt --spikeIndelReps R run (tools.spike_scan_lists --indel writes the
lists); the bedgraphs from the pages; the full-depth files those of a run without the flags; the run log's opening line, pass lines
and its count of host-decided verdicts against the records of smc_scan_detect_keys."""
import argparse
import os
import re
import sys

import pytest

from conftest import ROOT
from smcounter_amd import abi, devplanes, spike
from smcounter_amd.tools import spike_scan_lists as lists

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line)
import test_gpu_spike as TS  # noqa: E402  (the small inputs)

pytestmark = pytest.mark.gpu
SEED = 20240607
SUFFIXES = TL.SUFFIXES
N_SENS = len(spike.SCAN_SENSITIVITY_HEADER)


def _contract(tmp_path, capsys, monkeypatch, bam, fa, loci, P, rule, stride, n_reps, targets):
    """-> (the sensitivity page's lines as fields, the verdicts smc_scan_detect_keys left to the host by its records, that number by
    the run log)."""
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    plain = TL._read(TL._run_cli(tmp_path, "o", bam, fa, bed, P), SUFFIXES)
    host_records, snv_calls = [], []
    real, real_snv = devplanes.scan_detect_keys, devplanes.scan_detect

    def spy(*a, **kw):
        rec, todo, ids = real(*a, **kw)
        host_records.append(int(((rec["mt_verdict"] >> 30) == abi.SCAN_HOST).sum()))
        assert len(todo) == host_records[-1]
        return rec, todo, ids
    monkeypatch.setattr(devplanes, "scan_detect_keys", spy)
    monkeypatch.setattr(devplanes, "scan_detect", lambda *a, **kw: snv_calls.append(1) or real_snv(*a, **kw))
    capsys.readouterr()
    text = ",".join("%g" % t for t in targets)
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, spikeScan=text, spikeScanReps=n_reps, spikeScanStride=stride, spikeScanIndel=rule,
                      dsSeed=SEED)
    log = capsys.readouterr().out
    monkeypatch.setattr(devplanes, "scan_detect_keys", real)
    monkeypatch.setattr(devplanes, "scan_detect", real_snv)
    assert host_records and not snv_calls
    assert TL._read(got, SUFFIXES) == plain, "the full-depth files changed with --spikeScanIndel"
    assert not [f for f in os.listdir(str(tmp_path)) if ".spikeAF" in f]
    # the passes as runs of their own
    names = lists.main(argparse.Namespace(runPath=None, bedTarget=bed, refGenome=fa, stride=stride, alt="transition", indel=rule,
                                          outPrefix=str(tmp_path / "scan")))
    n_skipped = int(open(str(tmp_path / "scan.passes.txt")).read().splitlines()[-1].split("\t")[1])
    want_sens, want_curve, ks = {}, {}, []
    for name in names:
        k = int(re.search(r"\.pass(\d+)\.txt$", name).group(1))
        ks.append(k)
        ref = TL._run_cli(tmp_path, "p%d" % k, bam, fa, bed, P, spikeAF=text, spikeVariants=name, spikeIndelReps=n_reps, dsSeed=SEED)
        sens = [l.split("\t") for l in open(ref + ".spikeAF.sensitivity.txt").read().splitlines()]
        assert sens[0] == list(spike.SENSITIVITY_HEADER)
        for f in sens[1:]:
            assert int(f[1]) % stride == k
            want_sens[(f[0], int(f[1]), f[4])] = f[:N_SENS]          # (without PI_MEAN and PI_MIN)
        curve = [l.split("\t") for l in open(ref + ".spikeAF.curve.txt").read().splitlines()]
        assert curve[0] == list(spike.curve_header(targets))
        for f in curve[1:]:
            want_curve[(f[0], int(f[1]))] = f
    capsys.readouterr()
    listed = [l.split("\t") for name in names for l in open(name).read().splitlines()]
    scanned = [(f[0], int(f[1])) for f in listed]
    texts = {(f[0], int(f[1])): (f[2], f[3]) for f in listed}
    in_order = [(c, p) for c, p in loci if (c, p) in set(scanned)]
    assert len(scanned) == len(set(scanned)) == len(in_order) and len(scanned) + n_skipped == len(set(loci))
    sens = [l.split("\t") for l in open(got + ".spikeScan.sensitivity.txt").read().splitlines()]
    assert sens[0] == list(spike.SCAN_SENSITIVITY_HEADER)
    assert [(f[0], int(f[1])) for f in sens[1:]] == [cp for cp in in_order for _ in targets]
    for f in sens[1:]:
        assert f == want_sens[(f[0], int(f[1]), f[4])], (f, want_sens[(f[0], int(f[1]), f[4])])
        assert (f[2], f[3]) == texts[(f[0], int(f[1]))] and len(f[2]) != len(f[3])            # REF and ALT hold the indel's texts
    assert len(sens) - 1 == len(want_sens) == len(scanned) * len(targets)
    curve = [l.split("\t") for l in open(got + ".spikeScan.curve.txt").read().splitlines()]
    assert curve[0] == list(spike.curve_header(targets))
    assert [(f[0], int(f[1])) for f in curve[1:]] == in_order
    for f in curve[1:]:
        assert f == want_curve[(f[0], int(f[1]))]
    # the bedgraphs follow from the pages; the position is the anchor
    i_rate, i_t95 = spike.SCAN_SENSITIVITY_HEADER.index("RATE"), curve[0].index("T95")
    for t in targets:
        lines = open("%s.spikeScan%g.rate.bedgraph" % (got, t)).read().splitlines()
        mine = [f for f in sens[1:] if f[4] == "%g" % t]
        assert lines == ["%s\t%d\t%d\t%s" % (f[0], int(f[1]) - 1, int(f[1]), f[i_rate]) for f in mine] and len(mine) == len(scanned)
    t95 = {(f[0], int(f[1])): f[i_t95] for f in curve[1:]}
    lines = open(got + ".spikeScan.t95.bedgraph").read().splitlines()
    assert lines == ["%s\t%d\t%d\t%s" % (c, p - 1, p, "1" if t95.get((c, p), "NA") == "NA" else t95[(c, p)]) for c, p in loci]
    # the run log: the opening line names the rule and what a locus was skipped for; a line per pass; the closing line
    opening = re.findall(r"^--spikeScan: (\d+) loci in (\d+) passes of stride (\d+) \(--spikeScanIndel (\w+)\), (\d+) skipped for a letter "
                         r"inside the footprint that is not A, C, G or T or lies past the chromosome's end; (\d+) replicates x (\d+) targets$",
                         log, re.M)
    assert opening == [("%d" % len(scanned), "%d" % len(ks), "%d" % stride, rule, "%d" % n_skipped, "%d" % n_reps, "%d" % len(targets))]
    per_pass = re.findall(r"^--spikeScan pass (\d+): (\d+) variants, (\d+) copies, (\d+) builds, (\d+) verdicts decided by the host, [0-9.]+ s$",
                          log, re.M)
    assert [int(m[0]) for m in per_pass] == sorted(ks)
    assert sum(int(m[1]) for m in per_pass) == len(scanned)
    closing = re.findall(r"^--spikeScan: (\d+) loci x (\d+) targets x (\d+) replicates in (\d+) passes: .* (\d+) of (\d+) verdicts decided by the "
                         r"host, stage [0-9.]+ s$", log, re.M)
    assert len(closing) == 1
    assert [int(x) for x in closing[0][:4]] == [len(scanned), len(targets), n_reps, len(ks)]
    assert int(closing[0][5]) == len(scanned) * len(targets) * n_reps
    by_log = int(closing[0][4])
    assert by_log == sum(int(m[4]) for m in per_pass)
    return sens[1:], sum(host_records), by_log


TARGETS = {"del1": (0.3, 0.7), "dup2": (0.3, 0.7)}


@pytest.mark.parametrize("rule", ("del1", "dup2"))
def test_scan_equals_its_passes_on_the_synthetic_bam(tmp_path, capsys, monkeypatch, rule):
    """The file's first 32 loci, S = 8, R = 4, the SNV scan test's input and targets.  Both verdicts must occur, and the test says
    so: a comparison of nothing with nothing cannot pass."""
    bam, fa, loci, P, _ = TS._inputs("synth", str(tmp_path))
    n_reps = 4
    sens, by_records, by_log = _contract(tmp_path, capsys, monkeypatch, bam, fa, loci[:32], P, rule, 8, n_reps, TARGETS[rule])
    i_called = spike.SCAN_SENSITIVITY_HEADER.index("CALLED")
    called = [int(f[i_called]) for f in sens]
    print("CALLED per line:", called)
    assert any(c > 0 for c in called) and any(c < n_reps for c in called), called
    assert by_records == by_log


def test_scan_equals_its_passes_next_to_indels_and_clips(tmp_path, capsys, monkeypatch):
    """bam_cigars with del2: loci next to the file's own indels and clips, records that end inside a footprint, the bed's stretches
    not in position order."""
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    sens, by_records, by_log = _contract(tmp_path, capsys, monkeypatch, bam, fa, loci, P, "del2", 4, 3, (0.4,))
    print("verdicts decided by the host: %d by the records, %d by the log" % (by_records, by_log))
    called = [int(f[spike.SCAN_SENSITIVITY_HEADER.index("CALLED")]) for f in sens]
    print("CALLED per line:", called)
    assert by_records == by_log
