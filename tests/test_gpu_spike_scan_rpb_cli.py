"""--spikeScanRpb on the GPU, through the command line: every line of the two rpb pages against the line the same variant, target and
reads-per-barcode target have in the pass's own --spikeAF --spikeVariants pass<k>.txt --spikeReps R --spikeRpb <r...> run (for an indel
scan --spikeIndelReps R --spikeIndelRpb <r...>); the bedgraphs and the need page rederived from the pages; the scan's own pages and the
full-depth files those of the run without the flag; the run log's counts; a file without a barcode of two names refused under the
flag's name."""
import argparse
import os
import re
import sys

import pytest

from conftest import ROOT
from smcounter_amd import abi, cli, devplanes, dsaf, spike
from smcounter_amd.tools import spike_scan_lists as lists

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import ds_rpb_restate  # noqa: E402
import spike_rpb_restate as RR  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line)
import test_gpu_spike as TS  # noqa: E402  (the small inputs)

pytestmark = pytest.mark.gpu
SEED = 20240607
SUFFIXES = TL.SUFFIXES
SENS = spike.SCAN_RPB_SENSITIVITY_HEADER
PAGE = spike.cell_sensitivity_header(spike.RPB_AXIS)
DROP = [PAGE.index(c) for c in ("PI_MEAN", "PI_MIN")]


def _lines(path):
    return [l.split("\t") for l in open(path).read().splitlines()]


def _scan_files(prefix, targets):
    names = [".spikeScan.sensitivity.txt", ".spikeScan.curve.txt", ".spikeScan.t95.bedgraph"] + [".spikeScan%g.rate.bedgraph" % t for t in targets]
    return [open(prefix + n, "rb").read() for n in names]


def _contract(tmp_path, capsys, monkeypatch, bam, fa, loci, P, stride, n_reps, targets, rpbs, rule=None):
    """-> (the rpb sensitivity page's lines as fields, the verdicts the detect entry left to the host by its records)."""
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    text, rtext = ",".join("%g" % t for t in targets), ",".join("%g" % r for r in rpbs)
    more = dict(spikeScanIndel=rule) if rule else {}
    plain = TL._read(TL._run_cli(tmp_path, "o", bam, fa, bed, P), SUFFIXES)
    without = _scan_files(TL._run_cli(tmp_path, "o", bam, fa, bed, P, spikeScan=text, spikeScanReps=n_reps, spikeScanStride=stride,
                                      dsSeed=SEED, **more), targets)
    assert not [f for f in os.listdir(str(tmp_path)) if ".rpb." in f or ".dsRpb" in f or ".r95." in f]
    host_records, selects = [], []
    entry = "scan_detect_keys" if rule else "scan_detect"
    real, real_sel, real_one = getattr(devplanes, entry), devplanes.select_copies_reads, devplanes.select_run

    def spy(*a, **kw):
        out = real(*a, **kw)
        host_records.append(int(((out[0]["mt_verdict"] >> 30) == abi.SCAN_HOST).sum()))
        return out

    def spy_sel(eng, runs, A, lo, d_masks, n_words, copy_stride, n_masks):
        selects.append((len(runs), n_masks, copy_stride == n_masks * n_words))
        return real_sel(eng, runs, A, lo, d_masks, n_words, copy_stride, n_masks)

    def no_single(*a, **kw):
        raise AssertionError("the scan made a single select_run call")
    monkeypatch.setattr(devplanes, entry, spy)
    monkeypatch.setattr(devplanes, "select_copies_reads", spy_sel)
    monkeypatch.setattr(devplanes, "select_run", no_single)
    capsys.readouterr()
    got = TL._run_cli(tmp_path, "o", bam, fa, bed, P, spikeScan=text, spikeScanReps=n_reps, spikeScanStride=stride, spikeScanRpb=rtext,
                      dsSeed=SEED, **more)
    log = capsys.readouterr().out
    monkeypatch.setattr(devplanes, entry, real)
    monkeypatch.setattr(devplanes, "select_copies_reads", real_sel)
    monkeypatch.setattr(devplanes, "select_run", real_one)
    assert TL._read(got, SUFFIXES) == plain, "the full-depth files changed with --spikeScanRpb"
    assert _scan_files(got, targets) == without, "the scan's own pages changed with --spikeScanRpb"
    assert not [f for f in os.listdir(str(tmp_path)) if ".spikeAF" in f]
    # the passes as runs of their own
    names = lists.main(argparse.Namespace(runPath=None, bedTarget=bed, refGenome=fa, stride=stride, alt="transition", outPrefix=str(tmp_path / "scan"),
                                          **(dict(indel=rule) if rule else {})))
    want_sens, want_curve, ks = {}, {}, []
    reps = dict(spikeIndelReps=n_reps, spikeIndelRpb=rtext) if rule else dict(spikeReps=n_reps, spikeRpb=rtext)
    for name in names:
        k = int(re.search(r"\.pass(\d+)\.txt$", name).group(1))
        ks.append(k)
        ref = TL._run_cli(tmp_path, "p%d" % k, bam, fa, bed, P, spikeAF=text, spikeVariants=name, dsSeed=SEED, **reps)
        sens = _lines(ref + ".spikeAF.rpb.sensitivity.txt")
        assert sens[0] == list(PAGE)
        for f in sens[1:]:
            want_sens[(f[0], int(f[1]), f[4], f[5])] = [x for n, x in enumerate(f) if n not in DROP]      # (N_MEAN stays)
        curve = _lines(ref + ".spikeAF.rpb.curve.txt")
        assert curve[0] == list(spike.depth_curve_header(targets, False, spike.RPB_AXIS))
        for f in curve[1:]:
            want_curve[(f[0], int(f[1]), f[4])] = f
    capsys.readouterr()
    scanned = [(l.split("\t")[0], int(l.split("\t")[1])) for name in names for l in open(name).read().splitlines()]
    in_order = [(c, p) for c, p in loci if (c, p) in set(scanned)]
    sens = _lines(got + ".spikeScan.rpb.sensitivity.txt")
    assert sens[0] == list(SENS) and "N_MEAN" in SENS and "PI_MEAN" not in SENS
    assert [(f[0], int(f[1]), f[4], f[5]) for f in sens[1:]] == \
        [(c, p, "%g" % t, "%g" % r) for c, p in in_order for t in targets for r in rpbs]
    for f in sens[1:]:
        assert f == want_sens[(f[0], int(f[1]), f[4], f[5])], (f, want_sens[(f[0], int(f[1]), f[4], f[5])])
    assert len(sens) - 1 == len(want_sens) == len(scanned) * len(targets) * len(rpbs)
    curve = _lines(got + ".spikeScan.rpb.curve.txt")
    assert curve[0] == list(spike.depth_curve_header(targets, False, spike.RPB_AXIS))
    assert [(f[0], int(f[1]), f[4]) for f in curve[1:]] == [(c, p, d) for c, p in in_order for d in ["full"] + ["%g" % r for r in rpbs]]
    for f in curve[1:]:
        assert f == want_curve[(f[0], int(f[1]), f[4])], (f, want_curve[(f[0], int(f[1]), f[4])])
    assert len(curve) - 1 == len(want_curve)
    # the bedgraphs follow from the pages
    i_rate, i_t95, i_nm = SENS.index("RATE"), curve[0].index("T95"), SENS.index("N_MEAN")
    for t in targets:
        for r in rpbs:
            mine = [f for f in sens[1:] if f[4] == "%g" % t and f[5] == "%g" % r]
            assert open("%s.spikeScan%g.dsRpb%g.rate.bedgraph" % (got, t, r)).read().splitlines() == \
                ["%s\t%d\t%d\t%s" % (f[0], int(f[1]) - 1, int(f[1]), f[i_rate]) for f in mine] and len(mine) == len(scanned)
    for r in rpbs:
        t95 = {(f[0], int(f[1])): f[i_t95] for f in curve[1:] if f[4] == "%g" % r}
        assert open("%s.spikeScan.dsRpb%g.t95.bedgraph" % (got, r)).read().splitlines() == \
            ["%s\t%d\t%d\t%s" % (c, p - 1, p, "1" if t95.get((c, p), "NA") == "NA" else t95[(c, p)]) for c, p in loci]
    # the need page: R95 over the listed r ascending with full depth on top, read from the top - rederived from the scan's page and the rpb page
    full = {(f[0], int(f[1]), f[4]): f for f in _lines(got + ".spikeScan.sensitivity.txt")[1:]}
    n_full = {(f[0], int(f[1])): f[4] for f in _lines(got + ".spikeScan.curve.txt")[1:]}
    i_frate = spike.SCAN_SENSITIVITY_HEADER.index("RATE")
    need = _lines(got + ".spikeScan.rpb.need.txt")
    assert need[0] == ["CHROM", "POS", "REF", "ALT", "TARGET", "N", "R95", "N95"]
    assert [(f[0], int(f[1]), f[4]) for f in need[1:]] == [(c, p, "%g" % t) for c, p in in_order for t in targets]
    r95 = {}
    for f in need[1:]:
        c, p, t = f[0], int(f[1]), f[4]
        axis = [(float("inf"), float(full[(c, p, t)][i_frate]), "full", dsaf.frac_text(float(n_full[(c, p)])))]
        axis += [(float(g[5]), float(g[i_rate]), g[5], g[i_nm]) for g in sens[1:] if (g[0], int(g[1]), g[4]) == (c, p, t)]
        best = None
        for d in sorted(axis, key=lambda x: -x[0]):
            if not d[1] >= 0.95:
                break
            best = d
        assert f[5] == n_full[(c, p)]
        assert f[6:] == (["NA"] * 2 if best is None else [best[2], best[3]]), (f, axis)
        r95[(c, p, t)] = f[6]
    above = "%g" % (2 * max([P.rpb] + list(rpbs)))
    for t in targets:
        number = lambda w: above if w == "NA" else "%g" % P.rpb if w == "full" else w
        assert open("%s.spikeScan%g.r95.bedgraph" % (got, t)).read().splitlines() == \
            ["%s\t%d\t%d\t%s" % (c, p - 1, p, number(r95.get((c, p, "%g" % t), "NA"))) for c, p in loci]
    # the run log: the passes' lines count the cells' builds too; one line more names the r, the cells and the selections; a line per r
    per_pass = re.findall(r"^--spikeScan pass (\d+): (\d+) variants, (\d+) copies, (\d+) builds, (\d+) verdicts decided by the host, [0-9.]+ s$",
                          log, re.M)
    assert [int(m[0]) for m in per_pass] == sorted(ks)
    assert all(int(m[3]) == int(m[2]) * (1 + len(rpbs)) for m in per_pass)
    closing = re.findall(r"^--spikeScan: (\d+) loci x (\d+) targets x (\d+) replicates in (\d+) passes: .* (\d+) copies built and called, "
                         r"(\d+) of (\d+) verdicts decided by the host, stage [0-9.]+ s$", log, re.M)
    assert len(closing) == 1
    assert int(closing[0][4]) == sum(int(m[3]) for m in per_pass)
    assert int(closing[0][5]) == sum(int(m[4]) for m in per_pass) == sum(host_records)
    assert int(closing[0][6]) == len(scanned) * len(targets) * n_reps * (1 + len(rpbs))
    last = re.findall(r"^--spikeScanRpb: reads-per-barcode targets (\S+): (\d+) cells per pass, (\d+) select_copies_reads calls$", log, re.M)
    assert last == [(rtext, "%d" % (len(targets) * len(rpbs)), "%d" % len(selects))]
    assert selects and all(m == len(rpbs) and tight for _, m, tight in selects)
    # (one selection call per batch of copies, whatever the number of r: the copies of all calls are the copies built)
    assert sum(b for b, _, _ in selects) * (1 + len(rpbs)) == int(closing[0][4])
    per_r = re.findall(r"^--spikeScanRpb (\S+): sampler philox, seed (\d+), probKeep (\S+), threshold (\d+), (\d+) of (\d+) read names kept "
                       r"\(mtDepth (\d+)\)$", log, re.M)
    assert [m[0] for m in per_r] == ["%g" % r for r in rpbs] and all(int(m[1]) == SEED and int(m[6]) == P.mtDepth for m in per_r)
    assert all(0 < int(m[4]) <= int(m[5]) for m in per_r)
    return sens[1:], sum(host_records)


def test_scan_rpb_equals_its_passes_on_the_synthetic_bam(tmp_path, capsys, monkeypatch):
    """The file's first 16 loci, S = 4, R = 3, targets 0.3 and 0.7, the two smallest r of the --spikeRpb tests on this file.  Both
    verdicts must occur among the cells, and the test says so: a comparison of nothing with nothing cannot pass."""
    bam, fa, loci, P, _ = TS._inputs("synth", str(tmp_path))
    n_reps = 3
    sens, _ = _contract(tmp_path, capsys, monkeypatch, bam, fa, loci[:16], P, 4, n_reps, (0.3, 0.7), RR.RPB_TARGETS[:2])
    called = [int(f[SENS.index("CALLED")]) for f in sens]
    print("CALLED per cell line:", called)
    assert any(c > 0 for c in called) and any(c < n_reps for c in called), called


def test_indel_scan_rpb_equals_its_passes_next_to_indels_and_clips(tmp_path, capsys, monkeypatch):
    """bam_cigars with --spikeScanIndel del2 --spikeScanRpb r, S = 4, R = 3, target 0.4: the selections' records at the batched stride
    with their renumbered ids, the CIGAR words and pairs at the copies'."""
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    sens, by_records = _contract(tmp_path, capsys, monkeypatch, bam, fa, loci, P, 4, 3, (0.4,), RR.RPB_TARGETS[:1], rule="del2")
    called = [int(f[SENS.index("CALLED")]) for f in sens]
    print("verdicts decided by the host: %d; CALLED per cell line:" % by_records, called)


def test_a_file_without_a_multi_name_barcode_is_refused_under_the_flag(tmp_path):
    """--dsRpbSampler philox's refusal, named after this flag, and no page of the read axis written."""
    bam, fa, loci, P = ds_restate.make_case(str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci[:8])
    one = ds_rpb_restate.write_one_name_per_barcode(bam, str(tmp_path / "one.bam"))
    with pytest.raises(SystemExit, match=r"--spikeScanRpb 1\.5: .*one\.bam has no barcode with more than one read name"):
        cli.main(dict(outPrefix=str(tmp_path / "bad"), bamFile=one, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, hpLen=P.hpLen, refGenome=fa,
                      spikeScan="0.3", spikeScanReps=2, spikeScanRpb="1.5,3", dsSeed=SEED))
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("bad.")]
