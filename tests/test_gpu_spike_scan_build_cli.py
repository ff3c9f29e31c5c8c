"""--spikeScanBuild listed through the command line: every output file of the scan, and every full-depth file, byte for byte the
same run's with `whole`; the run log's pass lines count the builds made the whole way - none where the listed builder takes the run,
all of them on a run with unflagged reads."""
import dataclasses
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line)
import test_gpu_spike as TS  # noqa: E402  (the small inputs)

pytestmark = pytest.mark.gpu
SEED = 20240607
PASS_LINE = re.compile(r"^--spikeScan pass (\d+): (\d+) variants, (\d+) copies, (\d+) builds, (\d+) of them whole, (\d+) verdicts decided by the "
                       r"host, [0-9.]+ s$", re.M)
CLOSING = re.compile(r"^--spikeScanBuild listed: (\d+) listed builds, (\d+) whole fallbacks, (\d+) replicate-0 row checks$", re.M)


def _files(tmp_path, tag):
    """Every file the run with prefix `tag` wrote, by its name behind the prefix; the files are removed (the next run takes the name)."""
    out = {}
    for f in sorted(os.listdir(str(tmp_path))):
        if f.startswith(tag + "."):
            out[f[len(tag):]] = open(str(tmp_path / f), "rb").read()
            os.remove(str(tmp_path / f))
    return out


def _both(tmp_path, capsys, bam, fa, loci, P, flags=(), **kw):
    """The scan `whole` and `listed` with the same prefix -> (the listed run's pass lines as integers, its closing line's)."""
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, dsSeed=SEED, **kw)
    whole = _files(tmp_path, "o")
    capsys.readouterr()
    TL._run_cli(tmp_path, "o", bam, fa, bed, P, flags=flags, dsSeed=SEED, spikeScanBuild="listed", **kw)
    log = capsys.readouterr().out
    listed = _files(tmp_path, "o")
    assert sorted(whole) == sorted(listed) and any(".spikeScan." in n for n in whole) and ".smCounter.all.txt" in whole
    for name in whole:
        assert whole[name] == listed[name], "%s differs between --spikeScanBuild whole and listed" % name
    lines = [[int(x) for x in m] for m in PASS_LINE.findall(log)]
    closing = [[int(x) for x in m] for m in CLOSING.findall(log)]
    assert lines and len(closing) == 1
    assert closing[0][1] == sum(l[4] for l in lines) and closing[0][0] + closing[0][1] == sum(l[3] for l in lines)
    return lines, closing[0]


def _inputs(name, tmp_path):
    if name == "synth":
        bam, fa, loci, P, _ = TS._inputs("synth", str(tmp_path))
        return bam, fa, loci[:32], P, dict(spikeScan="0.3,0.7", spikeScanReps=4, spikeScanStride=8)
    bam, fa, loci, P = ds_restate.load_fixture(name, str(tmp_path))
    return bam, fa, loci, P, dict(spikeScan="0.4", spikeScanReps=3, spikeScanStride=4)


@pytest.mark.parametrize("name", ("synth", "bam_cigars"))
@pytest.mark.parametrize("axis", ("plain", "indel", "depth", "rpb", "filter"))
def test_listed_equals_whole(tmp_path, capsys, name, axis):
    bam, fa, loci, P, kw = _inputs(name, tmp_path)
    if axis == "indel":
        kw["spikeScanIndel"] = "del1"
    if axis == "depth":
        kw["spikeScanDepth"] = "0.5"
    if axis == "rpb":
        kw["spikeScanRpb"] = "2"
    lines, closing = _both(tmp_path, capsys, bam, fa, loci, P, flags=["--spikeScanFilter"] if axis == "filter" else (), **kw)
    assert all(l[4] == 0 for l in lines), "a pass fell back to whole builds: %r" % lines
    assert closing[0] > 0 and closing[1] == 0 and closing[2] > 0


@pytest.mark.parametrize("cell", ("spikeScanDepth", "spikeScanRpb", "filter"))
def test_listed_equals_whole_indel_scan_with_an_axis(tmp_path, capsys, cell):
    """--spikeScanIndel beside the other axes: the selections of the indel copies, and the FILTER words, through the listed builder."""
    bam, fa, loci, P, kw = _inputs("bam_cigars", tmp_path)
    if cell != "filter":
        kw[cell] = "0.5" if cell == "spikeScanDepth" else "2"
    lines, closing = _both(tmp_path, capsys, bam, fa, loci, P, flags=["--spikeScanFilter"] if cell == "filter" else (), spikeScanIndel="del1", **kw)
    assert all(l[4] == 0 for l in lines), "a pass fell back to whole builds: %r" % lines
    assert closing[0] > 0 and closing[1] == 0 and closing[2] > 0


def test_listed_equals_whole_with_lod_on_the_deep_fixture(tmp_path, capsys):
    bam, fa, loci, P = ds_restate.load_fixture("bam_deep", str(tmp_path))
    lines, closing = _both(tmp_path, capsys, bam, fa, loci, P, flags=["--lod"], spikeScan="0.2", spikeScanReps=2, spikeScanStride=8,
                           spikeScanAlt="transversion")
    assert all(l[4] == 0 for l in lines) and closing[1] == 0 and closing[2] > 0


def test_unflagged_reads_go_the_whole_way_and_are_counted(tmp_path, capsys):
    bam, fa, loci, P = ds_restate.load_fixture("bam_unflagged", str(tmp_path))
    lines, closing = _both(tmp_path, capsys, bam, fa, loci, P, spikeScan="0.4", spikeScanReps=3, spikeScanStride=4)
    assert closing[1] > 0 and sum(l[4] for l in lines) == closing[1]


@pytest.mark.parametrize("sampler,cell", (("reference", None), ("philox", None), ("philox", "spikeScanDepth"), ("philox", "spikeScanRpb")))
def test_listed_equals_whole_over_the_barcode_cap(tmp_path, capsys, sampler, cell):
    """A barcode cap of 8, far below every locus's barcodes: the listed loci go through the down-sampling of the shared tail - the
    reference's on the host from u_gid / u_finc, or smc_philox_marks over the dense descriptors, in one call for copies that keep the
    run's barcode ids and in one per copy for the renumbered ones of --spikeScanRpb."""
    bam, fa, loci, P, kw = _inputs("synth", tmp_path)
    if cell is not None:
        kw[cell] = "0.5" if cell == "spikeScanDepth" else "2"
    lines, closing = _both(tmp_path, capsys, bam, fa, loci, dataclasses.replace(P, maxMT=8), sampler=sampler, **kw)
    assert all(l[4] == 0 for l in lines), "a pass fell back to whole builds: %r" % lines
    assert closing[0] > 0 and closing[1] == 0 and closing[2] > 0
