"""--lod on the GPU: smc_lod_table (csrc/k_lod.inc) against the tool's find_lod (scipy's CDF) depth by depth, its edge cases and
refusals, and the command line's LOD files against tools.mt_depths_lod.main fed the depth column of each output's own .all.txt."""
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, cli, lod
from smcounter_amd.py2compat import py2_round
from smcounter_amd.tools import mt_depths_lod as tool

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import lod_restate  # noqa: E402

pytestmark = pytest.mark.gpu
MAXIT = 1000
SEED = 1234567


@pytest.mark.parametrize("mt_depth", lod_restate.MT_DEPTHS)
def test_table_rounded_equals_the_tool_at_every_depth_checked(engine0, mt_depth):
    """Every depth 0 .. 2 x mtDepth for mtDepth 450 and 1000, every third for 3612 and 8000: zero mismatches allowed.  A mismatch
    is printed with both unrounded roots and both iteration counts (the tool's side through the restatement's root)."""
    needed = tool.barcodes_needed(mt_depth)
    roots, iters = engine0.lod_table(needed, 2 * mt_depth)
    assert roots.dtype == np.float64 and iters.dtype == np.int32 and len(roots) == len(iters) == 2 * mt_depth + 1
    bad, far = [], 0.0
    for d in lod_restate.depths_checked(mt_depth, 3):
        want = tool.find_lod(d, needed)
        r_root, r_iters = lod_restate.find_root(d, needed)
        far = max(far, abs(float(roots[d]) - r_root))
        if round(float(roots[d]), 4) != want:
            bad.append(dict(depth=d, tool=want, device_root=float(roots[d]), restated_root=r_root, device_iters=int(iters[d]),
                            restated_iters=r_iters))
    print("mtDepth %d needed %d: max |device root - restated root| = %.3g, largest iteration count %d" % (mt_depth, needed, far, iters.max()))
    assert not bad, bad[:10]
    assert iters.max() < MAXIT


def test_edge_cases_and_refusals(engine0):
    roots, iters = engine0.lod_table(1, 0)
    assert roots.tolist() == [1.0] and iters.tolist() == [0]
    roots, iters = engine0.lod_table(1, 4)
    assert roots.tolist() == [1.0] * 5 and iters.tolist() == [0] * 5                 # fewer than 5 barcodes
    roots, iters = engine0.lod_table(50, 40)
    assert roots.tolist() == [1.0] * 41 and iters.tolist() == [0] * 41               # needed > depth: no sign change
    roots, iters = engine0.lod_table(1, 200)                                         # needed = 1: one barcode is enough
    assert (roots[:5] == 1.0).all() and ((roots[5:] > 0) & (roots[5:] < 1)).all() and (np.diff(roots[5:]) < 0).all()
    assert [round(float(r), 4) for r in roots] == [tool.find_lod(d, 1) for d in range(201)]
    assert 0 < iters[5:].min() and iters.max() < MAXIT
    for needed, max_depth in ((0, 10), (-3, 10), (8, -1), (8, (1 << 24) + 1), (1 << 40, 10)):
        with pytest.raises(_lib.SmcError, match="smc_lod_table"):
            engine0.lod_table(needed, max_depth)
    # (the raw entry: a refusal is an error code and a message, the buffers are not looked at)
    rc = engine0.L.smc_lod_table(engine0.ctx, 0, 10, None, None)
    assert rc < 0 and b"smc_lod_table" in engine0.L.smc_last_error()
    roots, iters = engine0.lod_table(8, 100)                                         # (and the context still works)
    assert round(float(roots[100]), 4) == tool.find_lod(100, 8)


def test_two_calls_return_identical_bytes(engine0):
    a = engine0.lod_table(17, 7224)
    engine0.lod_table(6, 900)                                                        # (another table in between, the same scratch)
    b = engine0.lod_table(17, 7224)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def _run_cli(tmp, tag, bam, fa, bed, P, flags=(), **kw):
    prefix = str(tmp / tag)
    opts = dict(outPrefix=prefix, bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, hpLen=P.hpLen, minBQ=P.minBQ,
                minMQ=P.minMQ, mismatchThr=P.mismatchThr, mtDrop=P.mtDrop, maxMT=P.maxMT, primerDist=P.primerDist, refGenome=fa, **kw)
    cli.main(cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in opts.items()] + list(flags)))
    return prefix


SUFFIXES = (".smCounter.all.txt", ".smCounter.cut.txt", ".smCounter.cut.vcf")
LOD_SUFFIXES = (".lod.bedgraph", ".lod.bedgraph.quantiles.txt")


def _read(prefix, suffixes):
    return [open(prefix + s, "rb").read() for s in suffixes]


def _tool_files(tmp, all_txt, column, mt_depth):
    """What tools.mt_depths_lod.main writes from `column` of an output's .all.txt: (bedgraph bytes, quantiles bytes)."""
    lines = open(all_txt).read().split("\n")
    head = lines[0].split("\t")
    i_chrom, i_pos, i_col = head.index("CHROM"), head.index("POS"), head.index(column)
    fin, fout = str(tmp / "tool.in"), str(tmp / "tool.bedgraph")
    with open(fin, "w") as fh:
        for line in lines[1:]:
            if line:
                f = line.split("\t")
                fh.write("%s|%d|%d|%s\n" % (f[i_chrom], int(f[i_pos]) - 1, int(f[i_pos]), f[i_col] or "NA"))
    tool.main([str(mt_depth), fin, fout])
    return _read(fout, ("", ".quantiles.txt"))


@pytest.mark.parametrize("name", ("bam_deep", "bam_cigars"))
def test_cli_lod_files_equal_the_tool_on_each_output(tmp_path, name):
    bam, fa, loci, P = ds_restate.load_fixture(name, str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    d_half = max(1, int(py2_round(0.5 * P.mtDepth)))
    # the plain run
    before = _read(_run_cli(tmp_path, "p", bam, fa, bed, P), SUFFIXES)
    assert not [f for f in os.listdir(str(tmp_path)) if ".lod." in f]
    for column, kw in (("UMT", {}), ("MT", dict(lodDepth="MT"))):
        got = _run_cli(tmp_path, "p", bam, fa, bed, P, flags=["--lod"], **kw)
        assert _read(got, SUFFIXES) == before, "%s: --lod changed the full-depth files" % name
        assert _read(got, LOD_SUFFIXES) == _tool_files(tmp_path, got + SUFFIXES[0], column, P.mtDepth), (name, column)
        assert len(open(got + ".lod.summary.txt").read().splitlines()) == 2
    n_loci = len(open(got + LOD_SUFFIXES[0]).read().splitlines())
    assert n_loci == len(loci)
    # the grid: four outputs more, each at its own mtDepth
    kw = dict(dsMT="0.5", dsRpb="2", dsSeed=SEED)
    outs = [("", P.mtDepth, P.rpb), (".dsMT0.5", d_half, P.rpb), (".dsRpb2", P.mtDepth, 2.0), (".dsMT0.5.dsRpb2", d_half, 2.0)]
    g0 = _run_cli(tmp_path, "g", bam, fa, bed, P, flags=["--dsGrid"], **kw)
    before = {s: _read(g0 + s, SUFFIXES) for s, _, _ in outs}
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("g.") and ".lod." in f]
    for column, extra in (("UMT", {}), ("MT", dict(lodDepth="MT"))):
        g = _run_cli(tmp_path, "g", bam, fa, bed, P, flags=["--dsGrid", "--lod"], **dict(kw, **extra))
        for s, d, _ in outs:
            assert _read(g + s, SUFFIXES) == before[s], "%s%s: --lod changed the files" % (name, s)
            assert _read(g + s, LOD_SUFFIXES) == _tool_files(tmp_path, g + s + SUFFIXES[0], column, d), (name, s, column)
        summary = [l.split("\t") for l in open(g + ".lod.summary.txt").read().splitlines()]
        assert summary[0] == list(lod.SUMMARY_HEADER)
        assert [l[:5] for l in summary[1:]] == [["g" + s, "%d" % d, "%g" % r, "%d" % tool.barcodes_needed(d), "%d" % len(loci)]
                                                for s, d, r in outs]
        for l, (s, _, _) in zip(summary[1:], outs):
            q = [x.split("|")[1] for x in open(g + s + LOD_SUFFIXES[1]).read().splitlines()]
            assert l[7:] == q


def test_host_planes_run_writes_the_same_lod_files(tmp_path, monkeypatch):
    bam, fa, loci, P = ds_restate.load_fixture("bam_deep", str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    dev = _run_cli(tmp_path, "dev", bam, fa, bed, P, flags=["--lod"])
    monkeypatch.setenv("SMC_PLANES", "host")
    host = _run_cli(tmp_path, "host", bam, fa, bed, P, flags=["--lod"])
    assert _read(host, LOD_SUFFIXES) == _read(dev, LOD_SUFFIXES)
    assert _read(host, SUFFIXES[:2]) == _read(dev, SUFFIXES[:2])
    monkeypatch.delenv("SMC_PLANES")
    monkeypatch.setenv("SMC_BAM_DECODER", "python")
    py = _run_cli(tmp_path, "py", bam, fa, bed, P, flags=["--lod"])
    assert _read(py, LOD_SUFFIXES) == _read(dev, LOD_SUFFIXES)
