"""--lod without a GPU: the kernel's formulation against the tool (scipy's CDF), the files against the tool's, the host bookkeeping,
the flags and their refusals, the ABI entry."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, cli, lod
from smcounter_amd.tools import mt_depths_lod as tool

sys.path.insert(0, os.path.join(ROOT, "tests"))
import bam_fixture  # noqa: E402
import lod_restate  # noqa: E402


@pytest.mark.parametrize("mt_depth", lod_restate.MT_DEPTHS)
def test_direct_sum_restatement_equals_the_tool_at_every_depth_checked(mt_depth):
    """Every depth 0 .. 2 x mtDepth for mtDepth 450 and 1000, every sixteenth for 3612 and 8000: no difference, no exclusion."""
    needed = tool.barcodes_needed(mt_depth)
    bad = [(d, lod_restate.find_lod(d, needed), tool.find_lod(d, needed)) for d in lod_restate.depths_checked(mt_depth, 16)]
    bad = [b for b in bad if b[1] != b[2]]
    assert not bad, bad[:10]


def test_needed_is_the_tools():
    assert lod.barcodes_needed is tool.barcodes_needed
    assert [lod.barcodes_needed(d) for d in (0, 450, 1000, 3612, 8000)] == [4, 6, 8, 17, 32]


class _ToolEngine(object):
    """Stands in for engine.Engine: tables from the tool's find_lod (already rounded: rounding again changes nothing)."""

    def __init__(self):
        self.calls = []

    def lod_table(self, needed, max_depth):
        self.calls.append((needed, max_depth))
        return (np.array([tool.find_lod(d, needed) for d in range(max_depth + 1)], np.float64),
                np.full(max_depth + 1, 7, np.int32))


def _rows(used, all_mt, status):
    r = np.zeros(len(used), abi.ROW_DTYPE)
    r["used_mt"], r["all_mt"], r["status"] = used, all_mt, status
    return r


def test_write_lod_equals_the_tool_on_the_same_loci(tmp_path):
    """Hand-made loci: depth < 5, depth NA (a Zero_Coverage row, a bad-input row), needed > depth, ordinary depths."""
    mt_depth = 1000
    needed = tool.barcodes_needed(mt_depth)                       # 8
    used = [0, 3, 4, 5, 7, 8, 9, 50, 999, 1000, 2000, 12, 640]
    status = [0] * len(used)
    status[0], status[11] = abi.ST_ZERO_COVERAGE, abi.ST_BAD_INPUT
    status[7] = abi.ST_DOWNSAMPLED                                # (a flag that leaves the row callable)
    rows = _rows(used, [u + 5 for u in used], status)
    chrom = ["chr1"] * 6 + ["chrX"] * 7
    pos = [100 + 3 * i for i in range(len(used))]
    for col, field in (("UMT", "used_mt"), ("MT", "all_mt")):
        lods = lod.locus_lods(rows, col, needed, lod.LodTables(_ToolEngine()))
        assert lods[0] == 1.0 and lods[11] == 1.0 and (col == "MT" or (lods[1] == lods[2] == lods[4] == 1.0))
        prefix = str(tmp_path / ("o" + col))
        lod.write_lod(prefix, chrom, pos, lods)
        fin = tmp_path / (col + ".in")
        callable_ = [s & 0xff == 0 and not s & abi.ST_BAD_INPUT for s in status]
        fin.write_text("".join("%s|%d|%d|%s\n" % (c, p - 1, p, int(v) if ok else "NA")
                               for c, p, v, ok in zip(chrom, pos, rows[field], callable_)))
        want = str(tmp_path / ("tool" + col + ".bedgraph"))
        tool.main([str(mt_depth), str(fin), want])
        assert open(prefix + ".lod.bedgraph", "rb").read() == open(want, "rb").read()
        assert open(prefix + ".lod.bedgraph.quantiles.txt", "rb").read() == open(want + ".quantiles.txt", "rb").read()
    assert open(prefix + ".lod.bedgraph").readline() == "chr1\t99\t100\t1\n"


def test_locus_lods_reads_non_callable_rows_as_na():
    rows = _rows([600, 600, 600, 600], [700] * 4, [0, abi.ST_ZERO_COVERAGE, abi.ST_BAD_INPUT, abi.ST_UNDERFLOW | abi.ST_DOWNSAMPLED])
    got = lod.locus_lods(rows, "UMT", 8, lod.LodTables(_ToolEngine()))
    want = tool.find_lod(600, 8)
    assert 0 < want < 1 and got.tolist() == [want, 1.0, 1.0, want]
    with pytest.raises(ValueError):
        lod.locus_lods(rows, "PI", 8, lod.LodTables(_ToolEngine()))


def test_tables_ask_the_engine_once_per_needed_and_only_grow():
    eng = _ToolEngine()
    t = lod.LodTables(eng)
    a = t.lods(8, [10, 40, 25])
    assert eng.calls == [(8, 40)] and a.tolist() == [tool.find_lod(d, 8) for d in (10, 40, 25)]
    t.lods(8, [40, 0, 39]); t.ensure(8, 12); t.lods(8, [])
    assert eng.calls == [(8, 40)] and t.size(8) == 41
    t.lods(6, [30])
    assert eng.calls == [(8, 40), (6, 30)]
    t.lods(8, [41])
    assert eng.calls == [(8, 40), (6, 30), (8, 41)] and t.size(8) == 42 and t.size(6) == 31
    t.ensure(8, 5)
    assert t.size(8) == 42 and t.max_iters(8) == 7 and len(eng.calls) == 3


def test_run_lods_makes_one_table_per_needed_for_the_deepest_output():
    from smcounter_amd.params import VcParams
    eng = _ToolEngine()
    cols = [lod.DepthCols() for _ in range(3)]
    cols[0].add(_rows([30, 900], [40, 950], [0, 0])); cols[0].add(_rows([20], [25], [0]))
    cols[1].add(_rows([10, 400], [40, 950], [0, 0])); cols[1].add(_rows([7], [25], [abi.ST_ZERO_COVERAGE]))
    cols[2].add(_rows([30, 1200], [40, 1300], [0, 0])); cols[2].add(_rows([20], [25], [0]))
    outs = lod.run_lods(eng, [VcParams(mtDepth=1000, rpb=3.0), VcParams(mtDepth=450, rpb=3.0), VcParams(mtDepth=1000, rpb=2.0)], cols, "UMT")
    assert sorted(eng.calls) == [(6, 400), (8, 1200)]
    assert [o["needed"] for o in outs] == [8, 6, 8] and [o["table"] for o in outs] == [1201, 401, 1201]
    assert outs[1]["lods"].tolist() == [tool.find_lod(10, 6), tool.find_lod(400, 6), 1.0]
    assert outs[2]["rows"]["used_mt"].dtype == np.int32 and outs[2]["rows"]["used_mt"].tolist() == [30, 1200, 20]


def test_summary_layout(tmp_path):
    rows = _rows([600, 3, 900, 50], [700, 9, 950, 60], [0, 0, 0, abi.ST_ZERO_COVERAGE])
    lods = lod.locus_lods(rows, "UMT", 8, lod.LodTables(_ToolEngine()))
    e0 = lod.summary_entry(str(tmp_path / "run"), 1000, 8.6, 8, rows, "UMT", lods)
    e1 = lod.summary_entry(str(tmp_path / "run.dsMT0.5"), 500, 8.6, 6, _rows([1], [1], [abi.ST_ZERO_COVERAGE]), "UMT", np.array([1.0]))
    lod.write_summary(str(tmp_path / "run"), [e0, e1])
    lines = open(str(tmp_path / "run.lod.summary.txt")).read().split("\n")
    assert lines[0].split("\t") == ["output", "mtDepth", "rpb", "needed", "loci", "lociLodBelow1", "meanDepth", "q1", "q5", "q10", "q50",
                                    "q90", "q95", "q99"]
    q = [tool._fmt(v) for v in np.quantile(lods, tool.PROBS)]
    assert lines[1].split("\t") == ["run", "1000", "8.6", "8", "4", "2", "501"] + q
    assert lines[2].split("\t") == ["run.dsMT0.5", "500", "8.6", "6", "1", "0", "NA"] + ["1"] * 7
    assert lines[3:] == [""]


def _cli_args(tmp, **kw):
    case = bam_fixture.make_case(str(tmp))
    d = dict(outPrefix=str(tmp / "o"), bamFile=case["bam"], bedTarget=case["bed"], mtDepth=12, rpb=3.0, hpLen=8, refGenome=case["fasta"])
    d.update(kw)
    return d


def _ns(d, flags=()):
    return cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in d.items()] + list(flags))


def _no_outputs(tmp):
    return not [f for f in os.listdir(str(tmp)) if ".smCounter." in f or ".lod." in f]


def test_flags_parse(tmp_path):
    ns = _ns(_cli_args(tmp_path))
    assert ns.lod is False and ns.lodDepth is None
    ns = _ns(_cli_args(tmp_path), ["--lod"])
    assert ns.lod is True and ns.lodDepth is None
    ns = _ns(_cli_args(tmp_path, lodDepth="MT"), ["--lod"])
    assert ns.lod is True and ns.lodDepth == "MT"
    with pytest.raises(SystemExit):
        _ns(_cli_args(tmp_path, lodDepth="PI"), ["--lod"])


def test_lod_depth_without_lod_is_refused_before_any_file(tmp_path):
    with pytest.raises(SystemExit, match="--lodDepth chooses the barcode depth --lod reads: it needs --lod"):
        cli.main(_ns(_cli_args(tmp_path, lodDepth="UMT")))
    assert _no_outputs(tmp_path)


def test_lod_under_two_processes_is_refused_before_any_file(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--lod runs in one process only"):
        cli.main(_ns(_cli_args(tmp_path), ["--lod"]))
    assert _no_outputs(tmp_path)


def test_param_file_without_the_keys_leaves_lod_off(tmp_path):
    d = _cli_args(tmp_path)
    pf = tmp_path / "params.txt"
    pf.write_text("\n".join("--%s=%s" % kv for kv in d.items()) + "\n")
    ns = cli.build_parser().parse_args(("@" + str(pf),))          # (what main() does with --paramFile)
    assert ns.lod is False and ns.lodDepth is None
    pf.write_text("\n".join(["--%s=%s" % kv for kv in d.items()] + ["--lod", "--lodDepth=MT"]) + "\n")
    ns = cli.build_parser().parse_args(("@" + str(pf),))
    assert ns.lod is True and ns.lodDepth == "MT"


def test_abi_entry_is_declared_and_bound():
    L = _lib.load(with_torch=False)
    assert L.smc_abi_version() == 11
    assert "smc_lod_table" in _lib.SYMBOLS and hasattr(L, "smc_lod_table")
    hdr = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"\bint\s+smc_lod_table\s*\(\s*smc_ctx\s*\*", hdr) and "#define SMC_ABI_VERSION 11" in hdr
