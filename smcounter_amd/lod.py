"""--lod: the theoretical limit of detection of every locus of a run, from its barcode depth (reference: mt_depths_lod.R:1-49; the
offline restatement is tools/mt_depths_lod.py).

The LOD depends on (needed, depth) alone - `needed` from the output's own mtDepth (barcodes_needed), depth the locus's barcode
count - so a run needs one TABLE per `needed`, over depth 0 .. the largest depth met: the GPU makes it (smc_lod_table, one lane per
depth, R's root search in FP64), the host rounds it to 4 decimals with the tool's own `round(root, 4)` and looks every locus up.
The files are the tool's: `<prefix>.lod.bedgraph` and `<prefix>.lod.bedgraph.quantiles.txt`, written by the tool's writers."""
from __future__ import annotations

import os

import numpy as np

from . import abi
from .tools import mt_depths_lod as _tool
from .tools.mt_depths_lod import barcodes_needed            # noqa: F401  (needed = ceiling((14 + 0.012 mtDepth) / 3.5))

DEPTH_COLS = {"UMT": "used_mt", "MT": "all_mt"}            # --lodDepth -> the row field (the columns of .smCounter.all.txt)
SUMMARY_HEADER = ("output", "mtDepth", "rpb", "needed", "loci", "lociLodBelow1", "meanDepth") + tuple(
    "q%d" % round(p * 100) for p in _tool.PROBS)


class LodTables(object):
    """One table per `needed`, grown to the largest depth asked for (several outputs of a run share a `needed`).  `engine`: anything
    with lod_table(needed, max_depth) -> (roots float64[max_depth + 1], iters int32[max_depth + 1]) - engine.Engine."""

    def __init__(self, engine):
        self.engine = engine
        self._lods, self._iters = {}, {}

    def ensure(self, needed: int, max_depth: int) -> None:
        """The table of `needed` covers depth 0 .. max_depth afterwards (made anew, larger, when it did not; never smaller)."""
        needed, max_depth = int(needed), max(0, int(max_depth))
        have = self._lods.get(needed)
        if have is not None and len(have) > max_depth:
            return
        roots, iters = self.engine.lod_table(needed, max_depth)
        # the tool's rounding, value by value (np.round scales and divides: not the same function on ties of the decimal text)
        self._lods[needed] = np.array([round(float(r), 4) for r in roots], np.float64)
        self._iters[needed] = np.asarray(iters, np.int32)

    def lods(self, needed: int, depths) -> np.ndarray:
        """LOD of every depth (int array, all >= 0), rounded to 4 decimals as the tool prints it."""
        depths = np.asarray(depths, np.int64)
        self.ensure(needed, int(depths.max()) if len(depths) else 0)
        return self._lods[int(needed)][depths]

    def size(self, needed: int) -> int:
        return len(self._lods[int(needed)])

    def max_iters(self, needed: int) -> int:
        return int(self._iters[int(needed)].max())


class DepthCols(object):
    """What --lod keeps of an output's rows, batch by batch: all_mt, used_mt and status as int32 arrays (12 bytes per locus, not the
    432-byte rows)."""
    FIELDS = ("all_mt", "used_mt", "status")

    def __init__(self):
        self._parts = {f: [] for f in self.FIELDS}

    def add(self, rows) -> None:
        for f in self.FIELDS:
            self._parts[f].append(np.array(rows[f], np.int32))          # (a copy: the rows live in the engine's staging memory)

    def done(self):
        return {f: np.concatenate(p) if p else np.zeros(0, np.int32) for f, p in self._parts.items()}


def callable_loci(rows) -> np.ndarray:
    """The rows that carry numbers (rows.format_rows' rule): no Zero_Coverage, no SMC_ST_BAD_INPUT."""
    status = np.asarray(rows["status"])
    return ((status & 0xff) == 0) & ((status & abi.ST_BAD_INPUT) == 0)


def _depths(rows, depth_col: str):
    if depth_col not in DEPTH_COLS:
        raise ValueError("--lodDepth: UMT or MT expected, got %r" % (depth_col,))
    ok = callable_loci(rows)
    return ok, np.where(ok, np.maximum(np.asarray(rows[DEPTH_COLS[depth_col]], np.int64), 0), 0)


def locus_lods(rows, depth_col: str, needed: int, tables: LodTables) -> np.ndarray:
    """The LOD of every row: the table of `needed` at the row's `depth_col` ("UMT": used_mt, the barcodes that vote; "MT": all_mt).  A
    row that is not callable has no depth (the .all.txt column is empty): NA -> 1.0, as mt_depths_lod.R:27-28 treats a non-number."""
    ok, depths = _depths(rows, depth_col)
    out = tables.lods(needed, depths)
    out[~ok] = 1.0
    return out


def write_lod(prefix: str, chrom, pos, lods) -> None:
    """<prefix>.lod.bedgraph (chrom, pos - 1, pos, LOD: 0-based half-open, one line per locus in the order given) and
    <prefix>.lod.bedgraph.quantiles.txt, through the tool's writers."""
    lods = [float(v) for v in lods]
    path = prefix + ".lod.bedgraph"
    _tool.write_bedgraph(path, ((c, str(int(p) - 1), str(int(p)), v) for c, p, v in zip(chrom, pos, lods)))
    _tool.write_quantiles(path + ".quantiles.txt", lods)


def summary_entry(prefix: str, mt_depth: int, rpb: float, needed: int, rows, depth_col: str, lods):
    """The line of one output in <outPrefix>.lod.summary.txt (write_summary)."""
    ok, depths = _depths(rows, depth_col)
    lods = np.asarray(lods, np.float64)
    mean = float(depths[ok].mean()) if ok.any() else float("nan")
    return (os.path.basename(prefix), int(mt_depth), float(rpb), int(needed), len(lods), int((lods < 1.0).sum()), mean) + tuple(
        float(q) for q in _tool.quantiles(lods))


def write_summary(out_prefix: str, entries) -> None:
    """<outPrefix>.lod.summary.txt: a header and one TAB-separated line per output of the run, in the order given (the order the
    files were written in) - output prefix (basename), mtDepth, rpb, needed, loci, loci with LOD < 1, mean depth of the callable loci
    (the column --lodDepth chose; NA without any), and the seven quantiles of the quantiles file."""
    num = lambda x: "NA" if x != x else _tool._fmt(x)
    with open(out_prefix + ".lod.summary.txt", "w") as fh:
        fh.write("\t".join(SUMMARY_HEADER) + "\n")
        for e in entries:
            fh.write("\t".join([e[0], "%d" % e[1], "%g" % e[2], "%d" % e[3], "%d" % e[4], "%d" % e[5]] + [num(x) for x in e[6:]]) + "\n")


def run_lods(engine, param_list, cols, depth_col: str):
    """The LODs of every output of a run while its engine is alive: `param_list[i]` the VcParams output i was called with (its mtDepth
    gives `needed`), `cols[i]` its DepthCols.  One table per distinct `needed`, sized once for the deepest output that uses it.
    -> per output a dict: needed, rows (the three columns), lods, table (its size), iters (the largest iteration count in it)."""
    tables = LodTables(engine)
    outs = [dict(needed=barcodes_needed(P.mtDepth), rows=c.done()) for P, c in zip(param_list, cols)]
    deepest = {}
    for o in outs:
        d = _depths(o["rows"], depth_col)[1]
        deepest[o["needed"]] = max(deepest.get(o["needed"], 0), int(d.max()) if len(d) else 0)
    for needed, d in deepest.items():
        tables.ensure(needed, d)
    for o in outs:
        o["lods"] = locus_lods(o["rows"], depth_col, o["needed"], tables)
        o["table"], o["iters"] = tables.size(o["needed"]), tables.max_iters(o["needed"])
    return outs
