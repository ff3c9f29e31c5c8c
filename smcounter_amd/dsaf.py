"""--dsAF on the host side of a run: the command line's checks of the listed variants, and <outPrefix>.dsAF.detection.txt, the
titration on one page (which listed variant the caller still finds at which achieved allele fraction).

The semantics are tools/ds_allele_fraction.py's (DESIGN.md "--dsAF"); the pre-pass that finds the carriers on the GPU is
devplanes.ds_af_rules.

--dsAFReps: the carrier table the device draws the replicates' masks and counts from, and the two files that turn R x T calls into
a detection rate with an interval - <outPrefix>.dsAF.replicates.txt and .dsAF.sensitivity.txt (the replicate stage itself is
devplanes.ds_af_replicates).

--dsAFDepth: the four <outPrefix>.dsAF.depth.* files - the same three pages over the cells (target t, barcode fraction f), and the
curve: per listed variant and barcode depth the detection rate at every target, and the smallest target still found (t95).
"""
from __future__ import annotations

import math

import numpy as np

from .py2compat import py2_round, py2_str
from .rows import HEADER_ALL

DETECTION_HEADER = ("CHROM", "POS", "REF", "ALT", "TARGET", "N", "V", "AF", "K", "UMT", "VMT", "VMF", "PI", "FILTER", "CALLED")
FULL = "full"                  # the TARGET column of the full-depth output's lines
_COL = {name: i for i, name in enumerate(HEADER_ALL)}


def frac_text(x: float) -> str:
    """An allele fraction or a keep probability as the other columns print their fractions: rounded as Python 2 rounds (6 decimals
    here: a target of 0.0025 and its keep probability need them), printed as Python 2's str()."""
    return py2_str(py2_round(float(x), 6))


def target_text(t) -> str:
    return FULL if t is None else "%g" % t


def read_output(prefix: str):
    """-> (all: (chrom, pos) -> the row's fields of <prefix>.smCounter.all.txt, cut: (chrom, pos) -> (REF, ALT list) of .cut.txt)."""
    rows, cut = {}, {}
    with open(prefix + ".smCounter.all.txt") as fh:
        next(fh, None)
        for line in fh:
            f = line.rstrip("\n").split("\t")
            rows[(f[0], f[1])] = f
    with open(prefix + ".smCounter.cut.txt") as fh:
        next(fh, None)
        for line in fh:
            f = line.rstrip("\n").split("\t")
            cut[(f[0], f[1])] = (f[2], f[3].split(","))
    return rows, cut


def detection_line(v, target, n2: int, v2: int, k: float, row, cut, lod=None) -> str:
    """One line: the variant `v` (chrom, pos, ref, alt) in one output.  `target` None: the full-depth output; `row`: the fields of the
    output's .all.txt row at the locus (None: no row); `cut`: (REF, ALT list) of its .cut.txt line there, or None; `lod`: the locus's
    LOD with --lod."""
    get = lambda name: (row[_COL[name]] if row is not None and len(row) > _COL[name] else "")
    called = 1 if cut is not None and cut[0] == v.ref and v.alt in cut[1] else 0
    f = [v.chrom, "%d" % v.pos, v.ref, v.alt, target_text(target), "%d" % n2, "%d" % v2, frac_text(float(v2) / n2 if n2 else 0.0), frac_text(k),
         get("UMT"), get("VMT"), get("VMF"), get("PI"), get("FILTER"), "%d" % called]
    if lod is not None:
        f.append("%.15g" % lod)
    return "\t".join(f)


def write_detection(out_prefix: str, variants, outputs, loc_index=None) -> None:
    """<outPrefix>.dsAF.detection.txt: a header, then for every variant a line per output - full depth first, then the targets in the
    order given.  `outputs`: per output (target or None, prefix, titrate()'s rows of that target or None, that output's LODs by locus
    index or None); `loc_index`: (chrom, pos text) -> locus index, for the LODs."""
    read = [read_output(prefix) for _, prefix, _, _ in outputs]
    with_lod = any(l is not None for _, _, _, l in outputs)
    with open(out_prefix + ".dsAF.detection.txt", "w") as fh:
        fh.write("\t".join(DETECTION_HEADER + (("LOD",) if with_lod else ())) + "\n")
        for i, v in enumerate(variants):
            key = (v.chrom, "%d" % v.pos)
            for (target, _, res_rows, lods), (rows, cut) in zip(outputs, read):
                r = (res_rows or outputs[1][2])[i]
                n2, v2, k = (r["N"], r["V"], 1.0) if target is None else (r["N2"], r["V2"], r["k"])
                lod = float(lods[loc_index[key]]) if lods is not None else None
                fh.write(detection_line(v, target, n2, v2, k, rows.get(key), cut.get(key), lod) + "\n")


def check_variants(variants, loc_list) -> None:
    """Every listed variant must be a locus of --bedTarget; ValueError names the first that is not."""
    loci = set((c, int(p)) for c, p in loc_list)
    for v in variants:
        if (v.chrom, v.pos) not in loci:
            raise ValueError("--dsAFVariants: %s:%d %s>%s is not a locus of --bedTarget" % (v.chrom, v.pos, v.ref, v.alt))


# ---- --dsAFReps
REPS_MIN, REPS_MAX = 2, 1000
REPLICATES_HEADER = DETECTION_HEADER[:5] + ("REP", "SEED") + DETECTION_HEADER[5:]
SENSITIVITY_HEADER = ("CHROM", "POS", "REF", "ALT", "TARGET", "REPS", "CALLED", "RATE", "LO95", "HI95", "AF_MEAN", "AF_MIN", "AF_MAX",
                      "V_MIN", "V_MAX", "PI_MEAN", "PI_MIN")
WILSON_Z = 1.959963984540054


def rep_seeds(seed: int, n_reps: int):
    """The seed of every replicate: s_j = (seed + j) mod 2^64 (replicate 0 is the run's own --dsAF draw)."""
    return [(int(seed) + j) & 0xFFFFFFFFFFFFFFFF for j in range(int(n_reps))]


def carrier_table(carries, thr):
    """The table the replicates are drawn from -> (idents: the sorted unique uint64 identities of the barcodes that carry at least
    one listed variant, uint64 [C, T]: per carrier and target the smallest threshold among the variants it carries).  carries[v]: the
    identities that carry variant v; thr[t][v]: titrate()'s threshold of v at target t (up to 2^32).  A barcode is dropped at t when
    any variant it carries draws it out (tools/ds_allele_fraction.py step 3): u(b) >= the smallest of them."""
    carries = [np.unique(np.asarray(c, np.uint64)) for c in carries]
    idents = np.unique(np.concatenate(carries)) if carries else np.zeros(0, np.uint64)
    table = np.full((len(idents), len(thr)), 1 << 32, np.uint64)
    for t, row in enumerate(thr):
        for c, h in zip(carries, row):
            at = np.searchsorted(idents, c)
            table[at, t] = np.minimum(table[at, t], np.uint64(h))
    return idents, table


def wilson(called: int, reps: int, z: float = WILSON_Z):
    """The Wilson score interval of called / reps -> (lo, hi), clamped to [0, 1]."""
    n, p = float(reps), float(called) / float(reps)
    den = 1.0 + z * z / n
    mid = (p + z * z / (2.0 * n)) / den
    half = z * math.sqrt(p * (1.0 - p) / n + z * z / (4.0 * n * n)) / den
    return max(0.0, mid - half), min(1.0, mid + half)


def replicate_entry(row_text, threshold: int, trf, rm):
    """One replicate's raw row at a listed locus (None: no row) as the run's files would hold it -> (the fields of its .all.txt line,
    (REF, ALT list) of its .cut.txt line or None): the row through postfilter.apply_repeat_filters, then the writers' cut rule."""
    from . import postfilter, writers
    if row_text is None:
        return None, None
    row = list(postfilter.apply_repeat_filters([row_text], trf, rm))[0]
    hit = writers.cut_row(row, threshold)
    return row.split("\t"), (None if hit is None else (hit[1]["REF"], hit[1]["ALT"].split(",")))


def replicate_line(v, target, rep: int, seed: int, n2: int, v2: int, k: float, row, cut) -> str:
    """detection_line() of one replicate with REP and SEED behind TARGET (no LOD column)."""
    f = detection_line(v, target, n2, v2, k, row, cut).split("\t")
    return "\t".join(f[:5] + ["%d" % rep, "%d" % seed] + f[5:])


def _pi(row) -> float:
    text = row[_COL["PI"]] if row is not None and len(row) > _COL["PI"] else ""
    try:
        return float(text)
    except ValueError:
        return 0.0


def sensitivity_line(v, target, reps, lod=None) -> str:
    """One line of the sensitivity table: variant `v` at `target` over its replicates.  `reps`: per replicate (N', V', row fields or
    None, cut or None) - what replicate_line() takes; `lod`: the locus's LOD in the run's own output of that target, with --lod."""
    n = len(reps)
    called = sum(1 for _, _, _, cut in reps if cut is not None and cut[0] == v.ref and v.alt in cut[1])
    lo, hi = wilson(called, n)
    afs = [float(v2) / n2 if n2 else 0.0 for n2, v2, _, _ in reps]
    pis = [_pi(row) for _, _, row, _ in reps]
    f = [v.chrom, "%d" % v.pos, v.ref, v.alt, target_text(target), "%d" % n, "%d" % called, frac_text(float(called) / n), frac_text(lo),
         frac_text(hi), frac_text(sum(afs) / n), frac_text(min(afs)), frac_text(max(afs)), "%d" % min(v2 for _, v2, _, _ in reps),
         "%d" % max(v2 for _, v2, _, _ in reps), frac_text(sum(pis) / n), frac_text(min(pis))]
    if lod is not None:
        f.append("%.15g" % lod)
    return "\t".join(f)


def write_replicates(out_prefix: str, variants, targets, seeds, ks, entries) -> None:
    """<outPrefix>.dsAF.replicates.txt: a header, then a line per listed variant (file order), target (the order given) and replicate
    (ascending).  ks[t][v]: the keep probability; entries[(v, t)]: per replicate (N', V', row fields or None, cut or None)."""
    with open(out_prefix + ".dsAF.replicates.txt", "w") as fh:
        fh.write("\t".join(REPLICATES_HEADER) + "\n")
        for i, v in enumerate(variants):
            for t, target in enumerate(targets):
                for j, (n2, v2, row, cut) in enumerate(entries[(i, t)]):
                    fh.write(replicate_line(v, target, j, seeds[j], n2, v2, ks[t][i], row, cut) + "\n")


def write_sensitivity(out_prefix: str, variants, targets, entries, lods=None) -> None:
    """<outPrefix>.dsAF.sensitivity.txt: a header, then a line per listed variant and target.  lods[t][v] (with --lod): the LOD of the
    variant's locus in the run's .dsAF<t> output."""
    with open(out_prefix + ".dsAF.sensitivity.txt", "w") as fh:
        fh.write("\t".join(SENSITIVITY_HEADER + (("LOD",) if lods is not None else ())) + "\n")
        for i, v in enumerate(variants):
            for t, target in enumerate(targets):
                fh.write(sensitivity_line(v, target, entries[(i, t)], None if lods is None else float(lods[t][i])) + "\n")


# ---- --dsAFDepth
DEPTH_DETECTION_HEADER = DETECTION_HEADER[:5] + ("FRACTION", "MTDEPTH") + DETECTION_HEADER[5:]
DEPTH_REPLICATES_HEADER = DEPTH_DETECTION_HEADER[:7] + ("REP", "SEED") + DEPTH_DETECTION_HEADER[7:]
DEPTH_SENSITIVITY_HEADER = SENSITIVITY_HEADER[:5] + ("FRACTION", "MTDEPTH") + SENSITIVITY_HEADER[5:] + ("N_MEAN",)
CURVE_HEADER = ("CHROM", "POS", "REF", "ALT", "DEPTH", "MTDEPTH", "N_MEAN")
T95_RATE = 0.95
NA = "NA"


def t95(targets, rates, level: float = T95_RATE):
    """The smallest listed target whose detection rate is at least `level` TOGETHER WITH the rate of every larger listed target (a
    rate that dips below `level` above it disqualifies it: the curve is read from the top), or None.  `targets` in any order."""
    best = None
    for t, r in sorted(zip(targets, rates), key=lambda x: -x[0]):
        if not r >= level:
            break
        best = t
    return best


def _cell_fields(line: str, frac: float, mt_depth: int):
    f = line.split("\t")
    return f[:5] + ["%g" % frac, "%d" % mt_depth] + f[5:]


def depth_detection_line(v, target, frac, mt_depth, n2, v2, k, row, cut, lod=None) -> str:
    """detection_line() of variant `v` in cell (target, frac) with FRACTION and MTDEPTH behind TARGET."""
    return "\t".join(_cell_fields(detection_line(v, target, n2, v2, k, row, cut, lod), frac, mt_depth))


def depth_replicate_line(v, target, frac, mt_depth, rep: int, seed: int, n2, v2, k, row, cut) -> str:
    f = _cell_fields(detection_line(v, target, n2, v2, k, row, cut), frac, mt_depth)
    return "\t".join(f[:7] + ["%d" % rep, "%d" % seed] + f[7:])


def _n_mean(reps) -> float:
    return sum(float(n2) for n2, _, _, _ in reps) / len(reps)


def _called(v, reps) -> int:
    return sum(1 for _, _, _, cut in reps if cut is not None and cut[0] == v.ref and v.alt in cut[1])


def depth_sensitivity_line(v, target, frac, mt_depth, reps, lod=None) -> str:
    """sensitivity_line() of a cell with FRACTION and MTDEPTH behind TARGET and the mean N' behind PI_MIN (then LOD)."""
    f = _cell_fields(sensitivity_line(v, target, reps), frac, mt_depth) + [frac_text(_n_mean(reps))]
    if lod is not None:
        f.append("%.15g" % lod)
    return "\t".join(f)


def curve_line(v, depth, mt_depths, targets, per_target, lod=None) -> str:
    """One line of the curve: variant `v` at one barcode depth (`depth` None: full, else f).  `mt_depths`: the mtDepth of every target's
    output at that depth (printed once when equal, else joined by commas); `per_target[t]`: the replicates of target targets[t] there,
    as sensitivity_line() takes them.  RATE@ columns in ascending target order, then T95."""
    order = sorted(range(len(targets)), key=lambda t: targets[t])
    rates = [float(_called(v, per_target[t])) / len(per_target[t]) for t in range(len(targets))]
    best = t95(targets, rates)
    depths = ["%d" % d for d in mt_depths]
    f = [v.chrom, "%d" % v.pos, v.ref, v.alt, FULL if depth is None else "%g" % depth, depths[0] if len(set(depths)) == 1 else ",".join(depths),
         frac_text(sum(_n_mean(p) for p in per_target) / len(per_target))] + [frac_text(rates[t]) for t in order] + \
        [NA if best is None else "%g" % best]
    if lod is not None:
        f.append("%.15g" % lod)
    return "\t".join(f)


def curve_header(targets, with_lod: bool = False):
    return CURVE_HEADER + tuple("RATE@%g" % t for t in sorted(targets)) + ("T95",) + (("LOD",) if with_lod else ())


def write_depth_detection(out_prefix: str, variants, cells, counts, ks, loc_index=None) -> None:
    """<outPrefix>.dsAF.depth.detection.txt: a header, then a line per listed variant and cell (targets outer, fractions inner).
    `cells`: per cell (target index, target, fraction, mtDepth, output prefix, that output's LODs by locus index or None);
    counts[v][cell] = (N', V'); ks[t][v]: the keep probability."""
    read = [read_output(c[4]) for c in cells]
    with_lod = any(c[5] is not None for c in cells)
    with open(out_prefix + ".dsAF.depth.detection.txt", "w") as fh:
        fh.write("\t".join(DEPTH_DETECTION_HEADER + (("LOD",) if with_lod else ())) + "\n")
        for i, v in enumerate(variants):
            key = (v.chrom, "%d" % v.pos)
            for c, ((t, target, frac, depth, _, lods), (rows, cut)) in enumerate(zip(cells, read)):
                lod = float(lods[loc_index[key]]) if lods is not None else None
                fh.write(depth_detection_line(v, target, frac, depth, int(counts[i][c][0]), int(counts[i][c][1]), ks[t][i], rows.get(key),
                                              cut.get(key), lod) + "\n")


def write_depth_replicates(out_prefix: str, variants, cells, seeds, ks, entries) -> None:
    """<outPrefix>.dsAF.depth.replicates.txt: a line per listed variant, cell and replicate.  entries[(v, cell)]: per replicate (N', V',
    row fields or None, cut or None)."""
    with open(out_prefix + ".dsAF.depth.replicates.txt", "w") as fh:
        fh.write("\t".join(DEPTH_REPLICATES_HEADER) + "\n")
        for i, v in enumerate(variants):
            for c, (t, target, frac, depth, _, _) in enumerate(cells):
                for j, (n2, v2, row, cut) in enumerate(entries[(i, c)]):
                    fh.write(depth_replicate_line(v, target, frac, depth, j, seeds[j], n2, v2, ks[t][i], row, cut) + "\n")


def write_depth_sensitivity(out_prefix: str, variants, cells, entries, loc_index=None) -> None:
    """<outPrefix>.dsAF.depth.sensitivity.txt: a line per listed variant and cell; LOD: the locus's in the run's own output of the cell."""
    with_lod = any(c[5] is not None for c in cells)
    with open(out_prefix + ".dsAF.depth.sensitivity.txt", "w") as fh:
        fh.write("\t".join(DEPTH_SENSITIVITY_HEADER + (("LOD",) if with_lod else ())) + "\n")
        for i, v in enumerate(variants):
            for c, (t, target, frac, depth, _, lods) in enumerate(cells):
                lod = float(lods[loc_index[(v.chrom, "%d" % v.pos)]]) if lods is not None else None
                fh.write(depth_sensitivity_line(v, target, frac, depth, entries[(i, c)], lod) + "\n")


def write_depth_curve(out_prefix: str, variants, targets, fracs, full, cells, full_entries, entries, loc_index=None) -> None:
    """<outPrefix>.dsAF.depth.curve.txt: a line per listed variant and barcode depth - `full` (the plain targets' outputs) first, then
    every fraction.  `full`: per target (mtDepth, the LODs of that target's .dsAF<t> output or None); full_entries[(v, t)] /
    entries[(v, cell)]: the replicates.  LOD: the locus's theoretical one at that depth, in the output of the LARGEST listed target
    there (the least diluted one, at the mtDepth the line shows for it) - its .dsAF<t> output on the `full` line, its cell at f."""
    T, F = len(targets), len(fracs)
    top = max(range(T), key=lambda t: targets[t])
    with_lod = any(c[5] is not None for c in cells)
    with open(out_prefix + ".dsAF.depth.curve.txt", "w") as fh:
        fh.write("\t".join(curve_header(targets, with_lod)) + "\n")
        for i, v in enumerate(variants):
            at = loc_index[(v.chrom, "%d" % v.pos)] if with_lod else None
            fh.write(curve_line(v, None, [d for d, _ in full], targets, [full_entries[(i, t)] for t in range(T)],
                                float(full[top][1][at]) if with_lod else None) + "\n")
            for k, f in enumerate(fracs):
                mine = [cells[t * F + k] for t in range(T)]
                fh.write(curve_line(v, f, [c[3] for c in mine], targets, [entries[(i, t * F + k)] for t in range(T)],
                                    float(mine[top][5][at]) if with_lod else None) + "\n")
