"""--dsAF on the host side of a run: the command line's checks of the listed variants, and <outPrefix>.dsAF.detection.txt, the
titration on one page (which listed variant the caller still finds at which achieved allele fraction).

The semantics are tools/ds_allele_fraction.py's (DESIGN.md "--dsAF"); the pre-pass that finds the carriers on the GPU is
devplanes.ds_af_rules.
"""
from __future__ import annotations

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
