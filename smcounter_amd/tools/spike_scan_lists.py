"""The pass lists of --spikeScan: which SNV the scan plants at which locus, and in which pass.

--spikeScan plants one SNV, REF>ALT by a fixed rule, at every locus of --bedTarget whose genome letter is A, C, G or T, and measures
how often the caller finds it.  Neighbouring spike-ins would interfere through the reads they share (every spiked read's NM grows), so
the loci are planted in PASSES: pass k (0 <= k < S, S the stride) holds the loci of every chromosome with pos mod S == k - two variants
of a pass are at least S apart.  A pass is by definition the run

    --spikeAF <targets> --spikeVariants <outPrefix>.pass<k>.txt --spikeReps R --dsSeed s

and this tool writes those files: the specification in code (DESIGN.md "--spikeScan").  Anyone can reproduce a pass of the scan with the
flags that exist; the command line makes its passes with scan_passes() below.

  <outPrefix>.pass<k>.txt   `chrom pos ref alt`, tab-separated, in locus order - one file per pass that holds a locus
  <outPrefix>.passes.txt    a header, one line `k variants file` per such pass, and a last line `#skipped n`: the loci whose genome
                            letter is not A, C, G or T (nothing is planted there)
"""
from __future__ import annotations

import argparse
import os

from . import ds_allele_fraction as af

ALT_RULES = {
    "transition": {"A": "G", "G": "A", "C": "T", "T": "C"},
    "transversion": {"A": "C", "C": "A", "G": "T", "T": "G"},
    "complement": {"A": "T", "T": "A", "C": "G", "G": "C"},
}
DEFAULT_STRIDE = 256
DEFAULT_ALT = "transition"


def scan_variants(loc_list, fasta, alt: str = DEFAULT_ALT):
    """The scan's SNV at every locus of `loc_list` ([(chrom, 1-based pos)], as bedops.expand_loci gives them; a locus listed twice
    counts once) -> (variants in locus order - tools.ds_allele_fraction.Variant -, the (chrom, pos) skipped for a letter that is not A,
    C, G or T).  ValueError: an unknown rule."""
    rule = ALT_RULES.get(alt)
    if rule is None:
        raise ValueError("--spikeScanAlt: one of %s expected, got %r" % (", ".join(sorted(ALT_RULES)), alt))
    out, skipped, seen = [], [], set()
    # (one fetch per stretch of consecutive positions: a panel is a few hundred intervals, not 20,000 single letters)
    i, n = 0, len(loc_list)
    while i < n:
        chrom, p0 = loc_list[i][0], int(loc_list[i][1])
        j = i
        while j + 1 < n and loc_list[j + 1][0] == chrom and int(loc_list[j + 1][1]) == p0 + (j + 1 - i):
            j += 1
        letters = fasta.fetch(chrom, p0 - 1, p0 + (j - i)).upper()
        for x in range(j - i + 1):
            pos = p0 + x
            if (chrom, pos) in seen:
                continue
            seen.add((chrom, pos))
            ref = letters[x] if x < len(letters) else ""
            if ref not in rule:
                skipped.append((chrom, pos))
                continue
            out.append(af.Variant(chrom, pos, ref, rule[ref], rule[ref], af.SNV))
        i = j + 1
    return out, skipped


def scan_passes(variants, stride: int):
    """-> [(k, the indices into `variants` of pass k, in the order given)] for every k in 0 .. stride - 1 that holds a locus."""
    stride = int(stride)
    if stride < 1:
        raise ValueError("--spikeScanStride: an integer >= 1 expected, got %r" % stride)
    by_k = {}
    for i, v in enumerate(variants):
        by_k.setdefault(v.pos % stride, []).append(i)
    return [(k, by_k[k]) for k in sorted(by_k)]


def write_lists(out_prefix: str, variants, passes, n_skipped: int):
    """The files of the module's docstring -> the pass files' names."""
    names = []
    for k, members in passes:
        names.append("%s.pass%d.txt" % (out_prefix, k))
        with open(names[-1], "w") as fh:
            for i in members:
                v = variants[i]
                fh.write("%s\t%d\t%s\t%s\n" % (v.chrom, v.pos, v.ref, v.alt))
    with open(out_prefix + ".passes.txt", "w") as fh:
        fh.write("#k\tvariants\tfile\n")
        for (k, members), name in zip(passes, names):
            fh.write("%d\t%d\t%s\n" % (k, len(members), name))
        fh.write("#skipped\t%d\n" % n_skipped)
    return names


def main(args):
    if args.runPath:
        os.chdir(args.runPath)
    from .. import bedops, fasta as _fasta
    try:
        variants, skipped = scan_variants(bedops.expand_loci(args.bedTarget), _fasta.FastaFile(args.refGenome), args.alt)
        passes = scan_passes(variants, args.stride)
    except (ValueError, OSError) as e:
        raise SystemExit(str(e))
    names = write_lists(args.outPrefix, variants, passes, len(skipped))
    print("%d loci in %d passes of stride %d (%s), %d skipped for a letter that is not A, C, G or T" %
          (len(variants), len(passes), args.stride, args.alt, len(skipped)))
    return names


def build_parser():
    parser = argparse.ArgumentParser(description="Write the --spikeVariants lists of the passes of --spikeScan")
    parser.add_argument("--runPath", default=None, help="path to working directory")
    parser.add_argument("--bedTarget", default=None, required=True, help="BED file of the target region")
    parser.add_argument("--refGenome", default=None, required=True, help="indexed FASTA")
    parser.add_argument("--stride", type=int, default=DEFAULT_STRIDE, help="S: pass k holds the loci with pos mod S == k")
    parser.add_argument("--alt", default=DEFAULT_ALT, help="the ALT rule: transition (A>G, G>A, C>T, T>C), transversion (A>C, C>A, G>T, "
                        "T>G) or complement (A>T, T>A, C>G, G>C)")
    parser.add_argument("--outPrefix", default=None, required=True, help="prefix of the files written")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
