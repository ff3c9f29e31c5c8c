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

--spikeScanIndel del<d>|dup<s> (--indel here) plants one deletion or one tandem duplication instead of the SNV at every locus P:
  del<d>   REF = genome[P .. P+d], ALT = genome[P]: the d letters behind the anchor go;
  dup<s>   REF = genome[P], ALT = genome[P] + genome[P+1 .. P+s]: the next s letters once more, a homopolymer's expansion inside a run;
d, s in 1 .. 255.  A locus is skipped when a letter of P .. P+d (P .. P+s) is not A, C, G or T or lies past the chromosome's end.  The
footprints are --spikeIndels' (spike_variants.footprint: [P, P+d+1] / [P, P+1]) and must be disjoint within a pass: S >= d + 2 for a
deletion, S >= 2 for a duplication (indel_min_stride).  A pass is then the run

    --spikeAF <targets> --spikeVariants <outPrefix>.pass<k>.txt --spikeIndelReps R --dsSeed s

and every list written parses under spike_variants.parse_variants(..., indels=True).

--spikeScanMnv L (--mnv here), L in 2 .. 8, plants one MNV of L adjacent letters at every locus P: REF = genome[P .. P+L-1], ALT = the
--alt rule applied to every letter, one phase set of L member SNVs named chrom:P with P as leader.  A locus is skipped when a position
of P .. P+L-1 is no locus of the target on that chromosome or its letter is not A, C, G or T.  Pass k holds the leaders with pos mod S
== k, the footprints of a pass must be disjoint: S >= L (mnv_min_stride).  The lists hold 4-column MNV lines `chrom pos REF ALT`, a
pass is the run

    --spikeAF <targets> --spikeVariants <outPrefix>.pass<k>.txt --spikeReps R --spikePhase --dsSeed s

and every list written parses under spike_variants.parse_variants(..., phased=True) into sets of exactly L members.
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


def parse_indel_rule(text, flag: str = "--spikeScanIndel"):
    """`del<d>` / `dup<s>` -> ("del" or "dup", the length).  ValueError: anything else, or a length outside 1 .. 255."""
    t = str(text).strip()
    if t[:3] in ("del", "dup") and t[3:].isdigit() and len(t) <= 9 and 1 <= int(t[3:]) <= af.MAX_INS:
        return t[:3], int(t[3:])
    raise ValueError("%s: del<d> or dup<s> with a length in 1 .. %d expected, got %r" % (flag, af.MAX_INS, text))


def indel_min_stride(rule) -> int:
    """The smallest stride at which the footprints of a pass are disjoint: d + 2 for del<d>, 2 for dup<s>."""
    kind, n = rule
    return n + 2 if kind == "del" else 2


def check_indel_stride(rule, stride: int, flag: str = "--spikeScanStride") -> None:
    """ValueError: a stride below indel_min_stride - two footprints of a pass would overlap."""
    if int(stride) < indel_min_stride(rule):
        raise ValueError("%s: a stride of %d with %s%d: the footprints of a pass would overlap, the smallest stride allowed is %d" %
                         (flag, int(stride), rule[0], rule[1], indel_min_stride(rule)))


def scan_indels(loc_list, fasta, rule):
    """scan_variants for --spikeScanIndel: the deletion or duplication of `rule` (parse_indel_rule's pair) anchored at every locus ->
    (variants in locus order, the (chrom, pos) skipped: a letter of the anchor and the n positions behind it that is not A, C, G or T,
    or the chromosome ends before them)."""
    kind, n = rule
    out, skipped, seen = [], [], set()
    i, m = 0, len(loc_list)
    while i < m:
        chrom, p0 = loc_list[i][0], int(loc_list[i][1])
        j = i
        while j + 1 < m and loc_list[j + 1][0] == chrom and int(loc_list[j + 1][1]) == p0 + (j + 1 - i):
            j += 1
        letters = fasta.fetch(chrom, p0 - 1, p0 + (j - i) + n).upper()     # (clipped at the chromosome's end: then the tail is short)
        for x in range(j - i + 1):
            pos = p0 + x
            if (chrom, pos) in seen:
                continue
            seen.add((chrom, pos))
            w = letters[x:x + n + 1]
            if len(w) != n + 1 or any(c not in "ACGT" for c in w):
                skipped.append((chrom, pos))
                continue
            ref, alt = (w, w[0]) if kind == "del" else (w[0], w)
            key, k = af.allele_key(ref, alt)
            out.append(af.Variant(chrom, pos, ref, alt, key, k))
        i = j + 1
    return out, skipped


MNV_MIN, MNV_MAX = 2, 8       # letters of --spikeScanMnv's MNV (spike_variants.PHASE_MAX_MEMBERS)


def parse_mnv(text, flag: str = "--spikeScanMnv") -> int:
    """L, the letters of the scan's MNV.  ValueError: no integer in MNV_MIN .. MNV_MAX."""
    try:
        n = text if isinstance(text, int) and not isinstance(text, bool) else int(str(text).strip())
    except ValueError:
        n = None
    if n is None or not MNV_MIN <= n <= MNV_MAX:
        raise ValueError("%s: an integer in %d .. %d expected (the letters of the MNV), got %r" % (flag, MNV_MIN, MNV_MAX, text))
    return n


def mnv_min_stride(L: int) -> int:
    """The smallest stride at which the footprints P .. P+L-1 of a pass are disjoint: L."""
    return int(L)


def check_mnv_stride(L: int, stride: int, flag: str = "--spikeScanStride") -> None:
    """ValueError: a stride below mnv_min_stride - two MNVs of a pass would share a position."""
    if int(stride) < mnv_min_stride(L):
        raise ValueError("%s: a stride of %d with an MNV of %d letters: the footprints of a pass would overlap, the smallest stride "
                         "allowed is %d" % (flag, int(stride), int(L), mnv_min_stride(L)))


def scan_mnvs(loc_list, fasta, L: int, alt: str = DEFAULT_ALT):
    """scan_variants for --spikeScanMnv: one MNV of L adjacent letters at every locus P - REF = genome[P .. P+L-1], ALT the rule of
    `alt` applied to every letter - as ONE phase set of L member SNVs named chrom:P, P the leader.
    -> (spike_variants.PhasedVariants: the member SNVs set by set, in the locus order of the leaders - set i holds the members
    i*L .. i*L+L-1, so a position stands once per set that covers it -, the leaders (chrom, P) in that order, the (chrom, pos) skipped:
    a position of P .. P+L-1 that is no locus of `loc_list` on that chromosome, or whose letter is not A, C, G or T).  A locus listed
    twice counts once; `loc_list` may be out of position order.  ValueError: an unknown rule, L outside MNV_MIN .. MNV_MAX."""
    from . import spike_variants as sv
    rule = ALT_RULES.get(alt)
    if rule is None:
        raise ValueError("--spikeScanAlt: one of %s expected, got %r" % (", ".join(sorted(ALT_RULES)), alt))
    L = parse_mnv(L)
    singles, _ = scan_variants(loc_list, fasta, alt)           # (every locus with a letter of the rule, each once, in locus order)
    letter = {(v.chrom, v.pos): v for v in singles}
    members, sets, leaders, skipped, seen = [], [], [], [], set()
    for chrom, pos in loc_list:
        pos = int(pos)
        if (chrom, pos) in seen:
            continue
        seen.add((chrom, pos))
        vs = [letter.get((chrom, pos + x)) for x in range(L)]
        if any(v is None for v in vs):
            skipped.append((chrom, pos))
            continue
        sets.append(sv.PhaseSet("%s:%d" % (chrom, pos), chrom, tuple(range(len(members), len(members) + L))))
        leaders.append((chrom, pos))
        members += vs
    return sv.PhasedVariants(members, sets), leaders, skipped


def mnv_passes(mnvs, stride: int):
    """scan_passes for scan_mnvs' variants -> [(k, the indices of the SETS of pass k, in the order given)]: pass k holds the leaders
    with pos mod stride == k."""
    return scan_passes([mnvs[s.members[0]] for s in mnvs.sets], stride)


def mnv_pass_variants(mnvs, set_indices):
    """The sets `set_indices` of scan_mnvs' variants as a list of their own - what parse_variants(phased=True) reads from the pass's
    file: a PhasedVariants of their members, set by set."""
    from . import spike_variants as sv
    members, sets = [], []
    for i in set_indices:
        s = mnvs.sets[i]
        sets.append(sv.PhaseSet(s.name, s.chrom, tuple(range(len(members), len(members) + len(s.members)))))
        members += [mnvs[k] for k in s.members]
    return sv.PhasedVariants(members, sets)


def write_mnv_lists(out_prefix: str, mnvs, passes, n_skipped: int):
    """write_lists for MNVs: a pass file holds one 4-column MNV line `chrom pos REF ALT` per set, REF and ALT the members' letters."""
    names = []
    for k, members in passes:
        names.append("%s.pass%d.txt" % (out_prefix, k))
        with open(names[-1], "w") as fh:
            for i in members:
                vs = [mnvs[m] for m in mnvs.sets[i].members]
                fh.write("%s\t%d\t%s\t%s\n" % (vs[0].chrom, vs[0].pos, "".join(v.ref for v in vs), "".join(v.alt for v in vs)))
    with open(out_prefix + ".passes.txt", "w") as fh:
        fh.write("#k\tvariants\tfile\n")
        for (k, members), name in zip(passes, names):
            fh.write("%d\t%d\t%s\n" % (k, len(members), name))
        fh.write("#skipped\t%d\n" % n_skipped)
    return names


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
    indel = getattr(args, "indel", None)
    mnv = getattr(args, "mnv", None)
    if mnv not in (None, ""):
        if indel not in (None, ""):
            raise SystemExit("--mnv cannot be combined with --indel: the scan plants an MNV OR an indel at every locus")
        try:
            L = parse_mnv(mnv, "--mnv")
            check_mnv_stride(L, args.stride, "--stride")
            loc_list, fa = bedops.expand_loci(args.bedTarget), _fasta.FastaFile(args.refGenome)
            mnvs, _, skipped = scan_mnvs(loc_list, fa, L, args.alt)
            passes = mnv_passes(mnvs, args.stride)
        except (ValueError, OSError) as e:
            raise SystemExit(str(e))
        names = write_mnv_lists(args.outPrefix, mnvs, passes, len(skipped))
        print("%d MNVs of %d letters in %d passes of stride %d (%s), %d loci skipped for a position of the footprint that is no locus of "
              "the target or whose letter is not A, C, G or T" % (len(mnvs.sets), L, len(passes), args.stride, args.alt, len(skipped)))
        return names
    try:
        loc_list, fa = bedops.expand_loci(args.bedTarget), _fasta.FastaFile(args.refGenome)
        if indel in (None, ""):
            variants, skipped = scan_variants(loc_list, fa, args.alt)
        else:
            rule = parse_indel_rule(indel, "--indel")
            check_indel_stride(rule, args.stride, "--stride")
            variants, skipped = scan_indels(loc_list, fa, rule)
        passes = scan_passes(variants, args.stride)
    except (ValueError, OSError) as e:
        raise SystemExit(str(e))
    names = write_lists(args.outPrefix, variants, passes, len(skipped))
    if indel in (None, ""):
        print("%d loci in %d passes of stride %d (%s), %d skipped for a letter that is not A, C, G or T" %
              (len(variants), len(passes), args.stride, args.alt, len(skipped)))
    else:
        print("%d loci in %d passes of stride %d (%s), %d skipped for a letter inside the footprint that is not A, C, G or T or lies past "
              "the chromosome's end" % (len(variants), len(passes), args.stride, indel, len(skipped)))
    return names


def build_parser():
    parser = argparse.ArgumentParser(description="Write the --spikeVariants lists of the passes of --spikeScan")
    parser.add_argument("--runPath", default=None, help="path to working directory")
    parser.add_argument("--bedTarget", default=None, required=True, help="BED file of the target region")
    parser.add_argument("--refGenome", default=None, required=True, help="indexed FASTA")
    parser.add_argument("--stride", type=int, default=DEFAULT_STRIDE, help="S: pass k holds the loci with pos mod S == k")
    parser.add_argument("--alt", default=DEFAULT_ALT, help="the ALT rule: transition (A>G, G>A, C>T, T>C), transversion (A>C, C>A, G>T, "
                        "T>G) or complement (A>T, T>A, C>G, G>C)")
    parser.add_argument("--indel", default=None, help="del<d> or dup<s>, d, s in 1 .. 255: the lists of --spikeScanIndel - a deletion of the "
                        "d letters behind every locus, or a tandem duplication of the next s - for --spikeIndelReps; --alt is not read")
    parser.add_argument("--mnv", default=None, help="L in 2 .. 8: the lists of --spikeScanMnv - one MNV of L adjacent letters at every "
                        "locus, --alt applied to every letter, as 4-column MNV lines for --spikeReps --spikePhase; needs --stride >= L")
    parser.add_argument("--outPrefix", default=None, required=True, help="prefix of the files written")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
