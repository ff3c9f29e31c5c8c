"""--spikeAF on the host side of a run: the command line's checks of the listed SNVs and targets, and
<outPrefix>.spikeAF.detection.txt - which planted variant the caller finds at which achieved allele fraction, on one page.

The semantics are tools/spike_variants.py's (DESIGN.md "--spikeAF"); the rewrite on the GPU is csrc/k_spike.inc (smc_spike_alleles),
the pre-pass that counts N, V0 and V1 and the rule that spikes every run of the main pass are devplanes.spike_rules / spike_run.
"""
from __future__ import annotations

from . import dsaf
from .tools import ds_allele_fraction as af
from .tools import spike_variants as sv

DETECTION_HEADER = ("CHROM", "POS", "REF", "ALT", "TARGET", "N", "V0", "S", "READS", "V1", "AF", "UMT", "VMT", "VMF", "PI", "FILTER", "CALLED")
MAX_TARGETS = 32               # (devplanes.SPIKE_MAX_TARGETS: every target holds a batch's device arrays)
DS_FLAGS = ("dsMT", "dsRpb", "dsGrid", "dsAF", "dsAFReps", "dsAFDepth")


def targets(args):
    """--spikeAF / --spikeVariants / --spikeMtDepth -> [(t, mtDepth of t, output prefix)]; [] without --spikeAF.  SystemExit: one flag
    without the other, a target outside (0, 1) or repeated, more than MAX_TARGETS, --spikeMtDepth of the wrong length, a down-sampling
    flag beside it."""
    text, vfile, depth = (getattr(args, f, None) for f in ("spikeAF", "spikeVariants", "spikeMtDepth"))
    if text in (None, ""):
        if vfile not in (None, ""):
            raise SystemExit("--spikeVariants lists the variants --spikeAF plants: it needs --spikeAF")
        if depth not in (None, ""):
            raise SystemExit("--spikeMtDepth gives the mtDepth of each --spikeAF target: it needs --spikeAF")
        return []
    if vfile in (None, ""):
        raise SystemExit("--spikeAF plants listed variants: it needs --spikeVariants")
    try:
        ts = af.parse_targets(text, "--spikeAF")
    except ValueError as e:
        raise SystemExit(str(e))
    if len(set("%g" % t for t in ts)) != len(ts):
        raise SystemExit("--spikeAF: a target is listed twice (the outputs' files would share a name), got %r" % text)
    if len(ts) > MAX_TARGETS:
        raise SystemExit("--spikeAF: %d targets, at most %d" % (len(ts), MAX_TARGETS))
    other = [f for f in DS_FLAGS if getattr(args, f, None) not in (None, "", False)]
    if other:
        raise SystemExit("--spikeAF cannot be combined with --%s in one run (spike-ins on a down-sampled file are not built)" % other[0])
    if depth in (None, ""):
        depths = [int(args.mtDepth)] * len(ts)
    else:
        try:
            depths = [int(x) for x in str(depth).split(",") if x.strip()]
        except ValueError:
            raise SystemExit("--spikeMtDepth: comma-separated integers expected, got %r" % depth)
        if len(depths) != len(ts):
            raise SystemExit("--spikeMtDepth: %d depths for %d --spikeAF targets" % (len(depths), len(ts)))
    return [(t, d, "%s.spikeAF%g" % (args.outPrefix, t)) for t, d in zip(ts, depths)]


def variants(args, loc_list, fasta):
    """The variants of --spikeVariants, checked: the file's refusals (tools.spike_variants.parse_variants: SNVs only), REF the
    genome's letter, every variant a locus of --bedTarget."""
    try:
        out = sv.parse_variants(args.spikeVariants, "--spikeVariants")
        sv.check_reference(out, fasta, "--spikeVariants")
        loci = set((c, int(p)) for c, p in loc_list)
        for v in out:
            if (v.chrom, v.pos) not in loci:
                raise ValueError("--spikeVariants: %s:%d %s>%s is not a locus of --bedTarget" % (v.chrom, v.pos, v.ref, v.alt))
    except (ValueError, OSError) as e:
        raise SystemExit(str(e))
    return out


def detection_line(v, target, r, row, cut, lod=None) -> str:
    """One line: variant `v` in one output.  `target` None: the full-depth output (nothing spiked: S and READS 0, V1 = V0); `r`: the
    pre-pass's numbers of that variant (and target); `row` / `cut` / `lod`: as dsaf.detection_line takes them."""
    f = dsaf.detection_line(v, target, r["N"], r["V0"], 1.0, row, cut, lod).split("\t")
    s, reads, v1 = (0, 0, r["V0"]) if target is None else (r["S"], r["READS"], r["V1"])
    return "\t".join(f[:5] + ["%d" % r["N"], "%d" % r["V0"], "%d" % s, "%d" % reads, "%d" % v1,
                              dsaf.frac_text(float(v1) / r["N"] if r["N"] else 0.0)] + f[9:])


def write_detection(out_prefix: str, variants, outputs, loc_index=None) -> None:
    """<outPrefix>.spikeAF.detection.txt: a header, then for every variant a line per output - full depth first, then the targets in
    the order given.  `outputs`: per output (target or None, prefix, the pre-pass's rows of that target (None: full depth), that
    output's LODs by locus index or None); `loc_index`: (chrom, pos text) -> locus index, for the LODs."""
    read = [dsaf.read_output(prefix) for _, prefix, _, _ in outputs]
    with_lod = any(l is not None for _, _, _, l in outputs)
    with open(out_prefix + ".spikeAF.detection.txt", "w") as fh:
        fh.write("\t".join(DETECTION_HEADER + (("LOD",) if with_lod else ())) + "\n")
        for i, v in enumerate(variants):
            key = (v.chrom, "%d" % v.pos)
            for (target, _, res_rows, lods), (rows, cut) in zip(outputs, read):
                r = (res_rows or outputs[1][2])[i]
                lod = float(lods[loc_index[key]]) if lods is not None else None
                fh.write(detection_line(v, target, r, rows.get(key), cut.get(key), lod) + "\n")
