"""--spikeAF on the host side of a run: the command line's checks of the listed SNVs and targets, and
<outPrefix>.spikeAF.detection.txt - which planted variant the caller finds at which achieved allele fraction, on one page.

--spikeReps: the three files that turn R x T spike-ins into a detection rate with an interval and an observed limit beside the
theoretical one - <outPrefix>.spikeAF.replicates.txt, .spikeAF.sensitivity.txt and .spikeAF.curve.txt (the replicate stage itself is
devplanes.spike_replicates).

--spikeDepth: the cells (target t, barcode fraction f) of the spike-ins - their flag, prefixes and mtDepths (depth_cells), and the four
pages <outPrefix>.spikeAF.depth.detection.txt, .replicates.txt, .sensitivity.txt and .curve.txt, which mirror .dsAF.depth.*.

--spikePhase: MNV lines and PS= entries of the variants file are phase sets, whose members share one draw (phase); the joint pages
<outPrefix>.spikeAF.phase.txt, .phase.replicates.txt and .phase.sensitivity.txt say how many molecules carry a whole set and whether
all of it was called.

--spikeIndels: the variants file may hold insertions and deletions too (indels; tools.spike_variants --indels is the rule); the
outputs and the detection page are --spikeAF's, V0 and V1 by the variant's INS / DEL key.

--spikeIndelReps / --spikeIndelDepth: --spikeReps and --spikeDepth on the --spikeIndels spike-in (indel_flags); the pages are those
of --spikeReps / --spikeDepth, from the same writers.

--spikeIndelPhase: phase sets whose members may be insertions and deletions (indel_phase; tools.spike_variants --phased --indels is
the rule): the variants file is read as --spikePhase reads it, under the rules of --spikeIndels; the pages are --spikePhase's.

--spikeRpb: the cells (target t, reads-per-barcode target r) of the spike-ins - the flag, the cells' prefixes and mtDepths (rpb_cells) -
and the pages <outPrefix>.spikeAF.rpb.detection.txt, .replicates.txt, .sensitivity.txt and .curve.txt from the depth pages' writers,
with RPB as their axis column (RPB_AXIS).

--spikeIndelRpb: --spikeRpb on the --spikeIndels spike-in (indel_flags refuses what does not go with it, indel_rpb_cells makes the cells
as rpb_cells does); the outputs' kind, the pages and their writers are --spikeRpb's.

--spikePhaseRpb: phase sets on the reads-per-barcode axis (phase_rpb_cells: the flag's refusals and --spikeRpb's cells); the run
writes what --spikeIndelRpb and --spikeIndelPhase write and, with RPB as the phase pages' axis column, <outPrefix>.spikeAF.rpb.phase.txt,
.rpb.phase.replicates.txt and .rpb.phase.sensitivity.txt - the joint numbers over the reads each cell keeps.

--spikeScan: one SNV at every locus of the target, planted in passes (tools.spike_scan_lists is the rule; scan reads the flags and
refuses what does not go with them); the pages <outPrefix>.spikeScan.sensitivity.txt and .curve.txt and the bedgraphs
<outPrefix>.spikeScan<t>.rate.bedgraph and .spikeScan.t95.bedgraph (write_scan) from the verdicts of devplanes.spike_scan, which keeps
the called rows on the GPU (smc_scan_detect).

--spikeScanIndel: the scan with one deletion (del<d>) or one tandem duplication (dup<s>) at every locus instead of the SNV (scan reads
and refuses the flag; tools.spike_scan_lists.scan_indels is the rule); the files and their writers are --spikeScan's, REF and ALT the
indel's texts at its anchor, the verdicts from smc_scan_detect_keys.

--spikeScanFilter: the scan's rates over the replicates that are called AND whose FILTER is PASS, and which of the 14 FILTER names
took the others away (scan reads the switch).  The two words per listed variant smc_scan_filter takes (scan_filter_words), its host
twin (scan_filter_host), a printed FILTER column as the same word (scan_filter_of_text), and the pages
<outPrefix>.spikeScan.filter.txt, .filter.curve.txt, .spikeScan<t>.passrate.bedgraph and .spikeScan.t95pass.bedgraph
(write_scan_filter) and, per axis, .spikeScan.depth.filter.txt / .spikeScan.rpb.filter.txt (write_scan_filter_cells).

--spikeScanMnvFilter: the same for the MNV scan (scan reads the switch) - a set is PASS in a replicate when every member is called and
every member's FILTER is PASS; the joint words are smc_scan_filter_sets' (abi.scan_filter_joint_rule), the pages
<outPrefix>.spikeScan.mnv.filter.txt, .mnv.filter.curve.txt, .spikeScan<t>.mnv.passrate.bedgraph and .spikeScan.mnv.t95pass.bedgraph
(write_scan_mnv_filter: write_scan_filter on the sets' MNVs).

The semantics are tools/spike_variants.py's (DESIGN.md "--spikeAF"); the rewrite on the GPU is csrc/k_spike.inc (smc_spike_alleles),
the pre-pass that counts N, V0 and V1 and the rule that spikes every run of the main pass are devplanes.spike_rules / spike_run.
"""
from __future__ import annotations

import re

from . import abi as _abi
from . import dsaf
from .tools import ds_allele_fraction as af
from .tools import spike_variants as sv

DETECTION_HEADER = ("CHROM", "POS", "REF", "ALT", "TARGET", "N", "V0", "S", "READS", "V1", "AF", "UMT", "VMT", "VMF", "PI", "FILTER", "CALLED")
MAX_TARGETS = 32               # (devplanes.SPIKE_MAX_TARGETS: every target holds a batch's device arrays)
DS_FLAGS = ("dsMT", "dsRpb", "dsGrid", "dsAF", "dsAFReps", "dsAFDepth")
MAX_CELLS = 32                 # (--spikeDepth: SMC_AF_DEPTH_MAX_CELLS; every cell holds a batch's device arrays)


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


def variants(args, loc_list, fasta, indels: bool = False):
    """The variants of --spikeVariants, checked: the file's refusals (tools.spike_variants.parse_variants: SNVs only, with
    --spikePhase MNV lines and PS= sets as well, with --spikeIndels - or `indels`: --spikeIndelReps, --spikeIndelDepth - insertions and
    deletions whose footprints do not overlap, with --spikeIndelPhase both), REF the genome's letters, every variant a locus of --bedTarget."""
    try:
        both = bool(getattr(args, "spikeIndelPhase", False)) or getattr(args, "spikePhaseRpb", None) not in (None, "")
        out = sv.parse_variants(args.spikeVariants, "--spikeVariants", phased=both or bool(getattr(args, "spikePhase", False)),
                                indels=both or bool(indels) or bool(getattr(args, "spikeIndels", False)))
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


# ---- --spikeIndels
def indels(args, spike_targets) -> bool:
    """--spikeIndels -> whether --spikeVariants may hold insertions and deletions.  SystemExit: without --spikeAF; beside --spikeReps,
    --spikeDepth or --spikePhase (what a replicate's or a cell's counters mean for an indel is not built)."""
    if not getattr(args, "spikeIndels", False):
        return False
    if not spike_targets:
        raise SystemExit("--spikeIndels lets --spikeVariants hold insertions and deletions for --spikeAF to plant: it needs --spikeAF")
    for flag in ("spikeReps", "spikeDepth", "spikePhase"):
        if getattr(args, flag, None) not in (None, "", False):
            raise SystemExit("--spikeIndels cannot be combined with --%s in one run (replicates, depths and phase sets of indel spike-ins "
                             "are not built)" % flag)
    return True


# ---- --spikeIndelReps, --spikeIndelDepth
def indel_flags(args, spike_targets):
    """--spikeIndelReps / --spikeIndelDepth -> (R or None, the fractions' text or None); --spikeIndelRpb is checked here with them - its
    text is indel_rpb_cells' to read: beside --spikeRpb (--spikeIndelRpb takes the targets), beside --spikeIndelDepth or
    --spikeIndelPhase (not built), without --spikeAF, and what follows for all three.  SystemExit: beside --spikeIndels, --spikeReps,
    --spikeDepth (the flag that covers it is named) or --spikePhase; --spikeIndelReps without --spikeAF and --spikeVariants,
    --spikeIndelDepth without --spikeAF; R no integer or outside REPS_MIN .. REPS_MAX.  (The fractions are depth_cells' to check.)"""
    r, text, rp = getattr(args, "spikeIndelReps", None), getattr(args, "spikeIndelDepth", None), getattr(args, "spikeIndelRpb", None)
    r, text, rp = (None if r in (None, "") else r), (None if text in (None, "") else text), (None if rp in (None, "") else rp)
    if r is None and text is None and rp is None:
        return None, None
    mine = "--spikeIndelReps" if r is not None else "--spikeIndelDepth" if text is not None else "--spikeIndelRpb"
    if rp is not None:
        # (--spikeIndelRpb: the reads-per-barcode targets are indel_rpb_cells' to check)
        if getattr(args, "spikeRpb", None) not in (None, ""):
            raise SystemExit("--spikeIndelRpb cannot be combined with --spikeRpb in one run: --spikeIndelRpb takes the targets")
        for flag in ("spikeIndelDepth", "spikeIndelPhase"):
            if getattr(args, flag, None) not in (None, "", False):
                raise SystemExit("--spikeIndelRpb cannot be combined with --%s in one run (the combination is not built)" % flag)
    if getattr(args, "spikeIndels", False):
        raise SystemExit("%s implies the rules of --spikeIndels: leave --spikeIndels out" % mine)
    if getattr(args, "spikeReps", None) not in (None, ""):
        raise SystemExit("%s cannot be combined with --spikeReps in one run: --spikeIndelReps R replicates the spike-ins itself" % mine)
    if getattr(args, "spikeDepth", None) not in (None, ""):
        raise SystemExit("%s cannot be combined with --spikeDepth in one run: --spikeIndelDepth takes the barcode fractions" % mine)
    if getattr(args, "spikePhase", False):
        raise SystemExit("%s cannot be combined with --spikePhase in one run (phase sets of indel spike-ins are not built)" % mine)
    if not spike_targets:
        raise SystemExit("--spikeIndelReps replicates the spike-ins of --spikeAF, insertions and deletions among them: it needs --spikeAF "
                         "and --spikeVariants" if r is not None else
                         "--spikeIndelRpb thins the reads of the --spikeAF spike-ins, insertions and deletions among them: it needs --spikeAF"
                         if text is None else
                         "--spikeIndelDepth thins the barcodes of the --spikeAF spike-ins, insertions and deletions among them: it needs --spikeAF")
    if r is not None:
        r = reps(args, spike_targets, "spikeIndelReps")
    return r, text


# ---- --spikeIndelPhase
def indel_phase(args, spike_targets) -> bool:
    """--spikeIndelPhase -> whether --spikeVariants is read for phase sets whose members may be insertions and deletions.  SystemExit,
    each naming the flag to use instead: beside --spikeIndels or --spikePhase (it implies both), beside --spikeReps or --spikeDepth
    (--spikeIndelReps / --spikeIndelDepth stand beside it); without --spikeAF."""
    if not getattr(args, "spikeIndelPhase", False):
        return False
    if getattr(args, "spikeIndels", False):
        raise SystemExit("--spikeIndelPhase implies the rules of --spikeIndels: leave --spikeIndels out")
    if getattr(args, "spikePhase", False):
        raise SystemExit("--spikeIndelPhase reads --spikeVariants as --spikePhase does: leave --spikePhase out")
    if getattr(args, "spikeReps", None) not in (None, ""):
        raise SystemExit("--spikeIndelPhase cannot be combined with --spikeReps in one run: use --spikeIndelReps R beside it")
    if getattr(args, "spikeDepth", None) not in (None, ""):
        raise SystemExit("--spikeIndelPhase cannot be combined with --spikeDepth in one run: use --spikeIndelDepth beside it")
    if not spike_targets:
        raise SystemExit("--spikeIndelPhase plants the phase sets of --spikeVariants, insertions and deletions among their members: it "
                         "needs --spikeAF and --spikeVariants")
    return True


# ---- --spikeReps
REPS_MIN, REPS_MAX = dsaf.REPS_MIN, dsaf.REPS_MAX
REPLICATES_HEADER = DETECTION_HEADER[:5] + ("REP", "SEED") + DETECTION_HEADER[5:]
SENSITIVITY_HEADER = ("CHROM", "POS", "REF", "ALT", "TARGET", "REPS", "CALLED", "RATE", "LO95", "HI95", "AF_MEAN", "AF_MIN", "AF_MAX",
                      "S_MIN", "S_MAX", "V_MIN", "V_MAX", "PI_MEAN", "PI_MIN")
CURVE_HEADER = ("CHROM", "POS", "REF", "ALT", "N")


def reps(args, spike_targets, flag: str = "spikeReps"):
    """--spikeReps -> R, or None without the flag.  SystemExit: without --spikeAF, R no integer or outside REPS_MIN .. REPS_MAX.
    `flag`: the flag read and named ("spikeIndelReps")."""
    r = getattr(args, flag, None)
    if r in (None, ""):
        return None
    if not spike_targets:
        raise SystemExit("--%s replicates the spike-ins of --spikeAF: it needs --spikeAF" % flag)
    try:
        if isinstance(r, float) and r != int(r):
            raise ValueError(r)
        r = int(r)
    except ValueError:
        raise SystemExit("--%s: an integer in %d .. %d expected, got %r" % (flag, REPS_MIN, REPS_MAX, r))
    if not (REPS_MIN <= r <= REPS_MAX):
        raise SystemExit("--%s: the number of replicates must lie in %d .. %d, got %d" % (flag, REPS_MIN, REPS_MAX, r))
    return r


def replicate_line(v, target, rep: int, seed: int, r, row, cut) -> str:
    """detection_line() of one replicate with REP and SEED behind TARGET (no LOD column).  `r`: dict(N, V0, S, READS, V1) of that
    replicate."""
    f = detection_line(v, target, r, row, cut).split("\t")
    return "\t".join(f[:5] + ["%d" % rep, "%d" % seed] + f[5:])


def _called(v, per) -> int:
    return sum(1 for _, _, cut in per if cut is not None and cut[0] == v.ref and v.alt in cut[1])


def sensitivity_line(v, target, per, lod=None) -> str:
    """One line of the sensitivity table: variant `v` at `target` over its replicates.  `per`: per replicate (dict(N, V0, S, READS,
    V1), row fields or None, cut or None) - what replicate_line() takes; a replicate without a row counts PI as 0; `lod`: the locus's
    LOD in the run's own output of that target, with --lod."""
    n = len(per)
    called = _called(v, per)
    lo, hi = dsaf.wilson(called, n)
    afs = [float(r["V1"]) / r["N"] if r["N"] else 0.0 for r, _, _ in per]
    pis = [dsaf._pi(row) for _, row, _ in per]
    ss, vs = [r["S"] for r, _, _ in per], [r["V1"] for r, _, _ in per]
    f = [v.chrom, "%d" % v.pos, v.ref, v.alt, dsaf.target_text(target), "%d" % n, "%d" % called, dsaf.frac_text(float(called) / n),
         dsaf.frac_text(lo), dsaf.frac_text(hi), dsaf.frac_text(sum(afs) / n), dsaf.frac_text(min(afs)), dsaf.frac_text(max(afs)),
         "%d" % min(ss), "%d" % max(ss), "%d" % min(vs), "%d" % max(vs), dsaf.frac_text(sum(pis) / n), dsaf.frac_text(min(pis))]
    if lod is not None:
        f.append("%.15g" % lod)
    return "\t".join(f)


def curve_header(targets, with_lod: bool = False):
    return CURVE_HEADER + tuple("RATE@%g" % t for t in sorted(targets)) + ("T95",) + (("LOD",) if with_lod else ())


def curve_line(v, n: int, targets, per_target, lod=None) -> str:
    """One line of the curve: variant `v` with N covering barcodes; per_target[t]: the replicates of targets[t] as sensitivity_line()
    takes them.  RATE@ columns in ascending target order, then T95 (dsaf.t95, or NA); `lod`: the theoretical limit beside it."""
    rates = [float(_called(v, per)) / len(per) for per in per_target]
    best = dsaf.t95(targets, rates)
    f = [v.chrom, "%d" % v.pos, v.ref, v.alt, "%d" % n] + [dsaf.frac_text(rates[t]) for t in sorted(range(len(targets)), key=lambda t: targets[t])] + \
        [dsaf.NA if best is None else "%g" % best]
    if lod is not None:
        f.append("%.15g" % lod)
    return "\t".join(f)


def write_replicates(out_prefix: str, variants, targets, seeds, entries) -> None:
    """<outPrefix>.spikeAF.replicates.txt: a header, then a line per listed variant (file order), target (the order given) and
    replicate (ascending).  entries[(v, t)]: per replicate (dict(N, V0, S, READS, V1), row fields or None, cut or None)."""
    with open(out_prefix + ".spikeAF.replicates.txt", "w") as fh:
        fh.write("\t".join(REPLICATES_HEADER) + "\n")
        for i, v in enumerate(variants):
            for t, target in enumerate(targets):
                for j, (r, row, cut) in enumerate(entries[(i, t)]):
                    fh.write(replicate_line(v, target, j, seeds[j], r, row, cut) + "\n")


def write_sensitivity(out_prefix: str, variants, targets, entries, lods=None) -> None:
    """<outPrefix>.spikeAF.sensitivity.txt: a header, then a line per listed variant and target.  lods[t][v] (with --lod): the LOD of
    the variant's locus in the run's .spikeAF<t> output."""
    with open(out_prefix + ".spikeAF.sensitivity.txt", "w") as fh:
        fh.write("\t".join(SENSITIVITY_HEADER + (("LOD",) if lods is not None else ())) + "\n")
        for i, v in enumerate(variants):
            for t, target in enumerate(targets):
                fh.write(sensitivity_line(v, target, entries[(i, t)], None if lods is None else float(lods[t][i])) + "\n")


def write_curve(out_prefix: str, variants, targets, entries, lods=None) -> None:
    """<outPrefix>.spikeAF.curve.txt: a header, then a line per listed variant - the observed limit (T95) beside, with --lod, the
    theoretical one: the locus's LOD in the output of the LARGEST listed target."""
    T = len(targets)
    top = max(range(T), key=lambda t: targets[t])
    with open(out_prefix + ".spikeAF.curve.txt", "w") as fh:
        fh.write("\t".join(curve_header(targets, lods is not None)) + "\n")
        for i, v in enumerate(variants):
            fh.write(curve_line(v, entries[(i, 0)][0][0]["N"], targets, [entries[(i, t)] for t in range(T)],
                                None if lods is None else float(lods[top][i])) + "\n")


# ---- --spikeDepth (and, with another axis, --spikeRpb)
# the cells' second axis on the pages below: (the pages' infix, the axis column's name); the column's text is "%g" of the cell's value
# (--spikeGrid: two columns, and a cell's value is the pair (f, r))
DEPTH_AXIS = ("depth", "FRACTION")
RPB_AXIS = ("rpb", "RPB")
GRID_AXIS = ("grid", ("FRACTION", "RPB"))


def _axis_columns(axis):
    return axis[1] if isinstance(axis[1], tuple) else (axis[1],)


def _axis_text(value):
    """The axis columns' text of a cell: "%g" of its value, or of each number of a pair."""
    return ["%g" % x for x in value] if isinstance(value, tuple) else ["%g" % value]


def cell_detection_header(axis=DEPTH_AXIS):
    return DETECTION_HEADER[:5] + _axis_columns(axis) + ("MTDEPTH",) + DETECTION_HEADER[5:]


def cell_replicates_header(axis=DEPTH_AXIS):
    h, n = cell_detection_header(axis), 6 + len(_axis_columns(axis))
    return h[:n] + ("REP", "SEED") + h[n:]


def cell_sensitivity_header(axis=DEPTH_AXIS):
    return SENSITIVITY_HEADER[:5] + _axis_columns(axis) + ("MTDEPTH",) + SENSITIVITY_HEADER[5:] + ("N_MEAN",)


DEPTH_DETECTION_HEADER = cell_detection_header()
DEPTH_REPLICATES_HEADER = cell_replicates_header()
DEPTH_SENSITIVITY_HEADER = cell_sensitivity_header()
DEPTH_CURVE_HEADER = dsaf.CURVE_HEADER


def depth_cells(args, spike_targets, flag: str = "spikeDepth"):
    """--spikeDepth -> (fractions, [(target index, t, f, mtDepth of the cell, output prefix)] for every --spikeAF target t and every
    fraction f, targets outer), or (None, []) without the flag.  A cell's mtDepth is what --dsMT f gets from its target's mtDepth.
    SystemExit: without --spikeAF, text that is no list of numbers, a fraction outside (0, 1] or listed twice, beyond MAX_CELLS
    cells.  `flag`: the flag read and named ("spikeIndelDepth")."""
    from .py2compat import py2_round
    text = getattr(args, flag, None)
    if text in (None, ""):
        return None, []
    if not spike_targets:
        raise SystemExit("--%s thins the barcodes of the --spikeAF spike-ins: it needs --spikeAF" % flag)
    try:
        fr = [float(x) for x in str(text).split(",") if x.strip()]
    except ValueError:
        raise SystemExit("--%s: comma-separated fractions in (0, 1] expected, got %r" % (flag, text))
    if not fr or any(not (0.0 < f <= 1.0) for f in fr):
        raise SystemExit("--%s: every fraction must lie in (0, 1], got %r" % (flag, text))
    if len(set("%g" % f for f in fr)) != len(fr):
        raise SystemExit("--%s: a fraction is listed twice (the cells' files would share a name), got %r" % (flag, text))
    if len(spike_targets) * len(fr) > MAX_CELLS:
        raise SystemExit("--%s: %d targets x %d fractions = %d cells, at most %d" % (flag, len(spike_targets), len(fr),
                                                                                      len(spike_targets) * len(fr), MAX_CELLS))
    return fr, [(k, t, f, max(1, int(py2_round(f * d))), "%s.dsMT%g" % (p, f)) for k, (t, d, p) in enumerate(spike_targets) for f in fr]


def _cell_fields(line: str, frac, mt_depth: int):
    f = line.split("\t")
    return f[:5] + _axis_text(frac) + ["%d" % mt_depth] + f[5:]


def depth_detection_line(v, target, frac, mt_depth, r, row, cut, lod=None) -> str:
    """detection_line() of variant `v` in cell (target, frac) with FRACTION and MTDEPTH behind TARGET.  `r`: the cell's achieved
    dict(N, V0, S, READS, V1)."""
    return "\t".join(_cell_fields(detection_line(v, target, r, row, cut, lod), frac, mt_depth))


def depth_replicate_line(v, target, frac, mt_depth, rep: int, seed: int, r, row, cut) -> str:
    f = _cell_fields(detection_line(v, target, r, row, cut), frac, mt_depth)
    n = 6 + len(_axis_text(frac))
    return "\t".join(f[:n] + ["%d" % rep, "%d" % seed] + f[n:])


def _n_mean(per) -> float:
    return sum(float(r["N"]) for r, _, _ in per) / len(per)


def depth_sensitivity_line(v, target, frac, mt_depth, per, lod=None) -> str:
    """sensitivity_line() of a cell with FRACTION and MTDEPTH behind TARGET and the mean N' behind PI_MIN (then LOD)."""
    f = _cell_fields(sensitivity_line(v, target, per), frac, mt_depth) + [dsaf.frac_text(_n_mean(per))]
    if lod is not None:
        f.append("%.15g" % lod)
    return "\t".join(f)


def depth_curve_header(targets, with_lod: bool = False, axis=DEPTH_AXIS):
    # (the curve's axis column is DEPTH for the barcode fractions - dsaf.CURVE_HEADER - and the axis's own name otherwise)
    head = DEPTH_CURVE_HEADER if axis is DEPTH_AXIS else DEPTH_CURVE_HEADER[:4] + (axis[1],) + DEPTH_CURVE_HEADER[5:]
    return head + tuple("RATE@%g" % t for t in sorted(targets)) + ("T95",) + (("LOD",) if with_lod else ())


def depth_curve_line(v, depth, mt_depths, targets, per_target, lod=None) -> str:
    """One line of the depth curve: variant `v` at one barcode depth (`depth` None: full, else f).  `mt_depths`: the mtDepth of every
    target's output at that depth (printed once when equal, else joined by commas); per_target[t]: the replicates of targets[t] there.
    RATE@ columns in ascending target order, then T95."""
    order = sorted(range(len(targets)), key=lambda t: targets[t])
    rates = [float(_called(v, per)) / len(per) for per in per_target]
    best = dsaf.t95(targets, rates)
    depths = ["%d" % d for d in mt_depths]
    f = [v.chrom, "%d" % v.pos, v.ref, v.alt, dsaf.FULL if depth is None else "%g" % depth,
         depths[0] if len(set(depths)) == 1 else ",".join(depths), dsaf.frac_text(sum(_n_mean(p) for p in per_target) / len(per_target))] + \
        [dsaf.frac_text(rates[t]) for t in order] + [dsaf.NA if best is None else "%g" % best]
    if lod is not None:
        f.append("%.15g" % lod)
    return "\t".join(f)


def write_depth_detection(out_prefix: str, variants, cells, counts, loc_index=None, axis=DEPTH_AXIS) -> None:
    """<outPrefix>.spikeAF.depth.detection.txt: a header, then a line per listed variant and cell (targets outer, fractions inner).
    `cells`: per cell (target index, target, fraction, mtDepth, output prefix, that output's LODs by locus index or None);
    counts[v][cell]: dict(N, V0, S, READS, V1), the cell's achieved numbers.  `axis` (RPB_AXIS: --spikeRpb): the page is
    .spikeAF.<axis[0]>.detection.txt, the cells' third field stands under the column axis[1]."""
    read = [dsaf.read_output(c[4]) for c in cells]
    with_lod = any(c[5] is not None for c in cells)
    with open("%s.spikeAF.%s.detection.txt" % (out_prefix, axis[0]), "w") as fh:
        fh.write("\t".join(cell_detection_header(axis) + (("LOD",) if with_lod else ())) + "\n")
        for i, v in enumerate(variants):
            key = (v.chrom, "%d" % v.pos)
            for c, ((_, target, frac, depth, _, lods), (rows, cut)) in enumerate(zip(cells, read)):
                lod = float(lods[loc_index[key]]) if lods is not None else None
                fh.write(depth_detection_line(v, target, frac, depth, counts[i][c], rows.get(key), cut.get(key), lod) + "\n")


def write_depth_replicates(out_prefix: str, variants, cells, seeds, entries, axis=DEPTH_AXIS) -> None:
    """<outPrefix>.spikeAF.depth.replicates.txt: a line per listed variant, cell and replicate.  entries[(v, cell)]: per replicate
    (dict(N, V0, S, READS, V1), row fields or None, cut or None)."""
    with open("%s.spikeAF.%s.replicates.txt" % (out_prefix, axis[0]), "w") as fh:
        fh.write("\t".join(cell_replicates_header(axis)) + "\n")
        for i, v in enumerate(variants):
            for c, (_, target, frac, depth, _, _) in enumerate(cells):
                for j, (r, row, cut) in enumerate(entries[(i, c)]):
                    fh.write(depth_replicate_line(v, target, frac, depth, j, seeds[j], r, row, cut) + "\n")


def write_depth_sensitivity(out_prefix: str, variants, cells, entries, loc_index=None, axis=DEPTH_AXIS) -> None:
    """<outPrefix>.spikeAF.depth.sensitivity.txt: a line per listed variant and cell; LOD: the locus's in the run's own output of the
    cell."""
    with_lod = any(c[5] is not None for c in cells)
    with open("%s.spikeAF.%s.sensitivity.txt" % (out_prefix, axis[0]), "w") as fh:
        fh.write("\t".join(cell_sensitivity_header(axis) + (("LOD",) if with_lod else ())) + "\n")
        for i, v in enumerate(variants):
            for c, (_, target, frac, depth, _, lods) in enumerate(cells):
                lod = float(lods[loc_index[(v.chrom, "%d" % v.pos)]]) if lods is not None else None
                fh.write(depth_sensitivity_line(v, target, frac, depth, entries[(i, c)], lod) + "\n")


def write_depth_curve(out_prefix: str, variants, targets, fracs, full, cells, full_entries, entries, loc_index=None, axis=DEPTH_AXIS) -> None:
    """<outPrefix>.spikeAF.depth.curve.txt: a line per listed variant and barcode depth - `full` (the targets' own outputs) first, then
    every fraction.  `full`: per target (mtDepth, the LODs of its .spikeAF<t> output or None); full_entries[(v, t)] / entries[(v,
    cell)]: the replicates.  LOD: the locus's theoretical one at that depth, in the output of the LARGEST listed target there."""
    T, F = len(targets), len(fracs)
    top = max(range(T), key=lambda t: targets[t])
    with_lod = any(c[5] is not None for c in cells)
    with open("%s.spikeAF.%s.curve.txt" % (out_prefix, axis[0]), "w") as fh:
        fh.write("\t".join(depth_curve_header(targets, with_lod, axis)) + "\n")
        for i, v in enumerate(variants):
            at = loc_index[(v.chrom, "%d" % v.pos)] if with_lod else None
            fh.write(depth_curve_line(v, None, [d for d, _ in full], targets, [full_entries[(i, t)] for t in range(T)],
                                      float(full[top][1][at]) if with_lod else None) + "\n")
            for k, f in enumerate(fracs):
                mine = [cells[t * F + k] for t in range(T)]
                fh.write(depth_curve_line(v, f, [c[3] for c in mine], targets, [entries[(i, t * F + k)] for t in range(T)],
                                          float(mine[top][5][at]) if with_lod else None) + "\n")


# ---- --spikeRpb
RPB_NOT_WITH = ("spikeDepth", "spikePhase", "spikeIndels", "spikeIndelReps", "spikeIndelDepth", "spikeIndelPhase")


def rpb_cells(args, spike_targets):
    """--spikeRpb -> (reads-per-barcode targets, [(target index, t, r, mtDepth of the cell, output prefix)] for every --spikeAF target t
    and every r, targets outer), or (None, []) without the flag.  A cell is called at its target's mtDepth (and at --rpb r).
    SystemExit: without --spikeAF, text that is no list of numbers, a target <= 0 or listed twice, beyond MAX_CELLS cells, beside a
    flag of RPB_NOT_WITH (the combination is not built)."""
    text = getattr(args, "spikeRpb", None)
    if text in (None, ""):
        return None, []
    if not spike_targets:
        raise SystemExit("--spikeRpb thins the reads of the --spikeAF spike-ins: it needs --spikeAF")
    for flag in RPB_NOT_WITH:
        if getattr(args, flag, None) not in (None, "", False):
            raise SystemExit("--spikeRpb cannot be combined with --%s in one run (the combination is not built)" % flag)
    return _rpb_cells(text, spike_targets, "spikeRpb")


def _rpb_cells(text, spike_targets, flag: str):
    """The reads-per-barcode targets of `text` and the cells they make with the --spikeAF targets; `flag`: the flag named."""
    try:
        rs = [float(x) for x in str(text).split(",") if x.strip()]
    except ValueError:
        raise SystemExit("--%s: comma-separated reads-per-barcode targets > 0 expected, got %r" % (flag, text))
    if not rs or any(not (r > 0.0 and r < float("inf")) for r in rs):
        raise SystemExit("--%s: every target must be a number > 0, got %r" % (flag, text))
    if len(set("%g" % r for r in rs)) != len(rs):
        raise SystemExit("--%s: a target is listed twice (the cells' files would share a name), got %r" % (flag, text))
    if len(spike_targets) * len(rs) > MAX_CELLS:
        raise SystemExit("--%s: %d targets x %d reads-per-barcode targets = %d cells, at most %d" %
                         (flag, len(spike_targets), len(rs), len(spike_targets) * len(rs), MAX_CELLS))
    return rs, [(k, t, r, d, "%s.dsRpb%g" % (p, r)) for k, (t, d, p) in enumerate(spike_targets) for r in rs]


# ---- --spikeGrid
GRID_NOT_WITH = ("spikePhase", "spikeIndels", "spikeIndelReps", "spikeIndelDepth", "spikeIndelRpb", "spikeIndelPhase", "spikePhaseRpb")
BUDGET_HEADER = ("CHROM", "POS", "REF", "ALT", "TARGET", "FRACTION", "RPB", "MTDEPTH", "KEPT_NAMES", "COST", "N_MEAN", "REPS", "CALLED", "RATE",
                 "LO95", "HI95", "CHEAPEST95")


def grid_cells(args, spike_targets):
    """--spikeGrid -> (fractions, reads-per-barcode targets, [(target index, t, (f, r), mtDepth of the cell, output prefix)] for every
    --spikeAF target t, --spikeDepth fraction f and --spikeRpb target r - targets outer, then fractions, then r), or (None, None, [])
    without the switch.  A cell is called at depth_cells' mtDepth of (t, f) and at --rpb r.  SystemExit: without --spikeAF or one of
    the two axis flags, beside a flag of GRID_NOT_WITH or a --spikeScan* flag (not built), what --spikeDepth and --spikeRpb refuse of
    their lists, beyond MAX_CELLS cells."""
    if not getattr(args, "spikeGrid", False):
        return None, None, []
    if not spike_targets:
        raise SystemExit("--spikeGrid calls the --spikeAF spike-ins on the --spikeDepth x --spikeRpb grid: it needs --spikeAF")
    for flag in ("spikeDepth", "spikeRpb"):
        if getattr(args, flag, None) in (None, ""):
            raise SystemExit("--spikeGrid calls every --spikeDepth fraction with every --spikeRpb target: it needs both --spikeDepth and "
                             "--spikeRpb (--%s is missing)" % flag)
    for flag in GRID_NOT_WITH + tuple(f for f in sorted(vars(args)) if f.startswith("spikeScan")):
        if getattr(args, flag, None) not in (None, "", False):
            raise SystemExit("--spikeGrid cannot be combined with --%s in one run (the combination is not built)" % flag)
    fracs, depth = depth_cells(args, spike_targets)
    rpbs, _ = _rpb_cells(args.spikeRpb, spike_targets, "spikeRpb")
    if len(spike_targets) * len(fracs) * len(rpbs) > MAX_CELLS:
        raise SystemExit("--spikeGrid: %d targets x %d fractions x %d reads-per-barcode targets = %d cells, at most %d" %
                         (len(spike_targets), len(fracs), len(rpbs), len(spike_targets) * len(fracs) * len(rpbs), MAX_CELLS))
    return fracs, rpbs, [(k, t, (f, r), d, "%s.dsRpb%g" % (p, r)) for k, t, f, d, p in depth for r in rpbs]


def budget_order(costs):
    """The budget page's order of a variant's cells at one target: by cost ascending, ties in the listed order -> indices."""
    return sorted(range(len(costs)), key=lambda c: (costs[c], c))


def budget_lines(v, target, cells, file_names: int, per_cell):
    """The budget page's lines of variant `v` at `target`: cells[c] = ((f, r), mtDepth, kept names of the cell file-wide), per_cell[c]
    the cell's replicates as sensitivity_line() takes them.  COST = kept names over the file's distinct read names; the lines by
    COST ascending (ties in the listed order); CHEAPEST95 is 1 on the first line whose RATE is at least 0.95."""
    costs = [float(kept) / file_names if file_names else 0.0 for _, _, kept in cells]
    out, found = [], False
    for c in budget_order(costs):
        (f, r), depth, kept = cells[c]
        per = per_cell[c]
        n, called = len(per), _called(v, per_cell[c])
        lo, hi = dsaf.wilson(called, n)
        rate = float(called) / n
        first = rate >= 0.95 and not found
        found = found or first
        out.append("\t".join([v.chrom, "%d" % v.pos, v.ref, v.alt, dsaf.target_text(target), "%g" % f, "%g" % r, "%d" % depth, "%d" % kept,
                              dsaf.frac_text(costs[c]), dsaf.frac_text(_n_mean(per)), "%d" % n, "%d" % called, dsaf.frac_text(rate),
                              dsaf.frac_text(lo), dsaf.frac_text(hi), "%d" % first]))
    return out


def write_budget(out_prefix: str, variants, cells, file_names: int, entries) -> None:
    """<outPrefix>.spikeAF.grid.budget.txt: per listed variant and target a line per cell of that target, cheapest first.  `cells`:
    per cell (target index, target, (f, r), mtDepth, output prefix, LODs or None, kept names) - the grid pages' tuples with the cell's
    kept read names file-wide behind; entries[(v, cell)]: the replicates."""
    with open(out_prefix + ".spikeAF.grid.budget.txt", "w") as fh:
        fh.write("\t".join(BUDGET_HEADER) + "\n")
        for i, v in enumerate(variants):
            for k in dict.fromkeys(c[0] for c in cells):
                mine = [c for c, cell in enumerate(cells) if cell[0] == k]
                for line in budget_lines(v, cells[mine[0]][1], [(cells[c][2], cells[c][3], cells[c][6]) for c in mine], file_names,
                                         [entries[(i, c)] for c in mine]):
                    fh.write(line + "\n")


# ---- --spikeIndelRpb
def indel_rpb_cells(args, spike_targets):
    """--spikeIndelRpb -> rpb_cells' (reads-per-barcode targets, cells), or (None, []) without the flag.  What the flag does not go
    with is indel_flags' to refuse (call it first); SystemExit here: without --spikeAF, text that is no list of numbers, a target <= 0
    or listed twice, beyond MAX_CELLS cells."""
    text = getattr(args, "spikeIndelRpb", None)
    if text in (None, ""):
        return None, []
    if not spike_targets:
        raise SystemExit("--spikeIndelRpb thins the reads of the --spikeAF spike-ins, insertions and deletions among them: it needs --spikeAF")
    return _rpb_cells(text, spike_targets, "spikeIndelRpb")


# ---- --spikePhaseRpb
def phase_rpb_cells(args, spike_targets):
    """--spikePhaseRpb -> rpb_cells' (reads-per-barcode targets, cells), or (None, []) without the flag.  The flag implies the rules of
    --spikeIndelPhase (and so of --spikeIndels and --spikePhase) and takes the targets as --spikeIndelRpb does.  SystemExit, each naming
    the flag to use instead where there is one: beside --spikeRpb or --spikeIndelRpb (this flag takes the targets), beside
    --spikeIndels, --spikePhase or --spikeIndelPhase (implied), beside --spikeReps (--spikeIndelReps), beside --spikeDepth or
    --spikeIndelDepth (not built); without --spikeAF; text that is no list of numbers, a target <= 0 or listed twice, beyond MAX_CELLS
    cells."""
    text = getattr(args, "spikePhaseRpb", None)
    if text in (None, ""):
        return None, []
    for flag in ("spikeRpb", "spikeIndelRpb"):
        if getattr(args, flag, None) not in (None, ""):
            raise SystemExit("--spikePhaseRpb cannot be combined with --%s in one run: --spikePhaseRpb takes the targets" % flag)
    for flag in ("spikeIndels", "spikePhase", "spikeIndelPhase"):
        if getattr(args, flag, False):
            raise SystemExit("--spikePhaseRpb implies the rules of --%s: leave --%s out" % (flag, flag))
    if getattr(args, "spikeReps", None) not in (None, ""):
        raise SystemExit("--spikePhaseRpb cannot be combined with --spikeReps in one run: use --spikeIndelReps R beside it")
    for flag in ("spikeDepth", "spikeIndelDepth"):
        if getattr(args, flag, None) not in (None, ""):
            raise SystemExit("--spikePhaseRpb cannot be combined with --%s in one run (phase sets in cells of barcode depths and "
                             "reads-per-barcode targets are not built)" % flag)
    if not spike_targets:
        raise SystemExit("--spikePhaseRpb thins the reads of the --spikeAF spike-ins, phase sets among them: it needs --spikeAF and "
                         "--spikeVariants")
    return _rpb_cells(text, spike_targets, "spikePhaseRpb")


# ---- --spikePhase
PHASE_NAMES = ("N_ALL", "V0_ALL", "S_ALL", "V1_ALL")


def phase_header(axis=DEPTH_AXIS):
    return ("SET", "CHROM", "POSITIONS", "REFS", "ALTS", "TARGET", axis[1], "MTDEPTH") + PHASE_NAMES + ("AF_ALL", "CALLED_ALL")


def phase_replicates_header(axis=DEPTH_AXIS):
    h = phase_header(axis)
    return h[:8] + ("REP", "SEED") + h[8:]


def phase_sensitivity_header(axis=DEPTH_AXIS):
    return phase_header(axis)[:8] + ("REPS", "CALLED_ALL", "RATE", "LO95", "HI95", "AF_MEAN", "AF_MIN", "AF_MAX")


PHASE_HEADER = phase_header()
PHASE_REPLICATES_HEADER = phase_replicates_header()
PHASE_SENSITIVITY_HEADER = phase_sensitivity_header()


def _phase_page(out_prefix: str, axis, page: str) -> str:
    # (the barcode fractions' pages are .spikeAF.phase<page>; another axis puts its infix in front: .spikeAF.rpb.phase<page>)
    return "%s.spikeAF.%sphase%s.txt" % (out_prefix, "" if axis is DEPTH_AXIS else axis[0] + ".", page)


def phase(args, spike_targets) -> bool:
    """--spikePhase -> whether the variants file is read for phase sets.  SystemExit: without --spikeAF."""
    if not getattr(args, "spikePhase", False):
        return False
    if not spike_targets:
        raise SystemExit("--spikePhase plants the phase sets of --spikeVariants together: it needs --spikeAF")
    return True


def _af_all(r) -> float:
    return float(r["V1_ALL"]) / r["N_ALL"] if r["N_ALL"] else 0.0


def _set_fields(pset, variants, target, frac, mt_depth):
    vs = [variants[k] for k in pset.members]
    return [pset.name, pset.chrom, ",".join("%d" % v.pos for v in vs), ",".join(v.ref for v in vs), ",".join(v.alt for v in vs),
            dsaf.target_text(target), dsaf.FULL if frac is None else "%g" % frac, "%d" % mt_depth]


def called_all(pset, variants, cut) -> int:
    """1 when `cut` ((chrom, pos text) -> (REF, ALT list) of an output's .cut.txt) has every member of the set with its ALT - per
    member the comparison of the detection page's CALLED (dsaf.detection_line), whatever its kind: an insertion's or a deletion's line
    stands at its anchor with the listed REF and ALT texts."""
    for k in pset.members:
        v = variants[k]
        c = cut.get((v.chrom, "%d" % v.pos))
        if c is None or c[0] != v.ref or v.alt not in c[1]:
            return 0
    return 1


def phase_line(pset, variants, target, frac, mt_depth, r, called: int) -> str:
    """One line of the phase page: set `pset` in one output.  `target` None: the full-depth output; `frac` None: no --spikeDepth
    cell; `r`: dict(N_ALL, V0_ALL, S_ALL, V1_ALL) of the joint barcodes there."""
    return "\t".join(_set_fields(pset, variants, target, frac, mt_depth) + ["%d" % r[n] for n in PHASE_NAMES] +
                     [dsaf.frac_text(_af_all(r)), "%d" % called])


def phase_replicate_line(pset, variants, target, frac, mt_depth, rep: int, seed: int, r, called: int) -> str:
    f = phase_line(pset, variants, target, frac, mt_depth, r, called).split("\t")
    return "\t".join(f[:8] + ["%d" % rep, "%d" % seed] + f[8:])


def phase_sensitivity_line(pset, variants, target, frac, mt_depth, per) -> str:
    """One line of the phase sensitivity table; `per`: per replicate (dict(N_ALL, V0_ALL, S_ALL, V1_ALL), CALLED_ALL)."""
    n = len(per)
    called = sum(c for _, c in per)
    lo, hi = dsaf.wilson(called, n)
    afs = [_af_all(r) for r, _ in per]
    return "\t".join(_set_fields(pset, variants, target, frac, mt_depth) +
                     ["%d" % n, "%d" % called, dsaf.frac_text(float(called) / n), dsaf.frac_text(lo), dsaf.frac_text(hi),
                      dsaf.frac_text(sum(afs) / n), dsaf.frac_text(min(afs)), dsaf.frac_text(max(afs))])


def write_phase(out_prefix: str, variants, sets, outputs, axis=DEPTH_AXIS) -> None:
    """<outPrefix>.spikeAF.phase.txt: a header, then for every set a line per output - full depth first, then the targets, then the
    --spikeDepth cells.  `outputs`: per output (target or None, fraction or None, mtDepth, prefix, per set dict(N_ALL, V0_ALL, S_ALL,
    V1_ALL)).  `axis` (RPB_AXIS: --spikePhaseRpb): the page is .spikeAF.<axis[0]>.phase.txt, the outputs are the cells and their
    second field - the reads-per-barcode target - stands under the column axis[1]."""
    cuts = [dsaf.read_output(o[3])[1] for o in outputs]
    with open(_phase_page(out_prefix, axis, ""), "w") as fh:
        fh.write("\t".join(phase_header(axis)) + "\n")
        for g, pset in enumerate(sets):
            for (target, frac, depth, _, rows), cut in zip(outputs, cuts):
                fh.write(phase_line(pset, variants, target, frac, depth, rows[g], called_all(pset, variants, cut)) + "\n")


def write_phase_replicates(out_prefix: str, variants, sets, outputs, seeds, entries, axis=DEPTH_AXIS) -> None:
    """<outPrefix>.spikeAF.phase.replicates.txt: a line per set, output (targets, then cells: (target, fraction or None, mtDepth)) and
    replicate.  entries[(set, output)]: per replicate (dict(N_ALL, V0_ALL, S_ALL, V1_ALL), CALLED_ALL).  `axis`: write_phase's."""
    with open(_phase_page(out_prefix, axis, ".replicates"), "w") as fh:
        fh.write("\t".join(phase_replicates_header(axis)) + "\n")
        for g, pset in enumerate(sets):
            for c, (target, frac, depth) in enumerate(outputs):
                for j, (r, called) in enumerate(entries[(g, c)]):
                    fh.write(phase_replicate_line(pset, variants, target, frac, depth, j, seeds[j], r, called) + "\n")


def write_phase_sensitivity(out_prefix: str, variants, sets, outputs, entries, axis=DEPTH_AXIS) -> None:
    """<outPrefix>.spikeAF.phase.sensitivity.txt: a line per set and output; the arguments are write_phase_replicates'."""
    with open(_phase_page(out_prefix, axis, ".sensitivity"), "w") as fh:
        fh.write("\t".join(phase_sensitivity_header(axis)) + "\n")
        for g, pset in enumerate(sets):
            for c, (target, frac, depth) in enumerate(outputs):
                fh.write(phase_sensitivity_line(pset, variants, target, frac, depth, entries[(g, c)]) + "\n")


# ---- --spikeScan
SCAN_FLAGS = ("spikeScan", "spikeScanReps", "spikeScanStride", "spikeScanAlt")
SCAN_NOT_WITH = ("spikeAF", "spikeVariants", "spikeMtDepth", "spikeReps", "spikePhase", "spikeIndels", "spikeIndelReps", "spikeIndelDepth",
                 "spikeIndelPhase", "spikeDepth", "spikeRpb", "spikeIndelRpb", "spikePhaseRpb")
SCAN_NOT_WITH_DS = DS_FLAGS + ("dsMtDepth", "dsRpbMtDepth", "dsAFVariants", "dsAFMtDepth")
SCAN_BUILDS = ("whole", "listed")      # --spikeScanBuild: every copy a whole build of its run (the default), or smc_build_listed
SCAN_SENSITIVITY_HEADER = tuple(c for c in SENSITIVITY_HEADER if c not in ("PI_MEAN", "PI_MIN"))


def _scan_int(text, flag: str, lo: int, hi, what: str) -> int:
    try:
        if isinstance(text, float) and text != int(text):
            raise ValueError(text)
        n = int(str(text).strip()) if not isinstance(text, (int, float)) else int(text)
    except ValueError:
        raise SystemExit("--%s: an integer %s expected, got %r" % (flag, what, text))
    if n < lo or (hi is not None and n > hi):
        raise SystemExit("--%s: an integer %s expected, got %d" % (flag, what, n))
    return n


def _scan_fracs(text, flag: str, n_targets: int):
    """The barcode fractions of --spikeScanDepth / --spikeScanMnvDepth.  SystemExit naming `flag`: text that is no list of numbers, a
    fraction outside (0, 1] or listed twice, more than MAX_CELLS targets x fractions."""
    try:
        fr = [float(x) for x in str(text).split(",") if x.strip()]
    except ValueError:
        raise SystemExit("--%s: comma-separated fractions in (0, 1] expected, got %r" % (flag, text))
    if not fr or any(not (0.0 < f <= 1.0) for f in fr):
        raise SystemExit("--%s: every fraction must lie in (0, 1], got %r" % (flag, text))
    if len(set("%g" % f for f in fr)) != len(fr):
        raise SystemExit("--%s: a fraction is listed twice (the cells' files would share a name), got %r" % (flag, text))
    if n_targets * len(fr) > MAX_CELLS:
        raise SystemExit("--%s: %d targets x %d fractions = %d cells, at most %d" % (flag, n_targets, len(fr), n_targets * len(fr), MAX_CELLS))
    return fr


def scan(args):
    """--spikeScan / --spikeScanReps / --spikeScanStride / --spikeScanAlt -> dict(targets, reps, stride, alt), or None without
    --spikeScan.  SystemExit: a helper flag without --spikeScan, --spikeScan without --spikeScanReps, any other --spike* flag or a
    down-sampling flag beside it, a target outside (0, 1) or listed twice, more than MAX_TARGETS, R outside REPS_MIN .. REPS_MAX or no
    integer, a stride below 1 or no integer, an unknown ALT rule.
    --spikeScanIndel adds "indel": ("del" or "dup", the length) to the dict.  SystemExit: the flag without --spikeScan or beside
    --spikeScanAlt, a rule that is neither del<d> nor dup<s> with a length in 1 .. 255, a stride below the footprint's.
    --spikeScanDepth adds "fracs": the barcode fractions of the scan's depth axis.  SystemExit: the flag without --spikeScan, text that
    is no list of numbers, a fraction outside (0, 1] or listed twice, more than MAX_CELLS targets x fractions.
    --spikeScanRpb adds "rpbs": the reads-per-barcode targets of the scan's read axis.  SystemExit: the flag without --spikeScan or
    beside --spikeScanDepth (the t x f x r grid is not built), text that is no list of numbers, a target <= 0 or listed twice, more
    than MAX_CELLS targets x reads-per-barcode targets.
    --spikeScanFilter (a switch) adds "filter": True.  SystemExit: the switch without --spikeScan.
    --spikeScanBuild listed adds "build": "listed" (`whole`, the default, adds nothing: scan_build reads it).  SystemExit: the flag
    without --spikeScan, a value that is neither whole nor listed.
    --spikeScanMnv L adds "mnv": L, the letters of the MNV planted at every locus in place of the SNV.  SystemExit: the flag without
    --spikeScan, L no integer in 2 .. 8, a stride below L, the flag beside --spikeScanIndel, or beside --spikeScanDepth, --spikeScanRpb
    or --spikeScanFilter (not built).
    --spikeScanMnvFilter (a switch) adds "mnv_filter": True, the filter axis of the MNV scan.  SystemExit: the switch without
    --spikeScan or without --spikeScanMnv; beside --spikeScanDepth, --spikeScanRpb, --spikeScanFilter or --spikeScanIndel the refusals
    of --spikeScanMnv above fire first.
    --spikeScanMnvDepth adds "mnv_fracs": the barcode fractions of the MNV scan's depth axis.  SystemExit: as the switch's, and what
    --spikeScanDepth refuses of its text, named after this flag.
    --spikeScanMnvRpb adds "mnv_rpbs": the reads-per-barcode targets of the MNV scan's read axis.  SystemExit: as the switch's, the flag
    beside --spikeScanMnvDepth (the t x f x r grid is not built), and what --spikeScanRpb refuses of its text, named after this flag."""
    from .tools import spike_scan_lists as lists
    text, r, stride, alt = (getattr(args, f, None) for f in SCAN_FLAGS)
    indel = getattr(args, "spikeScanIndel", None)
    fracs = getattr(args, "spikeScanDepth", None)
    rpbs = getattr(args, "spikeScanRpb", None)
    flt = getattr(args, "spikeScanFilter", None)
    build = getattr(args, "spikeScanBuild", None)
    mnv = getattr(args, "spikeScanMnv", None)
    mnv_flt = getattr(args, "spikeScanMnvFilter", None)
    mnv_fracs = getattr(args, "spikeScanMnvDepth", None)
    mnv_rpbs = getattr(args, "spikeScanMnvRpb", None)
    given = lambda x: x not in (None, "", False)
    if not given(text):
        for flag, value in zip(SCAN_FLAGS[1:] + ("spikeScanIndel", "spikeScanDepth", "spikeScanRpb", "spikeScanFilter", "spikeScanBuild",
                                                 "spikeScanMnv", "spikeScanMnvFilter", "spikeScanMnvDepth", "spikeScanMnvRpb"),
                               (r, stride, alt, indel, fracs, rpbs, flt, build, mnv, mnv_flt, mnv_fracs, mnv_rpbs)):
            if given(value):
                raise SystemExit("--%s belongs to --spikeScan: it needs --spikeScan" % flag)
        return None
    if given(build) and str(build) not in SCAN_BUILDS:
        raise SystemExit("--spikeScanBuild: %s expected, got %r" % (" or ".join(SCAN_BUILDS), build))
    if given(indel) and given(alt):
        raise SystemExit("--spikeScanIndel cannot be combined with --spikeScanAlt: the scan plants an insertion or a deletion OR an SNV at "
                         "every locus, not both")
    if given(mnv):
        if given(indel):
            raise SystemExit("--spikeScanMnv cannot be combined with --spikeScanIndel: the scan plants an MNV OR an insertion or a deletion "
                             "at every locus (indel members in a scan are not built)")
        for flag, value in (("spikeScanDepth", fracs), ("spikeScanRpb", rpbs), ("spikeScanFilter", flt)):
            if given(value):
                raise SystemExit("--spikeScanMnv cannot be combined with --%s: the %s axis of an MNV scan is not built" %
                                 (flag, {"spikeScanDepth": "depth", "spikeScanRpb": "reads-per-barcode", "spikeScanFilter": "filter"}[flag]))
    for flag, value in (("spikeScanMnvFilter", mnv_flt), ("spikeScanMnvDepth", mnv_fracs), ("spikeScanMnvRpb", mnv_rpbs)):
        if given(value) and not given(mnv):
            raise SystemExit("--%s belongs to --spikeScanMnv: it needs --spikeScanMnv" % flag)
    for flag in SCAN_NOT_WITH:
        if given(getattr(args, flag, None)):
            raise SystemExit("--spikeScan cannot be combined with --%s in one run: the scan plants its own SNV at every locus of "
                             "--bedTarget (a pass of it is the --spikeAF --spikeReps run of tools/spike_scan_lists.py's list)" % flag)
    for flag in SCAN_NOT_WITH_DS:
        if given(getattr(args, flag, None)):
            raise SystemExit("--spikeScan cannot be combined with --%s in one run (a scan of a down-sampled file is not built)" % flag)
    if not given(r):
        raise SystemExit("--spikeScan measures a detection rate over replicates: it needs --spikeScanReps")
    try:
        ts = af.parse_targets(text, "--spikeScan")
    except ValueError as e:
        raise SystemExit(str(e))
    if len(set("%g" % t for t in ts)) != len(ts):
        raise SystemExit("--spikeScan: a target is listed twice (the targets' files would share a name), got %r" % text)
    if len(ts) > MAX_TARGETS:
        raise SystemExit("--spikeScan: %d targets, at most %d" % (len(ts), MAX_TARGETS))
    r = _scan_int(r, "spikeScanReps", REPS_MIN, REPS_MAX, "in %d .. %d" % (REPS_MIN, REPS_MAX))
    stride = lists.DEFAULT_STRIDE if not given(stride) else _scan_int(stride, "spikeScanStride", 1, None, ">= 1")
    alt = lists.DEFAULT_ALT if not given(alt) else str(alt)
    if alt not in lists.ALT_RULES:
        raise SystemExit("--spikeScanAlt: one of %s expected, got %r" % (", ".join(sorted(lists.ALT_RULES)), alt))
    out = dict(targets=ts, reps=r, stride=stride, alt=alt)
    if given(mnv):
        try:
            out["mnv"] = lists.parse_mnv(mnv)
            lists.check_mnv_stride(out["mnv"], stride)
        except ValueError as e:
            raise SystemExit(str(e))
    if given(mnv_flt):
        out["mnv_filter"] = True
    if given(indel):
        try:
            out["indel"] = lists.parse_indel_rule(indel)
            lists.check_indel_stride(out["indel"], stride)
        except ValueError as e:
            raise SystemExit(str(e))
    if given(fracs):
        out["fracs"] = _scan_fracs(fracs, "spikeScanDepth", len(ts))
    if given(mnv_fracs):
        out["mnv_fracs"] = _scan_fracs(mnv_fracs, "spikeScanMnvDepth", len(ts))
    if given(mnv_rpbs):
        if given(mnv_fracs):
            raise SystemExit("--spikeScanMnvRpb cannot be combined with --spikeScanMnvDepth in one run: the grid of targets x barcode "
                             "fractions x reads-per-barcode targets is not built")
        out["mnv_rpbs"] = _rpb_cells(mnv_rpbs, [(t, 0, "") for t in ts], "spikeScanMnvRpb")[0]
    if given(rpbs):
        if given(fracs):
            raise SystemExit("--spikeScanRpb cannot be combined with --spikeScanDepth in one run: the grid of targets x barcode fractions x "
                             "reads-per-barcode targets is not built")
        # (the targets' texts and limits are --spikeRpb's: the scan's targets stand where the --spikeAF targets do)
        out["rpbs"] = _rpb_cells(rpbs, [(t, 0, "") for t in ts], "spikeScanRpb")[0]
    if given(flt):
        out["filter"] = True
    if given(build) and str(build) != SCAN_BUILDS[0]:
        out["build"] = str(build)
    return out


SCAN_PASS_LINE = re.compile(r"^--spikeScan pass (\d+): (\d+) variants, (\d+) copies, (\d+) builds, (?:(\d+) of them whole, )?(\d+) verdicts decided "
                            r"by the host, ([0-9.]+) s$")


def scan_pass_line(line: str):
    """A pass line of the run log -> dict(k, variants, copies, builds, whole, host, seconds), or None for any other line; `whole` - the
    builds made by the whole-run builder - is None where the line has no such field (--spikeScanBuild whole)."""
    m = SCAN_PASS_LINE.match(line.rstrip("\n"))
    if m is None:
        return None
    k, variants, copies, builds, whole, host, seconds = m.groups()
    return dict(k=int(k), variants=int(variants), copies=int(copies), builds=int(builds), whole=None if whole is None else int(whole),
                host=int(host), seconds=float(seconds))


def scan_build(plan) -> str:
    """How the scan `plan` (scan()'s dict) builds its spiked copies: SCAN_BUILDS[0] unless --spikeScanBuild said otherwise."""
    return plan.get("build", SCAN_BUILDS[0])


def scan_entry(v, r, called: bool):
    """One replicate of the scan as sensitivity_line() and curve_line() take it: `r` dict(N, V0, S, READS, V1); no row is kept - a
    verdict stands where the .cut line would."""
    return r, None, ((v.ref, [v.alt]) if called else None)


def scan_sensitivity_line(v, target, per, lod=None) -> str:
    """sensitivity_line() without PI_MEAN and PI_MIN (the scan keeps no row); `lod`: the locus's LOD in the FULL-DEPTH output."""
    f = sensitivity_line(v, target, per).split("\t")[:len(SCAN_SENSITIVITY_HEADER)]
    if lod is not None:
        f.append("%.15g" % lod)
    return "\t".join(f)


def write_scan(out_prefix: str, loci, variants, targets, entries, lods=None) -> None:
    """The pages of --spikeScan.  `loci`: every locus of the target in order as (chrom, pos, index into `variants` or None for a locus
    skipped for its letter); entries[(i, t)]: the replicates of variant i at targets[t] (scan_entry); lods[i]: the full-depth
    output's LOD at variant i, with --lod.
      <outPrefix>.spikeScan.sensitivity.txt    a line per scanned locus and target (scan_sensitivity_line)
      <outPrefix>.spikeScan.curve.txt          curve_line per scanned locus
      <outPrefix>.spikeScan<t>.rate.bedgraph   chrom, pos - 1, pos, RATE of that target - the page's text - per scanned locus
      <outPrefix>.spikeScan.t95.bedgraph       chrom, pos - 1, pos, T95 - 1 where it is NA, as --lod writes "not detectable", and 1 at
                                               a skipped locus"""
    T = len(targets)
    rates, t95s = [[] for _ in range(T)], []
    i_rate, i_t95 = SCAN_SENSITIVITY_HEADER.index("RATE"), len(CURVE_HEADER) + T
    with open(out_prefix + ".spikeScan.sensitivity.txt", "w") as fs, open(out_prefix + ".spikeScan.curve.txt", "w") as fc:
        fs.write("\t".join(SCAN_SENSITIVITY_HEADER + (("LOD",) if lods is not None else ())) + "\n")
        fc.write("\t".join(curve_header(targets, lods is not None)) + "\n")
        for i, v in enumerate(variants):
            lod = None if lods is None else float(lods[i])
            for t, target in enumerate(targets):
                line = scan_sensitivity_line(v, target, entries[(i, t)], lod)
                rates[t].append(line.split("\t")[i_rate])
                fs.write(line + "\n")
            line = curve_line(v, entries[(i, 0)][0][0]["N"], targets, [entries[(i, t)] for t in range(T)], lod)
            t95s.append(line.split("\t")[i_t95])
            fc.write(line + "\n")
    for t, target in enumerate(targets):
        with open("%s.spikeScan%g.rate.bedgraph" % (out_prefix, target), "w") as fh:
            for chrom, pos, i in loci:
                if i is not None:
                    fh.write("%s\t%d\t%d\t%s\n" % (chrom, int(pos) - 1, int(pos), rates[t][i]))
    with open(out_prefix + ".spikeScan.t95.bedgraph", "w") as fh:
        for chrom, pos, i in loci:
            fh.write("%s\t%d\t%d\t%s\n" % (chrom, int(pos) - 1, int(pos), "1" if i is None or t95s[i] == dsaf.NA else t95s[i]))


# ---- --spikeScanMnv: the scan's pages when an MNV - one phase set of L member SNVs - is planted at every locus
SCAN_MNV_CURVE_HEADER = ("CHROM", "POS", "REF", "ALT", "N_ALL")


def scan_mnv_curve_header(targets):
    return SCAN_MNV_CURVE_HEADER + curve_header(targets)[len(CURVE_HEADER):]


def scan_mnv_variant(pset, variants):
    """The MNV of set `pset` as one variant at the leader's position: REF and ALT the members' letters."""
    vs = [variants[k] for k in pset.members]
    ref, alt = "".join(v.ref for v in vs), "".join(v.alt for v in vs)
    return af.Variant(vs[0].chrom, vs[0].pos, ref, alt, alt, af.SNV)


def write_scan_mnv(out_prefix: str, loci, variants, sets, targets, mt_depth: int, entries) -> None:
    """The pages of --spikeScanMnv.  `loci`: every locus of the target in order as (chrom, pos, index into `sets` or None for a skipped
    locus); `variants`: the member SNVs `sets` index; entries[(i, t)]: the replicates of set i at targets[t] as phase_sensitivity_line
    takes them - (dict(N_ALL, V0_ALL, S_ALL, V1_ALL), CALLED_ALL).
      <outPrefix>.spikeScan.mnv.sensitivity.txt   PHASE_SENSITIVITY_HEADER, then per scanned leader and target the line the set has at
                                                  that target, FRACTION `full`, in .spikeAF.phase.sensitivity.txt of the pass's own run
      <outPrefix>.spikeScan.mnv.curve.txt         CHROM POS REF ALT N_ALL, RATE@<t> ascending, T95: curve_line over the joint verdicts,
                                                  REF and ALT the L letters, N_ALL the joint barcodes at full depth
      <outPrefix>.spikeScan<t>.mnv.rate.bedgraph  chrom, pos - 1, pos, RATE of that target - the page's text - at the leader's position
      <outPrefix>.spikeScan.mnv.t95.bedgraph      chrom, pos - 1, pos, T95 - 1 where it is NA and at a skipped locus, as write_scan
    No LOD column with --lod: a theoretical limit is a one-locus number."""
    T = len(targets)
    rates, t95s = [[] for _ in range(T)], []
    i_rate, i_t95 = PHASE_SENSITIVITY_HEADER.index("RATE"), len(SCAN_MNV_CURVE_HEADER) + T
    with open(out_prefix + ".spikeScan.mnv.sensitivity.txt", "w") as fs, open(out_prefix + ".spikeScan.mnv.curve.txt", "w") as fc:
        fs.write("\t".join(PHASE_SENSITIVITY_HEADER) + "\n")
        fc.write("\t".join(scan_mnv_curve_header(targets)) + "\n")
        for i, pset in enumerate(sets):
            v = scan_mnv_variant(pset, variants)
            for t, target in enumerate(targets):
                line = phase_sensitivity_line(pset, variants, target, None, mt_depth, entries[(i, t)])
                rates[t].append(line.split("\t")[i_rate])
                fs.write(line + "\n")
            line = curve_line(v, entries[(i, 0)][0][0]["N_ALL"], targets,
                              [[scan_entry(v, r, bool(called)) for r, called in entries[(i, t)]] for t in range(T)])
            t95s.append(line.split("\t")[i_t95])
            fc.write(line + "\n")
    for t, target in enumerate(targets):
        with open("%s.spikeScan%g.mnv.rate.bedgraph" % (out_prefix, target), "w") as fh:
            for chrom, pos, i in loci:
                if i is not None:
                    fh.write("%s\t%d\t%d\t%s\n" % (chrom, int(pos) - 1, int(pos), rates[t][i]))
    with open(out_prefix + ".spikeScan.mnv.t95.bedgraph", "w") as fh:
        for chrom, pos, i in loci:
            fh.write("%s\t%d\t%d\t%s\n" % (chrom, int(pos) - 1, int(pos), "1" if i is None or t95s[i] == dsaf.NA else t95s[i]))


# ---- --spikeScanDepth: the scan's pages per barcode depth
SCAN_DEPTH_SENSITIVITY_HEADER = tuple(c for c in DEPTH_SENSITIVITY_HEADER if c not in ("PI_MEAN", "PI_MIN"))
SCAN_NEED_HEADER = ("CHROM", "POS", "REF", "ALT", "TARGET", "N", "F95", "MTDEPTH95", "N95")


def scan_depth_mt(mt_depth: int, frac: float) -> int:
    """The mtDepth of a cell at fraction `frac`: what --dsMT f (and --spikeDepth f) gets from the run's mtDepth."""
    from .py2compat import py2_round
    return max(1, int(py2_round(frac * mt_depth)))


def scan_depth_sensitivity_line(v, target, frac, mt_depth, per) -> str:
    """depth_sensitivity_line() without PI_MEAN and PI_MIN (the scan keeps no row); N_MEAN stays."""
    f = depth_sensitivity_line(v, target, frac, mt_depth, per).split("\t")
    drop = {DEPTH_SENSITIVITY_HEADER.index(c) for c in ("PI_MEAN", "PI_MIN")}
    return "\t".join(x for n, x in enumerate(f) if n not in drop)


def f95(depths, rates):
    """dsaf.t95's rule on the depth axis: the smallest of `depths` (the listed fractions and 1 = full) whose rate is at least 0.95
    together with every larger depth's, or None when full depth fails -> the index into `depths`, or None."""
    best = dsaf.t95(depths, rates)
    return None if best is None else next(n for n, d in enumerate(depths) if d == best)


def need_line(v, target, n: int, depths, mt_depths, rates, n_means) -> str:
    """One line of the need page: variant `v` at `target` with N covering barcodes at full depth; depths / mt_depths / rates / n_means:
    per depth of the axis (the listed fractions, then 1 = full) its mtDepth, detection rate and mean covering barcodes."""
    k = f95(depths, rates)
    return "\t".join([v.chrom, "%d" % v.pos, v.ref, v.alt, dsaf.target_text(target), "%d" % n] +
                     ([dsaf.NA] * 3 if k is None else ["%g" % depths[k], "%d" % mt_depths[k], dsaf.frac_text(n_means[k])]))


def write_scan_depth(out_prefix: str, loci, variants, targets, fracs, mt_depth: int, full_entries, entries, mnv=None) -> None:
    """The pages of --spikeScanDepth.  loci, variants, targets: write_scan's; full_entries[(i, t)]: the full-depth replicates of variant
    i at targets[t] (write_scan's entries); entries[(i, t, f)]: those of the cell at fracs[f] (scan_entry with the cell's counters).
      <outPrefix>.spikeScan.depth.sensitivity.txt   a line per scanned locus, target and fraction (scan_depth_sensitivity_line)
      <outPrefix>.spikeScan.depth.curve.txt         depth_curve_line per scanned locus: full, then every fraction
      <outPrefix>.spikeScan<t>.dsMT<f>.rate.bedgraph  chrom, pos - 1, pos, RATE of the cell - the page's text - per scanned locus
      <outPrefix>.spikeScan.dsMT<f>.t95.bedgraph    chrom, pos - 1, pos, T95 at that depth; 1 where it is NA and at a skipped locus
      <outPrefix>.spikeScan.depth.need.txt          need_line per scanned locus and target
      <outPrefix>.spikeScan<t>.f95.bedgraph         chrom, pos - 1, pos, F95 of the target; 2 - above the axis - where it is NA and at
                                                    a skipped locus
    `mnv` (write_scan_mnv_depth: per variant and cell the line of its sensitivity page): the same pages of an MNV scan - `.mnv` in
    every name, PHASE_SENSITIVITY_HEADER on the sensitivity page, N_ALL for N on the need page."""
    T, F = len(targets), len(fracs)
    stem = "" if mnv is None else ".mnv"
    mts = [scan_depth_mt(mt_depth, f) for f in fracs]
    depths = list(fracs) + ([] if any(f == 1.0 for f in fracs) else [1.0])
    depth_mts = mts + ([] if len(depths) == F else [mt_depth])
    head = SCAN_DEPTH_SENSITIVITY_HEADER if mnv is None else PHASE_SENSITIVITY_HEADER
    i_rate = head.index("RATE")
    i_t95 = len(DEPTH_CURVE_HEADER) + T
    rates = {}                                   # (t, f) -> per variant the page's RATE text
    t95s = [[] for _ in range(F)]
    f95s = [[] for _ in range(T)]
    with open("%s.spikeScan%s.depth.sensitivity.txt" % (out_prefix, stem), "w") as fs, \
            open("%s.spikeScan%s.depth.curve.txt" % (out_prefix, stem), "w") as fc, \
            open("%s.spikeScan%s.depth.need.txt" % (out_prefix, stem), "w") as fn:
        fs.write("\t".join(head) + "\n")
        fc.write("\t".join(depth_curve_header(targets)) + "\n")
        fn.write("\t".join(SCAN_NEED_HEADER if mnv is None else SCAN_MNV_NEED_HEADER) + "\n")
        for i, v in enumerate(variants):
            for t, target in enumerate(targets):
                for f, frac in enumerate(fracs):
                    line = scan_depth_sensitivity_line(v, target, frac, mts[f], entries[(i, t, f)]) if mnv is None else mnv[(i, t, f)]
                    rates.setdefault((t, f), []).append(line.split("\t")[i_rate])
                    fs.write(line + "\n")
                # (the axis: the listed fractions; full depth stands for 1 where 1 is not listed)
                per = [entries[(i, t, f)] for f in range(F)] + ([] if len(depths) == F else [full_entries[(i, t)]])
                line = need_line(v, target, full_entries[(i, t)][0][0]["N"], depths, depth_mts,
                                 [float(_called(v, p)) / len(p) for p in per], [_n_mean(p) for p in per])
                f95s[t].append(line.split("\t")[SCAN_NEED_HEADER.index("F95")])
                fn.write(line + "\n")
            fc.write(depth_curve_line(v, None, [mt_depth] * T, targets, [full_entries[(i, t)] for t in range(T)]) + "\n")
            for f, frac in enumerate(fracs):
                line = depth_curve_line(v, frac, [mts[f]] * T, targets, [entries[(i, t, f)] for t in range(T)])
                t95s[f].append(line.split("\t")[i_t95])
                fc.write(line + "\n")
    for t, target in enumerate(targets):
        for f, frac in enumerate(fracs):
            with open("%s.spikeScan%g.dsMT%g%s.rate.bedgraph" % (out_prefix, target, frac, stem), "w") as fh:
                for chrom, pos, i in loci:
                    if i is not None:
                        fh.write("%s\t%d\t%d\t%s\n" % (chrom, int(pos) - 1, int(pos), rates[(t, f)][i]))
        with open("%s.spikeScan%g%s.f95.bedgraph" % (out_prefix, target, stem), "w") as fh:
            for chrom, pos, i in loci:
                fh.write("%s\t%d\t%d\t%s\n" % (chrom, int(pos) - 1, int(pos), "2" if i is None or f95s[t][i] == dsaf.NA else f95s[t][i]))
    for f, frac in enumerate(fracs):
        with open("%s.spikeScan.dsMT%g%s.t95.bedgraph" % (out_prefix, frac, stem), "w") as fh:
            for chrom, pos, i in loci:
                fh.write("%s\t%d\t%d\t%s\n" % (chrom, int(pos) - 1, int(pos), "1" if i is None or t95s[f][i] == dsaf.NA else t95s[f][i]))


# ---- --spikeScanMnvDepth: the MNV scan's pages per barcode depth
SCAN_MNV_NEED_HEADER = tuple("N_ALL" if c == "N" else c for c in SCAN_NEED_HEADER)


def write_scan_mnv_depth(out_prefix: str, loci, variants, sets, targets, fracs, mt_depth: int, full_entries, entries) -> None:
    """The pages of --spikeScanMnvDepth.  loci, variants, sets, targets: write_scan_mnv's; full_entries[(i, t)]: the full-depth
    replicates of set i at targets[t] as phase_sensitivity_line takes them - (dict(N_ALL, V0_ALL, S_ALL, V1_ALL), CALLED_ALL);
    entries[(i, t, f)]: those of the cell at fracs[f].
      <outPrefix>.spikeScan.mnv.depth.sensitivity.txt   PHASE_SENSITIVITY_HEADER, then per scanned leader, target and fraction the
                                                        set's cell line in .spikeAF.phase.sensitivity.txt of the pass's own run
      <outPrefix>.spikeScan.mnv.depth.curve.txt         .spikeScan.depth.curve.txt's columns per leader - `full`, then every fraction -,
                                                        REF and ALT the L letters, N_MEAN the mean N_ALL of the cell
      <outPrefix>.spikeScan<t>.dsMT<f>.mnv.rate.bedgraph, .spikeScan.dsMT<f>.mnv.t95.bedgraph   as --spikeScanDepth's, over the joint rates
      <outPrefix>.spikeScan.mnv.depth.need.txt          SCAN_NEED_HEADER with N_ALL for N: F95 / MTDEPTH95 / N95 by need_line's rule over
                                                        the joint rates, N95 the mean N_ALL there
      <outPrefix>.spikeScan<t>.mnv.f95.bedgraph         F95 of the target; 2 where it is NA and at a skipped locus
    write_scan_depth with the joint counts standing where a variant's do."""
    mnvs = [scan_mnv_variant(pset, variants) for pset in sets]
    as_scan = lambda v, per: [scan_entry(v, dict(N=r["N_ALL"], V0=r["V0_ALL"], S=r["S_ALL"], READS=0, V1=r["V1_ALL"]), bool(c)) for r, c in per]
    mts = [scan_depth_mt(mt_depth, f) for f in fracs]
    lines = {(i, t, f): phase_sensitivity_line(sets[i], variants, targets[t], fracs[f], mts[f], per) for (i, t, f), per in entries.items()}
    write_scan_depth(out_prefix, loci, mnvs, targets, fracs, mt_depth, {(i, t): as_scan(mnvs[i], per) for (i, t), per in full_entries.items()},
                     {(i, t, f): as_scan(mnvs[i], per) for (i, t, f), per in entries.items()}, mnv=lines)


# ---- --spikeScanRpb: the scan's pages per reads-per-barcode target
SCAN_RPB_SENSITIVITY_HEADER = tuple(c for c in cell_sensitivity_header(RPB_AXIS) if c not in ("PI_MEAN", "PI_MIN"))
SCAN_RPB_NEED_HEADER = ("CHROM", "POS", "REF", "ALT", "TARGET", "N", "R95", "N95")


def r95(rpbs, rates, full_rate):
    """dsaf.t95's rule on the reads-per-barcode axis - the listed targets ascending, full depth on top: the smallest entry whose rate is
    at least 0.95 together with every larger entry's -> the index into `rpbs`, dsaf.FULL when only full depth passes, None when full
    depth fails."""
    top = float("inf")
    best = dsaf.t95(list(rpbs) + [top], list(rates) + [full_rate])
    return None if best is None else dsaf.FULL if best == top else next(n for n, r in enumerate(rpbs) if r == best)


def rpb_need_line(v, target, n: int, rpbs, rates, n_means, full_rate, full_n_mean) -> str:
    """One line of the reads-per-barcode need page: variant `v` at `target` with N covering barcodes at full depth; rates / n_means: per
    listed reads-per-barcode target its detection rate and mean covering barcodes; full_rate / full_n_mean: those of full depth."""
    k = r95(rpbs, rates, full_rate)
    return "\t".join([v.chrom, "%d" % v.pos, v.ref, v.alt, dsaf.target_text(target), "%d" % n] +
                     ([dsaf.NA] * 2 if k is None else [dsaf.FULL, dsaf.frac_text(full_n_mean)] if k == dsaf.FULL else
                      ["%g" % rpbs[k], dsaf.frac_text(n_means[k])]))


def write_scan_rpb(out_prefix: str, loci, variants, targets, rpbs, mt_depth: int, run_rpb: float, full_entries, entries, mnv=None) -> None:
    """The pages of --spikeScanRpb.  loci, variants, targets, full_entries: write_scan_depth's; entries[(i, t, r)]: the replicates of the
    cell at rpbs[r] (scan_entry with the cell's counters); mt_depth, run_rpb: the run's --mtDepth (every cell is called at it) and --rpb.
      <outPrefix>.spikeScan.rpb.sensitivity.txt     a line per scanned locus, target and r: the pass's .spikeAF.rpb.sensitivity.txt line
                                                    without PI_MEAN and PI_MIN (scan_depth_sensitivity_line)
      <outPrefix>.spikeScan.rpb.curve.txt           depth_curve_line per scanned locus: full, then every r
      <outPrefix>.spikeScan<t>.dsRpb<r>.rate.bedgraph  chrom, pos - 1, pos, RATE of the cell - the page's text - per scanned locus
      <outPrefix>.spikeScan.dsRpb<r>.t95.bedgraph   chrom, pos - 1, pos, T95 at that r; 1 where it is NA and at a skipped locus
      <outPrefix>.spikeScan.rpb.need.txt            rpb_need_line per scanned locus and target
      <outPrefix>.spikeScan<t>.r95.bedgraph         chrom, pos - 1, pos, R95 of the target as a number: `full` as run_rpb; twice the
                                                    larger of run_rpb and the largest listed r - above the axis - where it is NA and
                                                    at a skipped locus
    `mnv` (write_scan_mnv_rpb: per variant and cell the line of its sensitivity page): the same pages of an MNV scan - `.mnv` in every
    name, phase_sensitivity_header(RPB_AXIS) on the sensitivity page, N_ALL for N on the need page."""
    T, Rr = len(targets), len(rpbs)
    stem = "" if mnv is None else ".mnv"
    head = SCAN_RPB_SENSITIVITY_HEADER if mnv is None else phase_sensitivity_header(RPB_AXIS)
    i_rate = head.index("RATE")
    i_t95 = len(DEPTH_CURVE_HEADER) + T
    i_r95 = SCAN_RPB_NEED_HEADER.index("R95")
    above = "%g" % (2.0 * max([float(run_rpb)] + [float(r) for r in rpbs]))
    rates = {}                                   # (t, r) -> per variant the page's RATE text
    t95s = [[] for _ in range(Rr)]
    r95s = [[] for _ in range(T)]
    rate = lambda v, per: float(_called(v, per)) / len(per)
    with open("%s.spikeScan%s.rpb.sensitivity.txt" % (out_prefix, stem), "w") as fs, \
            open("%s.spikeScan%s.rpb.curve.txt" % (out_prefix, stem), "w") as fc, open("%s.spikeScan%s.rpb.need.txt" % (out_prefix, stem), "w") as fn:
        fs.write("\t".join(head) + "\n")
        fc.write("\t".join(depth_curve_header(targets, False, RPB_AXIS)) + "\n")
        fn.write("\t".join(SCAN_RPB_NEED_HEADER if mnv is None else SCAN_MNV_RPB_NEED_HEADER) + "\n")
        for i, v in enumerate(variants):
            for t, target in enumerate(targets):
                for r, rpb in enumerate(rpbs):
                    line = scan_depth_sensitivity_line(v, target, rpb, mt_depth, entries[(i, t, r)]) if mnv is None else mnv[(i, t, r)]
                    rates.setdefault((t, r), []).append(line.split("\t")[i_rate])
                    fs.write(line + "\n")
                per, full = [entries[(i, t, r)] for r in range(Rr)], full_entries[(i, t)]
                line = rpb_need_line(v, target, full[0][0]["N"], rpbs, [rate(v, p) for p in per], [_n_mean(p) for p in per], rate(v, full),
                                     _n_mean(full))
                r95s[t].append(line.split("\t")[i_r95])
                fn.write(line + "\n")
            fc.write(depth_curve_line(v, None, [mt_depth] * T, targets, [full_entries[(i, t)] for t in range(T)]) + "\n")
            for r, rpb in enumerate(rpbs):
                line = depth_curve_line(v, rpb, [mt_depth] * T, targets, [entries[(i, t, r)] for t in range(T)])
                t95s[r].append(line.split("\t")[i_t95])
                fc.write(line + "\n")
    for t, target in enumerate(targets):
        for r, rpb in enumerate(rpbs):
            with open("%s.spikeScan%g.dsRpb%g%s.rate.bedgraph" % (out_prefix, target, rpb, stem), "w") as fh:
                for chrom, pos, i in loci:
                    if i is not None:
                        fh.write("%s\t%d\t%d\t%s\n" % (chrom, int(pos) - 1, int(pos), rates[(t, r)][i]))
        with open("%s.spikeScan%g%s.r95.bedgraph" % (out_prefix, target, stem), "w") as fh:
            for chrom, pos, i in loci:
                text = above if i is None or r95s[t][i] == dsaf.NA else "%g" % run_rpb if r95s[t][i] == dsaf.FULL else r95s[t][i]
                fh.write("%s\t%d\t%d\t%s\n" % (chrom, int(pos) - 1, int(pos), text))
    for r, rpb in enumerate(rpbs):
        with open("%s.spikeScan.dsRpb%g%s.t95.bedgraph" % (out_prefix, rpb, stem), "w") as fh:
            for chrom, pos, i in loci:
                fh.write("%s\t%d\t%d\t%s\n" % (chrom, int(pos) - 1, int(pos), "1" if i is None or t95s[r][i] == dsaf.NA else t95s[r][i]))


# ---- --spikeScanMnvRpb: the MNV scan's pages per reads-per-barcode target
SCAN_MNV_RPB_NEED_HEADER = tuple("N_ALL" if c == "N" else c for c in SCAN_RPB_NEED_HEADER)


def write_scan_mnv_rpb(out_prefix: str, loci, variants, sets, targets, rpbs, mt_depth: int, run_rpb: float, full_entries, entries) -> None:
    """The pages of --spikeScanMnvRpb.  loci, variants, sets, targets, full_entries: write_scan_mnv_depth's; entries[(i, t, r)]: the
    replicates of the cell at rpbs[r], (dict(N_ALL, V0_ALL, S_ALL, V1_ALL), CALLED_ALL); mt_depth, run_rpb: write_scan_rpb's.
      <outPrefix>.spikeScan.mnv.rpb.sensitivity.txt   phase_sensitivity_header(RPB_AXIS), then per scanned leader, target and r the set's
                                                      cell line in .spikeAF.rpb.phase.sensitivity.txt of the pass's own run
      <outPrefix>.spikeScan.mnv.rpb.curve.txt         .spikeScan.rpb.curve.txt's columns per leader - `full`, then every r -, REF and ALT
                                                      the L letters, N_MEAN the mean N_ALL' of the cell
      <outPrefix>.spikeScan<t>.dsRpb<r>.mnv.rate.bedgraph, .spikeScan.dsRpb<r>.mnv.t95.bedgraph   as --spikeScanRpb's, over the joint rates
      <outPrefix>.spikeScan.mnv.rpb.need.txt          SCAN_RPB_NEED_HEADER with N_ALL for N: R95 / N95 by rpb_need_line's rule over the
                                                      joint rates, N95 the mean N_ALL' there
      <outPrefix>.spikeScan<t>.mnv.r95.bedgraph       R95 of the target, with the fill values of .spikeScan<t>.r95.bedgraph
    write_scan_rpb with the joint counts standing where a variant's do."""
    mnvs = [scan_mnv_variant(pset, variants) for pset in sets]
    as_scan = lambda v, per: [scan_entry(v, dict(N=r["N_ALL"], V0=r["V0_ALL"], S=r["S_ALL"], READS=0, V1=r["V1_ALL"]), bool(c)) for r, c in per]
    lines = {(i, t, r): phase_sensitivity_line(sets[i], variants, targets[t], rpbs[r], mt_depth, per) for (i, t, r), per in entries.items()}
    write_scan_rpb(out_prefix, loci, mnvs, targets, rpbs, mt_depth, run_rpb, {(i, t): as_scan(mnvs[i], per) for (i, t), per in full_entries.items()},
                   {(i, t, r): as_scan(mnvs[i], per) for (i, t, r), per in entries.items()}, mnv=lines)


# ---- --spikeScanFilter: the scan's rates over the replicates that are called AND PASS, and a tally per FILTER name
SCAN_FILTER_NAMES = tuple(name for _, name in _abi.SCAN_FILTER_NAMES)
SCAN_FILTER_HEADER = ("CHROM", "POS", "REF", "ALT", "TARGET", "REPS", "CALLED", "PASS", "RATE_PASS", "LO95", "HI95") + SCAN_FILTER_NAMES
_FILTER_BIT = {name: bit for bit, name in _abi.SCAN_FILTER_NAMES}
# (postfilter.load_repeat_regions' flag texts: RepeatMasker's Low_complexity is the LowC the low-complexity window gives)
_REPEAT_BIT = {"RepT": _abi.F_REPT, "RepS": _abi.F_REPS, "SL": _abi.F_SL, "Other_Repeat": _abi.F_OTHER_REPEAT, "LowC": _abi.F_LOWC}
SCAN_FILTER_PI_EDGE = 4.995     # round(PI, 2) >= 5 above it; py2's round decides within +- 1e-6 (smc_scan_filter's band)


def _repeat_bits(regions, chrom: str, pos: int) -> int:
    """The names the FIRST interval of `regions` with lo < pos <= hi holds (postfilter._apply_one's rule), as bits."""
    for lo, hi, flag in regions.get(chrom, ()):
        if lo < pos <= hi:
            bits = 0
            for name in flag.split(";"):
                if name:
                    bits |= _REPEAT_BIT[name]
            return bits
    return 0


def scan_filter_words(variants, hp_len: int, refprov, trf, rm):
    """The two words per listed variant smc_scan_filter takes -> (gate, always), uint32 [len(variants)] each.  gate: F_HP and / or
    F_LOWC of hpregion.is_hp_or_lowcomp on the variant's REF and ALT - rows.filter_string sets them where cand.vmf_lt_099; always:
    the names postfilter.apply_repeat_filters appends at the position from the run's `trf` / `rm` regions
    (postfilter.load_repeat_regions), RepeatMasker's LowC as F_LOWC.  Constants of the variant: nothing of a row is read."""
    import numpy as np
    from .hpregion import is_hp_or_lowcomp
    gate, always = np.zeros(len(variants), np.uint32), np.zeros(len(variants), np.uint32)
    for i, v in enumerate(variants):
        homop, lowcomp = is_hp_or_lowcomp(v.chrom, str(int(v.pos)), hp_len, v.ref, v.alt, refprov)
        gate[i] = (_abi.F_HP if homop else 0) | (_abi.F_LOWC if lowcomp else 0)
        always[i] = _repeat_bits(trf, v.chrom, int(v.pos)) | _repeat_bits(rm, v.chrom, int(v.pos))
    return gate, always


def scan_filter_host(row, gate: int, always: int) -> int:
    """k_scan_filter's word for one abi.ROW_DTYPE record, on the host: the same comparisons on the same doubles."""
    c0 = row["cand"][0]
    applied, pi = int(c0["flt_applied"]), float(c0["pi"])
    lo, hi = SCAN_FILTER_PI_EDGE - 1e-6, SCAN_FILTER_PI_EDGE + 1e-6
    w = 0
    if applied != 0:
        w = (int(c0["flt"]) & _abi.SCAN_FLT_DEVICE_MASK) | (int(gate) if int(c0["vmf_lt_099"]) != 0 else 0)
    if pi > hi:
        w |= int(always)
    if int(row["status"]) != 0 or int(row["biallelic"]) != 0 or not (pi < lo or pi > hi) or applied not in (0, 1):
        w |= _abi.SCAN_FLT_HOST
    return w


def scan_filter_of_text(text: str) -> int:
    """A printed FILTER column (after postfilter.apply_repeat_filters: PASS, or names joined by ';') as the word of its names' bits - a
    name counts once.  ValueError: a name that is none of the 14 (Zero_Coverage: no called row holds it)."""
    if text == "PASS":
        return 0
    w = 0
    for name in text.split(";"):
        if name not in _FILTER_BIT:
            raise ValueError("FILTER %r holds %r, none of %s" % (text, name, " ".join(SCAN_FILTER_NAMES)))
        w |= _FILTER_BIT[name]
    return w


def scan_filter_tally(called, words):
    """-> (replicates called, those whose word is 0 = PASS, per name of SCAN_FILTER_NAMES the called replicates whose word holds it)."""
    hit = [int(w) & _abi.SCAN_FLT_NAMES_MASK for c, w in zip(called, words) if c]
    return len(hit), sum(1 for w in hit if w == 0), [sum(1 for w in hit if w & bit) for bit, _ in _abi.SCAN_FILTER_NAMES]


def scan_filter_line(v, target, called, words) -> str:
    """One line of the filter page: variant `v` at `target`; called[j] / words[j]: replicate j's verdict and, where it is called, its
    FILTER word.  RATE_PASS = PASS / REPS with its Wilson interval (dsaf.wilson, as the sensitivity pages'), then the tally."""
    n = len(called)
    n_called, n_pass, tally = scan_filter_tally(called, words)
    lo, hi = dsaf.wilson(n_pass, n)
    return "\t".join([v.chrom, "%d" % v.pos, v.ref, v.alt, dsaf.target_text(target), "%d" % n, "%d" % n_called, "%d" % n_pass,
                      dsaf.frac_text(float(n_pass) / n), dsaf.frac_text(lo), dsaf.frac_text(hi)] + ["%d" % x for x in tally])


def scan_filter_curve_header(targets, first=CURVE_HEADER):
    return first + tuple("RATE_PASS@%g" % t for t in sorted(targets)) + ("T95_PASS",)


def scan_filter_curve_line(v, n: int, targets, rates) -> str:
    """curve_line() on the PASS rates: rates[t] of targets[t]; T95_PASS by dsaf.t95's rule."""
    best = dsaf.t95(targets, rates)
    return "\t".join([v.chrom, "%d" % v.pos, v.ref, v.alt, "%d" % n] +
                     [dsaf.frac_text(rates[t]) for t in sorted(range(len(targets)), key=lambda t: targets[t])] +
                     [dsaf.NA if best is None else "%g" % best])


def write_scan_filter(out_prefix: str, loci, variants, targets, ns, called, words, mnv: bool = False) -> None:
    """The pages of --spikeScanFilter.  loci, variants, targets: write_scan's; ns[i]: variant i's covering barcodes; called[i][t] /
    words[i][t]: per replicate the verdict and the FILTER word of variant i at targets[t].
      <outPrefix>.spikeScan.filter.txt            scan_filter_line per scanned locus and target
      <outPrefix>.spikeScan.filter.curve.txt      scan_filter_curve_line per scanned locus
      <outPrefix>.spikeScan<t>.passrate.bedgraph  chrom, pos - 1, pos, RATE_PASS of that target - the page's text - per scanned locus
      <outPrefix>.spikeScan.t95pass.bedgraph      chrom, pos - 1, pos, T95_PASS; 1 where it is NA and at a skipped locus
    `mnv` (write_scan_mnv_filter): the same pages of an MNV scan - `.mnv` in every name (.spikeScan.mnv.filter.txt, ...), the headers
    SCAN_MNV_FILTER_HEADER and SCAN_MNV_CURVE_HEADER's."""
    T = len(targets)
    rates, t95s = [[] for _ in range(T)], []
    stem, head, first = (".mnv", SCAN_MNV_FILTER_HEADER, SCAN_MNV_CURVE_HEADER) if mnv else ("", SCAN_FILTER_HEADER, CURVE_HEADER)
    i_rate, i_t95 = head.index("RATE_PASS"), len(first) + T
    with open("%s.spikeScan%s.filter.txt" % (out_prefix, stem), "w") as fs, open("%s.spikeScan%s.filter.curve.txt" % (out_prefix, stem), "w") as fc:
        fs.write("\t".join(head) + "\n")
        fc.write("\t".join(scan_filter_curve_header(targets, first)) + "\n")
        for i, v in enumerate(variants):
            mine = []
            for t, target in enumerate(targets):
                line = scan_filter_line(v, target, called[i][t], words[i][t])
                rates[t].append(line.split("\t")[i_rate])
                mine.append(float(scan_filter_tally(called[i][t], words[i][t])[1]) / len(called[i][t]))
                fs.write(line + "\n")
            line = scan_filter_curve_line(v, int(ns[i]), targets, mine)
            t95s.append(line.split("\t")[i_t95])
            fc.write(line + "\n")
    for t, target in enumerate(targets):
        with open("%s.spikeScan%g%s.passrate.bedgraph" % (out_prefix, target, stem), "w") as fh:
            for chrom, pos, i in loci:
                if i is not None:
                    fh.write("%s\t%d\t%d\t%s\n" % (chrom, int(pos) - 1, int(pos), rates[t][i]))
    with open("%s.spikeScan%s.t95pass.bedgraph" % (out_prefix, stem), "w") as fh:
        for chrom, pos, i in loci:
            fh.write("%s\t%d\t%d\t%s\n" % (chrom, int(pos) - 1, int(pos), "1" if i is None or t95s[i] == dsaf.NA else t95s[i]))


# ---- --spikeScanMnvFilter: the filter pages of an MNV scan - a set is PASS when every member is called and every member's FILTER is PASS
SCAN_MNV_FILTER_HEADER = tuple({"CALLED": "CALLED_ALL", "PASS": "PASS_ALL"}.get(c, c) for c in SCAN_FILTER_HEADER)


def write_scan_mnv_filter(out_prefix: str, loci, variants, sets, targets, n_alls, called, words) -> None:
    """The pages of --spikeScanMnvFilter.  loci, variants, sets: write_scan_mnv's; n_alls[i]: set i's joint barcodes at full depth;
    called[i][t] / words[i][t]: per replicate the joint verdict of set i at targets[t] and, where it is called, the joint FILTER word
    (abi.scan_filter_joint_rule: the OR of the members' names - a name counts once per replicate).
      <outPrefix>.spikeScan.mnv.filter.txt            CHROM POS REF ALT as .spikeScan.mnv.curve.txt has them, TARGET REPS CALLED_ALL
                                                      PASS_ALL RATE_PASS LO95 HI95 and the 14 names: scan_filter_line on the joint words
      <outPrefix>.spikeScan.mnv.filter.curve.txt      CHROM POS REF ALT N_ALL, RATE_PASS@<t> ascending, T95_PASS
      <outPrefix>.spikeScan<t>.mnv.passrate.bedgraph  RATE_PASS of that target at the leader's position
      <outPrefix>.spikeScan.mnv.t95pass.bedgraph      T95_PASS; 1 where it is NA and at a skipped locus"""
    write_scan_filter(out_prefix, loci, [scan_mnv_variant(pset, variants) for pset in sets], targets, n_alls, called, words, mnv=True)


def scan_filter_cells_header(axis=DEPTH_AXIS, head=SCAN_FILTER_HEADER):
    return head[:5] + (axis[1], "MTDEPTH") + head[5:]


def write_scan_filter_cells(out_prefix: str, variants, targets, values, mt_depths, called, words, axis=DEPTH_AXIS, mnv: bool = False) -> None:
    """<outPrefix>.spikeScan.depth.filter.txt (axis RPB_AXIS: .spikeScan.rpb.filter.txt): scan_filter_line per scanned locus, target
    and cell with the axis column and MTDEPTH behind TARGET.  values / mt_depths: the cells' fractions (reads-per-barcode targets)
    and mtDepths; called[i][t][f] / words[i][t][f]: per replicate.  `mnv`: <outPrefix>.spikeScan.mnv.depth.filter.txt of an MNV scan -
    `variants` the sets' MNVs (scan_mnv_variant), the joint verdicts and words, CALLED_ALL and PASS_ALL in the header."""
    with open("%s.spikeScan%s.%s.filter.txt" % (out_prefix, ".mnv" if mnv else "", axis[0]), "w") as fh:
        fh.write("\t".join(scan_filter_cells_header(axis, SCAN_MNV_FILTER_HEADER if mnv else SCAN_FILTER_HEADER)) + "\n")
        for i, v in enumerate(variants):
            for t, target in enumerate(targets):
                for f, value in enumerate(values):
                    fh.write("\t".join(_cell_fields(scan_filter_line(v, target, called[i][t][f], words[i][t][f]), value, mt_depths[f])) + "\n")
