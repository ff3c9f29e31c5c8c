"""Command line of the MI355X build: the reference's flags, inputs and output files
(smCounter.py:616-640 argParseInit, :645-909 main), with the per-locus worker pool replaced by batched
launches on one GPU.

    python -m smcounter_amd.cli --outPrefix example --bamFile example.bam --bedTarget example.bed \\
        --mtDepth 3612 --rpb 8.6 --refGenome hg19.fasta [...]

Differences that do not change results: `--nCPU` is accepted and ignored (the pool is gone);
`--bedtoolsPath` is accepted and ignored (merge/sort/intersect run in-process, bedops.py); when the two
repeat BEDs are absent the repeat flags are skipped with a note instead of failing inside bedtools.
"""
from __future__ import annotations

import argparse
import datetime
import os
import sys

from . import _lib, bamio, bedops, fasta, postfilter, runlog, vc, writers
from . import dist as smcdist
from .params import VcParams


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Variant calling using molecular barcodes (MI355X build)",
                                fromfile_prefix_chars="@")
    p.add_argument("--outPrefix", default=None, required=True, help="prefix for output files")
    p.add_argument("--bamFile", default=None, required=True, help="BAM file")
    p.add_argument("--bedTarget", default=None, required=True, help="BED file for target region")
    p.add_argument("--mtDepth", default=None, required=True, type=int, help="Mean MT depth")
    p.add_argument("--rpb", default=None, required=True, type=float, help="Mean read pairs per MT")
    p.add_argument("--nCPU", type=int, default=1, help="ignored: loci are batched onto the GPU")
    p.add_argument("--minBQ", type=int, default=20, help="minimum base quality allowed for analysis")
    p.add_argument("--minMQ", type=int, default=30, help="minimum mapping quality allowed for analysis")
    p.add_argument("--hpLen", type=int, default=10, help="Minimum length for homopolymers")
    p.add_argument("--mismatchThr", type=float, default=6.0, help="average number of mismatches per 100 bases allowed")
    p.add_argument("--mtDrop", type=int, default=0, help="Drop MTs with lower than or equal to X reads.")
    p.add_argument("--maxMT", type=int, default=0, help="Randomly downsample to X MTs; 0 = 2.0 * mean MT depth")
    p.add_argument("--primerDist", type=int, default=2, help="filter variants that are within X bases to primer")
    p.add_argument("--threshold", type=int, default=0, help="Minimum prediction index for a variant to be called; "
                                                             "0 = chosen from the mean MT depth")
    p.add_argument("--refGenome", default=None, required=False, help="indexed FASTA of the reference genome")
    p.add_argument("--bedTandemRepeats", default=None, help="bed for UCSC tandem repeats")
    p.add_argument("--bedRepeatMaskerSubset", default=None, help="bed for RepeatMasker simple repeats, low complexity, "
                                                                  "microsatellite regions")
    p.add_argument("--bedtoolsPath", default=None, help="ignored: BED operations run in-process")
    p.add_argument("--runPath", default=None, help="path to working directory")
    p.add_argument("--logFile", default=None, help="log file")
    p.add_argument("--paramFile", default=None, help="optional parameter file; if given it replaces every other "
                                                     "parameter except --logFile")
    p.add_argument("--device", type=int, default=0, help="GPU index (single process only: under torch.distributed.run "
                                                          "every rank uses GPU LOCAL_RANK and this flag is ignored)")
    p.add_argument("--batchReads", type=int, default=4_000_000, help="pileup reads per device batch")
    p.add_argument("--sampler", choices=("reference", "philox"), default="reference",
                   help="how a locus with more UMIs than the cap (maxMT, or 2 x mtDepth) is down-sampled.  reference (default): as "
                        "smCounter.py:496-498 does - Python 2's random.sample over the barcode texts, seeded with the position string, "
                        "reproduced on the host (the same rows as smCounter).  philox: on the GPU, a counter-based generator "
                        "(Philox4x32-10) keyed by position and --samplerSeed - NOT the reference's sample: the rows of such loci differ "
                        "from smCounter's (another random subset of the same size); the same for every run, launch shape and GPU count")
    p.add_argument("--samplerSeed", type=int, default=0, help="seed of --sampler philox")
    p.add_argument("--dsMT", default=None, help="in-run molecule down-sampling: comma-separated fractions f in (0, 1].  For each, the "
                                                "run is also called as if on the BAM that ds.mt.py --pct f --seed dsSeed writes (each barcode "
                                                "kept with probability f), at --mtDepth round(f x mtDepth); written to "
                                                "<outPrefix>.dsMT<f>.smCounter.{all,cut}.txt and .cut.vcf.  The BAM is decoded once; the "
                                                "drop is done on the GPU (needs the device plane builder; one process only)")
    p.add_argument("--dsSampler", choices=("reference", "philox"), default="reference",
                   help="which barcodes --dsMT keeps.  reference (default): exactly ds.mt.py's set - every placed read of the file, "
                        "barcodes in Python 2 dict order, one random.random() each, kept when r <= f.  philox: on the GPU, a "
                        "counter-based draw (Philox4x32-10) keyed by --dsSeed and a hash of the barcode text, kept when it falls below "
                        "f - NOT the reference's sample (another random subset of about the same size; nested across fractions), "
                        "without the pass over the whole file")
    p.add_argument("--dsSeed", type=int, default=1234567, help="seed of --dsMT (ds.mt.py --seed)")
    p.add_argument("--dsMtDepth", default=None, help="comma-separated --mtDepth of each --dsMT fraction; default "
                                                     "max(1, round(f x mtDepth)) (sets that fraction's maxMT default and its threshold)")
    p.add_argument("--dsRpb", default=None, help="in-run read down-sampling within barcodes: comma-separated targets r > 0 of mean "
                                                 "reads per barcode.  For each, the run is also called as if on the BAM that "
                                                 "ds.reads.withinMT.py --rpb r --seed dsSeed writes (whole read names kept: a barcode's "
                                                 "first always, every further one with the reference's probKeep), with --rpb r; written "
                                                 "to <outPrefix>.dsRpb<r>.smCounter.{all,cut}.txt and .cut.vcf.  The kept names are the "
                                                 "reference's exactly (one pass over the whole file, on the host); --dsSampler philox "
                                                 "is not available here (a shape-independent rule for reads needs the whole file's "
                                                 "first names and probKeep: see --dsRpbSampler).  With --dsMT: each target and each "
                                                 "fraction gets its own files from the same decode, no cross product.  Needs the device "
                                                 "plane builder; one process only")
    p.add_argument("--dsRpbMtDepth", default=None, help="comma-separated --mtDepth of each --dsRpb target; default --mtDepth")
    p.add_argument("--dsRpbSampler", choices=("reference", "philox"), default=None,
                   help="which read names --dsRpb keeps.  reference (default): exactly ds.reads.withinMT.py's set (the names grouped "
                        "and drawn on the host).  philox: the whole file's names grouped by barcode in a table on the GPU, probKeep "
                        "from its counts as the reference computes it, a barcode's first name always kept and every further one when a "
                        "counter-based draw (Philox4x32-10) keyed by --dsSeed and a hash of the full name falls below probKeep - NOT "
                        "the reference's sample (another random subset of about the same size; nested across targets), independent "
                        "of how the file is cut into runs.  Needs --dsRpb")
    p.add_argument("--dsGrid", action="store_true", default=False,
                   help="the cross product of --dsMT and --dsRpb: for every fraction f and every target r the run is also called as "
                        "if on the BAM that ds.mt.py --pct f, then ds.reads.withinMT.py --rpb r on its output (both --seed dsSeed) "
                        "write, at --mtDepth of f (--dsMtDepth, or max(1, round(f x mtDepth))) and --rpb r; written to "
                        "<outPrefix>.dsMT<f>.dsRpb<r>.smCounter.{all,cut}.txt and .cut.vcf, beside the files of every fraction and "
                        "target.  From the same decode.  --dsSampler and --dsRpbSampler both reference (the two scripts' names exactly) "
                        "or both philox (--dsSampler philox's barcodes, then --dsRpbSampler philox's rule with probKeep from the kept "
                        "barcodes' counts); at most %d cells.  Needs --dsMT and --dsRpb" % GRID_MAX_CELLS)
    p.add_argument("--dsAF", default=None, help="in-run dilution of listed variants: comma-separated target allele fractions t in (0, 1).  "
                                                "For each, the run is also called as if on the BAM that tools/ds_allele_fraction.py --af t "
                                                "--seed dsSeed writes for the variants of --dsAFVariants: the barcodes that carry a listed "
                                                "allele (more than half of their reads at the locus show it) are dropped whole, each with the "
                                                "probability that brings its variant's barcode fraction down to t (a fraction is never raised; "
                                                "an absent variant, or one every covering barcode carries, is left alone and reported); "
                                                "written to <outPrefix>.dsAF<t>.smCounter.{all,cut}.txt and .cut.vcf, and, one line per "
                                                "variant and output, <outPrefix>.dsAF.detection.txt.  The carriers are found on the GPU in a "
                                                "pre-pass over the runs around the listed loci; the BAM is then decoded once.  Not together "
                                                "with --dsMT, --dsRpb or --dsGrid; needs the device plane builder; one process only")
    p.add_argument("--dsAFVariants", default=None, help="the variants --dsAF dilutes, one per line: VCF lines (CHROM POS ID REF ALT ...; a "
                                                        ".cut.vcf of this program can be fed back) or `chrom pos ref alt`, tab-separated, "
                                                        "pos 1-based, `#` lines skipped.  One-letter substitutions, insertions X / XS (at most "
                                                        "%d inserted letters) and deletions XD / X; one variant per position, each a locus of "
                                                        "--bedTarget" % AF_MAX_INS)
    p.add_argument("--dsAFMtDepth", default=None, help="comma-separated --mtDepth of each --dsAF target; default --mtDepth")
    p.add_argument("--dsAFReps", type=int, default=None,
                   help="replicate dilutions: R in %d .. %d.  Replicate j = 0 .. R - 1 is the dilution of --dsAF with seed (dsSeed + j) "
                        "mod 2^64 and everything else unchanged (replicate 0 is the run's own .dsAF<t> output at the listed loci).  The "
                        "replicates' barcode draws and achieved counts are made on the GPU from the pre-pass's carriers, and only the runs "
                        "around the listed loci are called again, R times per target.  Every other file stays as it is; added: "
                        "<outPrefix>.dsAF.replicates.txt, one line per listed variant, target and replicate (the line that variant has in "
                        ".dsAF.detection.txt of a run with --dsSeed of that replicate, with REP and SEED), and "
                        "<outPrefix>.dsAF.sensitivity.txt, one line per variant and target: replicates called, the detection rate and its "
                        "Wilson score interval (95 %%%%), the achieved fractions, and with --lod the locus's LOD.  Needs --dsAF" % (REPS_MIN, REPS_MAX))
    p.add_argument("--lod", action="store_true", default=False,
                   help="the theoretical limit of detection of every locus, as the reference's mt_depths_lod.R computes it from the "
                        "barcode depth (the smallest allele fraction whose variant barcodes reach ceiling((14 + 0.012 x mtDepth) / 3.5) "
                        "with probability 0.95), for the full-depth output and for every --dsMT fraction, --dsRpb target and "
                        "--dsGrid cell at that output's own mtDepth: <prefix>.lod.bedgraph and <prefix>.lod.bedgraph.quantiles.txt "
                        "beside each output's files, and <outPrefix>.lod.summary.txt, one line per output.  The table of LODs by "
                        "depth is made on the GPU.  One process only")
    p.add_argument("--lodDepth", choices=("UMT", "MT"), default=None,
                   help="the barcode depth --lod reads.  UMT (default): the barcodes that vote at the locus (after --mtDrop and the "
                        "cap), the UMT column of .smCounter.all.txt.  MT: every barcode, the MT column.  Needs --lod")
    return p


REPS_MIN, REPS_MAX = 2, 1000   # (--dsAFReps: dsaf.REPS_MIN / REPS_MAX, SMC_AF_REP_MAX_REPS)
AF_MAX_INS = 255             # (smc_allele_carriers: SMC_AF_MAX_INS letters per listed insertion)
GRID_MAX_CELLS = 32          # (a launch takes at most SMC_RG_MAX_TARGETS masks; every cell holds a batch's device arrays)


def ds_fractions(args):
    """--dsMT / --dsMtDepth -> [(f, mtDepth of f, output prefix)]; [] without --dsMT."""
    from .py2compat import py2_round
    text = getattr(args, "dsMT", None)
    if text in (None, ""):
        return []
    try:
        fr = [float(x) for x in str(text).split(",") if x.strip()]
    except ValueError:
        raise SystemExit("--dsMT: comma-separated fractions in (0, 1] expected, got %r" % text)
    if not fr or any(not (0.0 < f <= 1.0) for f in fr):
        raise SystemExit("--dsMT: every fraction must lie in (0, 1], got %r" % text)
    dtext = getattr(args, "dsMtDepth", None)
    if dtext not in (None, ""):
        try:
            depths = [int(x) for x in str(dtext).split(",") if x.strip()]
        except ValueError:
            raise SystemExit("--dsMtDepth: comma-separated integers expected, got %r" % dtext)
        if len(depths) != len(fr):
            raise SystemExit("--dsMtDepth: %d depths for %d --dsMT fractions" % (len(depths), len(fr)))
    else:
        depths = [max(1, int(py2_round(f * args.mtDepth))) for f in fr]
    return [(f, d, "%s.dsMT%g" % (args.outPrefix, f)) for f, d in zip(fr, depths)]


def ds_rpb_targets(args):
    """--dsRpb / --dsRpbMtDepth -> [(r, mtDepth of r, output prefix)]; [] without --dsRpb."""
    text = getattr(args, "dsRpb", None)
    if text in (None, ""):
        if getattr(args, "dsRpbSampler", None) is not None:
            raise SystemExit("--dsRpbSampler chooses the read names --dsRpb keeps: it needs --dsRpb")
        return []
    try:
        rs = [float(x) for x in str(text).split(",") if x.strip()]
    except ValueError:
        raise SystemExit("--dsRpb: comma-separated reads-per-barcode targets > 0 expected, got %r" % text)
    if not rs or any(not (r > 0.0 and r < float("inf")) for r in rs):
        raise SystemExit("--dsRpb: every target must be a number > 0, got %r" % text)
    dtext = getattr(args, "dsRpbMtDepth", None)
    if dtext not in (None, ""):
        try:
            depths = [int(x) for x in str(dtext).split(",") if x.strip()]
        except ValueError:
            raise SystemExit("--dsRpbMtDepth: comma-separated integers expected, got %r" % dtext)
        if len(depths) != len(rs):
            raise SystemExit("--dsRpbMtDepth: %d depths for %d --dsRpb targets" % (len(depths), len(rs)))
    else:
        depths = [int(args.mtDepth)] * len(rs)
    if getattr(args, "dsSampler", "reference") == "philox" and not getattr(args, "dsGrid", False):
        # (--dsGrid decides on the pair of samplers itself: ds_grid_cells)
        raise SystemExit("--dsRpb keeps the reference's read names only: --dsSampler philox is not available with it (a rule for "
                         "reads that does not depend on how the file is cut into runs needs the whole file's first names and probKeep; "
                         "--dsRpbSampler philox is that rule)")
    return [(r, d, "%s.dsRpb%g" % (args.outPrefix, r)) for r, d in zip(rs, depths)]


def ds_af_targets(args):
    """--dsAF / --dsAFVariants / --dsAFMtDepth -> [(t, mtDepth of t, output prefix)]; [] without --dsAF.  Refused: one of --dsAF and
    --dsAFVariants without the other, a target outside (0, 1), --dsAF beside --dsMT, --dsRpb or --dsGrid."""
    from .tools import ds_allele_fraction as af
    text, vfile = getattr(args, "dsAF", None), getattr(args, "dsAFVariants", None)
    if text in (None, ""):
        if vfile not in (None, ""):
            raise SystemExit("--dsAFVariants lists the variants --dsAF dilutes: it needs --dsAF")
        if getattr(args, "dsAFMtDepth", None) not in (None, ""):
            raise SystemExit("--dsAFMtDepth gives the mtDepth of each --dsAF target: it needs --dsAF")
        return []
    if vfile in (None, ""):
        raise SystemExit("--dsAF dilutes listed variants: it needs --dsAFVariants")
    try:
        ts = af.parse_targets(text, "--dsAF")
    except ValueError as e:
        raise SystemExit(str(e))
    other = [f for f in ("dsMT", "dsRpb", "dsGrid") if getattr(args, f, None) not in (None, "", False)]
    if other:
        raise SystemExit("--dsAF cannot be combined with --%s in one run (the cross product is not built)" % other[0])
    dtext = getattr(args, "dsAFMtDepth", None)
    if dtext not in (None, ""):
        try:
            depths = [int(x) for x in str(dtext).split(",") if x.strip()]
        except ValueError:
            raise SystemExit("--dsAFMtDepth: comma-separated integers expected, got %r" % dtext)
        if len(depths) != len(ts):
            raise SystemExit("--dsAFMtDepth: %d depths for %d --dsAF targets" % (len(depths), len(ts)))
    else:
        depths = [int(args.mtDepth)] * len(ts)
    return [(t, d, "%s.dsAF%g" % (args.outPrefix, t)) for t, d in zip(ts, depths)]


def ds_af_reps(args, af_targets):
    """--dsAFReps -> R, or None without the flag.  Refused: without --dsAF, R outside REPS_MIN .. REPS_MAX."""
    reps = getattr(args, "dsAFReps", None)
    if reps in (None, ""):
        return None
    if not af_targets:
        raise SystemExit("--dsAFReps replicates the dilutions of --dsAF: it needs --dsAF")
    try:
        reps = int(reps)
    except ValueError:
        raise SystemExit("--dsAFReps: an integer in %d .. %d expected, got %r" % (REPS_MIN, REPS_MAX, reps))
    if not (REPS_MIN <= reps <= REPS_MAX):
        raise SystemExit("--dsAFReps: the number of replicates must lie in %d .. %d, got %d" % (REPS_MIN, REPS_MAX, reps))
    return reps


def ds_af_variants(args, loc_list):
    """The variants of --dsAFVariants, checked: the file's own refusals (tools.ds_allele_fraction.parse_variants) and every variant a
    locus of --bedTarget."""
    from . import dsaf
    from .tools import ds_allele_fraction as af
    try:
        variants = af.parse_variants(args.dsAFVariants)
        dsaf.check_variants(variants, loc_list)
    except (ValueError, OSError) as e:
        raise SystemExit(str(e))
    return variants


def ds_af_rules(args, params: VcParams, af_targets, variants, early, keep=None):
    """The devplanes.DsRule of every --dsAF target (the pre-pass on the GPU: devplanes.ds_af_rules) and the titration's numbers; the
    run log gets a line per variant and target.  `keep` (--dsAFReps): a dict for what the replicate stage starts from."""
    import dataclasses
    from . import devplanes
    from .tools import ds_allele_fraction as af
    plist = [dataclasses.replace(params, mtDepth=d) for _, d, _ in af_targets]
    if early is not None:
        eng = early.get()
    else:
        from .engine import Engine
        eng = _ENGINES.get(args.device) or _ENGINES.setdefault(args.device, Engine(args.device))
    try:
        rules, res = devplanes.ds_af_rules(args.bamFile, fasta.FastaFile(args.refGenome), variants, [t for t, _, _ in af_targets], plist,
                                           int(args.dsSeed), eng, keep=keep)
    except (ValueError, bamio.BamError) as e:
        raise SystemExit(str(e))
    for r in res:
        for v, row in zip(variants, r["rows"]):
            print(af.report_line(v, r["target"], row))
        print("--dsAF %g: seed %d, %d barcodes dropped" % (r["target"], int(args.dsSeed), len(r["dropped"])))
    return rules, res


def ds_grid_cells(args):
    """--dsGrid -> [(f, r, mtDepth of f, output prefix)] for every --dsMT fraction f and --dsRpb target r (fractions outer); [] without
    --dsGrid.  Refused: without both --dsMT and --dsRpb, with one philox and one reference sampler, beyond GRID_MAX_CELLS cells."""
    if not getattr(args, "dsGrid", False):
        return []
    fractions, targets = ds_fractions(args), ds_rpb_targets(args)
    if not fractions or not targets:
        raise SystemExit("--dsGrid calls every --dsMT fraction with every --dsRpb target: it needs both --dsMT and --dsRpb")
    bs, rs = getattr(args, "dsSampler", "reference") or "reference", getattr(args, "dsRpbSampler", None) or "reference"
    if bs != rs:
        raise SystemExit("--dsGrid needs --dsSampler and --dsRpbSampler to be the same sampler (both reference or both philox), got "
                         "--dsSampler %s and --dsRpbSampler %s" % (bs, rs))
    if len(fractions) * len(targets) > GRID_MAX_CELLS:
        raise SystemExit("--dsGrid: %d fractions x %d targets = %d cells, at most %d" % (len(fractions), len(targets),
                                                                                          len(fractions) * len(targets), GRID_MAX_CELLS))
    return [(f, r, d, "%s.dsMT%g.dsRpb%g" % (args.outPrefix, f, r)) for f, d, _ in fractions for r, _, _ in targets]


def ds_grid_rules(args, params: VcParams, cells, frac_rules, rpb_rules, grouped=None):
    """The devplanes.DsRule of every --dsGrid cell, after the fractions' and the targets' rules: the reference's names from the
    fractions' kept barcodes and the targets' grouping (`grouped`), or with the philox samplers from the targets' file-wide table; a
    cell whose kept barcodes have no barcode of two or more reads ends the run with a message."""
    import dataclasses
    from . import devplanes
    plist = [dataclasses.replace(params, mtDepth=d, rpb=r) for _, r, d, _ in cells]
    fr = [(f, r) for f, r, _, _ in cells]
    try:
        if (getattr(args, "dsRpbSampler", None) or "reference") == "philox":
            return devplanes.philox_grid_rules(args.bamFile, fr, plist, int(args.dsSeed), rpb_rules[0].groups)
        kept = {rule.frac: rule.kept for rule in frac_rules}
        return devplanes.reference_grid_rules(args.bamFile, fr, plist, int(args.dsSeed), kept, grouped)
    except ValueError as e:
        raise SystemExit(str(e))


def ds_rpb_rules(args, params: VcParams, targets, early=None, grouped=None):
    """The devplanes.DsRule of every --dsRpb target: the reference's read names (one pass over the whole file, here), or with
    --dsRpbSampler philox the file-wide table on the GPU (`early`: the engine coming up; else the process's engine); a file without a
    barcode of two or more reads, or whose names collide in the table's hashes, ends the run with a message."""
    import dataclasses
    from . import devplanes
    plist = [dataclasses.replace(params, mtDepth=d, rpb=r) for r, d, _ in targets]
    rs = [r for r, _, _ in targets]
    try:
        if (getattr(args, "dsRpbSampler", None) or "reference") == "philox":
            if early is not None:
                eng = early.get()
            else:
                from .engine import Engine
                eng = _ENGINES.get(args.device) or _ENGINES.setdefault(args.device, Engine(args.device))
            return devplanes.philox_read_rules(args.bamFile, rs, plist, int(args.dsSeed), eng)
        if grouped is not None:
            return devplanes.reference_read_rules(args.bamFile, rs, plist, int(args.dsSeed), grouped=grouped)
        return devplanes.reference_read_rules(args.bamFile, rs, plist, int(args.dsSeed))
    except ValueError as e:
        raise SystemExit(str(e))


def ds_rules(args, params: VcParams, fractions):
    """The devplanes.DsRule of every --dsMT fraction (the reference's sampler: one pass over the whole file, here)."""
    import dataclasses
    from . import devplanes
    plist = [dataclasses.replace(params, mtDepth=d) for _, d, _ in fractions]
    fr = [f for f, _, _ in fractions]
    if getattr(args, "dsSampler", "reference") == "philox":
        return [devplanes.DsRule(f, P, kept=None, seed=int(args.dsSeed)) for f, P in zip(fr, plist)]
    return devplanes.reference_rules(args.bamFile, fr, plist, int(args.dsSeed))


class _EarlyEngine(object):
    """Engine(device) created in a helper thread (binding the library, bringing up the GPU runtime, the context and its
    tables: ctypes calls, the interpreter lock is free meanwhile); get() joins and hands it over, or re-raises."""

    def __init__(self, device: int):
        import threading
        self._eng = self._err = None

        def work():
            try:
                from . import _lib
                from .engine import Engine
                _lib.load(with_torch=False)
                self._eng = _ENGINES.pop(device, None) or Engine(device)
            except BaseException as e:
                self._err = e
        self._t = threading.Thread(target=work, daemon=True)
        self._t.start()

    def get(self):
        self._t.join()
        if self._err is not None:
            raise self._err
        return self._eng


_ENGINES = {}          # device -> Engine kept for the process's next run (smc_create + the first allocations are ~ 0.1 s)


def _release_engine(eng):
    """The engine stays with the process: a second main() in the same process finds the context, its tables and its buffers
    again, and the command line does not spend 20 ms of its wall time freeing device memory the exiting process gives back
    anyway (SMC_CLOSE_ENGINE=1: close it, as round 2 did)."""
    if _lib.exp_env("SMC_CLOSE_ENGINE"):
        _ENGINES.pop(eng.device, None)
        eng.close()
    else:
        _ENGINES[eng.device] = eng


def call_shard(args, params: VcParams, loci, device: int, early=None):
    """The per-locus rows (strings, smCounter.py:599) of a run of loci: BAM decode -> device batches -> kernels."""
    from .engine import Engine
    ref = fasta.FastaFile(args.refGenome)
    eng = early.get() if early is not None else (_ENGINES.pop(device, None) or Engine(device))
    output = _Rows()
    decoder = os.environ.get("SMC_BAM_DECODER", "native")
    rules = getattr(args, "ds_rules", None) or None
    # (--lod: three int32 columns of every output's rows, full depth first, and the tables while the engine is alive)
    lod_cols = None
    if getattr(args, "lod", False):
        from . import lod as _lod
        lod_cols = [_lod.DepthCols() for _ in range(1 + len(rules or ()))]
    # (one process per GPU: the ranks of a node share its cores for decoding)
    # (LOCAL_WORLD_SIZE: WORLD_SIZE also counts the ranks of other nodes, which do not share these cores)
    per_node = int(os.environ.get("LOCAL_WORLD_SIZE") or os.environ.get("WORLD_SIZE", "1"))
    nthreads = bamio.host_threads(per_node)
    if rules is None and decoder == "python":                         # readable decoder, same batches
        batches = bamio.iter_pileup_batches(bamio.BamFile(args.bamFile), ref, loci, max_reads=args.batchReads)
    elif rules is None and os.environ.get("SMC_PLANES", "device") == "host":   # planes built by the host threads, then uploaded
        batches = bamio.iter_device_batches_native(args.bamFile, ref, loci, params, max_reads=args.batchReads,
                                                   nthreads=nthreads)
    else:
        # default: the host decodes alignments, the GPU builds the planes from them (k_build_planes) and they stay in HBM
        from . import devplanes
        # (a batch only lives in HBM here - 16 B per read - so it can be eight times the host-built default)
        # (--dsMT: the same batches at full depth and for every fraction - the device builder only, SMC_PLANES=host or
        # SMC_BAM_DECODER=python end with an error naming the first run)
        batches = devplanes.iter_resident_batches(args.bamFile, ref, loci, params, eng, max_reads=32 * args.batchReads,
                                                  nthreads=nthreads, all_planes=False, sampler=getattr(args, "sampler", "reference"),
                                                  sampler_seed=getattr(args, "samplerSeed", 0), ds_rules=rules,
                                                  force_host=rules is not None and (decoder == "python" or
                                                                                    os.environ.get("SMC_PLANES", "device") == "host"))
        # (a batch ahead in a helper thread: decoding and building batch i + 1 overlaps the kernels and the strings of batch i;
        # the two threads use different staging buffers of the engine, device work is ordered by the default stream)
        if not _lib.exp_env("SMC_NO_PREFETCH"):
            batches = _prefetch(batches, depth=1)
        ds_out = [_Rows() for _ in (rules or ())]
        for first, rb in batches:
            if rules is not None:
                rb, rbs = rb[0], rb[1:]
                for k, (rule, o, b) in enumerate(zip(rules, ds_out, rbs)):
                    o.add(vc.vc_resident(b, rule.params, ref, eng))
                    if lod_cols is not None:
                        lod_cols[1 + k].add(eng.last_rows)
            output.add(vc.vc_resident(rb, params, ref, eng))
            if lod_cols is not None:
                lod_cols[0].add(eng.last_rows)
            _report_boundary(eng.last_rows, rb.chrom, rb.pos)
        if getattr(args, "ds_af_keep", None) is not None:
            output.af_reps = _ds_af_replicates(args, rules, ref, eng, loci, ds_out)
        if lod_cols is not None:
            output.lod = _lod.run_lods(eng, [params] + [rule.params for rule in rules or ()], lod_cols, args.lodDepth or "UMT")
        _release_engine(eng)
        output.ds = [o.done() for o in ds_out]
        return output.done()
    for first, pb in _prefetch(batches):
        output.add(vc.vc_batch(pb, params, ref, eng=eng))
        if lod_cols is not None:
            lod_cols[0].add(eng.last_rows)
    if lod_cols is not None:
        output.lod = _lod.run_lods(eng, [params], lod_cols, args.lodDepth or "UMT")
    eng.close()
    return output.done()


def _ds_af_replicates(args, rules, ref, eng, loci, ds_out):
    """--dsAFReps after the run's batches: devplanes.ds_af_replicates over the runs the pre-pass kept, and the check that ties it to
    the run's own outputs - replicate 0 has the seed of the run, so its row at every listed locus must be the .dsAF<t> output's."""
    from . import devplanes
    variants, res = args.ds_af
    keep, args.ds_af_keep = args.ds_af_keep, None
    out = devplanes.ds_af_replicates(args.bamFile, ref, variants, [rule.af for rule in rules], [rule.params for rule in rules],
                                     int(args.dsSeed), int(args.ds_af_reps), eng, keep, res, sampler=getattr(args, "sampler", "reference"),
                                     sampler_seed=getattr(args, "samplerSeed", 0))
    index = {(c, int(p)): n for n, (c, p) in enumerate(loci)}
    for (k, t, j), line in out["rows"].items():
        v = variants[k]
        if j == 0 and line != ds_out[t][index[(v.chrom, v.pos)]]:
            raise RuntimeError("--dsAFReps: replicate 0 of %s:%d at target %g is not the row of the run's own output:\n%s\n%s" %
                               (v.chrom, v.pos, rules[t].af, line, ds_out[t][index[(v.chrom, v.pos)]]))
    return out


def call_shard_rows(args, params: VcParams, loci, device: int):
    """A rank's share as NUMBERS: (rows abi.ROW_DTYPE[n], reference letters, allele tables) - the distributed command line
    sends these to rank 0 (packed: dist.pack_shard) which prints every row; no strings are made on the other ranks."""
    import numpy as np
    from . import abi, devplanes
    from .engine import Engine
    if not len(loci):
        return np.zeros(0, abi.ROW_DTYPE), [], []
    ref = fasta.FastaFile(args.refGenome)
    eng = Engine(device)
    per_node = int(os.environ.get("LOCAL_WORLD_SIZE") or os.environ.get("WORLD_SIZE", "1"))
    nthreads = bamio.host_threads(per_node)
    parts, refs, tables = [], [], []
    try:
        if os.environ.get("SMC_PLANES", "device") == "host":
            for _, db in bamio.iter_device_batches_native(args.bamFile, ref, loci, params, max_reads=args.batchReads, nthreads=nthreads):
                parts.append(eng.call_batch_host(db, params)); refs += list(db.ref); tables += list(db.alleles)
        else:
            batches = devplanes.iter_resident_batches(args.bamFile, ref, loci, params, eng, max_reads=32 * args.batchReads,
                                                      nthreads=nthreads, all_planes=False, sampler=getattr(args, "sampler", "reference"),
                                                      sampler_seed=getattr(args, "samplerSeed", 0))
            for _, rb in _prefetch(batches, depth=1):
                parts.append(vc.vc_resident_rows(rb, params, eng)); refs += list(rb.ref); tables += list(rb.alleles)
    finally:
        eng.close()
    return (np.concatenate(parts) if parts else np.zeros(0, abi.ROW_DTYPE)), refs, tables


def _report_boundary(out_rows, chrom, pos):
    """Log the loci whose PI lies within 1e-8 of a printing / gating boundary (rows.pi_boundary_loci): their text may differ
    from the reference's in the last printed digit or in the FILTER gate although the numbers agree to ~ 3e-9."""
    if out_rows is None:
        return
    from . import rows as _rows
    idx = _rows.pi_boundary_loci(out_rows)
    for l in idx.tolist():
        print("note: prediction index of %s:%d lies within 1e-8 of a printing boundary" % (chrom[l], int(pos[l])), file=sys.stderr)
    import numpy as np
    from . import abi
    for l in np.flatnonzero((out_rows["status"] & abi.ST_UNDERFLOW) != 0).tolist():
        print("note: a barcode at %s:%d has so many fragments that the posterior arithmetic left the double range; the "
              "reference's own numbers there depend on its multiplication order" % (chrom[l], int(pos[l])), file=sys.stderr)


class _Rows(list):
    """The shard's row strings; keeps the native printer's per-row int(PI) (rows.RowLines.pred) alongside when every batch
    came with one, for the post-filter and the writers."""
    pred = None

    def __init__(self):
        super().__init__()
        self._parts = []

    def add(self, part):
        self.extend(part)
        self._parts.append(getattr(part, "pred", None))

    def done(self):
        if self._parts and all(p is not None for p in self._parts):
            import numpy as np
            self.pred = np.concatenate(self._parts)
        return self


def _prefetch(it, depth: int = 2):
    """Run a batch generator in a helper thread, `depth` batches ahead: the native decoder releases the GIL, so
    decoding batch i + 1 overlaps the GPU call and the string formatting of batch i."""
    import queue
    import threading
    q = queue.Queue(maxsize=depth)
    done = object()

    def work():
        try:
            for item in it:
                q.put(item)
            q.put(done)
        except BaseException as e:          # re-raised in the consumer
            q.put(e)
    threading.Thread(target=work, daemon=True).start()
    while True:
        item = q.get()
        if item is done:
            return
        if isinstance(item, BaseException):
            raise item
        yield item


def main(args) -> int:
    """Same contract as the reference's main(args): accepts a Namespace or a dict of argument values,
    returns the PI threshold used (smCounter.py:909)."""
    # The run builds a few long lists of strings and no reference cycles: the cyclic collector would only rescan them, again
    # and again (several milliseconds per 20,000 loci).  Off for the duration of the call.
    import gc
    gc_was_on = gc.isenabled()
    gc.disable()
    try:
        return _main(args)
    finally:
        if gc_was_on:
            gc.enable()


def _main(args) -> int:
    t0 = datetime.datetime.now()
    print("smCounter started at " + str(t0))
    parser = build_parser()
    if not isinstance(args, argparse.Namespace):
        args = parser.parse_args(["--{0}={1}".format(k, v) for k, v in args.items()])
    elif args.paramFile is not None:
        args = parser.parse_args(("@" + args.paramFile,))
    for k, v in vars(args).items():
        print((k, v))
    if args.runPath is not None:
        os.chdir(args.runPath)
    if not args.refGenome:
        raise SystemExit("--refGenome is required (indexed FASTA)")

    params = VcParams(minBQ=args.minBQ, minMQ=args.minMQ, mtDepth=args.mtDepth, rpb=args.rpb, hpLen=args.hpLen,
                      mismatchThr=args.mismatchThr, mtDrop=args.mtDrop, maxMT=args.maxMT, primerDist=args.primerDist)
    fractions = ds_fractions(args)
    targets = ds_rpb_targets(args)
    cells = ds_grid_cells(args)
    af_targets = ds_af_targets(args)
    args.ds_af_reps = ds_af_reps(args, af_targets)
    flag = " / ".join(f for f, on in (("--dsMT", fractions), ("--dsRpb", targets), ("--dsAF", af_targets)) if on)
    if flag and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("%s runs in one process only (not under torch.distributed.run with more than one rank)" % flag)
    if getattr(args, "lodDepth", None) is not None and not getattr(args, "lod", False):
        raise SystemExit("--lodDepth chooses the barcode depth --lod reads: it needs --lod")
    if getattr(args, "lod", False) and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--lod runs in one process only (not under torch.distributed.run with more than one rank): the writing rank "
                         "prints from gathered wire rows after its engine is gone, and the table of LODs is made on the GPU")
    host = [v for v, on in (("SMC_PLANES=host", os.environ.get("SMC_PLANES", "device") == "host"),
                            ("SMC_BAM_DECODER=python", os.environ.get("SMC_BAM_DECODER", "native") == "python")) if on]
    if flag and host:
        first = bedops.expand_loci(args.bedTarget)[:1]
        raise SystemExit("%s needs the device builder: the run at %s would be built on the host (%s)" %
                         (flag, "%s:%s" % first[0] if first else "(no targets)", host[0]))
    early = None
    if int(os.environ.get("WORLD_SIZE", "1")) == 1 and os.environ.get("SMC_BAM_DECODER", "native") != "python":
        # a single process: the GPU runtime and the context come up (~ 0.1 s) in a helper thread while the target is expanded
        early = _EarlyEngine(args.device)
    loc_list = bedops.expand_loci(args.bedTarget)
    rules = []
    args.ds_af = args.ds_af_keep = None
    try:
        if af_targets:
            # (--dsAF: the listed variants checked, then the pre-pass over the runs around them; --dsAFReps: its runs kept)
            variants = ds_af_variants(args, loc_list)
            keep = {} if args.ds_af_reps is not None else None
            rules, res = ds_af_rules(args, params, af_targets, variants, early, keep)
            args.ds_af = (variants, res)
            args.ds_af_keep = keep
        elif cells:
            # (--dsGrid: the reference's grouping of the names once, for the targets and the cells alike)
            from . import devplanes
            grouped = None if (args.dsRpbSampler or "reference") == "philox" else devplanes.group_placed_reads(args.bamFile)
            frac_rules = ds_rules(args, params, fractions)
            rules = frac_rules + ds_rpb_rules(args, params, targets, early, grouped=grouped)
            rules += ds_grid_rules(args, params, cells, frac_rules, rules[len(frac_rules):], grouped)
        else:
            rules = (ds_rules(args, params, fractions) if fractions else []) + (ds_rpb_rules(args, params, targets, early) if targets else [])
    except SystemExit:
        from . import devplanes
        devplanes.close_rules(rules)          # (a refused cell: the targets' file-wide table in HBM)
        if early is not None:                  # (the engine the helper brings up stays with the process, as after a run)
            try:
                _ENGINES.setdefault(args.device, early.get())
            except Exception:
                pass
        raise
    for rule in rules:
        if rule.grid:
            print("--dsGrid fraction %g x target %g: sampler %s, seed %d, probKeep %.6g, %d of %d read names kept (mtDepth %d)" %
                  (rule.frac, rule.target, rule.sampler, rule.seed, rule.prob_keep, len(rule.kept) if rule.kept is not None else rule.n_kept,
                   rule.n_names, rule.params.mtDepth))
        elif rule.level == "read":
            print("--dsRpb %g: sampler %s, seed %d, probKeep %.6g, %d of %d read names kept (mtDepth %d)" %
                  (rule.target, rule.sampler, rule.seed, rule.prob_keep, len(rule.kept) if rule.kept is not None else rule.n_kept,
                   rule.n_names, rule.params.mtDepth))
    args.ds_rules = rules or None
    try:
        return _run(args, params, fractions, targets, loc_list, early, t0, cells, af_targets)
    finally:
        from . import devplanes
        devplanes.close_rules(rules)          # (--dsRpbSampler philox: the file-wide table in HBM, whatever happened)
        if args.ds_af_keep is not None:       # (--dsAFReps: the pre-pass's runs, when the run ended before the replicate stage)
            devplanes.free_af_runs(args.ds_af_keep.get("runs"))


def _run(args, params, fractions, targets, loc_list, early, t0, cells=(), af_targets=()):
    # One process per GPU when launched through torch.distributed.run: rank r calls a contiguous range of the
    # ordered locus list (loci share nothing, smCounter.py:683-685) on GPU LOCAL_RANK, rank 0 gathers the rows
    # in submission order and writes the files.
    rank, local_rank, world = smcdist.init_from_env()
    if world == 1:
        # a single process never touches torch.distributed: bind the C ABI without importing PyTorch first
        # (about a second of start-up; the host-buffer entry point needs none of it)
        from . import _lib
        _lib.load(with_torch=False)
    if world > 1:
        # contiguous ranges balanced by depth, not by locus count (amplicon depth varies several-fold): the BAI's
        # linear index gives compressed bytes per 16 kb window without decoding anything; every rank computes the
        # same cuts
        cuts = smcdist.shard_by_reads(bamio.locus_weights(args.bamFile, loc_list), world)
        lo, hi = cuts[rank], cuts[rank + 1]
    else:
        lo, hi = 0, len(loc_list)
    if world == 1:
        output = call_shard(args, params, loc_list[lo:hi], args.device, **({"early": early} if early is not None else {}))
        vc.raise_on_exception(output, loc_list[lo:hi])
    else:
        # A failing locus (or a decoder error) on one rank must not leave the others waiting in the collective
        # until the RCCL timeout: every rank first agrees on a status, then all raise together or all gather.
        import torch.distributed as tdist
        import numpy as np
        import torch
        from . import abi
        err, payload = None, None
        try:
            r_rows, r_ref, r_tab = call_shard_rows(args, params, loc_list[lo:hi], local_rank)
            if len(r_rows) != hi - lo:
                raise RuntimeError("%d rows for %d loci" % (len(r_rows), hi - lo))
            payload = smcdist.pack_shard(abi.pack_wire(r_rows), r_ref, r_tab)
        except Exception as e:                       # reported by every rank below
            err = "rank %d: %s: %s" % (rank, type(e).__name__, e)
        try:
            failed = [m for m in smcdist.all_gather_status(err) if m]
            if failed:
                raise RuntimeError("smCounter failed on %d of %d ranks: %s" % (len(failed), world, " | ".join(failed)))
            # ONE gather of byte blocks: 168-byte wire rows + the rank's allele-string table; a rank whose
            # share is empty sends an empty table
            t = torch.from_numpy(payload)
            if tdist.get_backend() == "nccl":
                t = t.to(torch.device("cuda", local_rank))
            blocks = smcdist.gatherv_bytes(t, dst=0)
            tdist.barrier()
        finally:
            if tdist.is_initialized():
                tdist.destroy_process_group()
        if rank != 0:
            return writers.pi_threshold(args.mtDepth, args.threshold)
        wires, refs, tabs = [], [], []
        for b in blocks:
            w, rf, tb = smcdist.unpack_shard(b.cpu().numpy())
            wires.append(w); refs += rf; tabs += tb
        all_rows = abi.unpack_wire(np.concatenate(wires)) if wires else np.zeros(0, abi.ROW_DTYPE)
        view = vc.LocusView([c for c, _ in loc_list], [int(p) for _, p in loc_list], refs, tabs)
        output = vc._strings(all_rows, view, params, fasta.FastaFile(args.refGenome))
        _report_boundary(all_rows, view.chrom, view.pos)
        vc.raise_on_exception(output, loc_list)

    print("begin variant filtering and output")
    have_rep = [b for b in (args.bedTandemRepeats, args.bedRepeatMaskerSubset) if b and os.path.exists(b)]
    if len(have_rep) < 2:
        print("note: repeat tracks not given or not found; RepT/RepS/LowC/SL flags are not applied", file=sys.stderr)
    trf, rm = postfilter.load_repeat_regions(
        args.bedTarget,
        args.bedTandemRepeats if args.bedTandemRepeats and os.path.exists(args.bedTandemRepeats) else None,
        args.bedRepeatMaskerSubset if args.bedRepeatMaskerSubset and os.path.exists(args.bedRepeatMaskerSubset) else None)
    pred = getattr(output, "pred", None)                  # (single process: the printer's int(PI) per row)
    ds_outputs = getattr(output, "ds", None) or []        # (--dsMT / --dsRpb: the rows of every fraction, then of every target)
    lods = getattr(output, "lod", None)                   # (--lod: per output, in the same order, what lod.run_lods made)
    lod_entries = []

    def write_lod(k, prefix, mt_depth, rpb):
        # the LOD files of output k beside the files just written, its line in the run log and its entry for the summary
        from . import lod as _lod
        o = lods[k]
        _lod.write_lod(prefix, [c for c, _ in loc_list], [p for _, p in loc_list], o["lods"])
        print("--lod %s: %d barcodes needed (mtDepth %d), depth %s, table of %d depths, at most %d iterations" %
              (prefix, o["needed"], mt_depth, args.lodDepth or "UMT", o["table"], o["iters"]))
        lod_entries.append(_lod.summary_entry(prefix, mt_depth, rpb, o["needed"], o["rows"], args.lodDepth or "UMT", o["lods"]))
    output_raw = output                                   # (--dsAFReps: the replicates' rows hang on the shard's rows)
    output = postfilter.apply_repeat_filters(output, trf, rm, pred=pred)
    threshold = writers.pi_threshold(args.mtDepth, args.threshold)
    writers.write_outputs(args.outPrefix, output, threshold, pred=pred)
    if lods is not None:
        write_lod(0, args.outPrefix, args.mtDepth, args.rpb)
    # (--dsGrid: the cells' rows after them, each at its fraction's mtDepth)
    # (the reads per barcode an output was called with, for --lod's summary: --rpb for a fraction, r for a target or a cell)
    # (--dsAF: its targets alone - it is not combined with the other three - each at its mtDepth and the run's --rpb)
    rpbs = [args.rpb] * len(fractions) + [r for r, _, _ in targets] + [r for _, r, _, _ in cells] + [args.rpb] * len(af_targets)
    for k, ((d, prefix), o) in enumerate(zip([(d, p) for _, d, p in fractions + targets] + [(d, p) for _, _, d, p in cells] +
                                             [(d, p) for _, d, p in af_targets], ds_outputs)):
        vc.raise_on_exception(o, loc_list)
        o_pred = getattr(o, "pred", None)
        o = postfilter.apply_repeat_filters(o, trf, rm, pred=o_pred)
        writers.write_outputs(prefix, o, writers.pi_threshold(d, args.threshold), pred=o_pred)
        if lods is not None:
            write_lod(1 + k, prefix, d, rpbs[k])
    if lods is not None:
        from . import lod as _lod
        _lod.write_summary(args.outPrefix, lod_entries)
    if af_targets:
        # the titration on one page: every listed variant in the full-depth output and in every target's
        from . import dsaf
        variants, res = args.ds_af
        outs = [(None, args.outPrefix, None, lods[0]["lods"] if lods is not None else None)] + \
               [(t, p, r["rows"], lods[1 + k]["lods"] if lods is not None else None) for k, ((t, _, p), r) in enumerate(zip(af_targets, res))]
        loc_index = {(c, "%d" % int(q)): n for n, (c, q) in enumerate(loc_list)}
        dsaf.write_detection(args.outPrefix, variants, outs, loc_index)
        reps = getattr(output_raw, "af_reps", None)
        if reps is not None:
            # (--dsAFReps: every replicate's row as its own run would print and cut it, then the rates)
            entries = {}
            for i, v in enumerate(variants):
                for t, (target, d, _) in enumerate(af_targets):
                    thr_t = writers.pi_threshold(d, args.threshold)
                    per = []
                    for j in range(args.ds_af_reps):
                        row, cut = dsaf.replicate_entry(reps["rows"].get((i, t, j)), thr_t, trf, rm)
                        per.append((int(reps["counts"][i, j, t, 0]), int(reps["counts"][i, j, t, 1]), row, cut))
                    entries[(i, t)] = per
                    called = sum(1 for _, _, _, cut in per if cut is not None and cut[0] == v.ref and v.alt in cut[1])
                    print("--dsAFReps: %s:%d %s>%s at %g: called %d of %d" % (v.chrom, v.pos, v.ref, v.alt, target, called, args.ds_af_reps))
            targets_only = [t for t, _, _ in af_targets]
            dsaf.write_replicates(args.outPrefix, variants, targets_only, reps["seeds"], [[row["k"] for row in r["rows"]] for r in res], entries)
            lod_vt = None
            if lods is not None:
                lod_vt = [[float(lods[1 + t]["lods"][loc_index[(v.chrom, "%d" % v.pos)]]) for v in variants] for t in range(len(af_targets))]
            dsaf.write_sensitivity(args.outPrefix, variants, targets_only, entries, lod_vt)
            tm = reps["times"]
            print("--dsAFReps: replicate stage %.3f s (%d replicates x %d targets: %d builds in %d batches; counts %.4f s, masks %.4f s)" %
                  (tm["stage"], args.ds_af_reps, len(af_targets), tm["builds"], tm["batches"], tm["counts"], tm["masks"]))
    t1 = datetime.datetime.now()
    print("smCounter completed running at " + str(t1))
    print("smCounter total time: " + str(t1 - t0))
    return threshold


if __name__ == "__main__":
    ns = build_parser().parse_args()
    if ns.logFile:
        runlog.init(ns.logFile)
    try:
        main(ns)
    finally:
        runlog.close()
