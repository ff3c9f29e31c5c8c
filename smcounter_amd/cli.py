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
import collections
import dataclasses
import datetime
import os
import sys

import numpy as np

from . import _lib, abi, bamio, bedops, devplanes, fasta, postfilter, runlog, vc, writers
from . import dist as smcdist
from .engine import Engine
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
    p.add_argument("--dsAFDepth", default=None,
                   help="the dilutions of --dsAF at several barcode depths: comma-separated fractions f in (0, 1].  For every target t "
                        "and every f the run is also called on the CELL (t, f): a barcode stays when the --dsAF rule at t keeps it and "
                        "the --dsMT --dsSampler philox draw keeps it at f (two independent draws, both keyed by --dsSeed) - the .dsMT<f> "
                        "output of a --dsMT f --dsSampler philox run on the BAM tools/ds_allele_fraction.py --af t writes, at the "
                        "mtDepth --dsMT f would get from that target's mtDepth (max(1, round(f x mtDepth))); written to "
                        "<outPrefix>.dsAF<t>.dsMT<f>.smCounter.{all,cut}.txt and .cut.vcf (with --lod: its LOD files and summary line), "
                        "and, one line per variant and cell, <outPrefix>.dsAF.depth.detection.txt.  With --dsAFReps the cells are "
                        "replicated as the targets are: <outPrefix>.dsAF.depth.replicates.txt, .dsAF.depth.sensitivity.txt and "
                        ".dsAF.depth.curve.txt (per variant and depth the detection rate at every target and T95, the smallest "
                        "target found in 95 %%%% of the replicates together with every larger one).  The masks and counts of the cells "
                        "are made on the GPU; at most %d cells.  Needs --dsAF" % GRID_MAX_CELLS)
    p.add_argument("--spikeAF", default=None,
                   help="in-silico spike-ins: comma-separated target allele fractions t in (0, 1).  For each, the run is also called as if "
                        "on the BAM that tools/spike_variants.py --af t --seed dsSeed writes for the SNVs of --spikeVariants: per variant "
                        "and barcode one counter-based draw (Philox4x32-10 keyed by --dsSeed, the barcode text and the position) picks the "
                        "barcodes that get the variant, and every read of such a barcode that shows a plain base at the position gets "
                        "ALT there, its NM moving with it (a variant the sample carries already ends above t: reported, not corrected); "
                        "written to <outPrefix>.spikeAF<t>.smCounter.{all,cut}.txt and .cut.vcf (with --lod: its LOD files and summary "
                        "line), and, one line per variant and output, <outPrefix>.spikeAF.detection.txt.  The bases are rewritten on the "
                        "GPU, in a copy of each decoded run; the BAM is decoded once after a pre-pass over the runs around the listed "
                        "loci.  At most %d targets; not together with any --ds* down-sampling flag; needs the device plane builder; "
                        "one process only" % SPIKE_MAX_TARGETS)
    p.add_argument("--spikeVariants", default=None, help="the SNVs --spikeAF plants, one per line, in the format of --dsAFVariants: REF "
                                                         "and ALT one letter each out of A, C, G, T, REF the genome's letter; one variant "
                                                         "per position, each a locus of --bedTarget (insertions and deletions are refused)")
    p.add_argument("--spikeMtDepth", default=None, help="comma-separated --mtDepth of each --spikeAF target; default --mtDepth")
    p.add_argument("--spikeReps", type=int, default=None,
                   help="replicate spike-ins: R in %d .. %d.  Replicate j = 0 .. R - 1 is the spike-in of --spikeAF with seed (dsSeed + j) "
                        "mod 2^64 and everything else unchanged (replicate 0 is the run's own .spikeAF<t> output at the listed loci).  "
                        "What every replicate achieves (S, READS, V1) is counted on the GPU from the pre-pass's barcodes in one call, and "
                        "only the runs around the listed loci are spiked and called again, several replicates per call.  Every other "
                        "file stays as it is; added: <outPrefix>.spikeAF.replicates.txt, one line per listed variant, target and "
                        "replicate (the line that variant has in .spikeAF.detection.txt of a run with --dsSeed of that replicate, with "
                        "REP and SEED), <outPrefix>.spikeAF.sensitivity.txt, one line per variant and target: replicates called, the "
                        "detection rate and its Wilson score interval (95 %%%%), the achieved fractions, and with --lod the locus's "
                        "LOD, and <outPrefix>.spikeAF.curve.txt, one line per variant: the rate at every target and T95, the smallest "
                        "target found in 95 %%%% of the replicates together with every larger one.  Needs --spikeAF" % (REPS_MIN, REPS_MAX))
    p.add_argument("--spikePhase", action="store_true", default=False,
                   help="plant MNVs and same-molecule variant sets: --spikeVariants may then hold MNV lines (REF and ALT of one length, 2 "
                        "to 8 letters: one member SNV per letter that differs) and, on VCF lines, PS=<name> entries in column 8 (the "
                        "lines of one chromosome with one name are one set, at most 8 members).  The members of a set share one draw "
                        "per barcode - that of the member with the smallest position - so a barcode is spiked at all of them or at "
                        "none, as tools/spike_variants.py --phased does it.  Added when a set has two members or more: "
                        "<outPrefix>.spikeAF.phase.txt, one line per set and output with the barcodes that cover every member (N_ALL), "
                        "carry every member before (V0_ALL) and after spiking (V1_ALL), are spiked (S_ALL), and whether every member "
                        "was called (CALLED_ALL); with --spikeReps <outPrefix>.spikeAF.phase.replicates.txt and "
                        ".spikeAF.phase.sensitivity.txt.  Without the flag an MNV line is refused and PS= is not read.  Needs --spikeAF")
    p.add_argument("--spikeIndels", action="store_true", default=False,
                   help="plant insertions and deletions too: --spikeVariants may then hold, beside SNVs, insertions (REF X, ALT XS) and "
                        "deletions (REF XD, ALT X) of 1 to 255 letters out of ACGT, REF the genome's letters, no two footprints (the anchor "
                        "to the position behind the indel) overlapping.  A record of a spiked barcode takes the indel when the whole "
                        "footprint lies in one aligned operation of its CIGAR - SEQ, QUAL, CIGAR and NM are rewritten on the GPU, as "
                        "tools/spike_variants.py --indels does it; every other record is left alone.  The outputs are --spikeAF's, V0 "
                        "and V1 of .spikeAF.detection.txt by the variant's INS / DEL key.  Not with --spikeReps, --spikeDepth or "
                        "--spikePhase (--spikeIndelReps, --spikeIndelDepth and --spikeIndelPhase cover them).  Without the flag an indel line is refused.  Needs --spikeAF")
    p.add_argument("--spikeIndelReps", type=int, default=None,
                   help="--spikeIndels and --spikeReps R in one: --spikeVariants may hold SNVs, insertions and deletions (the rules of "
                        "--spikeIndels), and replicate j = 0 .. R - 1 is that spike-in with seed (dsSeed + j) mod 2^64 - a plain run on the "
                        "BAM tools/spike_variants.py --indels --af t --seed (dsSeed + j) writes.  The run writes what --spikeIndels writes "
                        "and <outPrefix>.spikeAF.replicates.txt, .spikeAF.sensitivity.txt and .spikeAF.curve.txt as --spikeReps does.  Per "
                        "covering barcode four numbers are counted once on the GPU (its reads, those that show ALT, those that show it when "
                        "the barcode is spiked, the records the rewrite changes then); several replicates' copies are written by one "
                        "call.  Refused: a run with a record whose CIGAR or length could pass 65535 through the listed indels; beside "
                        "--spikeIndels, --spikeReps, --spikeDepth or --spikePhase.  R in %d .. %d.  Needs --spikeAF" % (REPS_MIN, REPS_MAX))
    p.add_argument("--spikeIndelDepth", default=None,
                   help="--spikeDepth on the --spikeIndels spike-in: comma-separated barcode fractions f in (0, 1]; cells, files "
                        "(<outPrefix>.spikeAF<t>.dsMT<f>.*, .spikeAF.depth.detection.txt, with --spikeIndelReps .spikeAF.depth.replicates / "
                        ".sensitivity / .curve.txt), mtDepths and the limit of %d cells are --spikeDepth's.  Implies the rules of "
                        "--spikeIndels.  Needs --spikeAF" % GRID_MAX_CELLS)
    p.add_argument("--spikeIndelPhase", action="store_true", default=False,
                   help="--spikePhase under the rules of --spikeIndels: a phase set of --spikeVariants (an MNV line, or the lines of one "
                        "chromosome that share a PS=<name> entry of VCF column 8 - on insertion and deletion lines too) may hold SNVs, "
                        "insertions and deletions, at most 8 members; the footprints of ALL listed variants must be disjoint.  Every "
                        "member is drawn with the position of the set's leader (the smallest position, an SNV's or an anchor's), so a "
                        "barcode is spiked at every member or at none, and each member is then applied under its own rule, as "
                        "tools/spike_variants.py --phased --indels does it.  Writes what --spikeIndels writes and, when a set has two "
                        "members or more, <outPrefix>.spikeAF.phase.txt; beside --spikeIndelReps and / or --spikeIndelDepth also their "
                        "pages, the cells' lines and .spikeAF.phase.replicates.txt / .phase.sensitivity.txt.  Not with --spikeIndels, "
                        "--spikePhase (it implies both), --spikeReps or --spikeDepth (use --spikeIndelReps / --spikeIndelDepth).  Needs "
                        "--spikeAF")
    p.add_argument("--spikeDepth", default=None,
                   help="the spike-ins of --spikeAF at several barcode depths: comma-separated fractions f in (0, 1].  For every target t "
                        "and every f the run is also called on the CELL (t, f): the spike-in at t, of which a barcode stays when the "
                        "--dsMT --dsSampler philox draw keeps it at f (two independent draws, both keyed by --dsSeed) - the .dsMT<f> "
                        "output of a --dsMT f --dsSampler philox run on the BAM tools/spike_variants.py --af t writes, at the mtDepth "
                        "--dsMT f would get from that target's mtDepth (max(1, round(f x mtDepth))); written to "
                        "<outPrefix>.spikeAF<t>.dsMT<f>.smCounter.{all,cut}.txt and .cut.vcf (with --lod: its LOD files and summary line), "
                        "and, one line per variant and cell, <outPrefix>.spikeAF.depth.detection.txt.  With --spikeReps the cells are "
                        "replicated as the targets are: <outPrefix>.spikeAF.depth.replicates.txt, .spikeAF.depth.sensitivity.txt and "
                        ".spikeAF.depth.curve.txt (per variant and depth the detection rate at every target and T95).  What the cells "
                        "achieve is counted on the GPU in one call; at most %d cells.  Needs --spikeAF" % GRID_MAX_CELLS)
    p.add_argument("--spikeRpb", default=None,
                   help="the spike-ins of --spikeAF at several reads-per-barcode targets: comma-separated r > 0.  For every target t and "
                        "every r the run is also called on the CELL (t, r): the spike-in at t, then the --dsRpb r --dsRpbSampler philox "
                        "thinning with the same --dsSeed (two independent draws: one per barcode and position, one per read name) - the "
                        ".dsRpb<r> output of a --dsRpb r --dsRpbSampler philox run on the BAM tools/spike_variants.py --af t writes, at "
                        "that target's mtDepth and --rpb r; written to <outPrefix>.spikeAF<t>.dsRpb<r>.smCounter.{all,cut}.txt and "
                        ".cut.vcf (with --lod: its LOD files and summary line), and, one line per variant and cell, "
                        "<outPrefix>.spikeAF.rpb.detection.txt with the counts over the reads the cell keeps.  The file-wide table of "
                        "read names is built once; what the cells achieve is counted per read on the GPU in one call; at most %d "
                        "cells.  With --spikeReps the cells are replicated as the targets are, replicate j drawing both streams with "
                        "seed (dsSeed + j) mod 2^64: <outPrefix>.spikeAF.rpb.replicates.txt, .spikeAF.rpb.sensitivity.txt and "
                        ".spikeAF.rpb.curve.txt (per variant and r the detection rate at every target and T95).  SNV lists only; not "
                        "with --spikeDepth, --spikePhase or the --spikeIndel* flags.  Needs --spikeAF" % GRID_MAX_CELLS)
    p.add_argument("--spikeGrid", action="store_true", default=False,
                   help="a switch: --spikeDepth f1,.. and --spikeRpb r1,.. beside it give the two axes of a GRID.  For every --spikeAF "
                        "target t, fraction f and reads-per-barcode target r the run is also called on the CELL (t, f, r): the spike-in "
                        "at t, of which a record stays when the --dsGrid philox rule keeps it at (f, r) with the same --dsSeed (three "
                        "independent draws: the spike-in's, the barcode's, the read name's; probKeep of (f, r) over the barcodes kept at "
                        "f) - the .dsMT<f>.dsRpb<r> output of a --dsMT f --dsRpb r --dsGrid --dsSampler philox --dsRpbSampler philox "
                        "run on the BAM tools/spike_variants.py --af t writes, at the mtDepth max(1, round(f x mtDepth)) of (t, f) and "
                        "--rpb r; written to <outPrefix>.spikeAF<t>.dsMT<f>.dsRpb<r>.smCounter.{all,cut}.txt and .cut.vcf (with --lod: "
                        "its LOD files and summary line), and, one line per variant and cell, <outPrefix>.spikeAF.grid.detection.txt.  "
                        "The depth-only and reads-only cells either axis flag writes alone are NOT written: f = 1 gives the reads-only "
                        "column, a depth-only row is a --spikeDepth run.  With --spikeReps replicate j draws all three streams with seed "
                        "(dsSeed + j) mod 2^64 - its read thresholds are its own, probKeep moving with the barcodes it keeps: "
                        "<outPrefix>.spikeAF.grid.replicates.txt, .spikeAF.grid.sensitivity.txt and .spikeAF.grid.budget.txt (per "
                        "variant and target the cells by COST - the kept share of the file's read names - ascending, with the detection "
                        "rate and CHEAPEST95 on the cheapest cell whose rate reaches 0.95).  At most %d cells; SNV lists only; not with "
                        "--spikePhase, the --spikeIndel* flags, --spikePhaseRpb or --spikeScan*.  Without the switch --spikeDepth beside "
                        "--spikeRpb stays refused.  Needs --spikeAF, --spikeDepth and --spikeRpb" % GRID_MAX_CELLS)
    p.add_argument("--spikeIndelRpb", default=None,
                   help="--spikeRpb on the --spikeIndels spike-in: comma-separated reads-per-barcode targets r > 0; --spikeVariants may "
                        "hold SNVs, insertions and deletions (the rules of --spikeIndels).  Cell (t, r) is the .dsRpb<r> output of a "
                        "--dsRpb r --dsRpbSampler philox run on the BAM tools/spike_variants.py --indels --af t writes, both with "
                        "--dsSeed; cells, files (<outPrefix>.spikeAF<t>.dsRpb<r>.*, .spikeAF.rpb.detection.txt, with --spikeIndelReps "
                        ".spikeAF.rpb.replicates / .sensitivity / .curve.txt) and limits (%d cells) are --spikeRpb's; V0 and V1 are "
                        "counted by the variant's INS / DEL key over the reads the cell keeps, READS is the kept records the rewrite "
                        "changed.  Not with --spikeRpb, --spikeIndels, --spikeReps, --spikeDepth or --spikePhase; --spikeIndelDepth and "
                        "--spikeIndelPhase beside it are not built.  Needs --spikeAF" % GRID_MAX_CELLS)
    p.add_argument("--spikePhaseRpb", default=None,
                   help="phase sets at reads-per-barcode targets: comma-separated r > 0.  --spikeVariants is read under the rules of "
                        "--spikeIndelPhase (SNVs, MNV lines, insertions and deletions; PS=<name> sets of at most 8 members; all "
                        "footprints disjoint), and cell (t, r) is that spike-in at t - every member of a set drawn with its leader's "
                        "position - then the --dsRpb r --dsRpbSampler philox thinning with the same --dsSeed: the .dsRpb<r> output of a "
                        "--dsRpb r --dsRpbSampler philox run on the BAM tools/spike_variants.py --phased --indels --af t writes.  Writes "
                        "what --spikeIndelRpb and --spikeIndelPhase write and, when a set has two members or more, "
                        "<outPrefix>.spikeAF.rpb.phase.txt: per set and cell the barcodes that keep a read at every member (N_ALL), carry "
                        "every member before (V0_ALL) and after spiking (V1_ALL) over the kept reads, are spiked (S_ALL), and whether "
                        "every member was called in the cell (CALLED_ALL); with --spikeIndelReps R also "
                        "<outPrefix>.spikeAF.rpb.phase.replicates.txt and .rpb.phase.sensitivity.txt.  The joint numbers are counted "
                        "per read on the GPU in one call; at most %d cells.  Not with --spikeRpb, --spikeIndelRpb (this flag takes the "
                        "targets), --spikeIndels, --spikePhase, --spikeIndelPhase (implied), --spikeReps (use --spikeIndelReps), "
                        "--spikeDepth or --spikeIndelDepth (not built).  Needs --spikeAF" % GRID_MAX_CELLS)
    p.add_argument("--spikeScan", default=None,
                   help="a measured detection-rate map of the whole target: comma-separated target allele fractions t in (0, 1).  One "
                        "SNV, REF>ALT by --spikeScanAlt, is planted at every locus of --bedTarget whose genome letter is A, C, G or T, in "
                        "passes: pass k holds the loci with pos mod --spikeScanStride == k, and is by definition the run --spikeAF "
                        "<targets> --spikeVariants <the pass's list> --spikeReps R --dsSeed s (tools/spike_scan_lists.py writes the "
                        "lists).  Every run of the file is decoded once; the replicates' rows stay on the GPU, which says per replicate "
                        "and locus whether the SNV was called (smc_scan_detect) - only rows it cannot decide come to the host.  Writes "
                        "<outPrefix>.spikeScan.sensitivity.txt (a line per locus and target: .spikeAF.sensitivity.txt's without the PI "
                        "columns), .spikeScan.curve.txt (the rate at every target and T95), <outPrefix>.spikeScan<t>.rate.bedgraph per "
                        "target and .spikeScan.t95.bedgraph (1 where no listed target reaches 0.95) beside --lod's theoretical bedgraph; "
                        "no .spikeAF<t> output is written and the full-depth files stay as they are.  The cost grows with stride x R x "
                        "targets whole-panel builds.  Needs --spikeScanReps; not with any other --spike* or --ds* flag but --dsSeed; "
                        "one process only")
    p.add_argument("--spikeScanReps", default=None, help="R, the replicates of every --spikeScan pass: an integer in %d .. %d; replicate j "
                                                         "has seed (dsSeed + j) mod 2^64" % (REPS_MIN, REPS_MAX))
    p.add_argument("--spikeScanStride", default=None, help="S, an integer >= 1 (default 256): two SNVs of a --spikeScan pass are at least "
                                                           "S positions apart.  A smaller S means fewer passes and more reads shared "
                                                           "between a pass's spike-ins")
    p.add_argument("--spikeScanAlt", default=None, help="the ALT of --spikeScan: transition (default: A>G, G>A, C>T, T>C), transversion "
                                                        "(A>C, C>A, G>T, T>G) or complement (A>T, T>A, C>G, G>C)")
    p.add_argument("--spikeScanIndel", default=None,
                   help="--spikeScan with an indel instead of the SNV: del<d> plants the deletion of the d letters behind every locus P "
                        "(REF genome[P .. P+d], ALT genome[P]), dup<s> the tandem duplication of the next s (REF genome[P], ALT genome[P] + "
                        "genome[P+1 .. P+s]); d, s in 1 .. 255.  A locus is skipped when a letter of P .. P+d (P .. P+s) is not A, C, G or T "
                        "or lies past the chromosome's end.  A pass is by definition the run --spikeAF <targets> --spikeVariants <the "
                        "pass's list> --spikeIndelReps R --dsSeed s (tools/spike_scan_lists.py --indel writes the lists); the footprints "
                        "of a pass must be disjoint: --spikeScanStride >= d + 2 for a deletion, >= 2 for a duplication.  The allele id "
                        "of the planted key is resolved per replicate on the GPU from the build's own list of allele keys "
                        "(smc_scan_detect_keys); the files are --spikeScan's, REF and ALT the indel's texts at its anchor.  Needs "
                        "--spikeScan; not with --spikeScanAlt")
    p.add_argument("--spikeScanDepth", default=None,
                   help="f1,f2,...: --spikeScan (and --spikeScanIndel) also at these barcode fractions, each in (0, 1] and none listed "
                        "twice.  A pass is then by definition its run with --spikeDepth <fractions> (--spikeIndelDepth) beside "
                        "--spikeReps: the same draws, and a cell's mtDepth max(1, round(f x mtDepth)) with its own threshold.  The "
                        "copies of a batch are selected at every fraction by one smc_select_alignments_copies call.  Writes "
                        "<outPrefix>.spikeScan.depth.sensitivity.txt, .spikeScan.depth.curve.txt, .spikeScan.depth.need.txt (F95: the "
                        "smallest depth with a rate of 0.95 at it and above), <outPrefix>.spikeScan<t>.dsMT<f>.rate.bedgraph, "
                        ".spikeScan.dsMT<f>.t95.bedgraph and .spikeScan<t>.f95.bedgraph (2 where full depth fails); targets x "
                        "fractions at most %d.  With --lod these pages carry no LOD column.  Needs --spikeScan" % GRID_MAX_CELLS)
    p.add_argument("--spikeScanRpb", default=None,
                   help="r1,r2,...: --spikeScan (and --spikeScanIndel) also at these reads-per-barcode targets, each > 0 and none listed "
                        "twice.  A pass is then by definition its run with --spikeRpb <targets> (--spikeIndelRpb) beside --spikeReps: "
                        "the same draws and philox read sampler, a cell called at the scan's mtDepth with --rpb r.  The copies of a batch "
                        "are selected at every target by one smc_select_alignments_reads_copies call.  Writes "
                        "<outPrefix>.spikeScan.rpb.sensitivity.txt, .spikeScan.rpb.curve.txt, .spikeScan.rpb.need.txt (R95: the smallest "
                        "target with a rate of 0.95 at it and above, `full` when only the file's own reads reach it), "
                        "<outPrefix>.spikeScan<t>.dsRpb<r>.rate.bedgraph, .spikeScan.dsRpb<r>.t95.bedgraph and .spikeScan<t>.r95.bedgraph "
                        "(twice the largest of --rpb and the targets where full depth fails); targets x reads-per-barcode targets at most "
                        "%d.  With --lod these pages carry no LOD column.  Needs --spikeScan; not with --spikeScanDepth" % GRID_MAX_CELLS)
    p.add_argument("--spikeScanFilter", action="store_true", default=False,
                   help="--spikeScan's rates over the replicates that are called AND whose FILTER is PASS, and which flags took the "
                        "others away: behind every verdict the GPU decides the FILTER column of the row (smc_scan_filter: the device's "
                        "eight flags, HP / LowC and the repeat names of the planted variant from two words made once per listed variant) "
                        "- by definition the FILTER and CALLED columns of the pass's own .spikeAF.replicates.txt.  Writes "
                        "<outPrefix>.spikeScan.filter.txt (REPS, CALLED, PASS, RATE_PASS with its interval and a count per FILTER name), "
                        ".spikeScan.filter.curve.txt (RATE_PASS at every target and T95_PASS), <outPrefix>.spikeScan<t>.passrate.bedgraph "
                        "and .spikeScan.t95pass.bedgraph; with --spikeScanDepth / --spikeScanRpb also .spikeScan.depth.filter.txt / "
                        ".spikeScan.rpb.filter.txt.  Every other file of the scan stays as it is.  Needs --spikeScan")
    p.add_argument("--spikeScanMnv", default=None,
                   help="L in 2 .. 8: --spikeScan with an MNV of L adjacent letters instead of the SNV: at every locus P of --bedTarget REF = "
                        "genome[P .. P+L-1], ALT = --spikeScanAlt's rule applied to every letter, planted as ONE phase set of L member SNVs "
                        "named chrom:P (a barcode is spiked at all members or at none).  A locus is skipped when a position of P .. P+L-1 is "
                        "no locus of the target or its letter is not A, C, G or T.  A pass is by definition the run --spikeAF <targets> "
                        "--spikeVariants <the pass's list> --spikeReps R --spikePhase --dsSeed s (tools/spike_scan_lists.py --mnv writes the "
                        "lists); --spikeScanStride >= L.  The GPU decides per copy and set whether every member was called "
                        "(smc_scan_detect_sets).  Writes <outPrefix>.spikeScan.mnv.sensitivity.txt (the sets' lines of "
                        ".spikeAF.phase.sensitivity.txt), .spikeScan.mnv.curve.txt, <outPrefix>.spikeScan<t>.mnv.rate.bedgraph and "
                        ".spikeScan.mnv.t95.bedgraph in place of the SNV scan's pages; no LOD column with --lod.  Needs --spikeScan; beside "
                        "--spikeScanBuild, --spikeScanMnvFilter, --spikeScanMnvDepth and --spikeScanMnvRpb; not with --spikeScanIndel, --spikeScanDepth, --spikeScanRpb or "
                        "--spikeScanFilter (not built)")
    p.add_argument("--spikeScanMnvFilter", action="store_true", default=False,
                   help="--spikeScanMnv's rates over the replicates in which every member SNV is called AND every member's FILTER is "
                        "PASS, and which flags took the others away - by definition the FILTER and CALLED columns of the members' lines "
                        "in the pass's own .spikeAF.replicates.txt.  Behind every joint verdict the GPU decides the joint FILTER word of "
                        "the set on the same rows (smc_scan_filter_sets: the OR of the members' names, and which members are not PASS; "
                        "4 bytes per copy and set come down).  Writes <outPrefix>.spikeScan.mnv.filter.txt (REPS, CALLED_ALL, PASS_ALL, "
                        "RATE_PASS with its interval, and per FILTER name the called replicates in which a member holds it), "
                        ".spikeScan.mnv.filter.curve.txt (RATE_PASS at every target and T95_PASS), "
                        "<outPrefix>.spikeScan<t>.mnv.passrate.bedgraph and .spikeScan.mnv.t95pass.bedgraph.  Every other file of the MNV "
                        "scan stays as it is.  Needs --spikeScanMnv")
    p.add_argument("--spikeScanMnvDepth", default=None,
                   help="f1,f2,...: --spikeScanMnv also at these barcode fractions, each in (0, 1] and none listed twice: only barcodes that "
                        "cover ALL members carry an MNV, so N_ALL falls faster than N at amplicon ends.  A pass is then by definition its "
                        "run with --spikeDepth <fractions> beside --spikeReps --spikePhase: cell (t, f) is called at max(1, round(f x "
                        "mtDepth)) with its own threshold, and the set's cell line of that run's .spikeAF.phase.sensitivity.txt is the "
                        "definition.  The joint counts of every cell come from the one smc_spike_phase_counts call per pass, the copies of a "
                        "batch are selected at every fraction by one smc_select_alignments_copies call.  Writes "
                        "<outPrefix>.spikeScan.mnv.depth.sensitivity.txt, .spikeScan.mnv.depth.curve.txt, .spikeScan.mnv.depth.need.txt "
                        "(F95 over the joint rates, N95 the mean N_ALL there), <outPrefix>.spikeScan<t>.dsMT<f>.mnv.rate.bedgraph, "
                        ".spikeScan.dsMT<f>.mnv.t95.bedgraph and .spikeScan<t>.mnv.f95.bedgraph (2 where full depth fails); with "
                        "--spikeScanMnvFilter also .spikeScan.mnv.depth.filter.txt; targets x fractions at most %d; no LOD column with "
                        "--lod.  Needs --spikeScanMnv" % GRID_MAX_CELLS)
    p.add_argument("--spikeScanMnvRpb", default=None,
                   help="r1,r2,...: --spikeScanMnv also at these reads-per-barcode targets, each > 0 and none listed twice: thinning reads "
                        "can take a barcode out of one member's pileup, or flip its majority at one member only, so the joint numbers are "
                        "counted per record.  A pass is then by definition its run --spikeAF <targets> --spikeVariants <the pass's list> "
                        "--spikeIndelReps R --spikePhaseRpb <r...> --dsSeed s: the same draws and philox read sampler, a cell called at the "
                        "scan's mtDepth with --rpb r, and the set's cell line of that run's .spikeAF.rpb.phase.sensitivity.txt is the "
                        "definition.  The joint counts of every cell come from one smc_scan_phase_rpb_counts call per pass and run over "
                        "the run in barcode-major order - no per-variant record lists on the host -, the copies of a batch are selected at "
                        "every target by one smc_select_alignments_reads_copies call.  Writes <outPrefix>.spikeScan.mnv.rpb.sensitivity.txt, "
                        ".spikeScan.mnv.rpb.curve.txt, .spikeScan.mnv.rpb.need.txt (R95 over the joint rates, N95 the mean N_ALL there), "
                        "<outPrefix>.spikeScan<t>.dsRpb<r>.mnv.rate.bedgraph, .spikeScan.dsRpb<r>.mnv.t95.bedgraph and "
                        ".spikeScan<t>.mnv.r95.bedgraph; with --spikeScanMnvFilter also .spikeScan.mnv.rpb.filter.txt; targets x "
                        "reads-per-barcode targets at most %d; no LOD column with --lod.  Needs --spikeScanMnv; not with "
                        "--spikeScanMnvDepth" % GRID_MAX_CELLS)
    p.add_argument("--spikeScanBuild", default=None,
                   help="whole (default) or listed: how --spikeScan builds its spiked copies.  whole: every copy is a build of its whole "
                        "decoded run, however few of its loci the pass lists.  listed: one smc_build_listed call builds the listed loci "
                        "alone, for all copies of a batch at once, as a dense batch of copies x listed loci - byte for byte the whole "
                        "build's planes of those loci, so every file of the scan is the whole run's.  A batch holds as many copies as "
                        "their listed slots allow.  A run the listed builder declines (an alignment flagged neither READ1 nor READ2) is "
                        "built the whole way and counted in the pass's log line; the listed rows of replicate 0 are also made the whole "
                        "way and must be equal.  Beside every other flag of the scan, --spikeScanIndel among them.  Needs --spikeScan")
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
SPIKE_MAX_TARGETS = 32       # (--spikeAF: spike.MAX_TARGETS)
SCAN_MAX_PASS_VARIANTS = 4096   # (--spikeScan: SMC_AF_MAX_VARIANTS, the variants of one chromosome a rewrite call takes)
GRID_MAX_CELLS = 32          # (a launch takes at most SMC_RG_MAX_TARGETS masks; every cell holds a batch's device arrays)


def _ds_mt_depths(args, flag, n, what, default):
    """--<flag>, the comma-separated --mtDepth of each of the n `what` -> n depths; default() without the flag (called only then:
    tests hand these helpers namespaces that lack --mtDepth)."""
    text = getattr(args, flag, None)
    if text in (None, ""):
        return default()
    try:
        depths = [int(x) for x in str(text).split(",") if x.strip()]
    except ValueError:
        raise SystemExit("--%s: comma-separated integers expected, got %r" % (flag, text))
    if len(depths) != n:
        raise SystemExit("--%s: %d depths for %d %s" % (flag, len(depths), n, what))
    return depths


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
    depths = _ds_mt_depths(args, "dsMtDepth", len(fr), "--dsMT fractions", lambda: [max(1, int(py2_round(f * args.mtDepth))) for f in fr])
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
    depths = _ds_mt_depths(args, "dsRpbMtDepth", len(rs), "--dsRpb targets", lambda: [int(args.mtDepth)] * len(rs))
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
    depths = _ds_mt_depths(args, "dsAFMtDepth", len(ts), "--dsAF targets", lambda: [int(args.mtDepth)] * len(ts))
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


def ds_af_depth_cells(args, af_targets):
    """--dsAFDepth -> (fractions, [(target index, t, f, mtDepth of the cell, output prefix)] for every --dsAF target t and every fraction
    f, targets outer), or (None, []) without the flag.  A cell's mtDepth is what --dsMT f gets from its target's mtDepth.  Refused:
    without --dsAF, a fraction outside (0, 1], a repeated fraction, beyond GRID_MAX_CELLS cells."""
    from .py2compat import py2_round
    text = getattr(args, "dsAFDepth", None)
    if text in (None, ""):
        return None, []
    if not af_targets:
        raise SystemExit("--dsAFDepth thins the barcodes of the --dsAF dilutions: it needs --dsAF")
    try:
        fr = [float(x) for x in str(text).split(",") if x.strip()]
    except ValueError:
        raise SystemExit("--dsAFDepth: comma-separated fractions in (0, 1] expected, got %r" % text)
    if not fr or any(not (0.0 < f <= 1.0) for f in fr):
        raise SystemExit("--dsAFDepth: every fraction must lie in (0, 1], got %r" % text)
    if len(set("%g" % f for f in fr)) != len(fr):
        raise SystemExit("--dsAFDepth: a fraction is listed twice (the cells' files would share a name), got %r" % text)
    if len(af_targets) * len(fr) > GRID_MAX_CELLS:
        raise SystemExit("--dsAFDepth: %d targets x %d fractions = %d cells, at most %d" % (len(af_targets), len(fr), len(af_targets) * len(fr),
                                                                                             GRID_MAX_CELLS))
    return fr, [(k, t, f, max(1, int(py2_round(f * d))), "%s.dsMT%g" % (p, f)) for k, (t, d, p) in enumerate(af_targets) for f in fr]


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


@dataclasses.dataclass
class _Output:
    """One output of a run: the prefix of its files and the VcParams it is called with (params.mtDepth and params.rpb are its depth and
    its reads per barcode).  Output 0 of a run is the full-depth one; every other has a `rule`, once the rule makers below have run."""
    prefix: str
    params: VcParams
    kind: str = "full"          # full, dsMT, dsRpb, dsGrid, dsAF, dsAFDepth, spikeAF, spikeDepth or spikeRpb
    frac: float = None          # (dsMT, dsGrid, dsAFDepth, spikeDepth) the fraction of the barcodes
    target: float = None        # (dsRpb, dsGrid, spikeRpb) the reads per barcode asked for
    af: float = None            # (dsAF, dsAFDepth, spikeAF, spikeDepth, spikeRpb) the target allele fraction
    af_index: int = None        # (dsAFDepth, spikeDepth, spikeRpb) which --dsAF / --spikeAF target the cell belongs to
    rule: object = None         # the devplanes.DsRule that selects it; None: full depth


@dataclasses.dataclass
class _Plan:
    """What a run is to do beyond its command line: its outputs in the order they are called, written and summarised (full depth,
    fractions, targets, cells, allele fractions, their cells), the engine coming up, and the state of --dsAF."""
    outputs: list
    early: object = None
    variants: list = None       # (--dsAF) the listed variants and titrate()'s result per target
    res: list = None
    reps: int = None            # (--dsAFReps) R, and what the pre-pass kept for the replicate stage (None once that has taken it)
    keep: dict = None
    depth: dict = None          # (--dsAFDepth) "fracs", the cells' "params", and once the rules are made "rules" and "counts" [V, T, F, 2]
    spike: dict = None          # (--spikeAF) once the rules are made: "variants", and "res", the pre-pass's numbers per target
    spike_reps: int = None      # (--spikeReps) R; plan.spike then holds "keep", what the pre-pass kept (None once the stage has taken it)
    spike_depth: dict = None    # (--spikeDepth) "fracs", the cells' "params", and once the rules are made "rules" and "counts" [V][T x F]
    spike_rpb: dict = None      # (--spikeRpb, --spikeIndelRpb, --spikePhaseRpb: then also "flag") "targets", the cells' "params", and once the rules are made "rules" and "counts" [V][T x Rr]; --spikeGrid: also "fracs" and "reps", the cells are (t, f, r) and the counts [V][T x F x Rr]
    spike_indel_counters: bool = False   # (--spikeIndelReps, --spikeIndelDepth, --spikeIndelPhase, --spikeIndelRpb, --spikePhaseRpb) the spike-ins are --spikeIndels', four counters per covering barcode
    scan: dict = None           # (--spikeScan) spike.scan's dict; once the rules are made also "variants", "loci" and "passes"
    spike_phase: bool = False   # (--spikePhase, --spikeIndelPhase, --spikePhaseRpb) plan.spike then holds "phase": None, or devplanes.spike_rules' dict of the sets of two members or more

    @property
    def rules(self):
        return [o.rule for o in self.outputs if o.rule is not None]


def _engine_of(args, early):
    """The engine coming up in the helper thread, else the process's engine (it stays in _ENGINES; call_shard takes it out)."""
    if early is not None:
        return early.get()
    return _ENGINES.get(args.device) or _ENGINES.setdefault(args.device, Engine(args.device))


def ds_af_rules(args, outs, variants, early, keep=None, depth=None):
    """The devplanes.DsRule of every --dsAF output (the pre-pass on the GPU: devplanes.ds_af_rules) and the titration's numbers; the
    run log gets a line per variant and target.  `keep` (--dsAFReps): a dict for what the replicate stage starts from.  `depth`
    (--dsAFDepth): the plan's dict; it gets the cells' rules and counts."""
    from .tools import ds_allele_fraction as af
    eng = _engine_of(args, early)
    try:
        rules, res = devplanes.ds_af_rules(args.bamFile, fasta.FastaFile(args.refGenome), variants, [o.af for o in outs],
                                           [o.params for o in outs], int(args.dsSeed), eng, keep=keep,
                                           **({"depth": depth} if depth is not None else {}))
    except (ValueError, bamio.BamError) as e:
        raise SystemExit(str(e))
    for r in res:
        for v, row in zip(variants, r["rows"]):
            print(af.report_line(v, r["target"], row))
        print("--dsAF %g: seed %d, %d barcodes dropped" % (r["target"], int(args.dsSeed), len(r["dropped"])))
    return rules, res


def spike_rules(args, outs, variants, early, keep=None, depth=None, phase=None, indel_counters=False, rpb=None):
    """The devplanes.DsRule of every --spikeAF output (the pre-pass on the GPU: devplanes.spike_rules) and its numbers; the run log
    gets a line per variant and target.  `keep` (--spikeReps): a dict for what the replicate stage starts from.  `depth`
    (--spikeDepth): the plan's dict; it gets the cells' rules and counts.  `phase` (--spikePhase): a dict with the "sets" of two
    members or more; it gets their joint barcodes and counts.  `rpb` (--spikeRpb): the plan's dict; it gets the cells' rules and counts."""
    from .tools import spike_variants as sv
    eng = _engine_of(args, early)
    more = {k: v for k, v in (("keep", keep), ("depth", depth), ("phase", phase), ("rpb", rpb)) if v is not None}
    if indel_counters:
        more["indel_counters"] = True
    try:
        rules, res = devplanes.spike_rules(args.bamFile, fasta.FastaFile(args.refGenome), variants, [o.af for o in outs],
                                           [o.params for o in outs], int(args.dsSeed), eng, **more)
    except (ValueError, bamio.BamError) as e:
        raise SystemExit(str(e))
    for r in res:
        for v, row in zip(variants, r["rows"]):
            print(sv.report_line(v, r["target"], row))
    if phase is not None:
        for ps, per in zip(phase["sets"], phase["counts"]):
            for o, c in zip(outs, per):
                print("%s %g: set %s (%d members) N_ALL %d, V0_ALL %d, S_ALL %d, V1_ALL %d" %
                      ("--spikeIndelPhase" if getattr(args, "spikeIndelPhase", False) else "--spikePhaseRpb" if rpb is not None else "--spikePhase",
                       o.af, ps.name, len(ps.members), c["N_ALL"], c["V0_ALL"], c["S_ALL"], c["V1_ALL"]))
        if phase.get("rpb_counts") is not None:
            # (--spikePhaseRpb: the joint numbers over the reads each cell keeps)
            for ps, per in zip(phase["sets"], phase["rpb_counts"]):
                for (t, r), c in zip(((o.af, r) for o in outs for r in rpb["targets"]), per):
                    print("--spikePhaseRpb %g x target %g: set %s (%d members) N_ALL %d, V0_ALL %d, S_ALL %d, V1_ALL %d" %
                          (t, r, ps.name, len(ps.members), c["N_ALL"], c["V0_ALL"], c["S_ALL"], c["V1_ALL"]))
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


def ds_grid_rules(args, outs, frac_rules, rpb_rules, grouped=None):
    """The devplanes.DsRule of every --dsGrid cell, after the fractions' and the targets' rules: the reference's names from the
    fractions' kept barcodes and the targets' grouping (`grouped`), or with the philox samplers from the targets' file-wide table; a
    cell whose kept barcodes have no barcode of two or more reads ends the run with a message."""
    fr, plist = [(o.frac, o.target) for o in outs], [o.params for o in outs]
    try:
        if args.dsRpbSampler == "philox":
            return devplanes.philox_grid_rules(args.bamFile, fr, plist, int(args.dsSeed), rpb_rules[0].groups)
        kept = {rule.frac: rule.kept for rule in frac_rules}
        return devplanes.reference_grid_rules(args.bamFile, fr, plist, int(args.dsSeed), kept, grouped)
    except ValueError as e:
        raise SystemExit(str(e))


def ds_rpb_rules(args, outs, early=None, grouped=None):
    """The devplanes.DsRule of every --dsRpb target: the reference's read names (one pass over the whole file, here), or with
    --dsRpbSampler philox the file-wide table on the GPU (`early`: the engine coming up; else the process's engine); a file without a
    barcode of two or more reads, or whose names collide in the table's hashes, ends the run with a message."""
    rs, plist = [o.target for o in outs], [o.params for o in outs]
    try:
        if args.dsRpbSampler == "philox":
            return devplanes.philox_read_rules(args.bamFile, rs, plist, int(args.dsSeed), _engine_of(args, early))
        return devplanes.reference_read_rules(args.bamFile, rs, plist, int(args.dsSeed), grouped=grouped)
    except ValueError as e:
        raise SystemExit(str(e))


def ds_rules(args, outs):
    """The devplanes.DsRule of every --dsMT fraction (the reference's sampler: one pass over the whole file, here)."""
    fr, plist = [o.frac for o in outs], [o.params for o in outs]
    if args.dsSampler == "philox":
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


def _release_engine(eng, keep=True):
    """The engine stays with the process: a second main() in the same process finds the context, its tables and its buffers
    again, and the command line does not spend 20 ms of its wall time freeing device memory the exiting process gives back
    anyway (SMC_CLOSE_ENGINE=1: close it, as round 2 did).  `keep` False: an engine that took host-built batches is closed."""
    if keep and not _lib.exp_env("SMC_CLOSE_ENGINE"):
        _ENGINES[eng.device] = eng
    else:
        _ENGINES.pop(eng.device, None)      # (nothing there after call_shard or the helper thread took the engine out)
        eng.close()


@dataclasses.dataclass
class _Shard:
    """What call_shard hands back."""
    rows: list                  # the row strings of the full-depth output
    ds: tuple = ()              # the rows of every further output, in the plan's order
    lod: list = None            # (--lod) per output what lod.run_lods made
    af_reps: dict = None        # (--dsAFReps) what devplanes.ds_af_replicates made
    spike_reps: dict = None     # (--spikeReps) what devplanes.spike_replicates made
    scan: dict = None           # (--spikeScan) what devplanes.spike_scan made


def call_shard(args, params: VcParams, loci, device: int, early=None, plan=None):
    """The per-locus rows (strings, smCounter.py:599) of a run of loci, for every output of `plan` (none: the full-depth output
    alone): BAM decode -> device batches -> kernels."""
    ref = fasta.FastaFile(args.refGenome)
    eng = early.get() if early is not None else (_ENGINES.pop(device, None) or Engine(device))
    outputs = plan.outputs if plan is not None else [_Output(args.outPrefix, params)]
    rules = [o.rule for o in outputs[1:]] or None
    decoder = os.environ.get("SMC_BAM_DECODER", "native")
    # (one process per GPU: the ranks of a node share its cores for decoding)
    # (LOCAL_WORLD_SIZE: WORLD_SIZE also counts the ranks of other nodes, which do not share these cores)
    per_node = int(os.environ.get("LOCAL_WORLD_SIZE") or os.environ.get("WORLD_SIZE", "1"))
    nthreads = bamio.host_threads(per_node)
    resident = False
    if rules is None and decoder == "python":                         # readable decoder, same batches
        batches = _prefetch(bamio.iter_pileup_batches(bamio.BamFile(args.bamFile), ref, loci, max_reads=args.batchReads))
    elif rules is None and os.environ.get("SMC_PLANES", "device") == "host":   # planes built by the host threads, then uploaded
        batches = _prefetch(bamio.iter_device_batches_native(args.bamFile, ref, loci, params, max_reads=args.batchReads,
                                                             nthreads=nthreads))
    else:
        # default: the host decodes alignments, the GPU builds the planes from them (k_build_planes) and they stay in HBM
        resident = True
        # (a batch only lives in HBM here - 16 B per read - so it can be eight times the host-built default)
        # (--dsMT: the same batches at full depth and for every fraction - the device builder only, SMC_PLANES=host or
        # SMC_BAM_DECODER=python end with an error naming the first run)
        batches = devplanes.iter_resident_batches(args.bamFile, ref, loci, params, eng, max_reads=32 * args.batchReads,
                                                  nthreads=nthreads, all_planes=False, sampler=getattr(args, "sampler", "reference"),
                                                  sampler_seed=getattr(args, "samplerSeed", 0), ds_rules=rules,
                                                  # (--spikeRpb: the replicate stage reads the cells' file-wide table behind the last
                                                  # batch - main() owns the plan's tables and closes them whatever happens)
                                                  close_tables=plan is None or plan.spike_rpb is None,
                                                  force_host=rules is not None and (decoder == "python" or
                                                                                    os.environ.get("SMC_PLANES", "device") == "host"))
        # (a batch ahead in a helper thread: decoding and building batch i + 1 overlaps the kernels and the strings of batch i;
        # the two threads use different staging buffers of the engine, device work is ordered by the default stream)
        if not _lib.exp_env("SMC_NO_PREFETCH"):
            batches = _prefetch(batches, depth=1)
    call = vc.vc_resident if resident else vc.vc_batch
    rows = [_Rows() for _ in outputs]
    # (--lod: three int32 columns of every output's rows, and the tables while the engine is alive)
    lod_cols = None
    if getattr(args, "lod", False):
        from . import lod as _lod
        lod_cols = [_lod.DepthCols() for _ in outputs]
    # (the full-depth output is called last: the boundary notes read its rows in the engine's staging memory)
    order = list(range(1, len(outputs))) + [0]
    for first, b in batches:
        bs = b if rules is not None else [b]
        for k in order:
            rows[k].add(call(bs[k], outputs[k].params, ref, eng))
            if lod_cols is not None:
                lod_cols[k].add(eng.last_rows)
        if resident:
            _report_boundary(eng.last_rows, bs[0].chrom, bs[0].pos)
    shard = _Shard(rows[0].done(), [r.done() for r in rows[1:]])
    if plan is not None and plan.keep is not None:
        shard.af_reps = _ds_af_replicates(args, plan, ref, eng, loci, shard.ds)
    if plan is not None and plan.spike is not None and plan.spike.get("keep") is not None:
        shard.spike_reps = _spike_replicates(args, plan, ref, eng, loci, shard.ds)
    if plan is not None and plan.scan is not None:
        shard.scan = _spike_scan(args, plan, ref, eng, params)
    if lod_cols is not None:
        shard.lod = _lod.run_lods(eng, [o.params for o in outputs], lod_cols, args.lodDepth or "UMT")
    _release_engine(eng, keep=resident)
    return shard


def _ds_af_replicates(args, plan, ref, eng, loci, ds_rows):
    """--dsAFReps after the run's batches: devplanes.ds_af_replicates over the runs the pre-pass kept, and the check that ties it to
    the run's own outputs - replicate 0 has the seed of the run, so its row at every listed locus must be the .dsAF<t> output's."""
    variants = plan.variants
    # (the run's outputs behind the first: the targets, then with --dsAFDepth their cells - the order of the stage's cells)
    outs, targets = plan.outputs[1:], [o for o in plan.outputs if o.kind == "dsAF"]
    keep, plan.keep = plan.keep, None           # (the stage frees the kept runs itself, whatever happens in it)
    more = {"depth": plan.depth} if plan.depth is not None else {}
    out = devplanes.ds_af_replicates(args.bamFile, ref, variants, [o.af for o in targets], [o.params for o in targets], int(args.dsSeed),
                                     plan.reps, eng, keep, plan.res, sampler=getattr(args, "sampler", "reference"),
                                     sampler_seed=getattr(args, "samplerSeed", 0), **more)
    index = {(c, int(p)): n for n, (c, p) in enumerate(loci)}
    for (k, t, j), line in out["rows"].items():
        v = variants[k]
        if j == 0 and line != ds_rows[t][index[(v.chrom, v.pos)]]:
            raise RuntimeError("--dsAFReps: replicate 0 of %s:%d in %s is not the row of the run's own output:\n%s\n%s" %
                               (v.chrom, v.pos, outs[t].prefix, line, ds_rows[t][index[(v.chrom, v.pos)]]))
    return out


def _spike_replicates(args, plan, ref, eng, loci, ds_rows):
    """--spikeReps after the run's batches: devplanes.spike_replicates over the runs the pre-pass kept, and the check that ties it to
    the run's own outputs - replicate 0 has the seed of the run, so its row at every listed locus must be the .spikeAF<t> output's."""
    # (the run's outputs behind the first: the targets, then with --spikeDepth their cells - the order of the stage's rows)
    variants, outs, targets = plan.spike["variants"], plan.outputs[1:], [o for o in plan.outputs if o.kind == "spikeAF"]
    keep, plan.spike["keep"] = plan.spike["keep"], None      # (the stage frees the kept runs itself, whatever happens in it)
    more = {"depth": plan.spike_depth} if plan.spike_depth is not None else {}
    if plan.spike.get("phase") is not None:
        more["phase"] = plan.spike["phase"]
    if plan.spike_rpb is not None:
        more["rpb"] = plan.spike_rpb
    out = devplanes.spike_replicates(args.bamFile, ref, variants, [o.af for o in targets], [o.params for o in targets], int(args.dsSeed),
                                     plan.spike_reps, eng, keep, sampler=getattr(args, "sampler", "reference"),
                                     sampler_seed=getattr(args, "samplerSeed", 0), **more)
    index = {(c, int(p)): n for n, (c, p) in enumerate(loci)}
    for (k, t, j), line in out["rows"].items():
        v = variants[k]
        if j == 0 and line != ds_rows[t][index[(v.chrom, v.pos)]]:
            raise RuntimeError("--spikeReps: replicate 0 of %s:%d in %s is not the row of the run's own output:\n%s\n%s" %
                               (v.chrom, v.pos, outs[t].prefix, line, ds_rows[t][index[(v.chrom, v.pos)]]))
    return out


def _repeat_tracks(args):
    """The two repeat tracks of the command line as postfilter.load_repeat_regions takes them: None for one not given or not found."""
    return [b if b and os.path.exists(b) else None for b in (args.bedTandemRepeats, args.bedRepeatMaskerSubset)]


def _spike_scan(args, plan, ref, eng, params):
    """--spikeScan after the run's batches: devplanes.spike_scan over every run of the file, and a line per pass in the run log."""
    from . import spike as _spike
    scan = plan.scan
    threshold = writers.pi_threshold(params.mtDepth, args.threshold)
    repeats = postfilter.load_repeat_regions(args.bedTarget, *_repeat_tracks(args))
    depth = None
    if "fracs" in scan:
        cells = [dataclasses.replace(params, mtDepth=_spike.scan_depth_mt(params.mtDepth, f)) for f in scan["fracs"]]
        depth = dict(fracs=scan["fracs"], params=cells, thresholds=[writers.pi_threshold(c.mtDepth, args.threshold) for c in cells])
    mnv_axes = dict(flt=True) if "mnv_filter" in scan else {}
    if "mnv_fracs" in scan:
        cells = [dataclasses.replace(params, mtDepth=_spike.scan_depth_mt(params.mtDepth, f)) for f in scan["mnv_fracs"]]
        mnv_axes["depth"] = dict(fracs=scan["mnv_fracs"], params=cells, thresholds=[writers.pi_threshold(c.mtDepth, args.threshold) for c in cells])
    if "mnv_rpbs" in scan:
        # (a cell is called at the scan's mtDepth with --rpb r: the cut is the scan's own)
        mnv_axes["reads"] = dict(targets=scan["mnv_rpbs"], params=[dataclasses.replace(params, rpb=r) for r in scan["mnv_rpbs"]],
                                 thresholds=[threshold] * len(scan["mnv_rpbs"]))
    rpb = None
    if "rpbs" in scan:
        # (a cell is called at the scan's mtDepth with --rpb r: the cut is the scan's own)
        rpb = dict(targets=scan["rpbs"], params=[dataclasses.replace(params, rpb=r) for r in scan["rpbs"]],
                   thresholds=[threshold] * len(scan["rpbs"]))
    try:
        out = devplanes.spike_scan(args.bamFile, ref, scan["variants"], scan["passes"], scan["targets"], params, int(args.dsSeed), scan["reps"],
                                   eng, threshold, repeats, sampler=getattr(args, "sampler", "reference"),
                                   sampler_seed=getattr(args, "samplerSeed", 0), indel="indel" in scan, depth=depth, rpb=rpb,
                                   **(dict(flt=True) if "filter" in scan else {}),
                                   **(dict(build="listed") if _spike.scan_build(scan) == "listed" else {}),
                                   **(dict(mnv=scan["mnv"]) if "mnv" in scan else {}),
                                   **(dict(mnv_axes=mnv_axes) if mnv_axes else {}))
    except (ValueError, bamio.BamError) as e:
        raise SystemExit(str(e))
    listed = _spike.scan_build(scan) == "listed"
    for (k, _), st in zip(scan["passes"], out["passes"]):
        print("--spikeScan pass %d: %d variants, %d copies, %d builds, %s%d verdicts decided by the host, %.3f s" %
              (k, st["variants"], st["copies"], st["builds"], "%d of them whole, " % st["whole"] if listed else "", st["host"], st["seconds"]))
    if listed:
        print("--spikeScanBuild listed: %d listed builds, %d whole fallbacks, %d replicate-0 row checks" %
              tuple(sum(st[k] for st in out["passes"]) for k in ("listed", "whole", "checks")))
    return out


def call_shard_rows(args, params: VcParams, loci, device: int):
    """A rank's share as NUMBERS: (rows abi.ROW_DTYPE[n], reference letters, allele tables) - the distributed command line
    sends these to rank 0 (packed: dist.pack_shard) which prints every row; no strings are made on the other ranks."""
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
    world = int(os.environ.get("WORLD_SIZE", "1"))
    from . import spike as _spike
    # (--spikeScan first: it stands alone, and its refusals name what it cannot stand beside)
    scan = _spike.scan(args)
    fractions = ds_fractions(args)
    targets = ds_rpb_targets(args)
    cells = ds_grid_cells(args)
    af_targets = ds_af_targets(args)
    af_fracs, af_cells = ds_af_depth_cells(args, af_targets)
    spike_targets = _spike.targets(args)
    # (--spikePhaseRpb first: its refusals name the flag to use beside it)
    phase_rpbs, phase_rpb_cells = _spike.phase_rpb_cells(args, spike_targets)
    indel_phase = _spike.indel_phase(args, spike_targets)
    indel_reps, indel_depth = _spike.indel_flags(args, spike_targets)
    # (--spikeGrid: the two axis flags give the grid's axes - the cells take the place of both flags' own)
    grid_fracs, grid_rpbs, grid_cells = _spike.grid_cells(args, spike_targets)
    if grid_fracs is not None:
        _spike.indels(args, spike_targets)
        spike_fracs, spike_cells, spike_rpbs, spike_rpb_cells = None, [], grid_rpbs, [(k, t, r, d, p) for k, t, (_, r), d, p in grid_cells]
    else:
        spike_fracs, spike_cells = _spike.depth_cells(args, spike_targets, "spikeIndelDepth" if indel_depth is not None else "spikeDepth")
        _spike.indels(args, spike_targets)
        spike_rpbs, spike_rpb_cells = _spike.rpb_cells(args, spike_targets)
    indel_rpb = False
    if spike_rpbs is None:
        # (--spikeIndelRpb: the same cells and outputs, the spike-ins --spikeIndels')
        spike_rpbs, spike_rpb_cells = _spike.indel_rpb_cells(args, spike_targets)
        indel_rpb = spike_rpbs is not None
    if phase_rpbs is not None:
        # (--spikePhaseRpb: --spikeIndelRpb's cells and outputs under the rules of --spikeIndelPhase)
        spike_rpbs, spike_rpb_cells, indel_rpb, indel_phase = phase_rpbs, phase_rpb_cells, True, True
    at = lambda **kw: dataclasses.replace(params, **kw)
    plan = _Plan([_Output(args.outPrefix, params)] +
                 [_Output(p, at(mtDepth=d), "dsMT", frac=f) for f, d, p in fractions] +
                 [_Output(p, at(mtDepth=d, rpb=r), "dsRpb", target=r) for r, d, p in targets] +
                 [_Output(p, at(mtDepth=d, rpb=r), "dsGrid", frac=f, target=r) for f, r, d, p in cells] +
                 [_Output(p, at(mtDepth=d), "dsAF", af=t) for t, d, p in af_targets] +
                 [_Output(p, at(mtDepth=d), "dsAFDepth", frac=f, af=t, af_index=k) for k, t, f, d, p in af_cells] +
                 [_Output(p, at(mtDepth=d), "spikeAF", af=t) for t, d, p in spike_targets] +
                 [_Output(p, at(mtDepth=d), "spikeDepth", frac=f, af=t, af_index=k) for k, t, f, d, p in spike_cells] +
                 [_Output(p, at(mtDepth=d, rpb=r), "spikeRpb", target=r, af=t, af_index=k) for k, t, r, d, p in spike_rpb_cells],
                 reps=ds_af_reps(args, af_targets), spike_reps=indel_reps if indel_reps is not None else _spike.reps(args, spike_targets),
                 spike_phase=_spike.phase(args, spike_targets) or indel_phase,
                 spike_indel_counters=indel_reps is not None or indel_depth is not None or indel_phase or indel_rpb)
    if spike_fracs is not None:
        plan.spike_depth = dict(fracs=spike_fracs, params=[o.params for o in plan.outputs if o.kind == "spikeDepth"])
    if spike_rpbs is not None:
        plan.spike_rpb = dict(targets=spike_rpbs, params=[o.params for o in plan.outputs if o.kind == "spikeRpb"])
        if phase_rpbs is not None:
            plan.spike_rpb["flag"] = "--spikePhaseRpb"
        if grid_fracs is not None:
            # (--spikeGrid: the cells are --spikeRpb's with a fraction each; the pre-pass makes every replicate's thresholds up front)
            for o, (_, _, (f, _), _, _) in zip((o for o in plan.outputs if o.kind == "spikeRpb"), grid_cells):
                o.frac = f
            plan.spike_rpb.update(flag="--spikeGrid", fracs=grid_fracs, reps=plan.spike_reps)
    plan.scan = scan
    if af_fracs is not None:
        plan.depth = dict(fracs=af_fracs, params=[o.params for o in plan.outputs if o.kind == "dsAFDepth"])
    flag = " / ".join(f for f, on in (("--dsMT", fractions), ("--dsRpb", targets), ("--dsAF", af_targets), ("--spikeAF", spike_targets),
                                      ("--spikeScan", scan)) if on)
    if flag and world > 1:
        raise SystemExit("%s runs in one process only (not under torch.distributed.run with more than one rank)" % flag)
    if getattr(args, "lodDepth", None) is not None and not getattr(args, "lod", False):
        raise SystemExit("--lodDepth chooses the barcode depth --lod reads: it needs --lod")
    if getattr(args, "lod", False) and world > 1:
        raise SystemExit("--lod runs in one process only (not under torch.distributed.run with more than one rank): the writing rank "
                         "prints from gathered wire rows after its engine is gone, and the table of LODs is made on the GPU")
    host = [v for v, on in (("SMC_PLANES=host", os.environ.get("SMC_PLANES", "device") == "host"),
                            ("SMC_BAM_DECODER=python", os.environ.get("SMC_BAM_DECODER", "native") == "python")) if on]
    if flag and host:
        first = bedops.expand_loci(args.bedTarget)[:1]
        raise SystemExit("%s needs the device builder: the run at %s would be built on the host (%s)" %
                         (flag, "%s:%s" % first[0] if first else "(no targets)", host[0]))
    if world == 1 and os.environ.get("SMC_BAM_DECODER", "native") != "python":
        # a single process: the GPU runtime and the context come up (~ 0.1 s) in a helper thread while the target is expanded
        plan.early = _EarlyEngine(args.device)
    loc_list = bedops.expand_loci(args.bedTarget)
    try:
        _make_rules(args, plan, loc_list)
    except SystemExit:
        devplanes.close_rules(plan.rules)     # (a refused cell: the targets' file-wide table in HBM)
        if plan.early is not None:             # (the engine the helper brings up stays with the process, as after a run)
            try:
                _ENGINES.setdefault(args.device, plan.early.get())
            except Exception:
                pass
        raise
    for rule in plan.rules:
        if rule.level == "read":               # (a target or a cell)
            if rule.spike_rpb_cell:
                print("%s %s: sampler %s, seed %d, probKeep %.6g, %sthreshold %d, %d of %d read names kept (mtDepth %d)" %
                      (rule.flag, rule.label, rule.sampler, rule.seed, rule.prob_keep, "barcode threshold %d, read " % rule.bc_thr if rule.grid else "",
                       rule.thr, rule.n_kept, rule.n_names, rule.params.mtDepth))
                continue
            print("%s: sampler %s, seed %d, probKeep %.6g, %d of %d read names kept (mtDepth %d)" %
                  ("--dsGrid " + rule.label if rule.grid else "--dsRpb %g" % rule.target, rule.sampler, rule.seed, rule.prob_keep,
                   len(rule.kept) if rule.kept is not None else rule.n_kept, rule.n_names, rule.params.mtDepth))
    try:
        return _run(args, plan, loc_list, t0)
    finally:
        devplanes.close_rules(plan.rules)     # (--dsRpbSampler philox: the file-wide table in HBM, whatever happened)
        if plan.keep is not None:             # (--dsAFReps: the pre-pass's runs, when the run ended before the replicate stage)
            devplanes.free_af_runs(plan.keep.get("runs"))
        if plan.spike is not None and plan.spike.get("keep") is not None:     # (--spikeReps: the same)
            devplanes.free_af_runs(plan.spike["keep"].get("runs"))


def _make_rules(args, plan, loc_list):
    """The rule of every output but the first, each set on its output as soon as it is made: a refusal further on finds the device
    tables to close there.  (--dsGrid comes with fractions and targets, --dsAF without any of the three.)"""
    fr, rd, cell, af = ([o for o in plan.outputs if o.kind == kind] for kind in ("dsMT", "dsRpb", "dsGrid", "dsAF"))

    def put(outs, rules):
        for o, rule in zip(outs, rules):
            o.rule = rule
        return rules
    # (--dsGrid: the reference's grouping of the names once, for the targets and the cells alike)
    grouped = devplanes.group_placed_reads(args.bamFile) if cell and args.dsRpbSampler != "philox" else None
    if fr:
        frac_rules = put(fr, ds_rules(args, fr))
    if rd:
        rpb_rules = put(rd, ds_rpb_rules(args, rd, plan.early, grouped))
    if cell:
        put(cell, ds_grid_rules(args, cell, frac_rules, rpb_rules, grouped))
    if af:
        # (--dsAF: the listed variants checked, then the pre-pass over the runs around them; --dsAFReps: its runs kept)
        variants = ds_af_variants(args, loc_list)
        keep = {} if plan.reps is not None else None
        rules, res = ds_af_rules(args, af, variants, plan.early, keep, plan.depth)
        put(af, rules)
        if plan.depth is not None:
            put([o for o in plan.outputs if o.kind == "dsAFDepth"], plan.depth["rules"])
        plan.variants, plan.res, plan.keep = variants, res, keep
    sp = [o for o in plan.outputs if o.kind == "spikeAF"]
    if sp:
        # (--spikeAF: the listed SNVs checked, then the pre-pass over the runs around them)
        from . import spike as _spike
        variants = _spike.variants(args, loc_list, fasta.FastaFile(args.refGenome), indels=plan.spike_indel_counters)
        keep = {} if plan.spike_reps is not None else None
        from .tools import spike_variants as sv
        psets = sv.phase_sets(variants) if plan.spike_phase else []
        phase = dict(sets=psets) if psets else None
        rules, res = spike_rules(args, sp, variants, plan.early, keep, plan.spike_depth, phase, plan.spike_indel_counters, plan.spike_rpb)
        put(sp, rules)
        if plan.spike_rpb is not None:
            put([o for o in plan.outputs if o.kind == "spikeRpb"], plan.spike_rpb["rules"])
        if plan.spike_depth is not None:
            put([o for o in plan.outputs if o.kind == "spikeDepth"], plan.spike_depth["rules"])
        plan.spike = dict(variants=variants, res=res, keep=keep, phase=phase)
    if plan.scan is not None:
        # (--spikeScan: the scan's SNV of every locus and the passes, by the tool's own functions; two barcode texts with one
        # identity are refused here, as --spikeAF's pre-pass refuses them)
        from .tools import ds_allele_fraction as af, spike_scan_lists as lists
        try:
            af.unique_idents(bamio.placed_barcodes(args.bamFile), args.bamFile)
            if "mnv" in plan.scan:
                # (`variants`: the member SNVs with their sets; a pass holds indices of sets, `leaders` stand where the variants do below)
                variants, leaders, skipped = lists.scan_mnvs(loc_list, fasta.FastaFile(args.refGenome), plan.scan["mnv"], plan.scan["alt"])
                passes = lists.mnv_passes(variants, plan.scan["stride"])
            elif "indel" in plan.scan:
                variants, skipped = lists.scan_indels(loc_list, fasta.FastaFile(args.refGenome), plan.scan["indel"])
            else:
                variants, skipped = lists.scan_variants(loc_list, fasta.FastaFile(args.refGenome), plan.scan["alt"])
            if "mnv" not in plan.scan:
                passes = lists.scan_passes(variants, plan.scan["stride"])
        except (ValueError, OSError, bamio.BamError) as e:
            raise SystemExit(str(e))
        for k, members in passes:
            # (the rewrite takes a pass's whole list of a chromosome: smc_spike_alleles_reps' limit, and smc_spike_indels_reps')
            if "mnv" in plan.scan:              # (the rewrite's records are the member SNVs)
                chrom, n = collections.Counter(variants.sets[i].chrom for i in members).most_common(1)[0]
                n *= plan.scan["mnv"]
            else:
                chrom, n = collections.Counter(variants[i].chrom for i in members).most_common(1)[0]
            if n > SCAN_MAX_PASS_VARIANTS:
                raise SystemExit("--spikeScan: pass %d holds %d loci of %s, at most %d (a larger --spikeScanStride makes more and smaller "
                                 "passes)" % (k, n, chrom, SCAN_MAX_PASS_VARIANTS))
        index = {cp: i for i, cp in enumerate(leaders)} if "mnv" in plan.scan else {(v.chrom, v.pos): i for i, v in enumerate(variants)}
        seen, loci = set(), []
        for c, q in loc_list:
            if (c, int(q)) not in seen:
                seen.add((c, int(q)))
                loci.append((c, int(q), index.get((c, int(q)))))
        plan.scan.update(variants=variants, skipped=skipped, passes=passes, loci=loci, loc_list=loc_list)
        if "mnv" in plan.scan:
            print("--spikeScan: %d loci in %d passes of stride %d (--spikeScanMnv %d, %s), %d skipped for a position of the footprint that is "
                  "no locus of the target or whose letter is not A, C, G or T; %d replicates x %d targets" %
                  (len(leaders), len(passes), plan.scan["stride"], plan.scan["mnv"], plan.scan["alt"], len(skipped), plan.scan["reps"],
                   len(plan.scan["targets"])))
        elif "indel" in plan.scan:
            print("--spikeScan: %d loci in %d passes of stride %d (--spikeScanIndel %s%d), %d skipped for a letter inside the footprint "
                  "that is not A, C, G or T or lies past the chromosome's end; %d replicates x %d targets" %
                  ((len(variants), len(passes), plan.scan["stride"]) + plan.scan["indel"] + (len(skipped), plan.scan["reps"],
                                                                                              len(plan.scan["targets"]))))
        else:
            print("--spikeScan: %d loci in %d passes of stride %d (%s), %d skipped for a letter that is not A, C, G or T; %d replicates x %d "
                  "targets" % (len(variants), len(passes), plan.scan["stride"], plan.scan["alt"], len(skipped), plan.scan["reps"],
                               len(plan.scan["targets"])))


def _gather_ranks(args, params, loc_list, rank, local_rank, world):
    """One process per GPU when launched through torch.distributed.run: rank r calls a contiguous range of the ordered locus list
    (loci share nothing, smCounter.py:683-685) on GPU LOCAL_RANK, rank 0 gathers the rows in submission order -> every locus's row
    strings there, to be written; None on the other ranks."""
    import torch
    import torch.distributed as tdist
    # contiguous ranges balanced by depth, not by locus count (amplicon depth varies several-fold): the BAI's
    # linear index gives compressed bytes per 16 kb window without decoding anything; every rank computes the
    # same cuts
    cuts = smcdist.shard_by_reads(bamio.locus_weights(args.bamFile, loc_list), world)
    lo, hi = cuts[rank], cuts[rank + 1]
    # A failing locus (or a decoder error) on one rank must not leave the others waiting in the collective
    # until the RCCL timeout: every rank first agrees on a status, then all raise together or all gather.
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
        return None
    wires, refs, tabs = [], [], []
    for b in blocks:
        w, rf, tb = smcdist.unpack_shard(b.cpu().numpy())
        wires.append(w); refs += rf; tabs += tb
    all_rows = abi.unpack_wire(np.concatenate(wires)) if wires else np.zeros(0, abi.ROW_DTYPE)
    view = vc.LocusView([c for c, _ in loc_list], [int(p) for _, p in loc_list], refs, tabs)
    output = vc._strings(all_rows, view, params, fasta.FastaFile(args.refGenome))
    _report_boundary(all_rows, view.chrom, view.pos)
    return output


def _write_output(args, o, rows, loc_list, repeats, lod=None):
    """The files of output `o` from its raw rows: the repeat flags, the three files, and (`lod`: what lod.run_lods made for it) the
    LOD files beside them with their line in the run log -> its entry for the LOD summary, None without --lod."""
    pred = getattr(rows, "pred", None)                    # (single process: the printer's int(PI) per row)
    threshold = writers.pi_threshold(o.params.mtDepth, args.threshold)
    writers.write_outputs(o.prefix, postfilter.apply_repeat_filters(rows, *repeats, pred=pred), threshold, pred=pred)
    if lod is None:
        return None
    from . import lod as _lod
    depth_col = args.lodDepth or "UMT"
    _lod.write_lod(o.prefix, [c for c, _ in loc_list], [p for _, p in loc_list], lod["lods"])
    print("--lod %s: %d barcodes needed (mtDepth %d), depth %s, table of %d depths, at most %d iterations" %
          (o.prefix, lod["needed"], o.params.mtDepth, depth_col, lod["table"], lod["iters"]))
    return _lod.summary_entry(o.prefix, o.params.mtDepth, o.params.rpb, lod["needed"], lod["rows"], depth_col, lod["lods"])


def _af_reports(args, plan, shard, loc_list, repeats):
    """--dsAF: the titration on one page - every listed variant in the full-depth output and in every target's - and, with
    --dsAFReps, every replicate's row as its own run would print and cut it, then the rates."""
    from . import dsaf
    variants, res, af_outs, lods = plan.variants, plan.res, [o for o in plan.outputs if o.kind == "dsAF"], shard.lod
    outs = [(o.af, o.prefix, r["rows"] if r else None, lods[k]["lods"] if lods is not None else None)
            for k, (o, r) in enumerate(zip(plan.outputs, [None] + list(res)))]
    loc_index = {(c, "%d" % int(q)): n for n, (c, q) in enumerate(loc_list)}
    dsaf.write_detection(args.outPrefix, variants, outs, loc_index)
    reps = shard.af_reps
    ks = [[row["k"] for row in r["rows"]] for r in res]
    cell_outs = [o for o in plan.outputs if o.kind == "dsAFDepth"]
    if plan.depth is not None:
        # (--dsAFDepth: the same page over the cells; their outputs lie behind the targets')
        cells = [(o.af_index, o.af, o.frac, o.params.mtDepth, o.prefix, lods[1 + len(af_outs) + c]["lods"] if lods is not None else None)
                 for c, o in enumerate(cell_outs)]
        dsaf.write_depth_detection(args.outPrefix, variants, cells, plan.depth["counts"].reshape(len(variants), len(cells), 2), ks, loc_index)
    if reps is None:
        return

    def entries_of(outs, first, counts, what):
        """Every replicate of the outputs `outs` (the stage's cells from `first` on): the row as its own run prints and cuts it."""
        entries = {}
        for i, v in enumerate(variants):
            for t, o in enumerate(outs):
                thr_t = writers.pi_threshold(o.params.mtDepth, args.threshold)
                per = []
                for j in range(plan.reps):
                    row, cut = dsaf.replicate_entry(reps["rows"].get((i, first + t, j)), thr_t, *repeats)
                    per.append((int(counts[i, j, t, 0]), int(counts[i, j, t, 1]), row, cut))
                entries[(i, t)] = per
                called = sum(1 for _, _, _, cut in per if cut is not None and cut[0] == v.ref and v.alt in cut[1])
                print("--dsAFReps: %s:%d %s>%s at %s: called %d of %d" % (v.chrom, v.pos, v.ref, v.alt, what(o), called, plan.reps))
        return entries
    entries = entries_of(af_outs, 0, reps["counts"], lambda o: "%g" % o.af)
    targets_only = [o.af for o in af_outs]
    dsaf.write_replicates(args.outPrefix, variants, targets_only, reps["seeds"], ks, entries)
    lod_vt = None if lods is None else [[float(l["lods"][loc_index[(v.chrom, "%d" % v.pos)]]) for v in variants]
                                        for l in lods[1:1 + len(af_outs)]]
    dsaf.write_sensitivity(args.outPrefix, variants, targets_only, entries, lod_vt)
    if plan.depth is not None:
        dc = reps["depth_counts"]
        cell_entries = entries_of(cell_outs, len(af_outs), dc.reshape(dc.shape[0], dc.shape[1], len(cells), 2),
                                  lambda o: "%g x fraction %g" % (o.af, o.frac))
        dsaf.write_depth_replicates(args.outPrefix, variants, cells, reps["seeds"], ks, cell_entries)
        dsaf.write_depth_sensitivity(args.outPrefix, variants, cells, cell_entries, loc_index)
        full = [(o.params.mtDepth, lods[1 + t]["lods"] if lods is not None else None) for t, o in enumerate(af_outs)]
        dsaf.write_depth_curve(args.outPrefix, variants, targets_only, plan.depth["fracs"], full, cells, entries, cell_entries, loc_index)
    tm = reps["times"]
    over = "%d targets" % len(af_outs) + (" and %d cells" % len(cell_outs) if cell_outs else "")
    print("--dsAFReps: replicate stage %.3f s (%d replicates x %s: %d builds in %d batches; counts %.4f s, masks %.4f s)" %
          (tm["stage"], plan.reps, over, tm["builds"], tm["batches"], tm["counts"], tm["masks"]))


def _spike_cells(plan, lods, kind="spikeDepth"):
    """(--spikeDepth; `kind` "spikeRpb": --spikeRpb) per cell (target index, target, fraction or reads-per-barcode target, mtDepth,
    output prefix, that output's LODs or None), as spike's depth pages take them; the cells' outputs lie behind the targets'."""
    grid = kind == "spikeRpb" and plan.spike_rpb is not None and plan.spike_rpb.get("fracs") is not None
    return [(o.af_index, o.af, o.frac if kind == "spikeDepth" else (o.frac, o.target) if grid else o.target, o.params.mtDepth, o.prefix,
             lods[k]["lods"] if lods is not None else None) for k, o in enumerate(plan.outputs) if o.kind == kind]


def _spike_reports(args, plan, shard, loc_index, repeats):
    """--spikeReps: every replicate's row as its own run would print and cut it, then the rates and the curve."""
    from . import dsaf, spike as _spike
    variants, res, reps, lods = plan.spike["variants"], plan.spike["res"], shard.spike_reps, shard.lod
    outs = [o for o in plan.outputs if o.kind == "spikeAF"]
    targets, R = [o.af for o in outs], plan.spike_reps
    entries = {}
    for i, v in enumerate(variants):
        for t, o in enumerate(outs):
            thr_t = writers.pi_threshold(o.params.mtDepth, args.threshold)
            base = res[t]["rows"][i]
            per = []
            for j in range(R):
                row, cut = dsaf.replicate_entry(reps["rows"].get((i, t, j)), thr_t, *repeats)
                s, reads, v1 = (int(x) for x in reps["counts"][i, j, t])
                per.append((dict(N=base["N"], V0=base["V0"], S=s, READS=reads, V1=v1), row, cut))
            entries[(i, t)] = per
            print("--spikeReps: %s:%d %s>%s at %g: called %d of %d" % (v.chrom, v.pos, v.ref, v.alt, o.af, _spike._called(v, per), R))
    _spike.write_replicates(args.outPrefix, variants, targets, reps["seeds"], entries)
    lod_vt = None if lods is None else [[float(l["lods"][loc_index[(v.chrom, "%d" % v.pos)]]) for v in variants] for l in lods[1:1 + len(outs)]]
    _spike.write_sensitivity(args.outPrefix, variants, targets, entries, lod_vt)
    _spike.write_curve(args.outPrefix, variants, targets, entries, lod_vt)
    cell_entries = None
    for kind, info, axis in (("spikeDepth", plan.spike_depth, _spike.DEPTH_AXIS), ("spikeRpb", plan.spike_rpb, _spike.RPB_AXIS)):
        if info is None:
            continue
        # (--spikeDepth, --spikeRpb: the same three pages over the cells; their rows stand behind the targets' in the stage's)
        depth = kind == "spikeDepth"
        grid = not depth and info.get("fracs") is not None      # (--spikeGrid: the cells (t, f, r); the budget in the curve's place)
        if grid:
            axis = _spike.GRID_AXIS
        cells, T, dc = _spike_cells(plan, lods, kind), len(outs), reps["depth_counts" if depth else "rpb_counts"]
        cell_entries = {}
        for i, v in enumerate(variants):
            for c, o in enumerate(o for o in plan.outputs if o.kind == kind):
                thr_c = writers.pi_threshold(o.params.mtDepth, args.threshold)
                per = []
                for j in range(R):
                    row, cut = dsaf.replicate_entry(reps["rows"].get((i, T + c, j)), thr_c, *repeats)
                    per.append((dict(zip(("N", "V0", "S", "READS", "V1"), (int(x) for x in dc[i, j].reshape(-1, 5)[c]))), row, cut))
                cell_entries[(i, c)] = per
                if grid and per[0][0] != info["counts"][i][c]:
                    raise RuntimeError("--spikeGrid: %s:%d in %s: replicate 0 holds %r, the run's own cell %r" %
                                       (v.chrom, v.pos, o.prefix, per[0][0], info["counts"][i][c]))
                print("--spikeReps: %s:%d %s>%s at %g x %s%s %g: called %d of %d" % (v.chrom, v.pos, v.ref, v.alt, o.af, "fraction %g x " % o.frac if grid else "",
                                                                                     "fraction" if depth else "target",
                                                                                     o.frac if depth else o.target, _spike._called(v, per), R))
        _spike.write_depth_replicates(args.outPrefix, variants, cells, reps["seeds"], cell_entries, axis)
        _spike.write_depth_sensitivity(args.outPrefix, variants, cells, cell_entries, loc_index, axis)
        if grid:
            kept = [o.rule.n_kept for o in plan.outputs if o.kind == kind]
            _spike.write_budget(args.outPrefix, variants, [c + (n,) for c, n in zip(cells, kept)], info["file_names"], cell_entries)
            continue
        full = [(o.params.mtDepth, lods[1 + t]["lods"] if lods is not None else None) for t, o in enumerate(outs)]
        _spike.write_depth_curve(args.outPrefix, variants, targets, info["fracs"] if depth else info["targets"], full, cells, entries, cell_entries,
                                 loc_index, axis)
    phase = plan.spike.get("phase")
    if phase is not None:
        # (--spikePhase: a set is called in a replicate when every member is; the joint counts are the stage's own call's)
        F = len(plan.spike_depth["fracs"]) if plan.spike_depth is not None else 0
        p_outs = [(o.af, None, o.params.mtDepth) for o in outs] + \
                 [(o.af, o.frac, o.params.mtDepth) for o in plan.outputs if o.kind == "spikeDepth"]
        p_entries = {}
        for g, ps in enumerate(phase["sets"]):
            for c in range(len(p_outs)):
                t, f = (c, None) if c < len(outs) else divmod(c - len(outs), F)
                per = []
                for j in range(R):
                    got = reps["phase_counts"][g, j, t] if f is None else reps["phase_depth_counts"][g, j, t, f]
                    of = [(entries[(i, t)] if f is None else cell_entries[(i, c - len(outs))])[j] for i in ps.members]
                    per.append((dict(zip(_spike.PHASE_NAMES, (int(x) for x in got))),
                                int(all(_spike._called(variants[i], [e]) for i, e in zip(ps.members, of)))))
                p_entries[(g, c)] = per
        _spike.write_phase_replicates(args.outPrefix, variants, phase["sets"], p_outs, reps["seeds"], p_entries)
        _spike.write_phase_sensitivity(args.outPrefix, variants, phase["sets"], p_outs, p_entries)
        if reps.get("phase_rpb_counts") is not None:
            # (--spikePhaseRpb: the same two pages over the cells (t, r); replicate 0 is the run's own cell)
            r_outs = [(o.af, o.target, o.params.mtDepth) for o in plan.outputs if o.kind == "spikeRpb"]
            Rr = len(plan.spike_rpb["targets"])
            r_entries = {}
            for g, ps in enumerate(phase["sets"]):
                for c in range(len(r_outs)):
                    t, r = divmod(c, Rr)
                    per = []
                    for j in range(R):
                        got = dict(zip(_spike.PHASE_NAMES, (int(x) for x in reps["phase_rpb_counts"][g, j, t, r])))
                        per.append((got, int(all(_spike._called(variants[i], [cell_entries[(i, c)][j]]) for i in ps.members))))
                    if per[0][0] != phase["rpb_counts"][g][c]:
                        raise RuntimeError("--spikePhaseRpb: set %s at %g x target %g: replicate 0 holds %r, the run's own cell %r" %
                                           (ps.name, r_outs[c][0], r_outs[c][1], per[0][0], phase["rpb_counts"][g][c]))
                    r_entries[(g, c)] = per
            _spike.write_phase_replicates(args.outPrefix, variants, phase["sets"], r_outs, reps["seeds"], r_entries, _spike.RPB_AXIS)
            _spike.write_phase_sensitivity(args.outPrefix, variants, phase["sets"], r_outs, r_entries, _spike.RPB_AXIS)
    tm = reps["times"]
    print("--spikeReps: replicate stage %.3f s (%d replicates x %d targets: counts call %.4f s, %d rewrite calls, %d builds in %d batches, "
          "%.3f s)" % (tm["stage"], R, len(outs), tm["counts"], tm["rewrites"], tm["builds"], tm["batches"], tm["calls"]))


def _scan_reports(args, plan, shard):
    """--spikeScan: the two pages and the bedgraphs from the stage's verdicts and counts, and the closing line of the run log."""
    from . import spike as _spike
    scan, out = plan.scan, shard.scan
    variants, targets, R = scan["variants"], scan["targets"], scan["reps"]
    if "mnv" in scan:
        return _scan_mnv_reports(args, plan, shard)
    entries = {}
    for i, v in enumerate(variants):
        n, v0 = out["base"][i]
        for t in range(len(targets)):
            entries[(i, t)] = [_spike.scan_entry(v, dict(N=n, V0=v0, S=int(s), READS=int(reads), V1=int(v1)), bool(out["called"][i, t, j]))
                               for j, (s, reads, v1) in enumerate(out["counts"][i, :, t].tolist())]
    lods = None
    if shard.lod is not None:
        # (--lod: the full-depth output's LOD at the locus - the scan has no output of its own per target)
        at, first = {}, shard.lod[0]["lods"]
        for n, (c, q) in enumerate(scan["loc_list"]):
            at.setdefault((c, int(q)), n)
        lods = [float(first[at[(v.chrom, v.pos)]]) for v in variants]
    _spike.write_scan(args.outPrefix, scan["loci"], variants, targets, entries, lods)
    tm = out["times"]
    print("--spikeScan: %d loci x %d targets x %d replicates in %d passes: %d runs decoded once each (%.3f s), %d copies built and "
          "called, %d of %d verdicts decided by the host, stage %.3f s" %
          (len(variants), len(targets), R, len(scan["passes"]), tm["runs"], tm["decode"], sum(st["builds"] for st in out["passes"]),
           sum(st["host"] for st in out["passes"]), len(variants) * len(targets) * R * (1 + len(scan.get("fracs", scan.get("rpbs", ())))),
           tm["stage"]))
    if "fracs" in scan:
        fracs = scan["fracs"]
        cells = {}
        for i, v in enumerate(variants):
            for t in range(len(targets)):
                for f in range(len(fracs)):
                    cells[(i, t, f)] = [_spike.scan_entry(v, dict(N=int(n), V0=int(v0), S=int(s), READS=int(reads), V1=int(v1)),
                                                          bool(out["depth_called"][i, t, f, j]))
                                        for j, (n, v0, s, reads, v1) in enumerate(out["depth_counts"][i, :, t, f].tolist())]
        _spike.write_scan_depth(args.outPrefix, scan["loci"], variants, targets, fracs, plan.outputs[0].params.mtDepth, entries, cells)
        print("--spikeScanDepth: fractions %s: %d cells per pass, %d select_copies calls" %
              (",".join("%g" % f for f in fracs), len(targets) * len(fracs), sum(st["selects"] for st in out["passes"])))
    if "rpbs" in scan:
        rpbs = scan["rpbs"]
        cells = {}
        for i, v in enumerate(variants):
            for t in range(len(targets)):
                for r in range(len(rpbs)):
                    cells[(i, t, r)] = [_spike.scan_entry(v, dict(N=int(n), V0=int(v0), S=int(s), READS=int(reads), V1=int(v1)),
                                                          bool(out["rpb_called"][i, t, r, j]))
                                        for j, (n, v0, s, reads, v1) in enumerate(out["rpb_counts"][i, :, t, r].tolist())]
        params = plan.outputs[0].params
        _spike.write_scan_rpb(args.outPrefix, scan["loci"], variants, targets, rpbs, params.mtDepth, params.rpb, entries, cells)
        print("--spikeScanRpb: reads-per-barcode targets %s: %d cells per pass, %d select_copies_reads calls" %
              (",".join("%g" % r for r in rpbs), len(targets) * len(rpbs), sum(st["selects"] for st in out["passes"])))
        for r, rule in zip(rpbs, out["rpb_rules"]):
            print("--spikeScanRpb %g: sampler philox, seed %d, probKeep %.6g, threshold %d, %d of %d read names kept (mtDepth %d)" %
                  (r, rule["seed"], rule["prob_keep"], rule["thr"], rule["n_kept"], rule["n_names"], params.mtDepth))
    if "filter" in scan:
        _scan_filter_reports(args, plan, shard)


def _scan_mnv_reports(args, plan, shard):
    """--spikeScanMnv: the two pages and the bedgraphs from the stage's joint verdicts and counts, and the closing lines of the run log."""
    from . import spike as _spike
    scan, out = plan.scan, shard.scan
    variants, targets, R = scan["variants"], scan["targets"], scan["reps"]
    sets = variants.sets
    entries = {}
    for i in range(len(sets)):
        for t in range(len(targets)):
            entries[(i, t)] = [(dict(zip(_spike.PHASE_NAMES, (int(x) for x in out["joint_counts"][i, j, t]))), int(out["joint_called"][i, t, j]))
                               for j in range(R)]
    _spike.write_scan_mnv(args.outPrefix, scan["loci"], variants, sets, targets, plan.outputs[0].params.mtDepth, entries)
    tm = out["times"]
    print("--spikeScan: %d loci x %d targets x %d replicates in %d passes: %d runs decoded once each (%.3f s), %d copies built and "
          "called, %d of %d verdicts decided by the host, stage %.3f s" %
          (len(sets), len(targets), R, len(scan["passes"]), tm["runs"], tm["decode"], sum(st["builds"] for st in out["passes"]),
           sum(st["host"] for st in out["passes"]), len(variants) * len(targets) * R, tm["stage"]))
    closing = "--spikeScanMnv %d: %d sets scanned, %d loci skipped, %d of %d joint verdicts decided by the host" % \
        (scan["mnv"], len(sets), len(scan["skipped"]), out["joint_host"],
         len(sets) * len(targets) * R * (1 + len(scan.get("mnv_fracs", scan.get("mnv_rpbs", ())))))
    mt_depth, fracs, rpbs = plan.outputs[0].params.mtDepth, scan.get("mnv_fracs"), scan.get("mnv_rpbs")
    if rpbs is not None:
        cells = {(i, t, r): [(dict(zip(_spike.PHASE_NAMES, (int(x) for x in out["joint_rpb_counts"][i, j, t, r]))),
                              int(out["joint_rpb_called"][i, t, r, j])) for j in range(R)]
                 for i in range(len(sets)) for t in range(len(targets)) for r in range(len(rpbs))}
        _spike.write_scan_mnv_rpb(args.outPrefix, scan["loci"], variants, sets, targets, rpbs, mt_depth, plan.outputs[0].params.rpb, entries, cells)
    if fracs is not None:
        cells = {(i, t, f): [(dict(zip(_spike.PHASE_NAMES, (int(x) for x in out["joint_depth_counts"][i, j, t, f]))),
                              int(out["joint_depth_called"][i, t, f, j])) for j in range(R)]
                 for i in range(len(sets)) for t in range(len(targets)) for f in range(len(fracs))}
        _spike.write_scan_mnv_depth(args.outPrefix, scan["loci"], variants, sets, targets, fracs, mt_depth, entries, cells)
    if "mnv_filter" in scan:
        _spike.write_scan_mnv_filter(args.outPrefix, scan["loci"], variants, sets, targets, [int(out["joint_counts"][i, 0, 0, 0]) for i in range(len(sets))],
                                     out["joint_called"], out["joint_filter"])
        held = [(out["joint_called"], out["joint_filter"] & np.uint32(abi.SCAN_FLT_NAMES_MASK))]
        if fracs is not None:
            _spike.write_scan_filter_cells(args.outPrefix, [_spike.scan_mnv_variant(ps, variants) for ps in sets], targets, fracs,
                                           [_spike.scan_depth_mt(mt_depth, f) for f in fracs], out["joint_depth_called"], out["joint_depth_filter"],
                                           mnv=True)
            held.append((out["joint_depth_called"], out["joint_depth_filter"] & np.uint32(abi.SCAN_FLT_NAMES_MASK)))
        if rpbs is not None:
            _spike.write_scan_filter_cells(args.outPrefix, [_spike.scan_mnv_variant(ps, variants) for ps in sets], targets, rpbs,
                                           [mt_depth] * len(rpbs), out["joint_rpb_called"], out["joint_rpb_filter"], _spike.RPB_AXIS, mnv=True)
            held.append((out["joint_rpb_called"], out["joint_rpb_filter"] & np.uint32(abi.SCAN_FLT_NAMES_MASK)))
        closing += "; --spikeScanMnvFilter: %d of %d called sets PASS, the FILTER of %d decided by the host; %s" % \
            (sum(int((c & (w == 0)).sum()) for c, w in held), sum(int(c.sum()) for c, _ in held), out["joint_filter_host"],
             ", ".join("%s %d" % (name, sum(int((c & ((w & bit) != 0)).sum()) for c, w in held)) for bit, name in abi.SCAN_FILTER_NAMES))
    if fracs is not None:
        closing += "; --spikeScanMnvDepth: fractions %s: %d cells per pass, %d builds (S x R x T x (1 + F)), %d select_copies calls" % \
            (",".join("%g" % f for f in fracs), len(targets) * len(fracs), sum(st["builds"] for st in out["passes"]),
             sum(st["selects"] for st in out["passes"]))
    if rpbs is not None:
        closing += "; --spikeScanMnvRpb: reads-per-barcode targets %s: %d cells per pass, %d builds (S x R x T x (1 + Rr)), " \
                   "%d select_copies_reads calls" % (",".join("%g" % r for r in rpbs), len(targets) * len(rpbs),
                                                     sum(st["builds"] for st in out["passes"]), sum(st["selects"] for st in out["passes"]))
    print(closing)
    for r, rule in zip(rpbs or (), out.get("rpb_rules", ())):
        print("--spikeScanMnvRpb %g: sampler philox, seed %d, probKeep %.6g, threshold %d, %d of %d read names kept (mtDepth %d)" %
              (r, rule["seed"], rule["prob_keep"], rule["thr"], rule["n_kept"], rule["n_names"], mt_depth))


def _scan_filter_reports(args, plan, shard):
    """--spikeScanFilter: the filter pages from the stage's verdicts and FILTER words, and the closing line of the run log."""
    from . import spike as _spike
    scan, out = plan.scan, shard.scan
    variants, targets = scan["variants"], scan["targets"]
    mt_depth = plan.outputs[0].params.mtDepth
    _spike.write_scan_filter(args.outPrefix, scan["loci"], variants, targets, [n for n, _ in out["base"]], out["called"], out["filter"])
    held = [(out["called"], out["filter"])]
    if "fracs" in scan:
        _spike.write_scan_filter_cells(args.outPrefix, variants, targets, scan["fracs"], [_spike.scan_depth_mt(mt_depth, f) for f in scan["fracs"]],
                                       out["depth_called"], out["depth_filter"])
        held.append((out["depth_called"], out["depth_filter"]))
    if "rpbs" in scan:
        _spike.write_scan_filter_cells(args.outPrefix, variants, targets, scan["rpbs"], [mt_depth] * len(scan["rpbs"]), out["rpb_called"],
                                       out["rpb_filter"], _spike.RPB_AXIS)
        held.append((out["rpb_called"], out["rpb_filter"]))
    n_called = sum(int(c.sum()) for c, _ in held)
    n_pass = sum(int((c & (w == 0)).sum()) for c, w in held)
    totals = [sum(int((c & ((w & bit) != 0)).sum()) for c, w in held) for bit, _ in abi.SCAN_FILTER_NAMES]
    print("--spikeScanFilter: %d of %d called records PASS, the FILTER of %d decided by the host; %s" %
          (n_pass, n_called, out["filter_host"], ", ".join("%s %d" % (name, n) for (_, name), n in zip(abi.SCAN_FILTER_NAMES, totals))))


def _run(args, plan, loc_list, t0):
    params = plan.outputs[0].params
    rank, local_rank, world = smcdist.init_from_env()
    if world == 1:
        # a single process never touches torch.distributed: bind the C ABI without importing PyTorch first
        # (about a second of start-up; the host-buffer entry point needs none of it)
        _lib.load(with_torch=False)
        # (the keywords only when there is something in them: a stand-in for call_shard may know neither)
        more = {k: v for k, v in (("early", plan.early), ("plan", plan if len(plan.outputs) > 1 or plan.scan is not None else None))
                if v is not None}
        shard = call_shard(args, params, loc_list, args.device, **more)
        if not isinstance(shard, _Shard):                  # (a plain list of row strings: the full-depth output alone)
            shard = _Shard(shard)
    else:
        rows = _gather_ranks(args, params, loc_list, rank, local_rank, world)
        if rows is None:
            return writers.pi_threshold(params.mtDepth, args.threshold)
        shard = _Shard(rows)
    vc.raise_on_exception(shard.rows, loc_list)
    print("begin variant filtering and output")
    tracks = _repeat_tracks(args)
    if None in tracks:
        print("note: repeat tracks not given or not found; RepT/RepS/LowC/SL flags are not applied", file=sys.stderr)
    repeats = postfilter.load_repeat_regions(args.bedTarget, *tracks)
    lod_entries = []
    for k, (o, rows) in enumerate(zip(plan.outputs, [shard.rows] + list(shard.ds))):
        if k:                                              # (output 0 was looked at before this stage began)
            vc.raise_on_exception(rows, loc_list)
        lod_entries.append(_write_output(args, o, rows, loc_list, repeats, shard.lod[k] if shard.lod is not None else None))
    if shard.lod is not None:
        from . import lod as _lod
        _lod.write_summary(args.outPrefix, lod_entries)
    if plan.variants is not None:
        _af_reports(args, plan, shard, loc_list, repeats)
    if plan.spike is not None:
        # (--spikeAF: every listed variant in the full-depth output and in every target's, on one page)
        from . import spike as _spike
        lods = shard.lod
        outs = [(o.af, o.prefix, r["rows"] if r else None, lods[k]["lods"] if lods is not None else None)
                for k, (o, r) in enumerate(zip(plan.outputs, [None] + list(plan.spike["res"])))]
        loc_index = {(c, "%d" % int(q)): n for n, (c, q) in enumerate(loc_list)}
        _spike.write_detection(args.outPrefix, plan.spike["variants"], outs, loc_index)
        if plan.spike_depth is not None:
            _spike.write_depth_detection(args.outPrefix, plan.spike["variants"], _spike_cells(plan, lods), plan.spike_depth["counts"], loc_index)
        if plan.spike_rpb is not None:
            _spike.write_depth_detection(args.outPrefix, plan.spike["variants"], _spike_cells(plan, lods, "spikeRpb"),
                                         plan.spike_rpb["counts"], loc_index,
                                         _spike.GRID_AXIS if plan.spike_rpb.get("fracs") is not None else _spike.RPB_AXIS)
        phase = plan.spike.get("phase")
        if phase is not None:
            # (--spikePhase: every set in the full-depth output - nothing spiked there -, in every target's and in every cell's)
            sp = [o for o in plan.outputs if o.kind == "spikeAF"]
            full = [dict(c[0], S_ALL=0, V1_ALL=c[0]["V0_ALL"]) for c in phase["counts"]]
            p_outs = [(None, None, params.mtDepth, plan.outputs[0].prefix, full)] + \
                     [(o.af, None, o.params.mtDepth, o.prefix, [c[t] for c in phase["counts"]]) for t, o in enumerate(sp)] + \
                     [(o.af, o.frac, o.params.mtDepth, o.prefix, [c[k] for c in phase["depth_counts"]])
                      for k, o in enumerate(o for o in plan.outputs if o.kind == "spikeDepth")]
            _spike.write_phase(args.outPrefix, plan.spike["variants"], phase["sets"], p_outs)
            if phase.get("rpb_counts") is not None:
                # (--spikePhaseRpb: every set in every cell (t, r), counted over the reads the cell keeps)
                r_outs = [(o.af, o.target, o.params.mtDepth, o.prefix, [c[k] for c in phase["rpb_counts"]])
                          for k, o in enumerate(o for o in plan.outputs if o.kind == "spikeRpb")]
                _spike.write_phase(args.outPrefix, plan.spike["variants"], phase["sets"], r_outs, _spike.RPB_AXIS)
        if shard.spike_reps is not None:
            _spike_reports(args, plan, shard, loc_index, repeats)
    if shard.scan is not None:
        _scan_reports(args, plan, shard)
    t1 = datetime.datetime.now()
    print("smCounter completed running at " + str(t1))
    print("smCounter total time: " + str(t1 - t0))
    return writers.pi_threshold(params.mtDepth, args.threshold)


if __name__ == "__main__":
    ns = build_parser().parse_args()
    if ns.logFile:
        runlog.init(ns.logFile)
    try:
        main(ns)
    finally:
        runlog.close()
