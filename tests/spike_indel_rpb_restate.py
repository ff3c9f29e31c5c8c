"""Host restatement of --spikeIndelRpb (DESIGN.md "--spikeIndelRpb"): cell (t, r) of replicate j is the --spikeIndels spike-in at t with
seed s_j, of which a record stays when the --dsRpb philox rule keeps its read name with the same seed.  Everything is counted PER
RECORD, in numpy / Python: a record's four bits - covers, alt0, alt1, touch - come from spike_indel_restate.layout / resolve and
af.read_key as spike_indel_reps_restate.host_counters derives them per barcode; the grouping, probKeep and the read draw are
tests/ds_rpb_philox_restate.py's, the spike draw tests/spike_restate.py's.  Nothing from smc_spike_indel_read_bits,
smc_spike_indel_rpb_counts or the host code around them.  Shared by tests/test_spike_indel_rpb.py, tests/test_gpu_spike_indel_rpb.py
and tests/test_gpu_spike_indel_rpb_cli.py."""
import collections
import os
import sys

import numpy as np

from smcounter_amd import bamio
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ds_af_restate as R  # noqa: E402
import ds_rpb_philox_restate as rp  # noqa: E402
import spike_indel_reps_restate as QR  # noqa: E402
import spike_indel_restate as IR  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402
import spike_rpb_restate as RR  # noqa: E402

seeds, threshold = PR.seeds, PR.threshold
file_groups, read_thresholds = RR.file_groups, RR.read_thresholds
NAMES = RR.NAMES
ONE = 1 << 32
COVERS, ALT0, ALT1, TOUCH = 1, 2, 4, 8          # the bits of a record's byte
CASES = QR.CASES
# a covering record of a listed variant: its barcode text, its full read name, whether that name is its barcode's first in the file,
# whether it shows the variant's key as it is, whether it shows it when its barcode is spiked, whether the rewrite changes it then;
# `case`: which of CASES it is at a listed indel, or None
Rec = collections.namedtuple("Rec", "barcode name first alt0 alt1 touch case")
SEED = RR.SEED
# the synthetic input of the GPU tests: spike_rpb_restate's (6 reads per barcode, one base in ten miscalled, reads inside deletions);
# 1.5 and 3 thin, 20 keeps every name
SYNTH_CFG = RR.SYNTH_CFG
RPB_TARGETS = RR.RPB_TARGETS
SYNTH_LOCI = 160                                # (room for four listed variants 24 positions apart)


def record_bits(a, v, chrom, genome=None):
    """The four bits of record `a` (bamio's readable decoder) at listed variant `v`, and its case -> (byte, case); (0, None) for a
    record that does not span the position."""
    if not (a.pos < v.pos <= a.end):
        return 0, None
    units, at = IR.layout(a)
    shows = af.read_key(a, v.pos, chrom, genome) == af.variant_key(v, genome)
    u = IR.resolve(a, units, at, v)
    n = IR.length(v)
    if v.kind != af.SNV and (len(a.cigar) + 2 > IR.MAX16 or (v.kind == af.INS and a.l_seq + n > IR.MAX16)):
        u = None
    touch = u is not None
    case = None
    if v.kind == af.SNV:
        alt1 = touch
    else:
        anchor_ok = touch and a.seq[units[u]["q"]] == v.ref[0]
        alt1 = anchor_ok if touch else shows
        if touch and not anchor_ok:
            case = "anchor_mismatch"
        elif not touch and shows:
            case = "shows_it_already"
        elif not touch and v.pos - 1 < a.end <= IR.footprint(v)[1] - 1:
            case = "ends_in_footprint"
    return COVERS | (ALT0 if shows else 0) | (ALT1 if alt1 else 0) | (TOUCH if touch else 0), case


def placed_records(bam_path):
    """-> (the file's placed records in file order, the chromosome name of each tid)."""
    bam = bamio.BamFile(bam_path)
    bam._bg.seek(bam._first_record)
    recs = [a for a in bam._records() if a.tid >= 0 and not (a.flag & 4) and a.cigar]
    chrom_of = [name for name, _ in bam.refs]
    bam.close()
    return recs, chrom_of


def records(bam_path, fa_path, variants, groups=None):
    """Per listed variant (SNV, insertion, deletion) the records that span it, in file order -> [[Rec]]."""
    from smcounter_amd import fasta
    groups = groups or file_groups(bam_path)
    genome = fasta.FastaFile(fa_path) if fa_path is not None else None
    recs, chrom_of = placed_records(bam_path)
    out = [[] for _ in variants]
    for a in recs:
        chrom = chrom_of[a.tid]
        for k, v in enumerate(variants):
            if v.chrom != chrom or not (a.pos < v.pos <= a.end):
                continue
            bc = af.barcode_of(a.qname)
            assert bc is not None, "a placed record without a barcode: %s" % a.qname
            b, case = record_bits(a, v, chrom, genome)
            out[k].append(Rec(bc, a.qname, groups["is_first"][a.qname], bool(b & ALT0), bool(b & ALT1), bool(b & TOUCH), case))
    return out


def record_bytes(rows):
    """The byte smc_spike_indel_read_bits writes for each covering record, in their order."""
    return np.array([COVERS | (ALT0 if r.alt0 else 0) | (ALT1 if r.alt1 else 0) | (TOUCH if r.touch else 0) for r in rows], np.uint8)


def cases(rows):
    return {c: sum(1 for r in rows if r.case == c) for c in CASES}


def barcode_counters(rows):
    """-> (barcode texts, sorted, uint32 [n, 4] = (reads, alt0, alt1, touch) over ALL records): spike_indel_reps_restate.host_counters'."""
    texts = sorted({r.barcode for r in rows})
    at = {b: k for k, b in enumerate(texts)}
    cnt = np.zeros((len(texts), 4), np.uint32)
    for r in rows:
        cnt[at[r.barcode]] += np.array([1, r.alt0, r.alt1, r.touch], np.uint32)
    return texts, cnt


def kept(rows, rthr, seed):
    """bool per record: the --dsRpb philox rule keeps its name at read threshold `rthr` with `seed`."""
    if not rows:
        return np.zeros(0, bool)
    u = rp.draws(rp.fnv64([r.name for r in rows]), seed).astype(np.uint64)
    return np.array([r.first for r in rows], bool) | (u < np.uint64(rthr))


def kept_counters(rows, rthr, seed):
    """-> (barcode texts, sorted, int64 [n, 4] = (reads_r, alt0_r, alt1_r, touch_r) over the records kept at `rthr` with `seed`)."""
    texts = sorted({r.barcode for r in rows})
    cnt = np.zeros((len(texts), 4), np.int64)
    if not rows:
        return texts, cnt
    at = {b: k for k, b in enumerate(texts)}
    inv = np.array([at[r.barcode] for r in rows], np.int64)
    k = kept(rows, rthr, seed)
    for c, col in enumerate((np.ones(len(rows), bool), np.array([r.alt0 for r in rows], bool), np.array([r.alt1 for r in rows], bool),
                             np.array([r.touch for r in rows], bool))):
        cnt[:, c] = np.bincount(inv[k & col], minlength=len(texts))
    return texts, cnt


def cell_rule(cnt, u, thr):
    """(N', V0', S', READS', V1') from the kept records' four counters of every barcode and the spike draws; thr in [0, 2^32]."""
    reads, alt0, alt1, touch = (cnt[:, k].astype(np.int64) for k in range(4))
    there = reads > 0
    hit = np.asarray(u).astype(np.uint64) < np.uint64(thr)
    car0, car1 = 2 * alt0 > reads, 2 * alt1 > reads
    return [int(there.sum()), int((there & car0).sum()), int((there & hit).sum()), int(touch[there & hit].sum()),
            int((there & np.where(hit, car1, car0)).sum())]


def counts_from(recs, positions, thr, rthr, seed_list):
    """uint32 [V, R, T, Rr, 5] from per variant its covering records ([Rec]), the 1-based positions and the thresholds of both axes."""
    out = np.zeros((len(recs), len(seed_list), len(thr), len(rthr), 5), np.uint32)
    for i, (rows, pos) in enumerate(zip(recs, positions)):
        for j, s in enumerate(seed_list):
            for r, q in enumerate(rthr):
                texts, cnt = kept_counters(rows, q, s)
                u = SR.draw(texts, s, pos) if texts else np.zeros(0, np.uint64)
                for t, h in enumerate(thr):
                    out[i, j, t, r] = cell_rule(cnt, u, h)
    return out


def restate_counts(bam_path, fa_path, variants, targets, rpb_targets, seed, n_reps):
    """-> (uint32 [V, R, T, Rr, 5], the covering records, the read thresholds)."""
    groups = file_groups(bam_path)
    recs = records(bam_path, fa_path, variants, groups)
    rthr = read_thresholds(groups, rpb_targets)
    return counts_from(recs, [v.pos for v in variants], [threshold(t) for t in targets], rthr, seeds(seed, n_reps)), recs, rthr


def pick_shown_indel(bam_path, fa_path, loci, avoid=(), gap=24):
    """A listed deletion or insertion that some reads of the file show already and others, in the same barcodes, do not: the indel key
    of the pileups of `loci` with the most barcodes whose reads disagree about it, at least `gap` positions from every position of
    `avoid` -> IR.variant, or None."""
    pb = R.pileups(bam_path, fa_path, loci)
    best = None
    for l, (c, p) in enumerate(loci):
        if any(abs(int(p) - int(q)) < gap for q in avoid) or pb.ref[l] not in "ACGT":
            continue
        for key in pb.alleles[l]:
            if "|" not in key:
                continue
            _, reads, alt = R.counts(pb, l, key)
            v = R.variant_of_key(c, int(p), pb.ref[l], key)
            if not (set(v.ref) | set(v.alt)) <= set("ACGT") or max(len(v.ref), len(v.alt)) > 20:
                continue
            score = (int(((alt > 0) & (alt < reads)).sum()), int((alt > 0).sum()))
            if score[0] and (best is None or score > best[0]):
                best = (score, IR.variant(c, int(p), v.ref, v.alt))
    return best[1] if best else None


def synth_inputs(tmp):
    """-> (bam, fasta path, VcParams, the listed variants of synth_case)."""
    bam, fa, loci, P, variants = synth_case(tmp)
    return bam, fa, P, variants


def synth_case(tmp):
    """-> (bam, fasta path, loci, VcParams, listed variants sorted by position: an SNV at which barcodes disagree (spike_rpb_restate's pick),
    the insertion of GA and the deletion of 3 spike_indel_restate.pick_variants lists at the deepest loci, and an indel that some
    reads show already)."""
    bam, fa, loci, P, _ = R.synth_bam(tmp, SYNTH_CFG, SYNTH_LOCI)
    snv = RR.pick_mixed(bam, fa, loci, 1)[0]
    out = [IR.variant(snv.chrom, snv.pos, snv.ref, snv.alt)]
    shown = pick_shown_indel(bam, fa, loci, [v.pos for v in out])
    if shown is not None:
        out.append(shown)
    far = [(c, p) for c, p in loci if all(abs(int(p) - v.pos) >= 24 for v in out)]
    out += [v for v in IR.pick_variants(bam, fa, far, 2, gap=24)]
    return bam, fa, loci, P, sorted(out, key=lambda v: (v.chrom, v.pos))
