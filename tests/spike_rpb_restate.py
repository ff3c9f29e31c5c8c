"""Host restatement of --spikeRpb (DESIGN.md "--spikeRpb"): cell (t, r) of replicate j is the --spikeAF spike-in at t with seed s_j,
of which a record stays when the --dsRpb philox rule keeps its read name with the same seed - the name is its barcode's first,
file-wide, or its "dsRP" draw is below the read threshold of r.  Everything is counted PER RECORD, in numpy / Python: the grouping,
probKeep and the read draw are tests/ds_rpb_philox_restate.py's, the spike draw and the host pileups tests/spike_restate.py's and
tests/ds_af_restate.py's (bamio's readable decoder).  Nothing from smc_spike_read_bits, smc_spike_rpb_counts or the host code around
them.  Shared by tests/test_spike_rpb.py and tests/test_gpu_spike_rpb.py."""
import collections
import dataclasses
import os
import sys

import numpy as np

from smcounter_amd import bamio

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import ds_rpb_philox_restate as rp  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402

seeds, threshold = PR.seeds, PR.threshold
NAMES = ("N", "V0", "S", "READS", "V1")
ONE = 1 << 32
COVERS, ALT, SINGLE = 1, 2, 4          # the bits of a record's byte
# a covering record of a listed variant: its barcode text, its full read name, whether that name is its barcode's first in the file,
# whether the record shows ALT as it is, whether its allele key is a single letter
Rec = collections.namedtuple("Rec", "barcode name first alt single")
# the synthetic input of the GPU tests: ds_af_restate.SYNTH_CFG (6 reads per barcode) with one base in ten miscalled and more reads
# inside deletions, so that many barcodes hold reads that disagree and thinning can flip their majority; the targets 1.5 and 3 thin
# (probKeep about 0.15 and 0.6), 20 keeps every name (probKeep >= 1)
SEED = 20240607
SYNTH_CFG = dataclasses.replace(R.SYNTH_CFG, p_err=0.1, p_gap=0.03)
RPB_TARGETS = (1.5, 3, 20)


def file_groups(bam_path):
    """The file-wide grouping of the placed read names (ds.reads.withinMT.py:37-58) -> rp.group's dict, with `is_first`: name -> bool."""
    g = rp.group(ds_restate.placed_qnames(bam_path))
    g["is_first"] = dict(zip(g["names"], (bool(x) for x in g["first"])))
    return g


def read_thresholds(groups, rpb_targets):
    """floor(probKeep_r x 2^32) clamped to [0, 2^32], per reads-per-barcode target."""
    return [rp.threshold(rp.prob_keep(groups["counts"], float(r))) for r in rpb_targets]


def records(bam_path, fa_path, variants, groups=None):
    """Per listed SNV the records of its pileup, in file order -> [[Rec]]."""
    groups = groups or file_groups(bam_path)
    pb = R.pileups(bam_path, fa_path, [(v.chrom, v.pos) for v in variants])
    bam = bamio.BamFile(bam_path)
    out = []
    try:
        for l, v in enumerate(variants):
            recs = bam.fetch(v.chrom, v.pos - 1, v.pos)
            sl = pb.locus_slice(l)
            assert len(recs) == sl.stop - sl.start, "the pileup of %s:%d is not the records that span it" % (v.chrom, v.pos)
            rows = []
            for k, a in enumerate(recs):
                i = sl.start + k
                key = pb.alleles[l][int(pb.allele[i])]
                rows.append(Rec(pb.umi_names[l][int(pb.umi[i])], a.qname, groups["is_first"][a.qname], key == v.alt, len(key) == 1))
            out.append(rows)
    finally:
        bam.close()
    return out


def pick_mixed(bam_path, fa_path, loci, n=3):
    """Listed SNVs at which thinning reads can flip a barcode: the `n` loci with the most barcodes whose reads disagree about one
    non-reference letter (0 < alt < reads; then the most carriers), that letter the ALT -> variants sorted by position."""
    pb = R.pileups(bam_path, fa_path, loci)
    found = []
    for l, (c, p) in enumerate(loci):
        best = None
        for key in pb.alleles[l]:
            if len(key) == 1 and key in "ACGT" and key != pb.ref[l] and pb.ref[l] in "ACGT":
                _, reads, alt = R.counts(pb, l, key)
                score = (int(((alt > 0) & (alt < reads)).sum()), int((2 * alt > reads).sum()))
                if best is None or score > best[0]:
                    best = (score, key)
        if best is not None and best[0][0]:
            found.append((best[0], -l, R.V(c, p, pb.ref[l], best[1], best[1])))
    return sorted((v for _, _, v in sorted(found, reverse=True)[:n]), key=lambda v: (v.chrom, v.pos))


def synth_inputs(tmp):
    """-> (bam, fasta path, VcParams, three listed SNVs at the loci with the most barcodes of disagreeing reads)."""
    bam, fa, loci, P, _ = R.synth_bam(tmp, SYNTH_CFG)
    return bam, fa, P, pick_mixed(bam, fa, loci, 3)


def record_bytes(rows):
    """The byte smc_spike_read_bits writes for each covering record, in their order."""
    return np.array([COVERS | (ALT if r.alt else 0) | (SINGLE if r.single else 0) for r in rows], np.uint8)


def barcode_counters(rows):
    """-> (barcode texts by first appearance, uint32 [n, 3] = (reads, alt0, single) over ALL records): spike_reps_restate.host_counters'."""
    texts = list(dict.fromkeys(r.barcode for r in rows))
    at = {b: k for k, b in enumerate(texts)}
    cnt = np.zeros((len(texts), 3), np.uint32)
    for r in rows:
        cnt[at[r.barcode]] += np.array([1, r.alt, r.single], np.uint32)
    return texts, cnt


def kept_counters(rows, rthr, seed):
    """-> (barcode texts by first appearance, int64 [n, 3] = (reads_r, alt_r, single_r) over the records kept at read threshold `rthr`
    with `seed`)."""
    texts = list(dict.fromkeys(r.barcode for r in rows))
    cnt = np.zeros((len(texts), 3), np.int64)
    if not rows:
        return texts, cnt
    at = {b: k for k, b in enumerate(texts)}
    inv = np.array([at[r.barcode] for r in rows], np.int64)
    u = rp.draws(rp.fnv64([r.name for r in rows]), seed).astype(np.uint64)
    kept = np.array([r.first for r in rows], bool) | (u < np.uint64(rthr))
    for c, col in enumerate((np.ones(len(rows), bool), np.array([r.alt for r in rows], bool), np.array([r.single for r in rows], bool))):
        cnt[:, c] = np.bincount(inv[kept & col], minlength=len(texts))
    return texts, cnt


def cell_rule(cnt, u, thr):
    """(N', V0', S', READS', V1') from the kept records' counters of every barcode and the spike draws; thr in [0, 2^32]."""
    reads, alt, single = cnt[:, 0], cnt[:, 1], cnt[:, 2]
    there = reads > 0
    hit = np.asarray(u).astype(np.uint64) < np.uint64(thr)
    car0, car1 = 2 * alt > reads, 2 * single > reads
    return [int(there.sum()), int((there & car0).sum()), int((there & hit).sum()), int(single[there & hit].sum()),
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
