"""Host restatement of --spikeIndelReps / --spikeIndelDepth (DESIGN.md "--spikeIndelReps / --spikeIndelDepth"): the FOUR counters per
listed variant and covering barcode - (reads, alt0, alt1, touch) - from a file's records as bamio's readable decoder gives them, laid
out base by base (spike_indel_restate.layout / resolve: not the kernel's walk), and the counts of every (variant, replicate, target[,
fraction]) from those counters and the two numpy Philox draws alone.  Also which of the cases that make three counters too few a file
holds.  Shared by tests/test_spike_indel_reps.py, tests/test_gpu_spike_indel_reps.py and tests/test_gpu_spike_indel_reps_cli.py."""
import os
import sys

import numpy as np

from smcounter_amd import bamio
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ds_af_depth_restate as DR  # noqa: E402  (the "dsMT" draw in numpy)
import spike_indel_restate as IR  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402

seeds, threshold, frac_thr = PR.seeds, PR.threshold, DR.frac_thr
CASES = ("anchor_mismatch", "shows_it_already", "ends_in_footprint")


def host_counters(bam_path, variants, fa=None):
    """-> (per variant (sorted barcode texts that cover it, uint32 [n, 4] = (reads, alt0, alt1, touch)), per variant {case: records}).
    reads: the barcode's records that span the position; alt0: those that show the variant's key; touch: those the rewrite changes
    when the barcode is hit - an SNV: the site a single-letter key; an insertion / a deletion: the footprint inside one M / = / X
    operation and inside l_seq, n_cig + 2 and l_seq (+ the inserted letters) within 16 bits; alt1: those that show the key when the
    barcode is hit - an SNV: touch; an insertion / a deletion: a touched record whose anchor letter is REF's, an untouched one that
    shows it already."""
    bam = bamio.BamFile(bam_path)
    bam._bg.seek(bam._first_record)
    recs = [a for a in bam._records() if a.tid >= 0 and not (a.flag & 4) and a.cigar]
    chrom_of = [name for name, _ in bam.refs]
    bam.close()
    genome = None
    if fa is not None:
        from smcounter_amd import fasta
        genome = fasta.FastaFile(fa)
    per = [dict() for _ in variants]
    cases = [dict.fromkeys(CASES, 0) for _ in variants]
    for a in recs:
        chrom, bc = chrom_of[a.tid], af.barcode_of(a.qname)
        here = [k for k, v in enumerate(variants) if v.chrom == chrom and a.pos < v.pos <= a.end]
        if not here or bc is None:
            continue
        units, at = IR.layout(a)
        for k in here:
            v = variants[k]
            shows = af.read_key(a, v.pos, chrom, genome) == af.variant_key(v, genome)
            u = IR.resolve(a, units, at, v)
            n = IR.length(v)
            if v.kind != af.SNV and (len(a.cigar) + 2 > IR.MAX16 or (v.kind == af.INS and a.l_seq + n > IR.MAX16)):
                u = None
            c = per[k].setdefault(bc, [0, 0, 0, 0])
            c[0] += 1
            c[1] += shows
            c[3] += u is not None
            if v.kind == af.SNV:
                c[2] += u is not None
                continue
            anchor_ok = u is not None and a.seq[units[u]["q"]] == v.ref[0]
            c[2] += anchor_ok if u is not None else shows
            cases[k]["anchor_mismatch"] += u is not None and not anchor_ok
            cases[k]["shows_it_already"] += u is None and shows
            cases[k]["ends_in_footprint"] += u is None and v.pos - 1 < a.end <= IR.footprint(v)[1] - 1
    out = []
    for p in per:
        names = sorted(p)
        out.append((names, np.array([p[b] for b in names], np.uint32).reshape(-1, 4)))
    return out, cases


def cell_rule(cnt, u, d, thr, dthr):
    """(N', V0', S', READS', V1') from the four counters and the two draws alone; thr / dthr in [0, 2^32]."""
    reads, alt0, alt1, touch = (cnt[:, k].astype(np.int64) for k in range(4))
    hit = np.asarray(u).astype(np.uint64) < np.uint64(thr)
    keep = np.asarray(d).astype(np.uint64) < np.uint64(dthr)
    return [int(keep.sum()), int((keep & (2 * alt0 > reads)).sum()), int((keep & hit).sum()), int(touch[keep & hit].sum()),
            int((keep & (2 * np.where(hit, alt1, alt0) > reads)).sum())]


def counts_from(counters, positions, thr, seed_list, dthr=None):
    """uint32 [V, R, T, 3] = (S, READS, V1), or with the fractions' thresholds `dthr` [V, R, T, F, 5] = (N', V0', S', READS', V1'),
    from per variant (barcode texts, uint32 [n, 4]), the 1-based positions and the thresholds."""
    cells = dthr is not None
    dthr = list(dthr) if cells else [1 << 32]
    out = np.zeros((len(counters), len(seed_list), len(thr), len(dthr), 5), np.uint32)
    for i, ((names, cnt), pos) in enumerate(zip(counters, positions)):
        for j, s in enumerate(seed_list):
            u = SR.draw(names, s, pos) if len(names) else np.zeros(0, np.uint64)
            d = DR.depth_draw(PR.idents(names), s)
            for t, h in enumerate(thr):
                for f, g in enumerate(dthr):
                    out[i, j, t, f] = cell_rule(cnt, u, d, h, g)
    return out if cells else out[:, :, :, 0, 2:]


def device_order(counters, idents_of):
    """The restated counters as the counts entries take them: (covers: uint64 identities, counters) per variant, by identity."""
    covers, cnts = [], []
    for names, cnt in counters:
        ids = idents_of(names)
        order = np.argsort(ids, kind="stable")
        covers.append(ids[order])
        cnts.append(cnt[order])
    return covers, cnts
