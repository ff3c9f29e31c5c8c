"""Host restatement of --spikePhase (DESIGN.md "--spikePhase"): a phase set is a group of listed SNVs whose members are all drawn
with the position of the set's leader - its smallest - in counter word 3.  The records are tests/spike_restate.py's restate() with
that one position swapped in the draw; the joint counts come from walking every read of the host-built pileups of the members'
positions (which barcode shows what at which member) and the two numpy Philox draws of tests/spike_depth_restate.py.  Nothing from
the kernel, from tools/spike_variants.py's parsing or drawing, or from smcounter_amd/spike.py's pages.  Shared by
tests/test_spike_phase.py and tests/test_gpu_spike_phase.py."""
import contextlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ds_af_depth_restate as DR  # noqa: E402  (the "dsMT" draw in numpy)
import ds_af_restate as R  # noqa: E402
import spike_depth_restate as DS  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402

NAMES = ("N_ALL", "V0_ALL", "S_ALL", "V1_ALL")
# the columns of a phase line / a phase replicate line
P_SET, P_TARGET, P_FRACTION, P_MTDEPTH, P_N, P_V0, P_S, P_V1, P_AF, P_CALLED = 0, 5, 6, 7, 8, 9, 10, 11, 12, 13
R_REP, R_SEED, R_N, R_V1, R_CALLED = 8, 9, 10, 13, 15


def lead_positions(variants, sets):
    """Per variant the 1-based position its draw takes: the smallest position of its set, its own outside every set.  `sets`: tuples
    of indexes into `variants`."""
    out = [v.pos for v in variants]
    for members in sets:
        assert len({variants[k].chrom for k in members}) == 1
        for k in members:
            out[k] = min(variants[m].pos for m in members)
    return out


@contextlib.contextmanager
def leader_draw(variants, sets):
    """Within the block, SR.restate draws every listed position with its leader's (all variants on one chromosome)."""
    assert len({v.chrom for v in variants}) == 1
    lead = {v.pos: p for v, p in zip(variants, lead_positions(variants, sets))}
    real = SR.draw
    SR.draw = lambda texts, seed, pos1: real(texts, seed, lead.get(pos1, pos1))
    try:
        yield
    finally:
        SR.draw = real


def restate(bam_path, fa_path, variants, sets, t, seed, mismatch_thr):
    """SR.restate with the sets' draws -> (records, stats)."""
    with leader_draw(variants, sets):
        return SR.restate(bam_path, fa_path, variants, t, seed, mismatch_thr)


def host_joint(bam_path, fa_path, variants, sets):
    """Per set (the texts of the barcodes that cover every member, sorted; uint32 [n, M, 3] = per member (reads, alt0, single)), the
    members ascending by position, from a walk over every read of the members' pileups."""
    pb = R.pileups(bam_path, fa_path, [(v.chrom, v.pos) for v in variants])
    per = []
    for l, v in enumerate(variants):
        sl = pb.locus_slice(l)
        seen = {}
        for i in range(sl.start, sl.stop):
            key = pb.alleles[l][int(pb.allele[i])]
            c = seen.setdefault(pb.umi_names[l][int(pb.umi[i])], [0, 0, 0])
            c[0] += 1
            c[1] += key == v.alt
            c[2] += len(key) == 1
        per.append(seen)
    out = []
    for members in sets:
        members = sorted(members, key=lambda k: variants[k].pos)
        names = sorted(set.intersection(*[set(per[k]) for k in members]))
        out.append((names, np.array([[per[k][b] for k in members] for b in names], np.uint32).reshape(len(names), len(members), 3)))
    return out


def cell_rule(cnt, u, d, thr, dthr):
    """(N_ALL', V0_ALL', S_ALL', V1_ALL') of one set from its joint barcodes' counters [n, M, 3] and the two draws."""
    c = np.asarray(cnt).astype(np.int64)
    assert c.ndim == 3 and c.shape[2] == 3
    car0 = (2 * c[:, :, 1] > c[:, :, 0]).all(axis=1)
    car1 = (2 * c[:, :, 2] > c[:, :, 0]).all(axis=1)
    hit = np.asarray(u).astype(np.uint64) < np.uint64(thr)
    keep = np.asarray(d).astype(np.uint64) < np.uint64(dthr)
    return [int(keep.sum()), int((keep & car0).sum()), int((keep & hit).sum()), int((keep & np.where(hit, car1, car0)).sum())]


def counts_from(joint, lead_pos, thr, dthr, seed_list):
    """uint32 [G, R, T, F, 4] from per set (barcode texts, uint32 [n, M, 3]), the leaders' 1-based positions and both axes' thresholds."""
    out = np.zeros((len(joint), len(seed_list), len(thr), len(dthr), 4), np.uint32)
    for g, ((names, cnt), pos) in enumerate(zip(joint, lead_pos)):
        for j, s in enumerate(seed_list):
            u = SR.draw(names, s, pos) if len(names) else np.zeros(0, np.uint64)
            d = DR.depth_draw(PR.idents(names), s)
            for t, h in enumerate(thr):
                for f, q in enumerate(dthr):
                    out[g, j, t, f] = cell_rule(cnt, u, d, h, q)
    return out


def restate_counts(bam_path, fa_path, variants, sets, targets, fracs, seed, n_reps):
    """-> (uint32 [G, R, T, F, 4], the host's joint barcodes); fracs: 1.0 stands for the full depth."""
    joint = host_joint(bam_path, fa_path, variants, sets)
    lead = [min(variants[k].pos for k in members) for members in sets]
    return counts_from(joint, lead, [PR.threshold(t) for t in targets], [DS.frac_thr(f) for f in fracs], PR.seeds(seed, n_reps)), joint


def mnv_line(chrom, pos, ref_text, alts, vcf=True, ps=None):
    """A variants-file line for the MNV that starts at 1-based `pos`: `ref_text` the reference's letters from there, `alts` {offset:
    letter}."""
    alt = "".join(alts.get(o, c) for o, c in enumerate(ref_text))
    if not vcf:
        return "%s\t%d\t%s\t%s\n" % (chrom, pos, ref_text, alt)
    return "%s\t%d\t.\t%s\t%s\t.\t.\t%s\n" % (chrom, pos, ref_text, alt, "PS=%s" % ps if ps else ".")


def snv_line(v, ps=None):
    return "%s\t%d\t.\t%s\t%s\t.\t.\t%s\n" % (v.chrom, v.pos, v.ref, v.alt, "PS=%s" % ps if ps else ".")
