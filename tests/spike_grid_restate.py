"""Host restatement of --spikeGrid (DESIGN.md "--spikeGrid"): cell (t, f, r) of replicate j is the --spikeAF spike-in at t with seed
s_j, of which a record stays when --dsGrid's philox rule keeps it with the same seed - its barcode's "dsMT" draw is below
floor(f x 2^32), and its read name is its barcode's first, file-wide, or its "dsRP" draw is below the read threshold of (s_j, f, r).
That threshold is floor(probKeep x 2^32) with probKeep of ds.reads.withinMT.py:58 over the barcodes KEPT AT f UNDER s_j: every
replicate has thresholds of its own.  Everything in numpy / Python, built on tests/spike_rpb_restate.py (the records and the read
rule), tests/ds_grid_restate.py (the barcode draw and the kept barcodes' counters) and tests/ds_rpb_philox_restate.py (grouping,
probKeep, the threshold).  Nothing from smc_spike_grid_counts, smc_read_groups_counts_frac_seeds or the host code around them."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ds_grid_restate as GR  # noqa: E402
import ds_rpb_philox_restate as rp  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402
import spike_rpb_restate as RR  # noqa: E402

seeds, threshold, frac_threshold = PR.seeds, PR.threshold, GR.frac_threshold
NAMES = RR.NAMES
ONE = 1 << 32
F_NAMES = ("barcodes", "one", "multi", "multi_names")        # smc_read_groups_counts_frac_seeds' four counters


def frac_counters(groups, fracs, seed):
    """int64 [F, 4] = (barcodes, one, multi, multi_names) of the barcodes the "dsMT" draw keeps at each fraction under `seed`, from
    rp.group's dict of the file's names."""
    ub = GR.bc_draws(rp.fnv64(groups["barcode"]), seed).astype(np.uint64)
    out = np.zeros((len(fracs), 4), np.int64)
    for k, f in enumerate(fracs):
        c = GR.counts_of(groups["barcode"], ub < np.uint64(frac_threshold(f)))
        out[k] = [c[n] for n in F_NAMES]
    return out


def seed_counters(groups, fracs, seed_list):
    """int64 [R, F, 4]: frac_counters per seed."""
    return np.stack([frac_counters(groups, fracs, s) for s in seed_list]) if len(seed_list) else np.zeros((0, len(fracs), 4), np.int64)


def keeps_a_multi_name_barcode(groups, fracs, seed_list):
    """Whether probKeep is defined at every (seed, fraction): a kept barcode of two or more names."""
    c = seed_counters(groups, fracs, seed_list)
    return bool((c[:, :, 3] > c[:, :, 2]).all())


def read_thresholds(groups, fracs, rpb_targets, seed_list):
    """-> (int [R][F][Rr] thresholds as a uint64 array, float64 probKeep of the same shape): per seed and fraction probKeep over the
    barcodes kept there."""
    c = seed_counters(groups, fracs, seed_list)
    thr = np.zeros((len(seed_list), len(fracs), len(rpb_targets)), np.uint64)
    prob = np.zeros(thr.shape, np.float64)
    for j in range(len(seed_list)):
        for k in range(len(fracs)):
            counts = dict(zip(F_NAMES, (int(x) for x in c[j, k])))
            for q, r in enumerate(rpb_targets):
                prob[j, k, q] = rp.prob_keep(counts, float(r))
                thr[j, k, q] = rp.threshold(prob[j, k, q])
    return thr, prob


def cell_rule(cnt, keep, u, thr):
    """(N', V0', S', READS', V1') from the kept records' counters of every barcode, whether the barcode rule keeps it, and the spike
    draws; thr in [0, 2^32]."""
    reads, alt, single = cnt[:, 0], cnt[:, 1], cnt[:, 2]
    there = np.asarray(keep, bool) & (reads > 0)
    hit = np.asarray(u).astype(np.uint64) < np.uint64(thr)
    car0, car1 = 2 * alt > reads, 2 * single > reads
    return [int(there.sum()), int((there & car0).sum()), int((there & hit).sum()), int(single[there & hit].sum()),
            int((there & np.where(hit, car1, car0)).sum())]


def counts_from(recs, positions, thr, bc_thr, rd_thr, seed_list):
    """uint32 [V, R, T, F, Rr, 5] from per variant its covering records ([spike_rpb_restate.Rec]), the 1-based positions, the spike
    thresholds, the barcode thresholds per fraction and the read thresholds rd_thr[j][f][r] of every replicate."""
    rd_thr = np.asarray(rd_thr, np.uint64)
    n_rr = rd_thr.shape[2] if rd_thr.ndim == 3 else 0
    out = np.zeros((len(recs), len(seed_list), len(thr), len(bc_thr), n_rr, 5), np.uint32)
    for i, (rows, pos) in enumerate(zip(recs, positions)):
        for j, s in enumerate(seed_list):
            texts = list(dict.fromkeys(r.barcode for r in rows))
            u = SR.draw(texts, s, pos) if texts else np.zeros(0, np.uint64)
            d = GR.bc_draws(PR.idents(texts), s).astype(np.uint64) if texts else np.zeros(0, np.uint64)
            for f, b in enumerate(bc_thr):
                keep = d < np.uint64(b)
                for r in range(n_rr):
                    same, cnt = RR.kept_counters(rows, int(rd_thr[j, f, r]), s)
                    assert same == texts
                    for t, h in enumerate(thr):
                        out[i, j, t, f, r] = cell_rule(cnt, keep, u, h)
    return out


def restate_counts(bam_path, fa_path, variants, targets, fracs, rpb_targets, seed, n_reps):
    """-> (uint32 [V, R, T, F, Rr, 5], the covering records, the read thresholds [R, F, Rr], probKeep [R, F, Rr])."""
    groups = RR.file_groups(bam_path)
    recs = RR.records(bam_path, fa_path, variants, groups)
    seed_list = seeds(seed, n_reps)
    rd_thr, prob = read_thresholds(groups, fracs, rpb_targets, seed_list)
    return counts_from(recs, [v.pos for v in variants], [threshold(t) for t in targets], [frac_threshold(f) for f in fracs], rd_thr,
                       seed_list), recs, rd_thr, prob


def cost_order(costs):
    """The budget page's order: the cells by cost ascending, ties in listed order -> indices."""
    return sorted(range(len(costs)), key=lambda c: (costs[c], c))


def cheapest95(rates_in_order):
    """CHEAPEST95 per line of the budget page: 1 on the first line whose rate is at least 0.95."""
    out, seen = [], False
    for r in rates_in_order:
        out.append(1 if (r >= 0.95 and not seen) else 0)
        seen = seen or r >= 0.95
    return out
