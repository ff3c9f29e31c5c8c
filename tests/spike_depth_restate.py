"""Host restatement of --spikeDepth (DESIGN.md "--spikeDepth"): cell (t, f) of replicate j is the --spikeAF spike-in at t with seed
s_j, of which a barcode stays when the --dsMT philox draw - restated in numpy, domain "dsMT" - is below floor(f x 2^32).  The counts
come from tests/spike_reps_restate.py's host counters and the two numpy Philox draws; the cells' records are spike_restate.restate's
filtered by the kept barcodes; the sensitivity and curve lines are computed from replicate lines.  Nothing from the kernel, from
smcounter_amd/spike.py's pages or from the replicate stage.  Shared by tests/test_spike_depth.py and tests/test_gpu_spike_depth.py."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ds_af_depth_restate as DR  # noqa: E402  (the "dsMT" draw in numpy)
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402

seeds, threshold, frac_thr = PR.seeds, PR.threshold, DR.frac_thr
NAMES = ("N", "V0", "S", "READS", "V1")
# the columns of a cell's replicate line
FRACTION, MTDEPTH, REP, SEED, N, V0, S, READS, V1, PI, CALLED = 5, 6, 7, 8, 9, 10, 11, 12, 13, 18, 20


def depth_keep(texts, f, seed):
    """Which of these barcode texts the --dsMT philox draw keeps at fraction f."""
    return DR.depth_draw(PR.idents(texts), seed) < np.uint64(frac_thr(f))


def cell_rule(cnt, u, d, thr, dthr):
    """(N', V0', S', READS', V1') from the three counters and the two draws alone; thr / dthr in [0, 2^32]."""
    reads, alt0, single = (cnt[:, k].astype(np.int64) for k in range(3))
    hit = np.asarray(u).astype(np.uint64) < np.uint64(thr)
    keep = np.asarray(d).astype(np.uint64) < np.uint64(dthr)
    return [int(keep.sum()), int((keep & (2 * alt0 > reads)).sum()), int((keep & hit).sum()), int(single[keep & hit].sum()),
            int((keep & (2 * np.where(hit, single, alt0) > reads)).sum())]


def counts_from(counters, positions, thr, dthr, seed_list):
    """uint32 [V, R, T, F, 5] from per variant (barcode texts, uint32 [n, 3]), the 1-based positions and the thresholds of both axes."""
    out = np.zeros((len(counters), len(seed_list), len(thr), len(dthr), 5), np.uint32)
    for i, ((names, cnt), pos) in enumerate(zip(counters, positions)):
        for j, s in enumerate(seed_list):
            u = SR.draw(names, s, pos) if len(names) else np.zeros(0, np.uint64)
            d = DR.depth_draw(PR.idents(names), s)
            for t, h in enumerate(thr):
                for f, g in enumerate(dthr):
                    out[i, j, t, f] = cell_rule(cnt, u, d, h, g)
    return out


def restate_counts(bam_path, fa_path, variants, targets, fracs, seed, n_reps):
    """-> (uint32 [V, R, T, F, 5], the host counters)."""
    counters = PR.host_counters(bam_path, fa_path, variants)
    return counts_from(counters, [v.pos for v in variants], [threshold(t) for t in targets], [frac_thr(f) for f in fracs],
                       seeds(seed, n_reps)), counters


def cell_records(bam_path, fa_path, variants, t, f, seed, mismatch_thr, barcode_of):
    """spike_restate.restate's records of the barcodes the depth draw keeps at f -> (records, S' per variant from the spiked sets).
    barcode_of(rec_key) -> the record's barcode text."""
    records, stats = SR.restate(bam_path, fa_path, variants, t, seed, mismatch_thr)
    texts = sorted({barcode_of(k) for k in records})
    kept = {b for b, k in zip(texts, depth_keep(texts, f, seed)) if k}
    return {k: r for k, r in records.items() if barcode_of(k) in kept}, \
        [len([b for b, k in zip(sorted(st["spiked"]), depth_keep(sorted(st["spiked"]), f, seed)) if k]) for st in stats]


def _per(rep_lines, n_cells, n_reps, i, c):
    return rep_lines[(i * n_cells + c) * n_reps:(i * n_cells + c + 1) * n_reps]


def sensitivity_from(rep_lines, variants, cells, n_reps, frac_text):
    """The depth sensitivity table's lines (without LOD) from the cells' replicate lines (fields).  cells: (target, fraction) per cell,
    targets outer."""
    out = []
    for i, v in enumerate(variants):
        for c, (target, frac) in enumerate(cells):
            per = _per(rep_lines, len(cells), n_reps, i, c)
            called = sum(int(l[CALLED]) for l in per)
            lo, hi = PR.wilson(called, n_reps)
            afs = [int(l[V1]) / int(l[N]) if int(l[N]) else 0.0 for l in per]
            ss, vs = [int(l[S]) for l in per], [int(l[V1]) for l in per]
            pis = [float(l[PI]) if l[PI] else 0.0 for l in per]
            out.append([v.chrom, "%d" % v.pos, v.ref, v.alt, "%g" % target, "%g" % frac, per[0][MTDEPTH], "%d" % n_reps, "%d" % called,
                        frac_text(called / n_reps), frac_text(lo), frac_text(hi), frac_text(sum(afs) / n_reps), frac_text(min(afs)),
                        frac_text(max(afs)), "%d" % min(ss), "%d" % max(ss), "%d" % min(vs), "%d" % max(vs), frac_text(sum(pis) / n_reps),
                        frac_text(min(pis)), frac_text(sum(int(l[N]) for l in per) / n_reps)])
    return out


def curve_from(full_lines, full_depths, rep_lines, variants, targets, fracs, n_reps, frac_text):
    """The depth curve's lines (without LOD): per variant `full` - from the plain replicate lines (spike_reps_restate's columns) and the
    targets' mtDepths - then every fraction from the cells' replicate lines."""
    T, F = len(targets), len(fracs)
    order = sorted(range(T), key=lambda t: targets[t])
    out = []

    def line(v, depth, depths, groups, n_col, called_col):
        rates = [sum(int(l[called_col]) for l in g) / n_reps for g in groups]
        best = DR.t95(targets, rates)
        n_mean = sum(sum(int(l[n_col]) for l in g) / n_reps for g in groups) / T
        return [v.chrom, "%d" % v.pos, v.ref, v.alt, depth, depths[0] if len(set(depths)) == 1 else ",".join(depths), frac_text(n_mean)] + \
            [frac_text(rates[t]) for t in order] + ["NA" if best is None else "%g" % best]
    for i, v in enumerate(variants):
        out.append(line(v, "full", ["%d" % d for d in full_depths], [PR._per(full_lines, T, n_reps, i, t) for t in range(T)], PR.N, PR.CALLED))
        for k, f in enumerate(fracs):
            groups = [_per(rep_lines, T * F, n_reps, i, t * F + k) for t in range(T)]
            out.append(line(v, "%g" % f, [g[0][MTDEPTH] for g in groups], groups, N, CALLED))
    return out
