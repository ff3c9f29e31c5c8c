"""Host restatement of --spikeReps: tests/spike_restate.py once per replicate seed (host-built pileups, a numpy Philox), the counts
rule restated from (reads, alt0, single) alone, and the sensitivity and curve lines computed from replicate lines - not through
smcounter_amd/spike.py.  Shared by tests/test_spike_reps.py and tests/test_gpu_spike_reps.py."""
import contextlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ds_af_restate as R  # noqa: E402
import ds_rpb_philox_restate as rp  # noqa: E402
import spike_restate as SR  # noqa: E402

M64 = 0xFFFFFFFFFFFFFFFF
Z = 1.959963984540054
# the columns of a replicate line
REP, SEED, N, V0, S, READS, V1, PI, CALLED = 5, 6, 7, 8, 9, 10, 11, 16, 18


def seeds(seed, n_reps):
    return [(seed + j) & M64 for j in range(n_reps)]


def threshold(t):
    return int(math.floor(t * 4294967296.0))


@contextlib.contextmanager
def shared_pileups():
    """Within the block, SR.restate builds the host pileups of one (file, positions) once and reads them again for every seed and
    target (they depend on neither, and restate() only reads them)."""
    real, seen = R.pileups, {}

    def cached(bam_path, fa_path, positions):
        key = (bam_path, fa_path, tuple(positions))
        if key not in seen:
            seen[key] = real(bam_path, fa_path, positions)
        return seen[key]
    R.pileups = cached
    try:
        yield
    finally:
        R.pileups = real


def restate(bam_path, fa_path, variants, targets, seed, n_reps, mismatch_thr):
    """-> out[j][t] = SR.restate(..., targets[t], s_j): (records, stats)."""
    with shared_pileups():
        return [[SR.restate(bam_path, fa_path, variants, t, s, mismatch_thr) for t in targets] for s in seeds(seed, n_reps)]


def host_counters(bam_path, fa_path, variants):
    """Per variant (barcode texts, uint32 [n, 3] = (reads, alt0, single)) from the host-built pileup: the reads of every barcode at
    the position, those whose allele key is ALT, those whose key is a single letter."""
    pb = R.pileups(bam_path, fa_path, [(v.chrom, v.pos) for v in variants])
    out = []
    for l, v in enumerate(variants):
        sl = pb.locus_slice(l)
        names = pb.umi_names[l]
        cnt = np.zeros((len(names), 3), np.uint32)
        for i in range(sl.start, sl.stop):
            key = pb.alleles[l][int(pb.allele[i])]
            cnt[int(pb.umi[i])] += np.array([1, key == v.alt, len(key) == 1], np.uint32)
        out.append((list(names), cnt))
    return out


def idents(texts):
    return rp.fnv64(list(texts)).astype(np.uint64) if len(texts) else np.zeros(0, np.uint64)


def counts_rule(cnt, u, thr):
    """(S, READS, V1) from the three counters and the draws alone."""
    reads, alt0, single = (cnt[:, k].astype(np.int64) for k in range(3))
    hit = np.asarray(u).astype(np.uint64) < np.uint64(thr) if thr < (1 << 32) else np.ones(len(cnt), bool)
    return int(hit.sum()), int(single[hit].sum()), int((2 * np.where(hit, single, alt0) > reads).sum())


def wilson(called, reps):
    p = called / reps
    den = 1 + Z * Z / reps
    half = Z * math.sqrt(p * (1 - p) / reps + Z * Z / (4.0 * reps * reps)) / den
    mid = (p + Z * Z / (2.0 * reps)) / den
    return max(0.0, mid - half), min(1.0, mid + half)


def _per(rep_lines, n_targets, n_reps, i, t):
    return rep_lines[(i * n_targets + t) * n_reps:(i * n_targets + t + 1) * n_reps]


def sensitivity_from(rep_lines, variants, targets, n_reps, frac_text):
    """The sensitivity table's lines (without LOD) from the replicate lines (fields); `frac_text`: how a fraction is printed."""
    out = []
    for i, v in enumerate(variants):
        for t, target in enumerate(targets):
            per = _per(rep_lines, len(targets), n_reps, i, t)
            called = sum(int(l[CALLED]) for l in per)
            lo, hi = wilson(called, n_reps)
            afs = [int(l[V1]) / int(l[N]) if int(l[N]) else 0.0 for l in per]
            ss, vs = [int(l[S]) for l in per], [int(l[V1]) for l in per]
            pis = [float(l[PI]) if l[PI] else 0.0 for l in per]
            out.append([v.chrom, "%d" % v.pos, v.ref, v.alt, "%g" % target, "%d" % n_reps, "%d" % called, frac_text(called / n_reps), frac_text(lo),
                        frac_text(hi), frac_text(sum(afs) / n_reps), frac_text(min(afs)), frac_text(max(afs)), "%d" % min(ss), "%d" % max(ss),
                        "%d" % min(vs), "%d" % max(vs), frac_text(sum(pis) / n_reps), frac_text(min(pis))])
    return out


def curve_from(rep_lines, variants, targets, n_reps, frac_text):
    """The curve's lines (without LOD): per variant N, the rates in ascending target order, and the smallest target whose rate and
    that of every larger target is at least 0.95 (NA: none)."""
    out = []
    order = sorted(range(len(targets)), key=lambda t: targets[t])
    for i, v in enumerate(variants):
        rates = [sum(int(l[CALLED]) for l in _per(rep_lines, len(targets), n_reps, i, t)) / n_reps for t in range(len(targets))]
        best = None
        for t in reversed(order):
            if rates[t] < 0.95:
                break
            best = targets[t]
        out.append([v.chrom, "%d" % v.pos, v.ref, v.alt, _per(rep_lines, len(targets), n_reps, i, 0)[0][N]] + [frac_text(rates[t]) for t in order] +
                   ["NA" if best is None else "%g" % best])
    return out
