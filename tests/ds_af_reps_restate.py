"""Host restatement of --dsAFReps (DESIGN.md "--dsAFReps"): the keep masks and the achieved counts of R replicates made by calling
tools.ds_allele_fraction.titrate once per replicate with seed + j - the tool's own code, nothing from the replicate stage.  Shared by
tests/test_ds_af_reps.py and tests/test_gpu_ds_af_reps.py."""
import math

import numpy as np

from smcounter_amd.tools import ds_allele_fraction as af

M64 = 0xFFFFFFFFFFFFFFFF
Z = 1.959963984540054


def seeds(seed, n_reps):
    return [(int(seed) + j) & M64 for j in range(n_reps)]


def restate(run_idents, covers, carries, targets, seed, n_reps):
    """-> (keep: bool [R, T, n_ids] - barcode id g of the run stays in replicate j at target t; counts: uint32 [V, R, T, 2] = (N', V');
    dropped: [R][T] the sorted dropped identities)."""
    run_idents = np.asarray(run_idents, np.uint64)
    keep = np.zeros((n_reps, len(targets), len(run_idents)), bool)
    counts = np.zeros((len(covers), n_reps, len(targets), 2), np.uint32)
    dropped = []
    for j, s in enumerate(seeds(seed, n_reps)):
        res = af.titrate(covers, carries, list(targets), s)
        dropped.append([r["dropped"] for r in res])
        for t, r in enumerate(res):
            keep[j, t] = ~np.isin(run_idents, r["dropped"])
            for v, row in enumerate(r["rows"]):
                counts[v, j, t] = (row["N2"], row["V2"])
    return keep, counts, dropped


def pack(keep, n_words):
    """bool [..., n_ids] -> uint32 [..., n_words]: bit (g & 31) of word (g >> 5), zeros behind the last id."""
    bits = np.packbits(keep, axis=-1, bitorder="little")
    out = np.zeros(keep.shape[:-1] + (4 * n_words,), np.uint8)
    out[..., :bits.shape[-1]] = bits
    return out.view(np.uint32)


def thresholds(covers, carries, targets):
    """thr[t][v] of the titration (it does not depend on the seed)."""
    return [[row["thr"] for row in r["rows"]] for r in af.titrate(covers, carries, list(targets), 0)]


def wilson(called, reps):
    """The Wilson score interval in its closed form over counts: (2c + z^2 -/+ z sqrt(z^2 + 4c(n - c)/n)) / (2(n + z^2))."""
    c, n = float(called), float(reps)
    s = math.sqrt(Z * Z + 4.0 * c * (n - c) / n)
    return (2.0 * c + Z * Z - Z * s) / (2.0 * (n + Z * Z)), (2.0 * c + Z * Z + Z * s) / (2.0 * (n + Z * Z))
