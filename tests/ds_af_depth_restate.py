"""Host restatement of --dsAFDepth (DESIGN.md "--dsAFDepth"): a cell (t, f) of replicate j keeps a barcode when
tools.ds_allele_fraction.titrate(..., seed + j) does not drop it at t AND the --dsMT philox draw - restated here in numpy, domain
"dsMT" - is below floor(f x 2^32).  Nothing from the kernels or the replicate stage.  Shared by tests/test_ds_af_depth.py and
tests/test_gpu_ds_af_depth.py."""
import math

import numpy as np

from smcounter_amd.tools import ds_allele_fraction as af

M64 = 0xFFFFFFFFFFFFFFFF
MT_DOMAIN = 0x64734D54          # counter word 2 of the --dsMT draw ("dsMT")


def seeds(seed, n_reps):
    return [(int(seed) + j) & M64 for j in range(n_reps)]


def depth_draw(idents, seed):
    """Word 0 of Philox4x32-10(counter = (ident lo, ident hi, "dsMT", 0), key = (seed lo, seed hi)) of every identity, as uint64."""
    x = np.asarray(idents, np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1, c2, c3 = x & m32, x >> np.uint64(32), np.full(len(x), MT_DOMAIN, np.uint64), np.zeros(len(x), np.uint64)
    seed = int(seed) & M64
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & m32
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c0


def frac_thr(f):
    """The threshold of a fraction: floor(f x 2^32); 2^32 at f >= 1 (every draw lies below it)."""
    return 1 << 32 if f >= 1.0 else int(math.floor(f * 4294967296.0))


def depth_keep(idents, f, seed):
    return depth_draw(idents, seed) < np.uint64(frac_thr(f))


def restate(run_idents, covers, carries, targets, fracs, seed, n_reps):
    """-> (keep: bool [R, T, F, n_ids] - barcode id g of the run stays in cell (t, f) of replicate j; counts: uint32 [V, R, T, F, 2] =
    (N', V') recounted over the kept barcodes from the unique covering / carrying identities)."""
    run_idents = np.asarray(run_idents, np.uint64)
    cov = [np.unique(np.asarray(c, np.uint64)) for c in covers]
    car = [np.unique(np.asarray(c, np.uint64)) for c in carries]
    keep = np.zeros((n_reps, len(targets), len(fracs), len(run_idents)), bool)
    counts = np.zeros((len(cov), n_reps, len(targets), len(fracs), 2), np.uint32)
    for j, s in enumerate(seeds(seed, n_reps)):
        res = af.titrate(covers, carries, list(targets), s)
        for t, r in enumerate(res):
            for k, f in enumerate(fracs):
                keep[j, t, k] = ~np.isin(run_idents, r["dropped"]) & depth_keep(run_idents, f, s)
                for v in range(len(cov)):
                    counts[v, j, t, k] = (int((~np.isin(cov[v], r["dropped"]) & depth_keep(cov[v], f, s)).sum()),
                                          int((~np.isin(car[v], r["dropped"]) & depth_keep(car[v], f, s)).sum()))
    return keep, counts


def t95(targets, rates, level=0.95):
    """The smallest listed target such that it and every larger listed target have a rate >= level; None when the largest has not."""
    ok = [t for t in targets if all(r >= level for u, r in zip(targets, rates) if u >= t)]
    return min(ok) if ok else None
