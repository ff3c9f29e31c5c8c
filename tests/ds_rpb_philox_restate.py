"""Host restatement of the read-level philox sampler (--dsRpbSampler philox: csrc/k_read_groups.inc, devplanes.philox_read_rules) in
numpy, from the placed read names of a file in file order (ds_restate.placed_qnames): the grouping of ds.reads.withinMT.py:37-58, the
counters, the first names, probKeep and the kept names per target; and a BAM of many minimal placed records for the table's scale."""
import struct

import numpy as np

from smcounter_amd import bamio
from smcounter_amd.tools.ds_mt import barcode_of

DOMAIN = 0x64735250          # counter word 2 of the draw ("dsRP")


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 over uint32 arrays (c0, c1 arrays; c2, c3, k0, k1 scalars) -> the four output words."""
    M0, M1, W0, W1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57), 0x9E3779B9, 0xBB67AE85
    lo = np.uint64(0xFFFFFFFF)
    c0 = np.asarray(c0, np.uint64) & lo
    c1 = np.asarray(c1, np.uint64) & lo
    c2 = np.full(c0.shape, c2, np.uint64)
    c3 = np.full(c0.shape, c3, np.uint64)
    k0, k1 = int(k0) & 0xFFFFFFFF, int(k1) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0), p1 & lo, (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1), p0 & lo
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def draws(idents, seed):
    """Word 0 of Philox4x32-10(counter = (identity lo, identity hi, DOMAIN, 0), key = (seed lo, seed hi)) per identity."""
    x = np.asarray(idents, np.uint64)
    return philox4x32_10(x & np.uint64(0xFFFFFFFF), x >> np.uint64(32), DOMAIN, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]


def fnv64(texts):
    from smcounter_amd.devplanes import fnv64_array
    return fnv64_array(texts)


def threshold(prob):
    """floor(probKeep x 2^32), clamped to [0, 2^32]."""
    return 0 if not prob > 0.0 else min(1 << 32, int(np.floor(prob * 4294967296.0)))


def group(qnames):
    """The placed names in file order -> dict(names: distinct names by first appearance, barcode: per name, first: bool per name (its
    first record has the smallest ordinal of its barcode's records), counts: records / names / barcodes / one / multi / multi_names /
    first_names)."""
    q = np.asarray(qnames, dtype=object)
    names, first_ord, inv = np.unique(q, return_index=True, return_inverse=True)
    order = np.argsort(first_ord, kind="stable")
    names, first_ord = names[order], first_ord[order]
    bcs = np.array([barcode_of(n) for n in names], dtype=object)
    ub, b_inv = np.unique(bcs, return_inverse=True)
    b_inv = b_inv.reshape(-1)
    b_min = np.full(len(ub), np.iinfo(np.int64).max, np.int64)
    np.minimum.at(b_min, b_inv, first_ord)
    first = first_ord == b_min[b_inv]
    per_bc = np.bincount(b_inv, minlength=len(ub))
    counts = dict(records=len(q), names=len(names), barcodes=len(ub), one=int((per_bc == 1).sum()), multi=int((per_bc >= 2).sum()),
                  multi_names=int(per_bc[per_bc >= 2].sum()), first_names=int(first.sum()))
    return dict(names=list(names), barcode=list(bcs), first=first, counts=counts)


def prob_keep(counts, r):
    one, multi, multi_names = counts["one"], counts["multi"], counts["multi_names"]
    return 1.0 * (r - 1.0) * (one + multi) / (multi_names - multi)      # ds.reads.withinMT.py:58 (ZeroDivisionError like it)


def restate(qnames, targets, seed):
    """group() plus, per target r: probKeep, thr and the kept names (bool per name) -> dict(..., probs, thr, keep: [bool arrays],
    kept: [sets of names], u: the draws)."""
    g = group(qnames)
    g["ident"] = fnv64(g["names"])
    g["u"] = draws(g["ident"], seed)
    g["probs"], g["thr"], g["keep"], g["kept"] = [], [], [], []
    for r in targets:
        p = prob_keep(g["counts"], float(r))
        t = threshold(p)
        k = g["first"] | (g["u"].astype(np.uint64) < np.uint64(t) if t < (1 << 32) else np.ones(len(g["u"]), bool))
        g["probs"].append(p); g["thr"].append(t); g["keep"].append(k)
        g["kept"].append({n for n, x in zip(g["names"], k) if x})
    return g


def write_names_bam(path, n_records, names_per_barcode=4, records_per_name=2, seed=0):
    """A BAM of `n_records` minimal placed records (no CIGAR, no bases) on one reference, in position order: names
    'S:<barcode>:<i>' in barcodes of 1 .. 2 x names_per_barcode names, each name's records a few positions apart, one in 97 barcodes
    of a single name.  The file pass reads nothing but the names.  -> the placed names in file order."""
    rng = np.random.default_rng(seed)
    header = b"BAM\1" + struct.pack("<i", 0) + struct.pack("<i", 1) + struct.pack("<i", 5) + b"chrS\0" + struct.pack("<i", 1 << 30)
    recs, names = [], []
    pos, b = 0, 0
    while len(recs) < n_records:
        k = 1 if b % 97 == 0 else int(rng.integers(1, 2 * names_per_barcode + 1))
        for i in range(k):
            name = "S%d:BC%07d:%d" % (i % 3, b, i)
            for _ in range(records_per_name):
                if len(recs) == n_records:
                    break
                nb = name.encode() + b"\0"
                body = struct.pack("<iiBBHHHiiii", 0, pos, len(nb), 60, 4680, 0, 0, 0, -1, -1, 0) + nb
                recs.append(struct.pack("<i", len(body)) + body)
                names.append(name)
                pos += int(rng.integers(0, 3))
        b += 1
    bamio.write_raw(path, header, recs)
    return names
