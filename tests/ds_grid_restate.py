"""Host restatement of --dsGrid with the philox samplers (devplanes.philox_grid_rules, k_rg_reduce_frac / k_rg_masks_grid /
k_rg_kept_grid) in numpy, from the placed read names of a file in file order: the --dsMT barcode draw per name's barcode, the counters
of the barcodes kept at each fraction, probKeep per cell from them, and the kept names per cell."""
import numpy as np

import ds_rpb_philox_restate as rp
from smcounter_amd import bamio
from smcounter_amd.tools.ds_mt import barcode_of

BC_DOMAIN = 0x64734D54       # counter word 2 of the --dsMT draw ("dsMT", k_select_aln.inc SEL_DOMAIN)


def bc_draws(idents, seed):
    """Word 0 of Philox4x32-10(counter = (identity lo, identity hi, BC_DOMAIN, 0), key = (seed lo, seed hi)) per identity."""
    x = np.asarray(idents, np.uint64)
    return rp.philox4x32_10(x & np.uint64(0xFFFFFFFF), x >> np.uint64(32), BC_DOMAIN, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]


def frac_threshold(f):
    return 1 << 32 if f >= 1.0 else int(np.floor(f * 4294967296.0))


def counts_of(barcodes, keep):
    """The counters of the names `keep` selects, grouped by `barcodes` (one per name)."""
    b = np.asarray(barcodes, dtype=object)[np.asarray(keep, bool)]
    if not len(b):
        return dict(names=0, barcodes=0, one=0, multi=0, multi_names=0, first_names=0)
    _, per_bc = np.unique(b, return_counts=True)
    return dict(names=int(len(b)), barcodes=int(len(per_bc)), one=int((per_bc == 1).sum()), multi=int((per_bc >= 2).sum()),
                multi_names=int(per_bc[per_bc >= 2].sum()), first_names=int(len(per_bc)))


def restate(qnames, cells, seed):
    """rp.group() plus, per fraction f of `cells` [(f, r)], the barcodes kept (bool per name: its barcode's draw < thr_f) and their
    counters, and per cell probKeep, thr and the kept names -> dict(..., bc_keep: {f: bool per name}, fcounts: {f: counters},
    probs, thr, bc_thr, keep: [bool per name], kept: [sets of names])."""
    g = rp.group(qnames)
    g["ident"] = rp.fnv64(g["names"])
    g["u"] = rp.draws(g["ident"], seed)
    g["ub"] = bc_draws(rp.fnv64(g["barcode"]), seed)
    g["bc_keep"], g["fcounts"] = {}, {}
    for f in dict.fromkeys(f for f, _ in cells):
        t = frac_threshold(f)
        k = g["ub"].astype(np.uint64) < np.uint64(t) if t < (1 << 32) else np.ones(len(g["ub"]), bool)
        g["bc_keep"][f] = k
        g["fcounts"][f] = counts_of(g["barcode"], k)
    g["probs"], g["thr"], g["bc_thr"], g["keep"], g["kept"] = [], [], [], [], []
    for f, r in cells:
        p = rp.prob_keep(g["fcounts"][f], float(r))
        t = rp.threshold(p)
        rd = g["u"].astype(np.uint64) < np.uint64(t) if t < (1 << 32) else np.ones(len(g["u"]), bool)
        k = g["bc_keep"][f] & (g["first"] | rd)
        g["probs"].append(p); g["thr"].append(t); g["bc_thr"].append(frac_threshold(f)); g["keep"].append(k)
        g["kept"].append({n for n, x in zip(g["names"], k) if x})
    return g


def kept_barcodes(g, f):
    """The barcode texts kept at fraction f."""
    return {b for b, k in zip(g["barcode"], g["bc_keep"][f]) if k}


def one_multi_barcode_bam(src, dst, multi):
    """The first read name of every barcode of `src`, and every name of barcode `multi` -> dst, indexed: `multi` is the file's only
    barcode of two or more names."""
    header, recs = bamio.iter_raw_records(src)
    first = {}

    def chosen():
        for tid, q, raw in recs:
            if tid < 0:
                continue
            bc = barcode_of(q)
            if bc == multi or first.setdefault(bc, q) == q:
                yield raw
    bamio.write_raw(dst, header, chosen())
    bamio.write_bai(dst)
    return dst
