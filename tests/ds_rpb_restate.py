"""Host restatement of the read-level rule of smc_select_alignments_keyed (SMC_SEL_KEY_READ) in numpy, and the pieces the --dsRpb
tests share: a BAM written by tools.ds_reads_within_mt (the reference workflow), a run's mask over read-name ids, the comparison of a
selection with the decode of such a BAM (ids as partitions), and files the reference's sampler cannot or may not take."""
import argparse

import numpy as np

import ds_restate
from smcounter_amd import bamio


def select(A, keep_pair, start0):
    """The alignments of run `A` whose read-name id (pair_gid) is kept (bool per run-wide read-name id) -> ds_restate.select's dict,
    with the kept alignments' bc_gid and pair_gid renumbered by first kept appearance (the decoder's numbering of the down-sampled
    BAM).  (ds_restate.select keys on bc_gid: it is handed a copy of the run whose bc_gid holds pair_gid, and the kept records' own
    ids are put back afterwards.)"""
    aln = A["aln"]
    keyed = aln.copy()
    keyed["bc_gid"] = aln["pair_gid"]
    sel = ds_restate.select(dict(A, aln=keyed), keep_pair, start0)
    out = aln[sel["orig_index"]]
    for f in ("bc_gid", "pair_gid"):
        out[f] = first_seen(out[f])
    sel["aln"] = out
    return sel


def first_seen(x):
    """Ids renumbered by first appearance: two id columns are the same partition iff these are equal."""
    x = np.asarray(x)
    if not len(x):
        return x.astype(np.int64)
    u, first, inv = np.unique(x, return_index=True, return_inverse=True)
    rank = np.empty(len(u), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(u))
    return rank[inv.reshape(-1)]


def assert_same_run(sel, A_full, A_ds):
    """ds_restate.assert_same_run with the ids compared as partitions (same id <=> same id), not by rank: dropping reads can move a
    barcode's first appearance, so the down-sampled BAM's decoder may number the ids in another order."""
    a, b = sel["aln"].copy(), A_ds["aln"].copy()
    for f in ("bc_gid", "pair_gid"):
        a[f] = first_seen(a[f])
        b[f] = first_seen(b[f])
    ds_restate.assert_same_run(dict(sel, aln=a), A_full, dict(A_ds, aln=b))


def write_rpb_bam(src, dst, rpb, seed):
    """tools.ds_reads_within_mt (ds.reads.withinMT.py) -> dst, indexed."""
    from smcounter_amd.tools import ds_reads_within_mt
    ds_reads_within_mt.main(argparse.Namespace(runPath=None, inBam=src, outBam=dst, rpb=rpb, seed=seed))
    bamio.write_bai(dst)
    return dst


def pair_mask(bam, n_pair, kept):
    """bool per read-name id of the last run: its full name is in `kept` (through the names, not the identities)."""
    return np.array([bam.pair_name(g) in kept for g in range(int(n_pair))], bool)


def write_one_name_per_barcode(src, dst):
    """The placed records of `src` of the first read name of every barcode -> dst, indexed: no barcode has two names (the reference's
    probKeep divides by zero)."""
    from smcounter_amd.tools import ds_mt
    header, recs = bamio.iter_raw_records(src)
    first = {}

    def chosen():
        for tid, q, raw in recs:
            if tid >= 0 and first.setdefault(ds_mt.barcode_of(q), q) == q:
                yield raw
    bamio.write_raw(dst, header, chosen())
    bamio.write_bai(dst)
    return dst


def write_shared_read_ids(src, dst):
    """`src` with the last name field of every second and later record of a name changed ('x' -> 'y', same length): the read id
    (the name without its last field) of those reads then stands for two different names -> dst, indexed."""
    header, recs = bamio.iter_raw_records(src)
    seen = set()

    def patched():
        for tid, q, raw in recs:
            if tid >= 0 and q in seen and q.endswith("x"):
                raw = bytearray(raw)
                l_name = raw[12]
                assert raw[36 + l_name - 2] == ord("x")
                raw[36 + l_name - 2] = ord("y")
                raw = bytes(raw)
            seen.add(q)
            yield raw
    bamio.write_raw(dst, header, patched())
    bamio.write_bai(dst)
    return dst
