"""Host restatement of smc_select_alignments (csrc/k_select_aln.inc) in numpy, and the pieces the --dsMT tests share: a BAM
written by tools.ds_mt (the reference workflow), a BED of a fixture's loci, the runs a fixture's loci fall into."""
import argparse
import json
import os

import numpy as np

from smcounter_amd import abi, bamio, fasta
from smcounter_amd.params import VcParams

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BIG = 1 << 40


def select(A, keep_gid, start0):
    """The kept alignments of run `A` (bool per run-wide barcode id) -> dict(aln, orig_index, loc, kept, deepest, slots): what
    smc_bam_alignments would hand out for the down-sampled BAM, up to the ids (kept as they were) and the pool offsets (the
    original pools')."""
    aln = A["aln"]
    keep_gid = np.asarray(keep_gid, bool)
    gid = aln["bc_gid"].astype(np.int64)
    keep = np.zeros(len(aln), bool)
    inside = gid < len(keep_gid)
    keep[inside] = keep_gid[gid[inside]]
    orig = np.flatnonzero(keep).astype(np.uint32)
    out = aln[orig]
    nl = int(A["nl"])
    p = int(start0) + np.arange(nl, dtype=np.int64)
    loc = np.zeros(nl, abi.DEV_LOCUS_DTYPE)
    if len(out):
        runmax = np.maximum.accumulate(out["end"].astype(np.int64))
        w0 = np.searchsorted(runmax, p, side="right")                 # first kept alignment whose end passes p
        w1 = np.maximum(w0, np.searchsorted(out["pos"].astype(np.int64), p, side="right"))
    else:
        w0 = w1 = np.zeros(nl, np.int64)
    diff = np.zeros(nl + 1, np.int64)
    lo = np.maximum(out["pos"].astype(np.int64), start0) - start0
    hi = np.minimum(out["end"].astype(np.int64), start0 + nl) - start0
    ok = lo < hi
    np.add.at(diff, lo[ok], 1)
    np.add.at(diff, hi[ok], -1)
    n = np.cumsum(diff[:-1])
    slots = (n + 3) // 4 * 4
    loc["w0"], loc["w1"], loc["n"] = w0, w1, n
    loc["slot_off"] = np.concatenate([[0], np.cumsum(slots)[:-1]]) if nl else []
    return dict(aln=out, orig_index=orig, loc=loc, kept=len(out), deepest=int(n.max()) if nl else 0, slots=int(slots.sum()))


def dense_rank(x):
    return np.unique(np.asarray(x), return_inverse=True)[1].reshape(-1)


def assert_same_run(sel, A_full, A_ds):
    """The restated selection of the full run vs the decoder's run of the down-sampled BAM: every field, the ids up to an
    order-preserving renumbering, CIGARs and bases through each one's own pools; the descriptors field for field."""
    a, b = sel["aln"], A_ds["aln"]
    assert len(a) == len(b)
    for f in ("pos", "end", "n_cig", "oflag", "mapq", "left_sp", "qalen", "l_seq", "pad"):
        assert np.array_equal(a[f], b[f]), f
    for f in ("bc_gid", "pair_gid"):
        assert np.array_equal(dense_rank(a[f]), dense_rank(b[f])), f
    for k in range(len(a)):
        c0, c1 = int(a["cig_off"][k]), int(b["cig_off"][k])
        nc = int(a["n_cig"][k])
        assert np.array_equal(A_full["cig"][c0:c0 + nc], A_ds["cig"][c1:c1 + nc])
        s0, s1, ls = int(a["seq_off"][k]), int(b["seq_off"][k]), int(a["l_seq"][k])
        assert np.array_equal(A_full["bq"][2 * s0:2 * (s0 + ls)], A_ds["bq"][2 * s1:2 * (s1 + ls)])
    assert A_ds["nl"] == A_full["nl"]
    for f in ("w0", "w1", "slot_off", "n"):
        assert np.array_equal(sel["loc"][f], A_ds["loc"][f]), f
    assert sel["slots"] == A_ds["n_slots"]


def write_ds_bam(src, dst, pct, seed):
    """tools.ds_mt (ds.mt.py) -> dst, indexed."""
    from smcounter_amd.tools import ds_mt
    ds_mt.main(argparse.Namespace(runPath=None, inBam=src, outBam=dst, pct=pct, seed=seed))
    bamio.write_bai(dst)
    return dst


def write_kept_bam(src, dst, kept):
    """The placed records of `src` whose barcode is in `kept` -> dst, indexed (a BAM for another keep rule)."""
    from smcounter_amd.tools import ds_mt
    header, recs = bamio.iter_raw_records(src)
    bamio.write_raw(dst, header, (raw for tid, q, raw in recs if tid >= 0 and ds_mt.barcode_of(q) in kept))
    bamio.write_bai(dst)
    return dst


def placed_qnames(path):
    _, recs = bamio.iter_raw_records(path)
    return [q for tid, q, _ in recs if tid >= 0]


def load_fixture(name, tmp):
    """tests/golden/<name>.npz -> (bam, fasta path, loci, VcParams)."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    bam, fa = os.path.join(tmp, name + ".bam"), os.path.join(tmp, name + ".fa")
    open(bam, "wb").write(bytes(z["bam"]))
    open(bam + ".bai", "wb").write(bytes(z["bai"]))
    open(fa, "wb").write(bytes(z["fasta"]))
    return bam, fa, [(c, int(p)) for c, p in meta["loci"]], VcParams(**meta["params"])


def make_case(tmp):
    """bam_fixture.make_case as (bam, fasta path, loci, VcParams)."""
    import bam_fixture
    case = bam_fixture.make_case(tmp)
    loci = [("chrQ", p) for a, b in ((280, 320), (598, 604)) for p in range(a + 1, b + 1)]
    return case["bam"], case["fasta"], loci, VcParams(mtDepth=12, rpb=3.0, hpLen=8)


def stretches(loci):
    """Runs of consecutive positions: [(chrom, lo0, hi0)] (0-based half-open)."""
    out = []
    for c, p in loci:
        if out and out[-1][0] == c and out[-1][2] == p - 1:
            out[-1][2] = p
        else:
            out.append([c, p - 1, p])
    return [tuple(x) for x in out]


def write_bed(path, loci):
    with open(path, "w") as fh:
        for c, lo, hi in stretches(loci):
            fh.write("%s\t%d\t%d\n" % (c, lo, hi))
    return path


def mask_of(bam, n_bc, kept):
    return np.array([bam.barcode_name(g) in kept for g in range(int(n_bc))], bool)
