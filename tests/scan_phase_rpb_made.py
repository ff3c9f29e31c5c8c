"""Made runs for smc_scan_phase_rpb_counts: the record lists of tests/test_gpu_spike_phase_rpb.py (_made: per set, per member its
[Rec]) laid out as ONE decoded run - an alignment per (barcode, read name), a record that stands under several members one alignment
with a byte at each of them - with the barcode ids shuffled against file order, alignments of another amplicon in between (bytes 0
at every bit row) and the bit rows as smc_spike_read_bits would have written them.  Shared by tests/test_scan_phase_rpb_rule.py (CPU)
and tests/test_gpu_scan_phase_rpb_counts.py."""
import os
import sys

import numpy as np

from smcounter_amd import devplanes

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import spike_phase_rpb_restate as ZR  # noqa: E402
from test_gpu_spike_phase_rpb import _csr, _made, _rec  # noqa: E402,F401

PR, XR = ZR.PR, ZR.XR
ONE = ZR.ONE
ALN_DTYPE = np.dtype([("bc_gid", "<u4"), ("pair_gid", "<u4")])


class MadeRun(object):
    """set_rows[g][m]: the [Rec] of member m of set g.  -> A (aln with bc_gid / pair_gid in file order, n_bc), idents per barcode id,
    p_idents / first per read-name id, bits uint8 [n_var, n_aln], rows[g]: the bit rows of set g's members, joint[g]: the run-wide ids
    of the barcodes with a record at every member (ascending), order: devplanes.run_barcode_major's arrays with `idents`.
    strangers: that many alignments of another amplicon per barcode of the run at the most (a byte of 0 in every bit row), and as many
    barcodes that no set knows."""

    def __init__(self, set_rows, seed=1, strangers=2):
        rng = np.random.RandomState(seed)
        reads, bytes_of = {}, {}                       # (barcode, name) -> first; (bit row, barcode, name) -> byte
        self.rows, v = [], 0
        for members in set_rows:
            self.rows.append(list(range(v, v + len(members))))
            for m, recs in enumerate(members):
                for r in recs:
                    key = (r.barcode, r.name)
                    assert reads.setdefault(key, bool(r.first)) == bool(r.first) and (v + m,) + key not in bytes_of
                    bytes_of[(v + m,) + key] = 1 | (2 if r.alt0 else 0) | (4 if r.alt1 else 0)
            v += len(members)
        texts = sorted({b for b, _ in reads})
        for b in texts + ["STRANGER%dACGT" % k for k in range(strangers)]:
            for k in range(int(rng.randint(0, strangers + 1))):
                reads[(b, "far:%s:%d" % (b, k))] = bool(rng.rand() < 0.3)
        keys = list(reads)
        rng.shuffle(keys)                              # file order
        texts = sorted({b for b, _ in keys})
        gid = dict(zip(texts, rng.permutation(len(texts))))                 # barcode ids shuffled against file order and text order
        self.texts = [None] * len(texts)
        for b, k in gid.items():
            self.texts[k] = b
        names = list(dict.fromkeys(n for _, n in keys))
        pair = {n: k for k, n in enumerate(names)}
        aln = np.zeros(len(keys), ALN_DTYPE)
        aln["bc_gid"] = [gid[b] for b, _ in keys]
        aln["pair_gid"] = [pair[n] for _, n in keys]
        self.A = dict(aln=aln, n_bc=len(texts))
        self.idents = PR.idents(self.texts)
        self.p_idents = XR.rp.fnv64(names).astype(np.uint64) if names else np.zeros(0, np.uint64)
        first_of = {n: f for (_, n), f in reads.items()}
        self.first = np.array([first_of[n] for n in names], bool)
        at = {key: i for i, key in enumerate(keys)}
        self.bits = np.zeros((v, len(keys)), np.uint8)
        for (row, b, n), byte in bytes_of.items():
            self.bits[row, at[(b, n)]] = byte
        self.joint = [np.sort(np.array([gid[b] for b in ZR.joint_names(members)], np.uint32)) for members in set_rows]
        self.order = dict(devplanes.run_barcode_major(self.A, self.p_idents, self.first), idents=self.idents)
        self.n_var, self.n_aln = v, len(keys)

    def rule(self, lead, seeds, thr, rthr, rows=None, joint=None, detail=None):
        return devplanes.scan_phase_rpb_counts_rule(self.order, self.bits, self.rows if rows is None else rows,
                                                    self.joint if joint is None else joint, lead, seeds, thr, rthr, detail)


def thinning_bites(detail, full):
    """From the rule's counters (per row int64 [R, n, M, Rr, 3], read threshold index `full` keeping every record): -> (a joint barcode
    keeps a read at one member and none at another at some (replicate, r), a barcode's majority (2 alt0 > reads) differs from the
    unthinned one at one member while another member's stays and both still hold reads)."""
    out_of_one = flips_at_one = False
    for c in detail:
        if c.shape[2] < 2:
            continue
        there = c[..., 0] > 0                                              # [R, n, M, Rr]
        out_of_one |= bool((there.any(axis=2) & ~there.all(axis=2)).any())
        car = 2 * c[..., 1] > c[..., 0]
        moved = (car != car[..., full:full + 1]) & there
        stays = (car == car[..., full:full + 1]) & there
        flips_at_one |= bool((moved.any(axis=2) & stays.any(axis=2) & there.all(axis=2)).any())
    return out_of_one, flips_at_one
