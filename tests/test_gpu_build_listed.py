"""smc_build_listed against the whole builder on the same device arrays: for every copy and listed locus the read words, the
umi_start / u_gid / u_finc stretch, the descriptor (apart from read_off4 / umi_off), the extras entries and the counters are byte
for byte those of smc_build_planes / smc_build_planes_w16 over the same records.  Outputs are poisoned and carry guard stretches:
nothing is written outside what the contract names, and two calls give the same bytes.

The unit of the listed builder is the locus's workgroup: 16 wavefronts that compact a window 1024 alignments a round and sort it 64
entries a wavefront step - so the hand-made depths are 1, 63, 64, 65 and 1025 (just over one round of the workgroup)."""
import ctypes
import dataclasses
import os
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, bamio, devplanes, synth
from smcounter_amd.engine import DevBuf
from smcounter_amd.params import VcParams

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402

pytestmark = pytest.mark.gpu
LOCUS = devplanes.LOCUS_DTYPE
POISON = 0xA5
GUARD = 64                      # words of guard stretch before and behind every output
ST_UNFLAGGED, ST_NARROW = 64, 32
COPY_DTYPE = np.dtype([("aln", "<u8"), ("cig", "<u8"), ("bq", "<u8"), ("loc", "<u8"), ("n_aln", "<i4"), ("n_bc", "<i4"),
                       ("n_pair", "<i4"), ("reserved", "<i4")])
assert COPY_DTYPE.itemsize == 48


def align4(n):
    return (int(n) + 3) & ~3


# ---- runs made by hand
def read(pos, cigar, seq, bc, name, r2=False, rev=False, qual=30, mapq=60, mmok=True, flagged=True):
    """cigar: [(op, len)] with BAM's op codes (0 M, 1 I, 2 D, 4 S); qual: one value or one per base."""
    q = [qual] * len(seq) if isinstance(qual, int) else list(qual)
    assert len(q) == len(seq) == sum(l for op, l in cigar if op in (0, 1, 4, 7, 8))
    return dict(pos=pos, cigar=cigar, seq=seq, qual=q, bc=bc, name=name, r2=r2, rev=rev, mapq=mapq, mmok=mmok, flagged=flagged)


def make_run(reads, nl, start0=1000):
    """The dict smc_build_planes' callers hand on (synth.generate_alignments' fields) for `reads` (positions are run offsets; put in
    file order: by position, stable)."""
    reads = sorted(reads, key=lambda r: r["pos"])
    aln = np.zeros(len(reads), abi.DEV_ALN_DTYPE)
    cig, bq, bcs, pairs = [], [], {}, {}
    for i, r in enumerate(reads):
        ref_len = sum(l for op, l in r["cigar"] if op in (0, 2, 3, 7, 8))
        lsp = r["cigar"][0][1] if r["cigar"][0][0] == 4 else 0
        rsp = r["cigar"][-1][1] if len(r["cigar"]) > 1 and r["cigar"][-1][0] == 4 else 0
        a = aln[i]
        a["pos"], a["end"] = start0 + r["pos"], start0 + r["pos"] + ref_len
        a["cig_off"], a["seq_off"], a["n_cig"] = len(cig), len(bq) // 2, len(r["cigar"])
        a["oflag"] = ((2 if r["r2"] else 1) if r["flagged"] else 0) | (4 if r["rev"] else 0) | (16 if r["mmok"] else 0)
        a["mapq"], a["left_sp"], a["qalen"], a["l_seq"] = r["mapq"], lsp, len(r["seq"]) - lsp - rsp, len(r["seq"])
        a["bc_gid"] = bcs.setdefault(r["bc"], len(bcs))
        a["pair_gid"] = pairs.setdefault((r["bc"], r["name"]), len(pairs))
        cig += [(l << 4) | op for op, l in r["cigar"]]
        for s, q in zip(r["seq"], r["qual"]):
            bq += [ord(s), q]
    loc = np.zeros(nl, abi.DEV_LOCUS_DTYPE)
    slot = 0
    for l in range(nl):
        p = start0 + l
        cover = np.flatnonzero((aln["pos"] <= p) & (p < aln["end"]))
        w1 = int((aln["pos"] <= p).sum())
        loc[l] = (int(cover[0]) if len(cover) else w1, w1, slot, len(cover))
        slot += align4(len(cover))
    bq = np.array(bq + [0] * 256, np.uint8)
    return dict(aln=aln, cig=np.array(cig or [0], np.uint32), bq=bq, loc=loc, nl=nl, n_slots=slot, n_bc=len(bcs), n_pair=len(pairs),
                status=int(any(not r["flagged"] for r in reads)), start0=start0)


def depth_run():
    """8 loci of one-base reads: depths 1, 63, 64, 65, 0, 1025, 12 (more barcodes than ds = 8), 4.  Barcodes and strands vary with the
    read; locus 7 holds a barcode whose two fragments interleave in file order."""
    reads, rng = [], np.random.RandomState(7)
    for l, d in enumerate((1, 63, 64, 65, 0, 1025, 12)):
        for k in range(d):
            b = int(rng.randint(0, max(1, d // 3))) if l != 6 else k
            reads.append(read(l, [(0, 1)], "ACGT"[int(rng.randint(4))], "bc%d_%d" % (l, b), "r%d" % int(rng.randint(0, 3)), r2=bool(rng.randint(2)),
                              rev=bool(rng.randint(2)), qual=int(rng.randint(10, 41)), mapq=int(rng.choice([10, 60])), mmok=bool(rng.randint(4))))
    for name in ("f1", "f2", "f1", "f2"):
        reads.append(read(7, [(0, 1)], "A", "bcX", name, r2=name == "f2"))
    return make_run(reads, 8), "ACGTACGT"


def extras_run(qual=30):
    """5 loci: at locus 1 the unusual letters R, Y, R, R in file order (two distinct extra alleles, the first met twice) among plain reads;
    at locus 2 a read that starts a 2-base insertion, one that starts a deletion, and (locus 3) the inside of that deletion; a soft clip."""
    reads = [read(0, [(0, 4)], "AAAA", "b0", "r0", qual=qual), read(0, [(0, 3)], "ARA", "b1", "r0", qual=qual), read(0, [(4, 2), (0, 3)], "TTAYA", "b2", "r0", r2=True, qual=qual),
             read(0, [(0, 2)], "ARA"[:2], "b3", "r0", rev=True, qual=qual), read(1, [(0, 2)], "RA", "b1", "r1", r2=True, rev=True, qual=qual),
             read(1, [(0, 2), (1, 2), (0, 1)], "CAGGT", "b4", "r0", qual=qual), read(1, [(0, 2), (2, 1), (0, 1)], "CAC", "b5", "r0", qual=qual),
             read(2, [(0, 2)], "AC", "b0", "r1", qual=qual)]
    return make_run(reads, 5), "AAACG"


# ---- the two builders on the same device arrays
def counts_of(A):
    return dict(nl=A["nl"], n_slots=A["n_slots"], n_bc=A["n_bc"], n_pair=A["n_pair"], deepest=int(A["loc"]["n"].max()) if len(A["loc"]) else 0)


def whole(eng, up, cnt, lo, P, bits, loc_host=None):
    """smc_build_planes (bits 32) / _w16 over the run in HBM -> dict of host arrays."""
    nl, ns = cnt["nl"], cnt["n_slots"]
    cp = abi.c_params(P)
    nu = ns + nl + 64
    d_w, d_us, d_g, d_f = DevBuf(eng, 4 * ns + 256), DevBuf(eng, 4 * nu), DevBuf(eng, 4 * nu), DevBuf(eng, 4 * nu)
    xcap = devplanes.build_xcap(nl)
    d_l, d_x, d_c = DevBuf(eng, 32 * nl), DevBuf(eng, 20 * xcap), DevBuf(eng, 8)
    bi = abi.SmcBuildIn(up.aln.data_ptr(), up.cig.data_ptr(), up.bq.data_ptr(), up.loc.data_ptr(), up.ref.data_ptr(), lo, nl, cnt["n_bc"], cnt["n_pair"],
                        cnt["deepest"], up.n_aln, loc_host.ctypes.data if loc_host is not None else None)
    try:
        if bits == 16:
            _lib.check(eng.L.smc_build_planes_w16(eng.ctx, ctypes.byref(cp), ctypes.byref(bi), 0, 0, d_w.data_ptr(), d_us.data_ptr(), d_g.data_ptr(),
                                                  d_f.data_ptr(), d_l.data_ptr(), d_x.data_ptr(), xcap, d_c.data_ptr(), None), "smc_build_planes_w16")
        else:
            _lib.check(eng.L.smc_build_planes(eng.ctx, ctypes.byref(cp), ctypes.byref(bi), 0, 0, d_w.data_ptr(), None, None, None, None, d_us.data_ptr(),
                                              d_g.data_ptr(), d_f.data_ptr(), d_l.data_ptr(), d_x.data_ptr(), xcap, d_c.data_ptr(), None), "smc_build_planes")
        c = d_c.download(np.uint32, 2)
        assert int(c[0]) <= xcap
        return dict(words=d_w.download(np.uint16 if bits == 16 else np.uint32, ns), us=d_us.download(np.uint32, nu), gid=d_g.download(np.uint32, nu),
                    finc=d_f.download(np.uint32, nu), loci=d_l.download(LOCUS, nl), x=d_x.download(np.uint32, 5 * int(c[0])).reshape(-1, 5), counters=c)
    finally:
        for b in (d_w, d_us, d_g, d_f, d_l, d_x, d_c):
            b.free()


class Listed(object):
    """One smc_build_listed call into poisoned outputs with guard stretches; the outputs on the host."""

    def __init__(self, eng, copies, ref, lo, nl, offsets, caps, P, bits, shared, xcap=64, slot_base=8, umi_base=5):
        B, G = len(copies), len(offsets)
        self.B, self.G, self.caps, self.bits, self.xcap, self.slot_base, self.umi_base = B, G, list(caps), bits, xcap, slot_base, umi_base
        self.S = S = int(sum(caps))
        desc = np.zeros(max(1, B), COPY_DTYPE)
        for c, (up, cnt) in enumerate(copies):
            desc[c] = (up.aln.data_ptr(), up.cig.data_ptr(), up.bq.data_ptr(), up.loc.data_ptr(), up.n_aln, cnt["n_bc"], cnt["n_pair"], 0)
        wb = bits // 8
        sizes = dict(words=(slot_base + B * S) * wb // 4 + 1, us=umi_base + B * (S + G) + 1, gid=umi_base + B * (S + G) + 1, finc=umi_base + B * (S + G) + 1,
                     loci=8 * B * G, x=5 * xcap * B, counters=2 * B)
        self.bufs = {k: DevBuf(eng, 4 * (n + 2 * GUARD) + 256) for k, n in sizes.items()}
        self.sizes = sizes
        for k, b in self.bufs.items():
            b.upload(np.full(4 * (sizes[k] + 2 * GUARD), POISON, np.uint8))
        d_desc = DevBuf(eng, desc.nbytes + 256).upload(desc)
        off, cp_ = np.array(list(offsets) + [0], np.uint32), np.array(list(caps) + [0], np.uint32)
        cp = abi.c_params(P)
        ptr = {k: b.data_ptr() + 4 * GUARD for k, b in self.bufs.items()}
        try:
            _lib.check(eng.L.smc_build_listed(eng.ctx, ctypes.byref(cp), d_desc.data_ptr(), B, int(shared), lo, nl, ref.data_ptr(), off.ctypes.data,
                                              cp_.ctypes.data, G, bits, slot_base, umi_base, ptr["words"], ptr["us"], ptr["gid"], ptr["finc"], ptr["loci"],
                                              ptr["x"], xcap, ptr["counters"], None), "smc_build_listed")
            self.raw = {k: b.download(np.uint8, 4 * (sizes[k] + 2 * GUARD)) for k, b in self.bufs.items()}
        finally:
            d_desc.free()
            for b in self.bufs.values():
                b.free()
        body = {k: v[4 * GUARD:len(v) - 4 * GUARD] for k, v in self.raw.items()}
        self.words = body["words"].view(np.uint16 if bits == 16 else np.uint32)
        self.us, self.gid, self.finc = (body[k].view(np.uint32) for k in ("us", "gid", "finc"))
        self.loci = body["loci"].view(LOCUS)
        self.x = body["x"].view(np.uint32).reshape(B, xcap, 5) if B else np.zeros((0, xcap, 5), np.uint32)
        self.counters = body["counters"].view(np.uint32).reshape(B, 2)

    def slot(self, c, g):
        return self.slot_base + c * self.S + int(sum(self.caps[:g]))

    def uoff(self, c, g):
        return self.umi_base + c * (self.S + self.G) + int(sum(self.caps[:g])) + g

    def untouched_outside(self, ds, declined=()):
        """Every byte outside what the contract names still holds the poison."""
        keep = {k: np.ones(len(v), bool) for k, v in self.raw.items()}           # True: must still be poison
        wb, base = self.bits // 8, 4 * GUARD

        def free(k, first, n, item):
            keep[k][base + first * item:base + (first + n) * item] = False
        for c in range(self.B):
            free("counters", 2 * c, 2, 4)
            if c in declined:
                continue
            free("x", 5 * self.xcap * c, 5 * min(int(self.counters[c, 0]), self.xcap), 4)
            for g in range(self.G):
                L = self.loci[c * self.G + g]
                free("loci", c * self.G + g, 1, 32)
                free("words", self.slot(c, g), align4(L["n_reads"]), wb)
                free("us", self.uoff(c, g), int(L["n_umi"]) + 1, 4)
                if ds > 0 and int(L["n_umi"]) > ds:
                    free("gid", self.uoff(c, g), int(L["n_umi"]), 4)
                    free("finc", self.uoff(c, g), int(L["n_umi"]), 4)
        for k, v in self.raw.items():
            bad = np.flatnonzero(keep[k] & (v != POISON))
            assert not len(bad), "%s: byte %d written outside the contract" % (k, int(bad[0]) - base)


def compare(W, Lb, c, offsets, ds):
    """Copy c of the listed batch `Lb` against the whole build `W` of the same records, per listed locus."""
    G = len(offsets)
    for g, a in enumerate(offsets):
        w, l = W["loci"][a], Lb.loci[c * G + g]
        for f in ("n_reads", "n_umi", "n_frag", "ref_allele", "n_alleles", "flags", "snp_mask"):
            assert int(w[f]) == int(l[f]), "locus %d (offset %d) copy %d: descriptor field %s %d, the whole build has %d" % (g, a, c, f, int(l[f]), int(w[f]))
        n, nu = int(w["n_reads"]), int(w["n_umi"])
        assert int(l["read_off4"]) * 4 == Lb.slot(c, g) and int(l["umi_off"]) == Lb.uoff(c, g)
        assert align4(n) <= Lb.caps[g]
        ws, ls = 4 * int(w["read_off4"]), Lb.slot(c, g)
        assert W["words"][ws:ws + align4(n)].tobytes() == Lb.words[ls:ls + align4(n)].tobytes(), "words of locus %d (offset %d) copy %d" % (g, a, c)
        wu, lu = int(w["umi_off"]), Lb.uoff(c, g)
        assert W["us"][wu:wu + nu + 1].tobytes() == Lb.us[lu:lu + nu + 1].tobytes(), "umi_start of locus %d copy %d" % (g, c)
        if ds > 0 and nu > ds:
            assert W["gid"][wu:wu + nu].tobytes() == Lb.gid[lu:lu + nu].tobytes() and W["finc"][wu:wu + nu].tobytes() == Lb.finc[lu:lu + nu].tobytes()
    wx = W["x"][np.isin(W["x"][:, 0], offsets)]
    wx = wx[np.lexsort((wx[:, 1], wx[:, 0]))]
    nx = int(Lb.counters[c, 0])
    assert nx == len(wx) and Lb.x[c, :nx].tobytes() == wx.tobytes(), "extras of copy %d: %r, the whole build has %r" % (c, Lb.x[c, :nx].tolist(), wx.tolist())
    assert int(Lb.counters[c, 1]) == int(W["counters"][1])


def check_case(eng, A, ref, offsets, P, bits=(16, 32), copies=1, mutate=None, expect_status=0):
    """Run `A` uploaded once; `copies` copies (copy c > 0: `mutate(A, c)`'s records and pools, the spans as they are) built whole and
    listed, shared order and an order per copy."""
    lo, nl = A["start0"], A["nl"]
    runs = [A] + [mutate(A, c) for c in range(1, copies)]
    ups = [devplanes.upload_run(eng, r, ref) for r in runs]
    caps = [align4(A["loc"]["n"][a]) for a in offsets]
    try:
        for b in bits:
            wholes = [whole(eng, up, counts_of(r), lo, P, b, r["loc"]) for up, r in zip(ups, runs)]
            for shared in ((1, 0) if copies > 1 else (0,)):
                got = [Listed(eng, [(up, counts_of(r)) for up, r in zip(ups, runs)], ups[0].ref, lo, nl, offsets, caps, P, b, shared) for _ in range(2)]
                for k in got[0].raw:
                    assert got[0].raw[k].tobytes() == got[1].raw[k].tobytes(), "two calls differ in %s" % k
                narrow = [b == 16 and bool(int(w["counters"][1]) & ST_NARROW) for w in wholes]
                if not any(narrow):
                    got[0].untouched_outside(P.ds)
                for c in range(copies):
                    if expect_status is not None:
                        assert int(wholes[c]["counters"][1]) == (expect_status if b == 16 else expect_status & ~ST_NARROW)
                    if narrow[c]:                                      # (the words are not to be used: both builders say so)
                        assert int(got[0].counters[c, 1]) == int(wholes[c]["counters"][1])
                    else:
                        compare(wholes[c], got[0], c, offsets, P.ds)
        return wholes, got[0]
    finally:
        for up in ups:
            up.free()


P8 = VcParams(mtDepth=4, rpb=3.0, minBQ=20, minMQ=30)       # ds = 8


def test_depths_offsets_and_the_barcode_cap(engine0):
    A, ref = depth_run()
    assert P8.ds == 8 and A["loc"]["n"].tolist() == [1, 63, 64, 65, 0, 1025, 12, 4]
    W, Lb = check_case(engine0, A, ref, list(range(8)), P8)                       # offsets 0 and nl - 1, a locus with no read, every depth
    assert int(Lb.loci[6]["n_umi"]) == 12 > P8.ds and int(Lb.loci[7]["n_umi"]) == 1 and int(Lb.loci[7]["n_frag"]) == 2
    check_case(engine0, A, ref, [5], P8)                                          # G = 1
    check_case(engine0, A, ref, [0, 7], P8)
    Lb = check_case(engine0, A, ref, [], P8)[1]                                   # G = 0: the counters alone
    assert Lb.counters.tolist() == [[0, 0]]


def test_three_copies_with_their_own_bases(engine0):
    A, ref = depth_run()

    def mutate(A, c):
        B = dict(A)
        B["bq"] = A["bq"].copy()
        B["bq"][0:2 * 1200:2 * (c + 1)] = ord("ACGT"[c])                          # other letters in copy c: a word of another copy would show
        B["bq"][1:2 * 1200:6] = 20 + 7 * c
        return B
    W, Lb = check_case(engine0, A, ref, [1, 3, 5, 6], P8, copies=3, mutate=mutate)
    assert len({W[c]["words"].tobytes() for c in range(3)}) == 3


def test_extra_alleles_indels_and_a_soft_clip(engine0):
    A, ref = extras_run()
    P = VcParams(mtDepth=100, rpb=3.0, minBQ=15, minMQ=20)
    W, Lb = check_case(engine0, A, ref, [0, 1, 2, 3, 4], P)
    x = Lb.x[0, :int(Lb.counters[0, 0])]
    at1 = x[x[:, 0] == 1]
    assert at1[:, 1].tolist() == [6, 7] and int(Lb.loci[1]["n_alleles"]) == 8      # R before Y, R met three times: one id
    assert sorted(np.int32(x[x[:, 0] == 2][:, 4]).tolist()) == [-1, 2]             # an insertion start and a deletion start at locus 2
    assert 5 in (Lb.words[Lb.slot(0, 3):Lb.slot(0, 3) + int(Lb.loci[3]["n_reads"])] & 15).tolist()   # the inside of the deletion: 'DEL'


def test_narrow_words(engine0):
    """A quality of 64: the 16-bit builds both say NARROW, the 32-bit builds are equal."""
    A, ref = extras_run(qual=64)
    P = VcParams(mtDepth=100, rpb=3.0, minBQ=15, minMQ=20)
    check_case(engine0, A, ref, [0, 1, 2], P, expect_status=ST_NARROW)


def test_an_unflagged_alignment_declines(engine0):
    A, ref = depth_run()
    A["aln"]["oflag"][700] &= 0xFC
    up = devplanes.upload_run(engine0, A, ref)
    try:
        Lb = Listed(engine0, [(up, counts_of(A))], up.ref, A["start0"], A["nl"], [1, 5], [64, 1028], P8, 32, 0)
    finally:
        up.free()
    assert Lb.counters.tolist() == [[0, ST_UNFLAGGED]]
    Lb.untouched_outside(P8.ds, declined=(0,))


def test_synthetic_run_with_general_cigars(engine0):
    cfg = synth.SynthConfig("S", 200, 40, 5, 20240, p_overlap=0.9, alt_locus_frac=0.3, alt_af=0.1)
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, 200, P, p_del_aln=0.05, p_ins_aln=0.05, p_clip=0.1)
    offsets = [0, 17, 64, 65, 130, 199]
    check_case(engine0, A, "ACGT" * 50, offsets, P)
    check_case(engine0, A, "ACGT" * 50, offsets, dataclasses.replace(P, maxMT=8), bits=(16,))


@pytest.mark.parametrize("name", ("bam_cigars", "bam_deep", "bam_deep25k"))
def test_fixture_runs(engine0, tmp_path, name):
    bam, fa, loci, P = ds_restate.load_fixture(name, str(tmp_path))
    nat = bamio.NativeBam(bam)
    from smcounter_amd import fasta
    fas = fasta.FastaFile(fa)
    seen = 0
    for chrom, lo, hi in ds_restate.stretches(loci):
        A = nat.alignments_run(chrom, lo, hi, ds_restate.BIG, P, 2)
        if A["status"] & 1 or not len(A["aln"]):
            continue
        A["start0"] = lo
        nl = A["nl"]
        deep = int(np.argmax(A["loc"]["n"]))
        offsets = sorted(set([0, nl - 1, deep] + list(range(0, nl, max(1, nl // 6)))))
        check_case(engine0, A, fas.fetch(chrom, lo, hi).upper(), offsets, P, expect_status=None)   # (bam_deep: qualities beyond 63)
        seen = max(seen, int(A["loc"]["n"].max()))
    assert seen >= dict(bam_cigars=1, bam_deep=10000, bam_deep25k=25600)[name]
    nat.close()


def test_selections_as_copies(engine0):
    """Copies given as the barcode-level selections of select_copies (each its own records and windows, ids as the run's): an order
    per copy.  (The renumbered ids of a read-level selection: test_read_level_selections_as_copies.)"""
    cfg = synth.SynthConfig("S", 128, 40, 4, 99, p_overlap=0.9, alt_locus_frac=0.3, alt_af=0.1)
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, 128, P)
    ref, lo, nl = "ACGT" * 32, A["start0"], 128
    up = devplanes.upload_run(engine0, A, ref)
    idents = np.arange(1, A["n_bc"] + 1, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    sels = devplanes.select_copies(engine0, [up, up, up], A, lo, idents, [11, 12, 13], [0.5])
    offsets = [3, 64, 127]
    caps = [align4(A["loc"]["n"][a]) for a in offsets]
    try:
        copies = [(sel, cnt) for sel, cnt, _ in sels.of[0]]
        for bits in (16, 32):
            Lb = Listed(engine0, copies, up.ref, lo, nl, offsets, caps, P, bits, 0)
            Lb.untouched_outside(P.ds)
            kept = set()
            for c, (sel, cnt) in enumerate(copies):
                W = whole(engine0, sel, cnt, lo, P, bits)
                compare(W, Lb, c, offsets, P.ds)
                kept.add(sel.n_aln)
            assert len(kept) > 1 and max(kept) < up.n_aln
    finally:
        sels.free(); up.free()


def test_read_level_selections_as_copies(engine0):
    """Copies given as the selections of select_copies_reads: whole read names dropped and the kept barcode and read-name ids
    renumbered per copy by first kept appearance; every copy is given its own n_bc and n_pair - and with them its own key widths."""
    cfg = synth.SynthConfig("S", 128, 40, 4, 99, p_overlap=0.9, alt_locus_frac=0.3, alt_af=0.1)
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, 128, P)
    ref, lo, nl = "ACGT" * 32, A["start0"], 128
    up = devplanes.upload_run(engine0, A, ref)
    n_words = (int(A["n_pair"]) + 31) // 32
    rng = np.random.RandomState(7)
    keep = [0.9, 0.5, 0.1]                                       # (the kept names, so the ids' widths, differ widely between the copies)
    masks = np.zeros((3, n_words), np.uint32)
    for c in range(3):
        bits_ = rng.random_sample(32 * n_words) < keep[c]
        masks[c] = np.packbits(bits_.reshape(-1, 32)[:, ::-1], axis=1).view(">u4").reshape(-1).astype(np.uint32)
    d_masks = DevBuf(engine0, masks.nbytes + 256).upload(masks)
    sels = devplanes.select_copies_reads(engine0, [up, up, up], A, lo, d_masks.data_ptr(), n_words, n_words, 1)
    offsets = [3, 64, 127]
    caps = [align4(A["loc"]["n"][a]) for a in offsets]
    try:
        copies = []
        for sel, cnt, _ in sels.of[0]:
            # (the selection call hands on the run's counts as bounds; the renumbered ids end far below them: each copy is given its
            # own tight counts, so the sort's key widths differ between the copies of one call)
            rec = sel.aln.download(np.uint32, 9 * sel.n_aln).reshape(-1, 9)
            copies.append((sel, dict(cnt, n_bc=int(rec[:, 7].max()) + 1, n_pair=int(rec[:, 8].max()) + 1)))
        assert len({sel.n_aln for sel, _ in copies}) == 3 and all(0 < sel.n_aln < up.n_aln for sel, _ in copies)
        assert len({cnt["n_pair"] for _, cnt in copies}) == 3 and len({cnt["n_bc"] for _, cnt in copies}) > 1
        assert all(cnt["n_pair"] < int(A["n_pair"]) for _, cnt in copies)
        for bits in (16, 32):
            Lb = Listed(engine0, copies, up.ref, lo, nl, offsets, caps, P, bits, 0)
            Lb.untouched_outside(P.ds)
            for c, (sel, cnt) in enumerate(copies):
                compare(whole(engine0, sel, cnt, lo, P, bits), Lb, c, offsets, P.ds)
    finally:
        sels.free(); up.free(); d_masks.free()


def test_the_dense_locus_field(engine0):
    """Flag bit 1 (SMC_LISTED_DENSE_LOCUS): an extras entry names its locus by its place g among the listed loci - nothing else moves."""
    A, ref = extras_run()
    P = VcParams(mtDepth=100, rpb=3.0, minBQ=15, minMQ=20)
    offsets = [1, 2, 4]
    caps = [align4(A["loc"]["n"][a]) for a in offsets]
    up = devplanes.upload_run(engine0, A, ref)
    try:
        for shared in (0, 1):
            plain = Listed(engine0, [(up, counts_of(A))] * 2, up.ref, A["start0"], A["nl"], offsets, caps, P, 32, shared)
            dense = Listed(engine0, [(up, counts_of(A))] * 2, up.ref, A["start0"], A["nl"], offsets, caps, P, 32, shared | 2)
            dense.untouched_outside(P.ds)
            for k in plain.raw:
                if k != "x":
                    assert plain.raw[k].tobytes() == dense.raw[k].tobytes(), k
            for c in range(2):
                n = int(plain.counters[c, 0])
                assert n > 0 and set(plain.x[c, :n, 0].tolist()) == {1, 2}
                assert plain.x[c, :n, 1:].tobytes() == dense.x[c, :n, 1:].tobytes()
                assert [offsets[g] for g in dense.x[c, :n, 0].tolist()] == plain.x[c, :n, 0].tolist()
    finally:
        up.free()


def test_refusals(engine0):
    A, ref = depth_run()
    up = devplanes.upload_run(engine0, A, ref)
    cp = abi.c_params(P8)
    d = DevBuf(engine0, 4096)
    one = np.array([3, 0], np.uint32)
    cap = np.array([68, 0], np.uint32)

    def call(ctx=engine0.ctx, copies=d.data_ptr(), B=1, nl=8, off=one, caps=cap, G=1, bits=32, words=d.data_ptr(), counters=d.data_ptr(), slot_base=0, flags=0):
        return engine0.L.smc_build_listed(ctx, ctypes.byref(cp), copies, B, flags, 1000, nl, up.ref.data_ptr(), off.ctypes.data if off is not None else None,
                                          caps.ctypes.data if caps is not None else None, G, bits, slot_base, 0, words, d.data_ptr(), d.data_ptr(), d.data_ptr(),
                                          d.data_ptr(), d.data_ptr(), 8, counters, None)
    try:
        for kw, text in ((dict(ctx=None), "NULL"), (dict(copies=None), "NULL"), (dict(words=None), "NULL"), (dict(counters=None), "NULL"), (dict(off=None), "NULL"),
                         (dict(B=-1), "copies"), (dict(B=1025), "copies"), (dict(G=-1), "listed loci"), (dict(G=65), "listed loci"), (dict(bits=8), "bits"),
                         (dict(off=np.array([8], np.uint32)), "offset 8 of 8"), (dict(off=np.array([3, 3], np.uint32), caps=np.array([4, 4], np.uint32), G=2), "ascend"),
                         (dict(off=np.array([4, 2], np.uint32), caps=np.array([4, 4], np.uint32), G=2), "ascend"), (dict(caps=np.array([66], np.uint32)), "capacity"),
                         (dict(slot_base=2), "boundary"), (dict(flags=4), "flags")):
            assert call(**kw) != 0, kw
            assert text in engine0.L.smc_last_error().decode(), (kw, engine0.L.smc_last_error())
    finally:
        d.free(); up.free()
