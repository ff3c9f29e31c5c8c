"""smc_scan_detect_keys on the GPU.

The hand-made case: one run of 16 alignments over 12 loci, B = 3 copies with records and pair pools of their own (strides that are no
multiple of a record's size, as the stage's are), G = 8 listed variants - two SNVs, three deletions, three insertions, the first and
the last locus among them.  Rows, records, pairs and extras lists are made in numpy.  Every resolved id against the index of the key's
text in the host's table of that (copy, locus) - devplanes.extras_table over the same entries with devplanes.synth_allele_key, the
restatement of smc_bam_allele_key; every CALLED / NOT against devplanes.scan_called_host on the same row printed with that table; every
HOST one of the documented reasons; the HOST list; nothing written outside the output buffers; two calls alike; the refusals.

The builder's numbering: a synthetic run of 32 loci spiked by spike_indel_run_copies into 3 copies at thresholds 2^32, 2^31 and 0; the
copies built with extras left in HBM and built eagerly; the device ids must be tables[l].index(key) of the eager build."""
import collections
import ctypes
import re

import numpy as np
import pytest

from smcounter_amd import _lib, abi, devplanes, synth, vc
from smcounter_amd.engine import DevBuf
from smcounter_amd.params import VcParams
from smcounter_amd.pileup import BASE_ALLELES
from smcounter_amd.tools import ds_allele_fraction as af

pytestmark = pytest.mark.gpu
B, NL, N_ALN, L_SEQ, THR, XCAP = 3, 12, 16, 10, 17, 9
REF = "ATACGTAGCGTCAGT"                                    # (three letters behind the last locus: the deletion listed there)
N_PAIRS = N_ALN * L_SEQ
SA, SB = 640, 384                                          # byte strides: >= 36 * 16 / 2 * 160, multiples of 4 / 2, SA no multiple of 36
EDGE = THR - 0.005
LO, HI = EDGE - 1e-6, EDGE + 1e-6
NONE, HOST_ID = abi.SCAN_ID_NONE, abi.SCAN_ID_HOST
V = lambda pos, ref, alt: af.Variant("chrT", pos, ref, alt, *af.allele_key(ref, alt))
VARIANTS = [V(1, "A", "G"), V(3, "ACG", "A"), V(4, "C", "CGT"), V(6, "TA", "T"), V(7, "A", "ATTT"), V(9, "C", "T"), V(10, "G", "GC"),
            V(12, "CAGT", "C")]
G = len(VARIANTS)
# per copy the extras entries in the list's order: (locus, allele id, alignment, query position, indel, the read's letters from the
# query position on).  The ids of a locus count up from 6 in any order of the LIST - the builder appends from many lanes.
ENTRIES = [
    [   # copy 0
        (2, 8, 0, 3, -2, "A"),          # the planted deletion, numbered third at its locus
        (2, 6, 1, 3, -1, "A"),          # a deletion of another length
        (2, 7, 2, 3, -2, "G"),          # the right length behind another anchor letter
        (3, 6, 4, 2, 2, "CGA"),         # one wrong inserted letter
        (3, 7, 3, 2, 2, "CGT"),         # the planted insertion
        (4, 6, 5, 1, 1, "GA"),          # an entry at a locus that is not listed
        (6, 6, 6, 6, 5, "ATTT"),        # an insertion clamped at the read's end to the three listed letters (10 - 7 = 3 of 5)
        (9, 7, 13, 4, 1, "GC"),         # two matching entries: must not happen - HOST
        (9, 6, 7, 4, 1, "GC"),
    ],
    [   # copy 1 (no entry at loci 11 and 3's wrong letter only)
        (2, 6, 1, 3, -1, "A"),          # only the other length: nobody shows the key
        (3, 6, 4, 2, 2, "CGA"),
        (5, 6, 8, 0, -1, "T"),          # a deletion at query position 0
        (6, 6, 6, 7, 3, "ATT"),         # clamped to two letters: INS|A|ATT, not the listed key
        (9, 6, 9, 4, 0, "N"),           # a letter key in front of the planted one
        (9, 7, 7, 4, 1, "GC"),
        (11, 6, 10, 9, -3, "C"),        # the last locus, the read's last base
        (0, 6, 11, 0, 1, "AG"),         # an insertion at the first locus, where an SNV is listed: its id stays the letter's
    ],
    [   # copy 2: a count of 12 above xcap = 9 - the entries behind the ninth are not read
        (9, 6, 7, 4, 1, "GC"),
        (11, 6, 99, 0, -3, "C"),        # an alignment beyond n_aln: unreadable - HOST
        (2, 6, 0, 3, -2, "A"),
        (5, 6, 8, 12, -1, "T"),         # a query position beyond l_seq: unreadable - HOST
        (3, 6, 3, 2, 2, "CGT"),
        (6, 6, 6, 6, 3, "ATTT"),        # the listed insertion unclamped
        (4, 6, 5, 1, 1, "GA"),
        (7, 6, 12, 1, -1, "G"),
        (0, 6, 11, 0, 1, "AG"),
        (9, 7, 13, 4, 1, "GC"),         # (behind xcap) would be a second match
        (5, 7, 14, 0, -1, "T"),         # (behind xcap)
        (2, 7, 15, 3, -2, "A"),         # (behind xcap)
    ],
]
# (what cand[0] holds: "alt" the resolved id, "other" another allele; PI; bi-allelic; status)
CASES = [
    ("alt", HI + 10.0, 0, 0), ("alt", 3.0, 0, 0), ("alt", EDGE, 0, 0), ("alt", LO, 0, 0), ("alt", HI, 0, 0),
    ("alt", float(np.nextafter(LO, -np.inf)), 0, 0), ("alt", float(np.nextafter(HI, np.inf)), 0, 0),
    ("other", 40.0, 0, 0), ("other", 40.0, 1, 0), ("alt", 40.0, 1, 0), ("alt", 40.0, 0, abi.ST_ZERO_COVERAGE),
]


class _Ref(object):
    def fetch(self, chrom, a, b):
        return REF[a:b]


def _make():
    """-> dict of the inputs; `tables[(c, l)]`: the host's allele table from the entries the kernel reads, or None where an entry of
    the locus names a record that cannot be read."""
    aln = np.zeros((B, N_ALN), abi.DEV_ALN_DTYPE)
    aln["l_seq"], aln["n_cig"], aln["seq_off"] = L_SEQ, 1, (np.arange(N_ALN) * L_SEQ)[None, :]
    aln["pos"], aln["end"] = 0, NL
    pairs = np.zeros((B, N_PAIRS, 2), np.uint8)
    pairs[:, :, 0], pairs[:, :, 1] = ord("N"), 30
    x = np.zeros((B, 16, 5), np.uint32)
    count = np.zeros((B, 2), np.uint32)
    for c, entries in enumerate(ENTRIES):
        count[c] = (len(entries), 0)
        for e, (l, aid, ai, qpos, indel, letters) in enumerate(entries):
            x[c, e] = (l, aid, ai, qpos, np.uint32(np.int32(indel)))
            if ai < N_ALN and qpos < L_SEQ:
                pairs[c, ai * L_SEQ + qpos:ai * L_SEQ + qpos + len(letters), 0] = np.frombuffer(letters.encode(), np.uint8)
    assert int(count[2, 0]) > XCAP and all(len(e) <= 16 for e in ENTRIES)
    var, ins = devplanes.af_run_variants(VARIANTS, "chrT", 0, _Ref())
    assert list(var["kind"]) == [0, 2, 1, 2, 1, 0, 1, 2] and (np.diff(var["locus"].astype(int)) > 0).all() and var["locus"][-1] == NL - 1
    tables = {}
    for c in range(B):
        xl = x[c, :min(int(count[c, 0]), XCAP)]
        key = devplanes.synth_allele_key(dict(aln=aln[c], seq=np.ascontiguousarray(pairs[c, :, 0])))
        for l in range(NL):
            mine = xl[xl[:, 0] == l]
            if any(int(ai) >= N_ALN or int(q) >= L_SEQ for ai, q in mine[:, 2:4].tolist()):
                tables[(c, l)] = None
            else:
                tables[(c, l)] = devplanes.extras_table(xl, l, key, "chrT", 0, _Ref())
    want = np.zeros((B, G), np.uint32)
    for c in range(B):
        for g, v in enumerate(VARIANTS):
            t = tables[(c, v.pos - 1)]
            if v.kind == af.SNV:
                want[c, g] = BASE_ALLELES.index(v.alt)
            else:
                want[c, g] = HOST_ID if t is None or t.count(v.key) > 1 else t.index(v.key) if v.key in t else NONE
    # rows: every locus a callable row whose candidate is a called letter; the listed ones by CASES
    rows = np.zeros((B, NL), abi.ROW_DTYPE)
    rows["cvg"], rows["all_frag"], rows["all_mt"], rows["used_frag"], rows["used_mt"] = 400, 400, 120, 380, 100
    rows["mt3"], rows["mt5"], rows["mt7"], rows["mt10"] = 90, 80, 70, 60
    rows["dp"], rows["umt"], rows["vsm"], rows["pi"] = 100, 25, 20, 1.5
    rows["cand"]["allele"][:, :, 0], rows["cand"]["allele"][:, :, 1] = 2, -1
    rows["cand"]["vdp"], rows["cand"]["vmt"], rows["cand"]["vsm"], rows["cand"]["pi"] = 40, 12, 9, 55.0
    rows["used_mt"] += (np.arange(B * NL) % 37).reshape(B, NL).astype(np.int32)
    case_of = {}
    for c in range(B):
        for g, v in enumerate(VARIANTS):
            l = v.pos - 1
            what, pi, bi, status = case = CASES[(c * G + g) % len(CASES)]
            case_of[(c, g)] = case
            other = BASE_ALLELES.index("T" if REF[l] != "T" and v.alt != "T" else "G" if REF[l] != "G" and v.alt != "G" else "C")
            resolved = int(want[c, g]) if int(want[c, g]) < HOST_ID else other
            cand = rows["cand"]
            cand["allele"][c, l, 0] = resolved if what == "alt" else other
            cand["pi"][c, l, 0], rows["biallelic"][c, l], rows["status"][c, l] = pi, bi, status
            if bi:
                cand["allele"][c, l, 1] = other if what == "alt" else resolved
                cand["pi"][c, l, 1] = 45.0
    return dict(aln=aln, pairs=pairs, x=x, count=count, var=var, ins=ins, tables=tables, want=want, rows=rows, case_of=case_of)


@pytest.fixture(scope="module")
def made():
    return _make()


def test_the_hand_made_ids_cover_every_listed_shape(made):
    """(no GPU work: the expectation itself, from the host's tables) every shape the issue lists is in the case."""
    want = made["want"]
    assert want[:, 0].tolist() == [2, 2, 2] and want[:, 5].tolist() == [1, 1, 1]           # the SNVs: the letters' fixed ids
    assert want[0].tolist() == [2, 8, 7, NONE, 6, 1, HOST_ID, NONE]
    assert want[1].tolist() == [2, NONE, NONE, 6, NONE, 1, 7, 6]
    assert want[2].tolist() == [2, 6, 6, HOST_ID, 6, 1, 6, HOST_ID]
    assert made["tables"][(0, 6)][6] == "INS|A|ATTT" and made["tables"][(1, 6)][6] == "INS|A|ATT"     # clamped at the read's end
    assert made["tables"][(1, 11)][6] == "DEL|CAGT|C" and made["tables"][(0, 2)][6:] == ["DEL|AC|A", "DEL|GCG|G", "DEL|ACG|A"]


class _Up(object):
    """The case's arrays in HBM, every buffer with a pad filled with 0xA5 behind it."""
    PAD, FILL = 512, 0xA5

    def __init__(self, eng, made):
        flat = lambda a: np.ascontiguousarray(a).view(np.uint8).reshape(-1)
        d_aln, d_bq = np.full(SA * B, self.FILL, np.uint8), np.full(SB * B, self.FILL, np.uint8)
        for c in range(B):
            d_aln[c * SA:c * SA + 36 * N_ALN] = flat(made["aln"][c])
            d_bq[c * SB:c * SB + 2 * N_PAIRS] = flat(made["pairs"][c])
        n = B * G
        self.inputs = [flat(made["rows"]), flat(made["var"]), flat(made["ins"]), d_aln, d_bq, np.zeros(64, np.uint8), flat(made["x"]),
                       flat(made["count"])]
        self.out_sizes = [4 * n, 16 * n, 4 * n, 4]                      # ids, records, HOST list, cursor
        self.sizes = [len(a) + self.PAD for a in self.inputs] + [s + self.PAD for s in self.out_sizes]
        self.bufs = [DevBuf(eng, s) for s in self.sizes]
        self.eng = eng
        self.reset()

    def reset(self):
        for b, s in zip(self.bufs, self.sizes):
            b.upload(np.full(s, self.FILL, np.uint8))
        for b, a in zip(self.bufs, self.inputs):
            b.upload(a)

    def state(self):
        return [b.download(np.uint8, s) for b, s in zip(self.bufs, self.sizes)]

    def call(self, made, var=None, **kw):
        p = [b.data_ptr() for b in self.bufs]
        var = made["var"] if var is None else var
        a = dict(n_copies=B, n_loci=NL, n_listed=len(var), n_ins=len(made["ins"]), sa=SA, sc=0, sb=SB, n_aln=N_ALN, cap_pairs=N_PAIRS,
                 x_stride=16 * 5, cnt_stride=2, xcap=XCAP, thr=float(THR))
        a.update(kw)
        return self.eng.L.smc_scan_detect_keys(self.eng.ctx, p[0], a["n_copies"], a["n_loci"], p[1], var.ctypes.data, a["n_listed"], p[2],
                                               a["n_ins"], p[3], a["sa"], p[5], a["sc"], p[4], a["sb"], a["n_aln"], a["cap_pairs"], p[6],
                                               a["x_stride"], p[7], a["cnt_stride"], a["xcap"], a["thr"], p[8], p[9], p[10], p[11],
                                               ctypes.c_void_p(0))

    def free(self):
        for b in self.bufs:
            b.free()


def _host_called(made, c, g):
    v = VARIANTS[g]
    l = v.pos - 1
    view = vc.LocusView(["chrT"], [v.pos], [REF[l]], [made["tables"][(c, l)]])
    text = vc._strings(made["rows"][c, l:l + 1].copy(), view, VcParams(mtDepth=250, rpb=3.0), _Ref())
    assert not text[0].startswith(vc.EXC_PREFIX), text[0]
    nothing = (collections.defaultdict(list), collections.defaultdict(list))
    return devplanes.scan_called_host(text[0], v, THR, nothing)


def test_ids_verdicts_host_list_and_nothing_else_written(engine0, made):
    up = _Up(engine0, made)
    try:
        _lib.check(up.call(made), "smc_scan_detect_keys")
        first = up.state()
        _lib.check(up.call(made), "smc_scan_detect_keys")
        second = up.state()
    finally:
        up.free()
    n = B * G
    ids = first[8][:4 * n].view(np.uint32).reshape(B, G)
    rec = first[9][:16 * n].view(abi.SCAN_VERDICT_DTYPE).reshape(B, G)
    n_host = int(first[11][:4].view(np.uint32)[0])
    todo = np.sort(first[10][:4 * n_host].view(np.uint32))
    print("ids:\n%s\nwant:\n%s" % (ids, made["want"]))
    assert np.array_equal(ids, made["want"])
    verdict = rec["mt_verdict"] >> 30
    seen = collections.Counter()
    for c in range(B):
        for g, v in enumerate(VARIANTS):
            r = made["rows"][c, v.pos - 1]
            what, pi, bi, status = made["case_of"][(c, g)]
            got = int(verdict[c, g])
            print("copy %d %s:%d %s>%s id %d: cand %d PI %.17g biallelic %d status %d -> %d" %
                  (c, v.chrom, v.pos, v.ref, v.alt, ids[c, g], r["cand"][0]["allele"], pi, bi, status, got))
            seen[got] += 1
            assert rec[c, g]["pi"].tobytes() == r["cand"][0]["pi"].tobytes() and int(rec[c, g]["vmt"]) == int(r["cand"][0]["vmt"])
            assert int(rec[c, g]["mt_verdict"]) & abi.SCAN_MT_MASK == int(r["used_mt"])
            shows = int(ids[c, g]) < HOST_ID and int(r["cand"][0]["allele"]) == int(ids[c, g])
            if got == abi.SCAN_HOST:
                # the documented reasons: two entries show the key or a record cannot be read; a bi-allelic row; a status that is not
                # 0; the planted allele in front with a PI inside the band
                assert int(ids[c, g]) == HOST_ID or bi != 0 or status != 0 or (shows and LO <= pi <= HI), (c, g)
            else:
                assert int(ids[c, g]) != HOST_ID and bi == 0 and status == 0 and not (shows and LO <= pi <= HI)
                assert got == (abi.SCAN_CALLED if shows and pi > HI else abi.SCAN_NOT)
                assert (got == abi.SCAN_CALLED) == _host_called(made, c, g), (c, g, made["case_of"][(c, g)])
                if int(ids[c, g]) == NONE:
                    assert got == abi.SCAN_NOT
    assert all(seen[v] >= 3 for v in (abi.SCAN_NOT, abi.SCAN_CALLED, abi.SCAN_HOST)), seen
    assert any(int(ids[c, g]) == HOST_ID and made["case_of"][(c, g)][1:] == (HI + 10.0, 0, 0) for c in range(B) for g in range(G)) or \
        any(int(ids[c, g]) == HOST_ID and made["case_of"][(c, g)][2:] == (0, 0) and not LO <= made["case_of"][(c, g)][1] <= HI
            for c in range(B) for g in range(G)), "no HOST verdict that only the id explains"
    assert todo.tolist() == np.flatnonzero(verdict.reshape(-1) == abi.SCAN_HOST).tolist()
    # the inputs as they went up; behind every output only the fill; the list's tail untouched
    for k, a in enumerate(up.inputs):
        assert first[k][:len(a)].tobytes() == a.tobytes() and (first[k][len(a):] == up.FILL).all(), k
    for k, size in zip((8, 9, 11), (4 * n, 16 * n, 4)):
        assert (first[k][size:] == up.FILL).all(), k
    assert (first[10][4 * n_host:] == up.FILL).all() and 0 < n_host < n
    # a second call: the same bytes (the list as a set)
    for k in (8, 9, 11):
        assert second[k].tobytes() == first[k].tobytes(), k
    assert np.array_equal(np.sort(second[10][:4 * n_host].view(np.uint32)), todo) and (second[10][4 * n_host:] == up.FILL).all()


def test_the_wrapper_and_an_empty_list(engine0, made):
    up = _Up(engine0, made)
    try:
        p = [b.data_ptr() for b in up.bufs]
        copies = dict(aln=p[3], cig=p[5], bq=p[4], strides=(SA, SB, 0), n_aln=N_ALN, cap_pairs=N_PAIRS)
        extras = dict(x=p[6], cnt=p[7], x_stride=80, cnt_stride=2, xcap=XCAP)
        rec, todo, ids = devplanes.scan_detect_keys(engine0, up.bufs[0], B, NL, made["var"], made["ins"], copies, extras, THR)
        assert np.array_equal(ids, made["want"]) and rec.shape == (B, G)
        assert todo.tolist() == np.flatnonzero((rec["mt_verdict"] >> 30).reshape(-1) == abi.SCAN_HOST).tolist()
        rec, todo, ids = devplanes.scan_detect_keys(engine0, up.bufs[0], B, NL, made["var"][:0], made["ins"], copies, extras, THR)
        assert rec.shape == (B, 0) and ids.shape == (B, 0) and len(todo) == 0
        # G = 0 through the entry: the cursor zeroed, nothing else touched
        up.reset()
        _lib.check(up.call(made, n_listed=0), "smc_scan_detect_keys")
        st = up.state()
        assert int(st[11][:4].view(np.uint32)[0]) == 0 and all((st[k] == up.FILL).all() for k in (8, 9, 10))
    finally:
        up.free()


def test_refusals_launch_nothing(engine0, made):
    up = _Up(engine0, made)
    var = made["var"]

    def wrong(g, **fields):
        w = var.copy()
        for k, val in fields.items():
            w[g][k] = val
        return w
    try:
        swapped = var.copy()
        swapped[[2, 3]] = swapped[[3, 2]]
        for kw, msg in ((dict(var=swapped), "ascending expected"),
                        (dict(var=wrong(G - 1, locus=NL)), "names locus %d of %d" % (NL, NL)),
                        (dict(var=wrong(1, kind=4)), "has kind 4"),
                        (dict(var=wrong(1, len=0)), "a length of 0"),
                        (dict(var=wrong(2, len=256)), "a length of 256"),
                        (dict(var=wrong(6, ins_off=len(made["ins"]))), "inserted letters at"),
                        (dict(var=wrong(0, letter=ord("N"))), "one of A, C, G, T expected"),
                        (dict(sa=SA + 2), "multiples of 4 / 4 / 2 expected"),
                        (dict(sc=6), "multiples of 4 / 4 / 2 expected"),
                        (dict(sb=SB + 1), "multiples of 4 / 4 / 2 expected"),
                        (dict(n_copies=65536), "at most 65535"),
                        (dict(thr=float("nan")), "not finite"),
                        (dict(n_loci=1 << 31), "2^31 records or rows")):
            with pytest.raises(_lib.SmcError, match=re.escape(msg)):
                _lib.check(up.call(made, **kw), "smc_scan_detect_keys")
        st = up.state()
        assert all((st[k] == up.FILL).all() for k in (8, 9, 10, 11))
    finally:
        up.free()


# ---- the builder's numbering
def test_ids_equal_the_eager_builds_tables_on_spiked_copies(engine0):
    from smcounter_amd.tools import spike_variants as sv
    eng = engine0
    cfg = synth.SynthConfig("K", 32, 40, 50, 4242, p_overlap=0.9, alt_locus_frac=0.3, alt_af=0.1)
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, 32, P, p_del_aln=0.03, p_ins_aln=0.02, p_clip=0.05)
    nl, lo = int(A["nl"]), int(A["start0"])
    fa = synth.CyclicRef()
    run_ref = synth.aln_ref_fetch(lo, lo + nl)
    chrom = synth.ALN_CHROM
    # a deletion, a duplication, an SNV and a longer deletion, footprints disjoint, every letter the genome's
    listed = []
    for off, kind, n in ((3, "del", 1), (9, "dup", 2), (14, "snv", 0), (20, "del", 3), (27, "dup", 1)):
        w = run_ref[off:off + n + 1]
        ref, alt = (w, w[0]) if kind == "del" else (w[0], w) if kind == "dup" else (w, "ACGT"[("ACGT".index(w) + 1) % 4])
        listed.append(af.Variant(chrom, lo + off + 1, ref, alt, *af.allele_key(ref, alt)))
    svar, pool, _ = devplanes.spike_indel_variants(listed, 0)
    var, ins = devplanes.af_run_variants(listed, chrom, lo, fa)
    up = devplanes.upload_run(eng, A, run_ref)
    idents = np.array([devplanes._fnv64("B%d" % g) for g in range(int(A["n_bc"]))], np.uint64)
    zeros = np.zeros(len(A["aln"]), np.int32)
    thr = [1 << 32, 1 << 31, 0]
    made = devplanes.spike_indel_run_copies(eng, up, A, svar, pool, idents, [11, 12, 13], thr, P.mismatchThr, zeros, zeros)
    sa, sb, sc = made["strides"]
    runs = [devplanes.RunOnDevice(devplanes._BufView(made["aln"], c * sa), devplanes._BufView(made["cig"], c * sc),
                                  devplanes._BufView(made["bq"], c * sb), up.loc, up.ref, up.n_aln, up.loc_host,
                                  pairs_used=int(made["totals"][c, 0])) for c in range(3)]
    xcap = devplanes.build_xcap(nl)
    d_x, d_cnt = DevBuf(eng, 20 * xcap * 3 + 256), DevBuf(eng, 8 * 3 + 256)
    run = devplanes.AfRun(chrom, lo, lo + nl, [], 0)
    run.A, run.nl, run.run_ref = A, nl, run_ref
    name = lambda g: "B%d" % g
    kept = lambda: (devplanes._KeptRun(runs[c], A, None, A, devplanes.synth_allele_key(A), name, lambda n: idents, copy=runs[c])
                    for c in range(3))
    batches = []
    try:
        extras = [devplanes.BuildExtras(devplanes._BufView(d_x, 20 * xcap * c), devplanes._BufView(d_cnt, 8 * c)) for c in range(3)]
        lazy = devplanes._build_copies(eng, run, 3, kept(), P, 32, "test", fa, eng.L.smc_build_max_depth(), "reference", 0, extras)
        batches.append(lazy)
        eager = devplanes._build_copies(eng, run, 3, kept(), P, 32, "test", fa, eng.L.smc_build_max_depth(), "reference", 0)
        batches.append(eager)
        assert lazy.tables == [] and len(eager.tables) == 3 * nl
        assert all(np.array_equal(a, b) for a, b in zip(lazy.LC, eager.LC))
        rows = np.zeros(3 * nl, abi.ROW_DTYPE)
        d_rows = DevBuf(eng, rows.nbytes + 256).upload(rows.view(np.uint8).reshape(-1))
        batches.append(d_rows)
        _, _, ids = devplanes.scan_detect_keys(
            eng, d_rows, 3, nl, var, ins,
            dict(aln=made["aln"].data_ptr(), cig=made["cig"].data_ptr(), bq=made["bq"].data_ptr(), strides=(sa, sb, sc), n_aln=up.n_aln,
                 cap_pairs=made["caps"][0]),
            dict(x=d_x.data_ptr(), cnt=d_cnt.data_ptr(), x_stride=5 * xcap, cnt_stride=2, xcap=xcap), THR)
        shown = 0
        for c in range(3):
            for g, v in enumerate(listed):
                table = eager.tables[c * nl + v.pos - 1 - lo]
                want = BASE_ALLELES.index(v.alt) if v.kind == af.SNV else table.index(v.key) if v.key in table else NONE
                print("copy %d (thr %d) %s:%d %s>%s: id %d, the eager table %r" % (c, thr[c], v.chrom, v.pos, v.ref, v.alt, ids[c, g], table[6:]))
                assert int(ids[c, g]) == want and table.count(v.key) <= 1
                shown += v.kind != af.SNV and want != NONE
                # (the table of one locus from the extras left in HBM is the eager build's)
                n_x = extras[c].n
                xl = extras[c].x.download(np.uint32, 5 * n_x).reshape(n_x, 5)
                assert devplanes.extras_table(xl, v.pos - 1 - lo, devplanes.copy_allele_key(runs[c], A, devplanes.synth_allele_key(A)),
                                              chrom, lo, fa) == table
        # every barcode spiked: every key is shown in copy 0; none spiked in copy 2 unless the file has it
        assert all(int(ids[0, g]) >= 6 and int(ids[0, g]) != NONE for g, v in enumerate(listed) if v.kind != af.SNV)
        assert shown >= 4
        assert sv.footprint(listed[3]) == (listed[3].pos, listed[3].pos + 4)
    finally:
        for b in batches + [d_x, d_cnt, made["aln"], made["bq"], made["cig"]]:
            b.free()
        up.free()
