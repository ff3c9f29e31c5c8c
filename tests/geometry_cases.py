"""Constructed alignments for the read-class pins (tests/test_geometry_ref.py, tests/test_gpu_geometry.py): every record is made by
rule - no random base anywhere - so that the shapes at which a plane builder can go wrong are all there and stay there:

  reference  one chromosome of 6,144 bases (a linear congruential sequence);
  targets    four runs of consecutive positions: the chromosome's first 30 bases; 210 loci from 0-based 1000 (tiles of 64 loci at
             1000, 1064, 1128, 1192; groups of 16 at 1000 + 16 k) - more than 256 alignments lie under the tile at 1064; 40 loci
             from 5400 (the shallow run: the far side of the long skips, and the alignments flagged neither READ1 nor READ2); the
             chromosome's last 30 bases;
  plain rows for read 1 / read 2 x forward / reverse and for a reverse record flagged both READ1 and READ2: lengths 15, 20, 21, 40, 41
             and 45 with the first base, and the position behind the last base, on, one before and one after the tile boundaries 1064 and
             1128 and the group boundary 1080; length 151 across three tiles; length 100 at MAPQ 255 in each of the nine phases of the
             quality cycle; a left soft clip reaching before a run's first position; a read at reference position 0 and one ending at
             the chromosome's last base;
  clips      5S40M, 40M6S, 3H4S38M (only a soft clip that is the FIRST operation is leftSP, smCounter.py:345: 0 here), 2H30M2H, 4S36M3H;
             2H4S16M, the same quirk on a read short enough to be within 20 of the barcode end and at or past the primer end at once;
  general    an insertion behind the last locus of a tile, a deletion across a tile boundary, an insertion / a deletion 1, 19, 20 and 21
             bases from either end, D next to I both ways, a skip of 50, a skip of 4,200 with targets on both sides, a CIGAR of 69
             operations;
  NM         absent, 0, 2, below the indel count, 4 beyond the indel count on 40 bases, and 3 or 4 mismatches on 50 bases (6.0 and 8.0
             per 100: on and over mismatchThr 6.0);
  qualities  0, 1, 19, 20, 21, 40, 41, 62, 63 in turn along every read; MAPQ 0, 29, 30, 60, 255.
Barcodes go round 31 names with the record, so every barcode has rows in every batch of 64 and every part of 256 rows of the deep tile.

PARAM_SETS crosses primerDist, minBQ, minMQ and mismatchThr (each value at least twice).  make_geometry_golden.py runs the
reference on every (set, locus) and asserts the coverage stated above (coverage_of there; unreachable_classes here)."""
import json
import os

import numpy as np

from smcounter_amd.params import VcParams

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "geometry")
FIXTURES = ("shapes",)
CHROM, L = "chrG", 6144
RUNS = ((0, 30), (1000, 1210), (5400, 5440), (L - 30, L))          # 0-based, half open
RUN_A, RUN_B = RUNS[1], RUNS[2]
TILE, GROUP = 64, 16
QUALS = (0, 1, 19, 20, 21, 40, 41, 62, 63)
MAPQS = (60, 255, 30, 60, 29, 255, 0, 60)
INSERT = "GATTACAGGC"
LIN_SPAN = 4096                                                      # BP2_LIN_SPAN (csrc/k_bp_emit2.inc)
# (primerDist, minBQ, minMQ, mismatchThr): every primerDist with two of the nine inclusion triples, every triple with two primerDist -
# what the reference tallies does not depend on primerDist, so the fixture stores nine captures for the eighteen sets
PRIMER_DISTS = (0, 1, 2, 19, 20, 21, 60, 200, 100000)
INCLUSION = ((20, 30, 6.0), (0, 0, 100.0), (1, 60, 6.0), (41, 30, 100.0), (63, 0, 6.0), (20, 61, 100.0), (1, 255, 6.0), (64, 30, 6.0),
             (41, 255, 100.0))
PARAM_SETS = tuple((PRIMER_DISTS[i % 9],) + INCLUSION[(i + 4 * (i // 9)) % 9] for i in range(18))
COMBOS = ((0x40, False), (0x40, True), (0x80, False), (0x80, True))  # (mate flag, reverse)
BOTH = (0xC0, True)                                                  # READ1 and READ2: the reference ends on 'R2' (smCounter.py:359-362)


def params_of(t):
    pd, bq, mq, thr = t
    return VcParams(mtDepth=2000, rpb=3.0, hpLen=8, minBQ=bq, minMQ=mq, mismatchThr=thr, primerDist=pd)   # (ds = 4000: nothing is sampled)


def set_id(t):
    return "pd%d-bq%d-mq%d-mm%g" % t


def reference_sequence():
    x, out = 20260, []
    for _ in range(L):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out.append("ACGT"[(x >> 16) & 3])
    return "".join(out)


def ref_span(cigar):
    return sum(l for op, l in cigar if op in (0, 2, 3, 7, 8))


def cigar_of(text):
    ops, n = [], ""
    for ch in text:
        if ch.isdigit():
            n += ch
        else:
            ops.append(("MIDNSHP=X".index(ch), int(n)))
            n = ""
    return ops


def records():
    """-> the records in file order (bamio.write_bam's dicts, + `tag`: what the record is there for)."""
    seq = reference_sequence()
    recs = []

    def add(tag, pos, cigar, flag, rev, nm="rule", subs=True, mapq=None, qoff=None):
        i = len(recs)
        cig = cigar_of(cigar) if isinstance(cigar, str) else list(cigar)
        assert pos >= 0 and pos + ref_span(cig) <= L, (tag, pos, cigar)
        out, x, k = [], pos, 0
        for op, l in cig:
            if op in (0, 7, 8):
                out.append(seq[x:x + l]); x += l
            elif op in (1, 4):
                out.append((INSERT * (l // len(INSERT) + 2))[k:k + l]); k += 1
            elif op in (2, 3):
                x += l
        s = list("".join(out))
        if subs and i % 6 == 1:                                      # another letter somewhere along the read; now and then an N
            j = (5 * i) % len(s)
            s[j] = "N" if i % 36 == 1 else {"A": "G", "C": "T", "G": "A", "T": "C"}[s[j]]
        if nm == "rule":
            nm = None if i % 7 == 3 else 2 if i % 11 == 5 else 0
        pair = i // 2
        recs.append(dict(tid=0, pos=pos, qname="f%d:NN:BC%02d:x" % (pair, pair % 31), flag=flag | (0x10 if rev else 0) | 1,
                         mapq=MAPQS[(i + i // 8) % 8] if mapq is None else mapq, cigar=cig, seq="".join(s),
                         qual=[QUALS[((4 * i if qoff is None else qoff) + j) % 9] for j in range(len(s))],
                         nm=nm, tag=tag))

    a0 = RUN_A[0]
    # ---- plain rows
    for flag, rev in COMBOS + (BOTH,):
        for ln in (15, 20, 21, 40, 41, 45):
            for edge in (a0 + TILE, a0 + TILE + GROUP, a0 + 2 * TILE):
                for d in (-1, 0, 1):
                    add("plain start", edge + d, "%dM" % ln, flag, rev)
                    add("plain end", edge + d - ln, "%dM" % ln, flag, rev)
        for start in (a0 + 20, a0 + TILE - 1, a0 + TILE + 1):
            add("plain 151", start, "151M", flag, rev)
        add("clip before the run", a0, "8S30M", flag, rev)
        add("clip before the run", RUN_B[0], "6S30M", flag, rev)
        add("position 0", 0, "30M", flag, rev)
        add("position 0", 0, "5S25M", flag, rev)
        add("last base", L - 40, "40M", flag, rev)
        add("last base", L - 35, "35M5S", flag, rev)
    # ---- clips, general CIGARs: the four (mate, strand) combinations each
    k = 0
    for flag, rev in COMBOS:
        for c in ("5S40M", "40M6S", "3H4S38M", "2H30M2H", "4S36M3H"):
            add("clip", a0 + 12 + k % 9, c, flag, rev); k += 1
        # (included under every set that includes anything of MAPQ 60: its last four bases are the only ones at or past the primer
        # end and within 20 of the barcode end at primerDist 0 - qualities 40, 41, 62, 63)
        add("clip", a0 + 14, "2H4S16M", flag, rev, nm=0, subs=False, mapq=60, qoff=7)
        add("clip", a0 + 15, "3H4S38M", flag, rev, nm=0, subs=False, mapq=60, qoff=3)      # (its last four bases: 40, 41, 62, 63)
        add("insertion behind a tile's last locus", a0 + TILE - 24, "24M2I20M", flag, rev)
        add("deletion across a tile boundary", a0 + 2 * TILE - 28, "26M5D20M", flag, rev)
        for n in (1, 19, 20, 21):
            for op in "ID":
                add("indel near the start", a0 + 2 * TILE + 4 + n % 5, "%dM1%s40M" % (n, op), flag, rev)
                add("indel near the end", a0 + 2 * TILE - 50 + n % 5, "40M1%s%dM" % (op, n), flag, rev)
        add("D next to I", a0 + 30, "20M2D1I20M", flag, rev)
        add("I next to D", a0 + 32, "20M1I2D20M", flag, rev)
        add("skip of 50", a0 + 8, "20M50N20M", flag, rev)
        add("long skip", RUN_A[1] - 15, "12M%dN25M" % (RUN_B[0] + 7 - (RUN_A[1] - 3)), flag, rev)
        add("NM below the indel count", a0 + 90, "20M2D20M", flag, rev, nm=1)
        add("a deletion on a read over the threshold", a0 + 92, "20M3D20M", flag, rev, nm=7, mapq=60)   # 100 * (7 - 3) / 40 = 10.0
        add("mismatches on the threshold", a0 + 100, "5S40M5S", flag, rev, nm=3)         # 100 * 3 / 50 = 6.0
        add("mismatches over the threshold", a0 + 101, "5S40M5S", flag, rev, nm=4)
        # (every quality at every distance from either end, on reads every set includes that includes anything)
        for q in range(9):
            add("plain 100, quality phase", a0 + 40 + q % 3, "100M", flag, rev, nm=0, mapq=255, qoff=q)
    for flag, rev in (COMBOS[0], COMBOS[3]):
        add("69 operations", a0 + 5, "3M1I3M1D" * 17 + "5M", flag, rev)
    # ---- flagged neither READ1 nor READ2, in the shallow run only (the listed builder declines a run that has one): behind a read 2 and
    # behind a read 1, never first in a pileup (a long read 1 before the run covers all of it)
    b0 = RUN_B[0]
    add("cover of the shallow run", b0 - 6, "50M", 0x40, False)
    add("before unflagged", b0 + 2, "30M", 0x80, True)
    add("unflagged", b0 + 3, "30M", 0, False)
    add("unflagged", b0 + 4, "4S26M", 0, True)
    add("before unflagged", b0 + 8, "30M", 0x40, False)
    add("unflagged", b0 + 9, "20M1I10M", 0, True)
    recs.sort(key=lambda r: r["pos"])                                # (stable: the file's order among equal positions is the order above)
    return recs


def loci():
    return [(CHROM, str(p + 1)) for lo, hi in RUNS for p in range(lo, hi)]


def run_of(pos0):
    for lo, hi in RUNS:
        if lo <= pos0 < hi:
            return lo, hi
    raise KeyError(pos0)


# ---- which of the 22 read classes (include/smcounter_hip.h) a parameter set can reach on these records
def unreachable_classes(t):
    """The classes no read of these records can have under the set - by the set's numbers alone:
      minBQ above every quality (64): no base is included and none has "quality fine" - only a read inside a deletion, whose quality IS
        minBQ (smCounter.py:418), is included: classes 3, 5 (an included indel start) and every regular class but "low quality" go;
      minBQ 0: no quality is low - "not included, low quality" (sub 1) goes;
      minMQ 0 and mismatchThr 100 (no record has that many mismatches): only a low quality excludes a read - "inside a deletion,
        not included" (class 0) and "not included, quality fine" (sub 0) go, and with minBQ 0 the not-included indel starts (2, 4) too;
      primerDist beyond the longest read (200, 100000): every read-2 base is within it - the read-2 classes without that bit go."""
    pd, bq, mq, thr = t
    gone = set()
    base = lambda rev, sub: 6 + 8 * rev + sub
    if bq > max(QUALS):
        gone |= {3, 5} | {base(r, s) for r in (0, 1) for s in (0, 2, 3, 4, 5, 6, 7)}
    if bq <= min(QUALS):
        gone |= {base(r, 1) for r in (0, 1)}
    if mq <= min(MAPQS) and thr >= 100.0:
        gone |= {0} | {base(r, 0) for r in (0, 1)}
        if bq <= min(QUALS):
            gone |= {2, 4}
    if pd >= 152:
        gone |= {base(r, s) for r in (0, 1) for s in (4, 5)}
    return sorted(gone)


def load_fixture(name, tmp_path):
    """-> (BAM path, FastaFile, loci, meta); meta["sets"][i] = dict(params=the four numbers, capture=index into meta["captures"],
    unreachable=[classes]), meta["captures"][c][l] the reference's tallies at locus l."""
    from smcounter_amd import fasta
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(bytes(z["meta"]).decode())
    bam, fa_path = str(tmp_path / (name + ".bam")), str(tmp_path / (name + ".fa"))
    open(bam, "wb").write(bytes(z["bam"]))
    open(bam + ".bai", "wb").write(bytes(z["bai"]))
    open(fa_path, "wb").write(bytes(z["fasta"]))
    return bam, fasta.FastaFile(fa_path), [tuple(x) for x in meta["loci"]], meta


def fixture_sets(name):
    """(parameter tuple, ...) of a stored fixture, for parametrising tests without unpacking the BAM."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return [tuple(s["params"]) for s in json.loads(bytes(z["meta"]).decode())["sets"]]


# ---- a built batch against the reference
def compare_locus(where, pile, t, words, table, umi_start, meta=None, dist=None):
    """The tallies of one locus's read words (and the distance lists of its `dist` plane) against the reference's: -> list of texts,
    one per difference (empty: equal).  Every word is also checked for the words-only contract: allele id < 16, quality <= 63."""
    import geometry_tallies as gt
    bad = []
    w = np.asarray(words, np.uint32)
    if len(w) and (int((w & 0xFF).max()) > 15 or int(((w >> 8) & 0xFF).max()) > max(63, t[1])):
        bad.append("%s: an allele id beyond 15 or a quality beyond 63" % where)
    got, got_l = gt.locus_tallies(w, table, umi_start, meta)
    want, want_l = gt.reference_tallies(pile, t[0], meta is not None)
    if got_l != want_l:
        bad.append("%s: cvg / allFrag / allMT %r, the reference has %r" % (where, got_l, want_l))
    if set(got) != set(want):
        bad.append("%s: allele keys %r, the reference has %r" % (where, sorted(got), sorted(want)))
    for key in sorted(set(got) & set(want)):
        for f, v in want[key].items():
            if got[key][f] != v:
                bad.append("%s allele %s: %s %d, the reference has %d" % (where, key, f, got[key][f], v))
    if dist is not None:
        gd, wd = gt.distance_lists(w, dist, table), gt.reference_distance_lists(pile)
        if gd != wd:
            key = sorted(k for k in set(gd) | set(wd) if gd.get(k) != wd.get(k))[0]
            for name in ("r1BcEndPos", "r2BcEndPos", "r2PrimerEndPos"):
                g, w_ = gd.get(key, {}).get(name, []), wd.get(key, {}).get(name, [])
                if g != w_:                                          # (the values one list has more of than the other)
                    more = lambda a, b: sorted(x for x in set(a) if a.count(x) > b.count(x))
                    bad.append("%s allele %s: %s has %d distances, the reference %d; too many of %r, too few of %r" % (
                        where, key, name, len(g), len(w_), more(g, w_)[:6], more(w_, g)[:6]))
    return bad


def compare_batch(what, meta, s, first, loci_desc, words, umi_start, tables, meta_plane=None, dist_plane=None):
    """Every locus of a built batch (`first`: its first locus's index among the fixture's loci; descriptors, read words (32-bit),
    umi_start, allele tables; optionally the raw meta and dist planes) against set s's reference tallies."""
    cap = meta["captures"][meta["sets"][s]["capture"]]
    t = tuple(meta["sets"][s]["params"])
    bad = []
    for l in range(len(loci_desc)):
        o, n = 4 * int(loci_desc["read_off4"][l]), int(loci_desc["n_reads"][l])
        uo, nu = int(loci_desc["umi_off"][l]), int(loci_desc["n_umi"][l])
        us = np.asarray(umi_start[uo:uo + nu + 1])
        assert n == 0 or (int(us[0]) & 0x7FFFFFFF) == 0 and (int(us[-1]) & 0x7FFFFFFF) == n
        where = "%s, set %s, locus %s:%s" % (what, set_id(t), meta["loci"][first + l][0], meta["loci"][first + l][1])
        bad += compare_locus(where, cap[first + l], t, words[o:o + n], tables[l], us,
                             None if meta_plane is None else meta_plane[o:o + n], None if dist_plane is None else dist_plane[o:o + n])
        if int(loci_desc["n_frag"][l]) != cap[first + l]["allFrag"]:
            bad.append("%s: n_frag %d, the reference's allFrag %d" % (where, int(loci_desc["n_frag"][l]), cap[first + l]["allFrag"]))
    return bad


def classes_seen(words):
    w = np.asarray(words, np.uint32)
    return set(np.unique(w[w != 0] >> np.uint32(27)).tolist())


def assert_equal(bad):
    assert not bad, "%d differences from the reference; first:\n%s" % (len(bad), "\n".join(bad[:8]))
