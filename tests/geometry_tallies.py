"""What a locus's read words say its reads add to the per-allele tallies of vc()'s pileup loop (smCounter.py:316-479), restated in
plain numpy for tests/test_geometry_ref.py and tests/test_gpu_geometry.py - and the same tallies taken from what the reference
itself held when vc() returned (oracle/ref_harness.py: capture_pileup), so that the two can be compared key by key.

The read word (include/smcounter_hip.h): bits 0-7 allele id, 8-15 base quality (minBQ for a read inside a deletion), bit 16 first
read of its fragment at the locus, bits 27-31 the read class.  The classes, from the table in that header's comment:
    0, 1            inside a deletion ('DEL'); + 1: included
    2 .. 5          insertion / deletion start: 2 + 2 * reverse + included
    6 + 8 * reverse + sub   a regular base, with sub
        0  not included, quality >= minBQ        1  not included, quality < minBQ (lowQReads)
        2  included read 1, distToBcEnd > 20     3  included read 1, distToBcEnd <= 20
        4 + (distToBcEnd <= 20) + 2 * (distToPrimerEnd <= primerDist)   included read 2
A 16-bit word is turned into a 32-bit one by devplanes.words32_from_16 before it gets here.  Nothing here calls smc_read_class."""
import numpy as np

FIELDS = ("alleleCnt", "forwardCnt", "reverseCnt", "lowQReads", "bqSum", "r1Inc", "r1Le20", "r2Inc", "r2Le20", "r2LePrimer")
N_CLASS = 22


def locus_tallies(words, table, umi_start=None, meta=None):
    """words: the locus's read words (uint32, one per read, no padding); table: its allele keys by id; umi_start: its stretch of the
    umi_start array (n_umi + 1 entries) -> (per key {field: count} for the keys with a read, dict(cvg, allFrag, allMT)).
    With `meta` (the raw-field plane of the same reads: bit 16 read 2, bits 19-20 kind) also r1Cnt / r2Cnt, which the reference counts
    for every read that is not inside a deletion, included or not."""
    w = np.asarray(words, np.uint32).astype(np.int64)
    allele, bq, cls = w & 0xFF, (w >> 8) & 0xFF, w >> 27
    assert (cls < N_CLASS).all(), "a read word without a read class"
    assert (allele < len(table)).all(), "an allele id beyond the locus's table"
    gap, start, base = cls < 2, (cls >= 2) & (cls < 6), cls >= 6
    rev = np.where(start, ((cls - 2) >> 1) & 1, np.where(base, (cls - 6) >> 3, 0))
    sub = np.where(base, (cls - 6) & 7, -1)
    r2 = sub >= 4
    cols = dict(alleleCnt=np.ones(len(w), np.int64), forwardCnt=~gap & (rev == 0), reverseCnt=~gap & (rev == 1), lowQReads=sub == 1,
                bqSum=bq, r1Inc=(sub == 2) | (sub == 3), r1Le20=sub == 3, r2Inc=r2, r2Le20=r2 & (((sub - 4) & 1) == 1),
                r2LePrimer=r2 & (((sub - 4) & 2) == 2))
    if meta is not None:
        m = np.asarray(meta, np.uint32).astype(np.int64)
        assert ((m & 0xFFFF) == (w & 0xFFFF)).all(), "meta and the read words disagree on allele or quality"
        is_r2, kind = (m >> 16) & 1, (m >> 19) & 3
        assert ((kind == 1) == gap).all() and ((kind >= 2) == start).all(), "meta's kind and the read class disagree"
        cols["r1Cnt"] = (kind != 1) & (is_r2 == 0)
        cols["r2Cnt"] = (kind != 1) & (is_r2 == 1)
    out = {}
    for a in np.unique(allele).tolist():
        sel = allele == a
        out[table[a]] = {f: int(np.asarray(c)[sel].sum()) for f, c in cols.items()}
    locus = dict(cvg=len(w), allFrag=int(((w >> 16) & 1).sum()))
    if umi_start is not None:
        locus["allMT"] = len(umi_start) - 1
    return out, locus


def distance_lists(words, dist, table):
    """The sorted end distances of the included regular reads, per allele key: dist = distToBcEnd | distToPrimerEnd << 16 (the raw
    `dist` plane) -> {key: dict(r1BcEndPos, r2BcEndPos, r2PrimerEndPos)} for the keys that have one."""
    w = np.asarray(words, np.uint32).astype(np.int64)
    d = np.asarray(dist, np.uint32).astype(np.int64)
    allele, cls = w & 0xFF, w >> 27
    sub = np.where(cls >= 6, (cls - 6) & 7, -1)
    r1, r2 = (sub == 2) | (sub == 3), sub >= 4
    out = {}
    for a in np.unique(allele[r1 | r2]).tolist():
        s1, s2 = r1 & (allele == a), r2 & (allele == a)
        out[table[a]] = dict(r1BcEndPos=sorted((d[s1] & 0xFFFF).tolist()), r2BcEndPos=sorted((d[s2] & 0xFFFF).tolist()),
                             r2PrimerEndPos=sorted((d[s2] >> 16).tolist()))
    return out


# ---- the same from the reference's own dictionaries
def reference_tallies(pile, primer_dist, with_pairs):
    """`pile`: a locus's entry of the fixture (make_geometry_golden.compact: the reference's dictionaries with the keys no read
    added to taken out and the distance lists sorted) -> locus_tallies' two answers as the reference has them."""
    out = {}
    for key, n in pile["alleleCnt"].items():
        r1, r2bc, r2pr = (pile[name].get(key, []) for name in ("r1BcEndPos", "r2BcEndPos", "r2PrimerEndPos"))
        assert len(r2bc) == len(r2pr)
        t = dict(alleleCnt=n, forwardCnt=pile["forwardCnt"].get(key, 0), reverseCnt=pile["reverseCnt"].get(key, 0),
                 lowQReads=pile["lowQReads"].get(key, 0), bqSum=pile["bqSum"].get(key, 0), r1Inc=len(r1), r1Le20=sum(x <= 20 for x in r1),
                 r2Inc=len(r2bc), r2Le20=sum(x <= 20 for x in r2bc), r2LePrimer=sum(x <= primer_dist for x in r2pr))
        if with_pairs:
            t.update(r1Cnt=pile["r1Cnt"].get(key, 0), r2Cnt=pile["r2Cnt"].get(key, 0))
        out[key] = t
    return out, dict(cvg=pile["cvg"], allFrag=pile["allFrag"], allMT=pile["allMT"])


def reference_distance_lists(pile):
    """The reference's lists as the `dist` plane can hold them: its two 16-bit fields are unsigned, a distance below zero (3H4S38M:
    the soft clip counts in query_position but not in leftSP, so the far end lies up to 4 before the read's last base) is stored
    as 0 - on the same side of `<= 20` and of every `<= primerDist`, which is never negative."""
    keys = set(pile["r1BcEndPos"]) | set(pile["r2BcEndPos"])
    return {k: {name: sorted(max(0, x) for x in pile[name].get(k, [])) for name in ("r1BcEndPos", "r2BcEndPos", "r2PrimerEndPos")}
            for k in keys}
