"""Host restatement of --spikeAF (DESIGN.md "--spikeAF") from HOST-BUILT pileups: per read of a listed position its barcode, its
allele key, its query position, its NM and its CIGAR's indel length, as bamio's readable decoder and pileup.PileupBatch give them,
with a numpy Philox - not through tools/spike_variants.py's own walking, drawing or counting.  Yields per record the rewritten
letters, NM' and the mismatch bit, and per variant the statistics.  Shared by tests/test_spike.py and tests/test_gpu_spike.py; also
the hand-made BAM whose reads hold every case of the rewrite rule by construction."""
import math
import os
import sys

import numpy as np

from smcounter_amd import bamio
from smcounter_amd.params import VcParams

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ds_af_restate as R  # noqa: E402
import ds_rpb_philox_restate as rp  # noqa: E402

SPIKE_DOMAIN = 0x73704146
V = R.V


def draw(texts, seed, pos1):
    """u_v(b) of every barcode text for the variant at 1-based pos1."""
    x = rp.fnv64(list(texts))
    return rp.philox4x32_10(x & np.uint64(0xFFFFFFFF), x >> np.uint64(32), SPIKE_DOMAIN, pos1 & 0xFFFFFFFF, seed & 0xFFFFFFFF,
                            (seed >> 32) & 0xFFFFFFFF)[0]


def rec_key(a):
    return (a.qname, a.flag, a.pos)


def restate(bam_path, fa_path, variants, t, seed, mismatch_thr):
    """-> (records: rec_key -> dict(edits {qpos: letter}, nm (the new one), inc, mmok, old {qpos: letter}, notes set()) for every
    record in the pileup of a listed position, stats: per variant dict(N, V0, S, READS, V1, NMINC, spiked: set of barcode texts))."""
    thr = int(math.floor(t * 4294967296.0))
    pb = R.pileups(bam_path, fa_path, [(v.chrom, v.pos) for v in variants])
    bam = bamio.BamFile(bam_path)
    records, stats = {}, []
    try:
        for l, v in enumerate(variants):
            recs = bam.fetch(v.chrom, v.pos - 1, v.pos)
            sl = pb.locus_slice(l)
            assert len(recs) == sl.stop - sl.start, "the pileup of %s:%d is not the records that span it" % (v.chrom, v.pos)
            names = pb.umi_names[l]
            u = dict(zip(names, (int(x) for x in draw(names, seed, v.pos)))) if names else {}
            reads, alt0, alt1 = ({n: 0 for n in names} for _ in range(3))
            n_rw = n_inc = 0
            for k, a in enumerate(recs):
                i = sl.start + k
                bc, key, qpos = names[int(pb.umi[i])], pb.alleles[l][int(pb.allele[i])], int(pb.qpos[i])
                assert int(pb.nm[i]) == a.nm and int(pb.qlen[i]) == a.l_seq
                r = records.setdefault(rec_key(a), dict(edits={}, old={}, nm=int(pb.nm[i]), inc=0, n_indel=int(pb.n_indel[i]),
                                                        l_seq=int(pb.qlen[i]), has_nm=a.has_nm, notes=set()))
                hit = u[bc] < thr
                single = len(key) == 1
                reads[bc] += 1
                alt0[bc] += key == v.alt
                alt1[bc] += single if hit else key == v.alt
                # (what the record shows there, for the tests' list of cases)
                if not single:
                    r["notes"].add("in_deletion" if key == "DEL" else "ins_behind" if key.startswith("INS") else "del_behind")
                else:
                    first = a.cigar[0][1] if a.cigar[0][0] == 4 else 0
                    if qpos == first:
                        r["notes"].add("first_base")
                        if first:
                            r["notes"].add("after_soft_clip")
                    if v.pos == a.end:
                        r["notes"].add("last_base")
                if hit and single:
                    r["edits"][qpos], r["old"][qpos] = v.alt, key
                    n_rw += 1
                    r["notes"].add("already_alt" if key == v.alt else "ref_letter" if key == v.ref else "third_letter")
                    if key == v.ref:
                        r["inc"] += 1
                        n_inc += 1
            stats.append(dict(N=len(names), V0=sum(2 * alt0[b] > reads[b] for b in names), S=sum(u[b] < thr for b in names), READS=n_rw,
                              NMINC=n_inc, V1=sum(2 * alt1[b] > reads[b] for b in names), spiked={b for b in names if u[b] < thr}))
    finally:
        bam.close()
    for r in records.values():
        mm = lambda nm: (100.0 * max(0, nm - r["n_indel"]) / r["l_seq"] if r["l_seq"] else 0.0) <= mismatch_thr
        r["mmok0"] = mm(r["nm"])
        r["nm"] += r["inc"]
        r["mmok"] = mm(r["nm"])
        if r["inc"] >= 2:
            r["notes"].add("two_positions")
        if r["inc"] and not r["has_nm"]:
            r["notes"].add("no_nm_tag")
        if r["mmok0"] and not r["mmok"]:
            r["notes"].add("flips_inccond")
    return records, stats


def expected_records(bam_path, records):
    """Every record of the input file as the spiked file must hold it: [(qname, flag, pos, cigar, seq, qual, nm, has_nm)]."""
    bam = bamio.BamFile(bam_path)
    bam._bg.seek(bam._first_record)
    out = []
    for a in bam._records():
        seq, nm, has_nm = a.seq, a.nm, a.has_nm
        r = records.get(rec_key(a)) if a.tid >= 0 and not (a.flag & 4) and a.cigar else None
        if r is not None and r["edits"]:
            s = list(seq)
            for q, letter in r["edits"].items():
                assert s[q] == r["old"][q]
                s[q] = letter
            seq = "".join(s)
            if r["inc"]:
                nm, has_nm = r["nm"], True
        out.append((a.qname, a.flag, a.pos, tuple(a.cigar), seq, bytes(a.qual), nm, has_nm))
    bam.close()
    return out


def file_records(bam_path):
    bam = bamio.BamFile(bam_path)
    bam._bg.seek(bam._first_record)
    out = [(a.qname, a.flag, a.pos, tuple(a.cigar), a.seq, bytes(a.qual), a.nm, a.has_nm) for a in bam._records()]
    bam.close()
    return out


# ---- the hand-made BAM: every case of the rewrite rule by construction
M, I, D, S = 0, 1, 2, 4
CASE_CHROM, P1, P2, P3 = "chrS", 101, 110, 130          # 1-based listed positions
N_BC = 14                                               # barcodes per read shape
CASES = ("first_base", "last_base", "in_deletion", "ins_behind", "del_behind", "after_soft_clip", "two_positions", "already_alt",
         "third_letter", "no_nm_tag", "flips_inccond")


def make_case(tmp):
    """-> (bam, fasta path, loci, VcParams, variants).  Ten read shapes around P1 (0-based 100), each for N_BC barcodes of two reads;
    30-base reads, so that at mismatchThr 6.0 a second mismatch flips incCond (100 x 2 / 30 > 6 >= 100 x 1 / 30)."""
    rng = np.random.Generator(np.random.PCG64(11))
    ref = "".join(rng.choice(list("ACGT"), size=400))
    other = lambda c, k=1: "ACGT"[("ACGT".index(c) + k) % 4]
    variants = [V(CASE_CHROM, p, ref[p - 1], other(ref[p - 1]), other(ref[p - 1])) for p in (P1, P2, P3)]
    fa = os.path.join(tmp, "spike.fa")
    with open(fa, "w") as fh:
        fh.write(">%s\n" % CASE_CHROM)
        for i in range(0, len(ref), 60):
            fh.write(ref[i:i + 60] + "\n")
    p = P1 - 1
    shapes = [                                      # (name, pos0, cigar, letter forced at P1's base (None: the reference's), nm)
        ("first", p, [(M, 30)], None, 0),                        # P1 the first aligned base; spans P2 too: NM + 2
        ("last", p - 29, [(M, 30)], None, 0),                    # P1 the last aligned base
        ("indel", p - 10, [(M, 8), (D, 5), (M, 22)], None, 5),   # P1 inside the deletion (P2 a plain base)
        ("insb", p - 5, [(M, 6), (I, 2), (M, 22)], None, 2),     # an insertion starts behind P1's base
        ("delb", p - 5, [(M, 6), (D, 3), (M, 24)], None, 3),     # a deletion starts behind P1's base
        ("clip", p, [(S, 5), (M, 25)], None, 0),                 # P1 the first base behind a leading soft clip
        ("alt", p - 12, [(M, 30)], "alt", 1),                    # shows ALT already
        ("third", p - 14, [(M, 30)], "third", 1),                # shows a third letter
        ("nonm", p - 16, [(M, 30)], None, None),                 # no NM tag
        ("flip", p - 18, [(M, 30)], None, 1),                    # one mismatch elsewhere: the increment flips incCond
        ("far", P3 - 1 - 15, [(M, 30)], None, 0),                # P3 alone
    ]
    recs = []
    for name, pos, cigar, force, nm in shapes:
        for b in range(N_BC):
            for mate in (0, 1):
                seq, x = [], pos
                for op, l in cigar:
                    if op == M:
                        seq.append(ref[x:x + l]); x += l
                    elif op == D:
                        x += l
                    else:
                        seq.append("".join(rng.choice(list("ACGT"), size=l)))
                seq = list("".join(seq))
                if force is not None:
                    seq[p - pos] = variants[0].alt if force == "alt" else other(ref[p], 2)
                if name == "flip":
                    seq[2] = other(seq[2])                       # (the mismatch its NM of 1 stands for)
                qual = rng.choice([25, 30, 37, 40], size=len(seq)).astype(np.uint8)
                recs.append(dict(tid=0, pos=pos, qname="m%s%d_%d:tag:%s%02d:x" % (name, b, mate, name.upper(), b),
                                 flag=(0x40 if mate == 0 else 0x80) | 0x1, mapq=60, cigar=cigar, seq="".join(seq), qual=qual.tolist(), nm=nm))
    recs.sort(key=lambda r: r["pos"])
    bam = os.path.join(tmp, "spike.bam")
    bamio.write_bam(bam, [(CASE_CHROM, len(ref))], recs, block=8000)
    bamio.write_bai(bam)
    loci = [(CASE_CHROM, q) for q in range(P1 - 4, P3 + 3)]
    return bam, fa, loci, VcParams(mtDepth=N_BC * len(shapes), rpb=2.0, hpLen=8), variants


def pick_positions(bam_path, fa_path, loci, n=3):
    """Listed SNVs for a fixture: the `n` loci with the deepest pileups that have a reference letter out of ACGT, each with the ALT
    that follows REF in ACGT -> variants sorted by position."""
    pb = R.pileups(bam_path, fa_path, loci)
    depth = np.diff(pb.read_off)
    out = []
    for l in np.argsort(-depth, kind="stable").tolist():
        if pb.ref[l] in "ACGT" and depth[l] > 0:
            alt = "ACGT"[("ACGT".index(pb.ref[l]) + 1) % 4]
            out.append(V(loci[l][0], loci[l][1], pb.ref[l], alt, alt))
        if len(out) == n:
            break
    return sorted(out, key=lambda v: (v.chrom, v.pos))
