"""Host restatement of --spikeIndels (DESIGN.md "--spikeIndels") over a file's records as bamio's readable decoder gives them: every
record is laid out base by base (one unit per aligned base, one block per other CIGAR operation), the listed variants are resolved on
that layout and marked in it, and CIGAR, SEQ and QUAL are read back from the marked layout - not through tools/spike_variants.py's
operation arithmetic nor the kernel's walk.  Draws by the numpy Philox of tests/ds_rpb_philox_restate.py.  Also the arrays a spiked
copy of a run must hold (expected_run), and the hand-made BAM whose reads hold every case of the rule by construction.  Shared by
tests/test_spike_indels.py and tests/test_gpu_spike_indels.py."""
import math
import os
import sys

import numpy as np

from smcounter_amd import bamio
from smcounter_amd.params import VcParams
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ds_rpb_philox_restate as rp  # noqa: E402
import spike_restate as SR  # noqa: E402

MLIKE = (0, 7, 8)
MAX16 = 65535
MMOK = 16
rec_key = SR.rec_key


def variant(chrom, pos, ref, alt):
    key, kind = af.allele_key(ref, alt)
    return af.Variant(chrom, pos, ref, alt, key, kind)


def length(v):
    return 0 if v.kind == af.SNV else len(v.alt) - 1 if v.kind == af.INS else len(v.ref) - 1


def footprint(v):
    """1-based closed interval."""
    return v.pos, v.pos + (0 if v.kind == af.SNV else 1 if v.kind == af.INS else length(v) + 1)


def layout(a):
    """-> (units, at): units in CIGAR order - dict(op, ci, x (0-based reference position or None), q (query position or None), n
    (bases / positions of a block; 1 for an aligned base)); at: reference position -> index of the aligned base's unit."""
    units, at = [], {}
    x, q = a.pos, 0
    for ci, (op, l) in enumerate(a.cigar):
        if op in MLIKE:
            for j in range(l):
                at.setdefault(x + j, len(units))
                units.append(dict(op=op, ci=ci, x=x + j, q=q + j, n=1))
            x += l
            q += l
        else:
            units.append(dict(op=op, ci=ci, x=x if op in (2, 3) else None, q=q if op in (1, 4) else None, n=l))
            if op in (2, 3):
                x += l
            elif op in (1, 4):
                q += l
    return units, at


def resolve(a, units, at, v):
    """-> the index of the unit variant `v` is written at when the record is eligible there (before the 16-bit limits), else None."""
    u = at.get(v.pos - 1)
    if u is None or units[u]["q"] >= a.l_seq:
        return None
    if v.kind == af.SNV:
        # a base with no insertion or deletion starting behind it
        last = u + 1 == len(units) or units[u + 1]["ci"] != units[u]["ci"]
        nxt = a.cigar[units[u]["ci"] + 1] if last and units[u]["ci"] + 1 < len(a.cigar) else None
        return None if nxt is not None and nxt[0] in (1, 2) and nxt[1] > 0 else u
    for p in range(v.pos - 1, footprint(v)[1]):
        w = at.get(p)
        if w is None or units[w]["ci"] != units[u]["ci"] or units[w]["q"] >= a.l_seq:
            return None
    return u


def rewrite(a, variants, hits):
    """Record `a` with the variants `hits` (indexes into `variants`, ascending by position) of its barcode ->
    dict(cigar, seq, qual, nm_inc, indel_inc, applied: [variant index], nm_incs: {variant index: increment}, relocated)."""
    units, at = layout(a)
    seq, qual = a.seq, bytes(a.qual)
    n_cig, l_seq = len(a.cigar), a.l_seq
    applied, incs = [], {}
    for k in hits:
        v = variants[k]
        u = resolve(a, units, at, v)
        if u is None:
            continue
        n = length(v)
        if v.kind != af.SNV and (n_cig + 2 > MAX16 or (v.kind == af.INS and l_seq + n > MAX16)):
            continue
        applied.append(k)
        if v.kind == af.SNV:
            incs[k] = int(seq[units[u]["q"]] == v.ref)
            units[u]["letter"] = v.alt
        elif v.kind == af.INS:
            incs[k] = n
            units[u]["ins"] = (k, v.alt[1:])
            n_cig, l_seq = n_cig + 2, l_seq + n
        else:
            incs[k] = n
            for p in range(v.pos, v.pos + n):
                units[at[p]]["gone"] = k
            n_cig, l_seq = n_cig + 2, l_seq - n
    ops, s, ql = [], [], []                      # ops: [group key, op, length]

    def put(key, op, n):
        if ops and ops[-1][0] == key:
            ops[-1][2] += n
        else:
            ops.append([key, op, n])
    seg = 0
    for u in units:
        if u["op"] not in MLIKE:
            put(("block", u["ci"]), u["op"], u["n"])
            if u["q"] is not None:
                s.append(seq[u["q"]:u["q"] + u["n"]])
                ql.append(qual[u["q"]:u["q"] + u["n"]])
            continue
        if "gone" in u:
            put(("del", u["gone"]), 2, 1)
            seg = ("behind", u["gone"])
            continue
        put(("base", u["ci"], seg), u["op"], 1)
        if u["q"] < a.l_seq:
            s.append(u.get("letter", seq[u["q"]]))
            ql.append(qual[u["q"]:u["q"] + 1])
        if "ins" in u:
            k, letters = u["ins"]
            put(("ins", k), 1, len(letters))
            s.append(letters)
            ql.append(qual[u["q"]:u["q"] + 1] * len(letters))
            seg = ("behind", k)
    relocated = any(variants[k].kind != af.SNV for k in applied)
    return dict(cigar=[(op, n) for _, op, n in ops], seq="".join(s), qual=b"".join(ql), nm_inc=sum(incs.values()),
                indel_inc=sum(i for k, i in incs.items() if variants[k].kind != af.SNV), applied=applied, nm_incs=incs, relocated=relocated)


def draws(idents, seed, pos1):
    x = np.asarray(idents, np.uint64)
    return rp.philox4x32_10(x & np.uint64(0xFFFFFFFF), x >> np.uint64(32), SR.SPIKE_DOMAIN, pos1 & 0xFFFFFFFF, seed & 0xFFFFFFFF,
                            (seed >> 32) & 0xFFFFFFFF)[0]


def mmok(nm, n_indel, l_seq, mismatch_thr):
    return (100.0 * max(0, nm - n_indel) / l_seq if l_seq else 0.0) <= mismatch_thr


def restate(bam_path, variants, thr, seed, mismatch_thr, fa=None):
    """`variants` (all on one chromosome) planted in the file's records at threshold `thr` (an integer in [0, 2^32], or one per
    variant) -> (records: rec_key -> dict(rewrite()'s fields, nm, n_indel, l_seq, mmok0, mmok, notes) for every placed record that
    spans a listed position, stats: per variant dict(N, V0, S, READS, NMINC, V1, spiked: set of barcode texts))."""
    order = sorted(range(len(variants)), key=lambda k: variants[k].pos)
    thr = [thr] * len(variants) if isinstance(thr, int) else list(thr)
    bam = bamio.BamFile(bam_path)
    bam._bg.seek(bam._first_record)
    recs = [a for a in bam._records() if a.tid >= 0 and not (a.flag & 4) and a.cigar]
    chrom_of = [name for name, _ in bam.refs]
    bam.close()
    texts = sorted({af.barcode_of(a.qname) for a in recs if af.barcode_of(a.qname) is not None})
    idents = rp.fnv64(texts)
    hit = {k: dict(zip(texts, (draws(idents, seed, variants[k].pos) < np.uint64(thr[k])).tolist())) for k in order}
    genome = None
    if fa is not None:
        from smcounter_amd import fasta
        genome = fasta.FastaFile(fa)
    records = {}
    per = [dict() for _ in variants]                 # barcode -> [reads, shows before, shows after]
    stats = [dict(READS=0, NMINC=0) for _ in variants]
    for a in recs:
        chrom, bc = chrom_of[a.tid], af.barcode_of(a.qname)
        here = [k for k in order if variants[k].chrom == chrom and a.pos < variants[k].pos <= a.end]
        if not here or bc is None:
            continue
        r = rewrite(a, variants, [k for k in here if hit[k][bc]])
        n_indel = sum(l for op, l in a.cigar if op in (1, 2))
        r.update(nm=a.nm + r["nm_inc"], n_indel=n_indel + r["indel_inc"], l_seq=len(r["seq"]) if a.l_seq else 0, has_nm=a.has_nm,
                 mmok0=mmok(a.nm, n_indel, a.l_seq, mismatch_thr), notes=set())
        r["mmok"] = mmok(r["nm"], r["n_indel"], r["l_seq"], mismatch_thr)
        records[rec_key(a)] = r
        units, at = layout(a)
        for k in here:
            v = variants[k]
            shows = af.read_key(a, v.pos, chrom, genome) == af.variant_key(v, genome)
            c = per[k].setdefault(bc, [0, 0, 0])
            c[0] += 1
            c[1] += shows
            if k in r["applied"] and v.kind != af.SNV:
                # (a rewritten read shows the variant's key when its anchor holds the listed letter; another letter there makes another key)
                c[2] += a.seq[units[at[v.pos - 1]]["q"]] == v.ref[0]
            else:
                c[2] += (k in r["applied"]) or shows
            if k in r["applied"]:
                stats[k]["READS"] += 1
                stats[k]["NMINC"] += r["nm_incs"][k] > 0
            if v.kind == af.SNV or not hit[k][bc]:
                continue
            # (what the record shows there, for the tests' list of cases)
            u, lo, hi = at.get(v.pos - 1), v.pos - 1, footprint(v)[1] - 1
            note = r["notes"].add
            if k in r["applied"]:
                if hi == a.end - 1:
                    note("eligible_by_one_at_the_end")
                first = a.cigar[0][1] if a.cigar[0][0] == 4 else 0
                if units[u]["q"] == first:
                    note("anchor_is_first_base")
                    if first:
                        note("behind_soft_clip")
                if units[u]["op"] in (7, 8):
                    note("splits_eq_or_x")
            else:
                if hi == a.end:
                    note("ineligible_by_one_at_the_end")
                if lo < a.end <= hi:
                    note("ends_in_footprint")
                if u is None:
                    note("anchor_in_deletion")
                elif any(p in at and units[at[p]]["ci"] != units[u]["ci"] for p in range(lo + 1, hi + 1)):
                    nxt = a.cigar[units[u]["ci"] + 1][0]
                    note("own_insertion_behind" if nxt == 1 else "own_deletion_behind" if nxt == 2 else "across_operations")
                if shows:
                    note("shows_it_already")
        kinds = [variants[k].kind for k in r["applied"]]
        if af.SNV in kinds and af.INS in kinds:
            r["notes"].add("snv_and_insertion")
        if af.INS in kinds and af.DEL in kinds:
            r["notes"].add("insertion_and_deletion")
        if r["relocated"] and not a.has_nm:
            r["notes"].add("no_nm_tag")
        if r["relocated"] and r["mmok0"] and not r["mmok"] and r["nm"] - r["n_indel"] == a.nm - n_indel:
            r["notes"].add("flips_mmok_by_length")
    for k, v in enumerate(variants):
        p = per[k]
        stats[k].update(N=len(p), V0=sum(2 * c[1] > c[0] for c in p.values()), S=sum(hit[k][b] for b in p),
                        V1=sum(2 * c[2] > c[0] for c in p.values()), spiked={b for b in p if hit[k][b]})
    return records, stats


def expected_records(bam_path, records):
    """Every record of the input file as the spiked file must hold it: [(qname, flag, pos, cigar, seq, qual, nm, has_nm)]."""
    bam = bamio.BamFile(bam_path)
    bam._bg.seek(bam._first_record)
    out = []
    for a in bam._records():
        cigar, seq, qual, nm, has_nm = tuple(a.cigar), a.seq, bytes(a.qual), a.nm, a.has_nm
        r = records.get(rec_key(a)) if a.tid >= 0 and not (a.flag & 4) and a.cigar else None
        if r is not None and r["applied"]:
            cigar, seq, qual = tuple(r["cigar"]), r["seq"], r["qual"]
            if r["nm_inc"]:
                nm, has_nm = r["nm"], True
        out.append((a.qname, a.flag, a.pos, cigar, seq, qual, nm, has_nm))
    bam.close()
    return out


def expected_run(A, recs, records, nm, n_indel):
    """The copy smc_spike_indels must write of run `A` (its host arrays; `recs`: the readable decoder's records of the run, in its
    order; nm / n_indel: the decoder's per alignment) -> dict(aln, bq, cig, nm, n_indel, totals (pairs, words), relocated: indexes)."""
    aln, nm, n_indel = A["aln"].copy(), np.array(nm[:len(A["aln"])], np.int32), np.array(n_indel[:len(A["aln"])], np.int32)
    bq, cig = [A["bq"].copy()], [A["cig"].copy()]
    n_pairs, n_cw = len(A["bq"]) // 2, len(A["cig"])
    assert len(recs) == len(aln) and [a.pos for a in recs] == aln["pos"].tolist()
    relocated = []
    for i, a in enumerate(recs):
        r = records.get(rec_key(a))
        if r is None:
            continue
        nm[i], n_indel[i] = r["nm"], r["n_indel"]
        aln["oflag"][i] = (int(aln["oflag"][i]) & (0xFF ^ MMOK)) | (MMOK if r["mmok"] else 0)
        if not r["relocated"]:
            for k, (old, new) in enumerate(zip(a.seq, r["seq"])):
                if old != new:
                    bq[0][2 * (int(aln["seq_off"][i]) + k)] = ord(new)
            continue
        relocated.append(i)
        pairs = np.empty(2 * len(r["seq"]), np.uint8)
        pairs[0::2], pairs[1::2] = np.frombuffer(r["seq"].encode(), np.uint8), np.frombuffer(r["qual"], np.uint8)
        aln["seq_off"][i], aln["cig_off"][i] = n_pairs, n_cw
        aln["qalen"][i] = int(aln["qalen"][i]) + len(r["seq"]) - int(aln["l_seq"][i])
        aln["l_seq"][i], aln["n_cig"][i] = len(r["seq"]), len(r["cigar"])
        bq.append(pairs)
        cig.append(np.array([(l << 4) | op for op, l in r["cigar"]], np.uint32))
        n_pairs, n_cw = n_pairs + len(r["seq"]), n_cw + len(r["cigar"])
    return dict(aln=aln, bq=np.concatenate(bq), cig=np.concatenate(cig), nm=nm, n_indel=n_indel, totals=(n_pairs, n_cw), relocated=relocated)


def file_records(bam_path):
    bam = bamio.BamFile(bam_path)
    bam._bg.seek(bam._first_record)
    out = [(a.qname, a.flag, a.pos, tuple(a.cigar), a.seq, bytes(a.qual), a.nm, a.has_nm) for a in bam._records()]
    bam.close()
    return out


# ---- the hand-made BAM: every case of the rule by construction
M, I, D, S, EQ = 0, 1, 2, 4, 7
CASE_CHROM = "chrI"
P_INS, P_SNV, P_DEL, P_FLIP = 101, 105, 110, 150          # 1-based listed positions
INS_LETTERS, DEL_LEN, FLIP_LEN = "GAT", 3, 14
N_BC = 4                                                  # barcodes (of one read) per read shape
CASES = ("ineligible_by_one_at_the_end", "eligible_by_one_at_the_end", "anchor_is_first_base", "across_operations", "anchor_in_deletion",
         "own_insertion_behind", "behind_soft_clip", "snv_and_insertion", "insertion_and_deletion", "no_nm_tag", "flips_mmok_by_length",
         "shows_it_already", "ends_in_footprint", "splits_eq_or_x")


def make_case(tmp):
    """-> (bam, fasta path, loci, VcParams, variants).  Read shapes of 30 bases around the listed insertion (anchor 0-based 100), SNV,
    deletion of 3 and deletion of 14, N_BC barcodes of one read each.  At mismatchThr 6.0 a read with one mismatch passes at 30 bases
    (3.3 per 100) and fails at the 16 the long deletion leaves (6.25)."""
    rng = np.random.Generator(np.random.PCG64(23))
    ref = "".join(rng.choice(list("ACGT"), size=400))
    other = lambda c, k=1: "ACGT"[("ACGT".index(c) + k) % 4]
    variants = [variant(CASE_CHROM, P_INS, ref[P_INS - 1], ref[P_INS - 1] + INS_LETTERS),
                variant(CASE_CHROM, P_SNV, ref[P_SNV - 1], other(ref[P_SNV - 1])),
                variant(CASE_CHROM, P_DEL, ref[P_DEL - 1:P_DEL + DEL_LEN], ref[P_DEL - 1]),
                variant(CASE_CHROM, P_FLIP, ref[P_FLIP - 1:P_FLIP + FLIP_LEN], ref[P_FLIP - 1])]
    fa = os.path.join(tmp, "spike_indel.fa")
    with open(fa, "w") as fh:
        fh.write(">%s\n" % CASE_CHROM)
        for i in range(0, len(ref), 60):
            fh.write(ref[i:i + 60] + "\n")
    p, pd, pf = P_INS - 1, P_DEL - 1, P_FLIP - 1
    shapes = [                                      # (name, pos0, cigar, inserted letters of its own or None, nm)
        ("lastno", p - 29, [(M, 30)], None, 0),                         # the anchor is the last aligned base: one base short
        ("lastok", p - 28, [(M, 30)], None, 0),                         # one aligned base behind the insertion: eligible by one
        ("first", p, [(M, 30)], None, 0),                               # the anchor is the first aligned base; holds the other two too
        ("behind", p + 1, [(M, 30)], None, 0),                          # starts behind the insertion's anchor: not in its pileup
        ("bound", p - 9, [(M, 10), (EQ, 20)], None, 0),                 # the footprint lies across two operations
        ("indel", p - 10, [(M, 8), (D, 5), (M, 22)], None, 5),          # the anchor inside a deletion
        ("ownins", p - 5, [(M, 6), (I, 2), (M, 22)], "CC", 2),          # an insertion of its own behind the anchor
        ("clip", p, [(S, 5), (M, 25)], None, 0),                        # the anchor is the first base behind a soft clip
        ("snvins", p - 20, [(M, 30)], None, 0),                         # insertion and SNV; ends on the deletion's anchor
        ("all", p - 3, [(M, 30)], None, 0),                             # insertion, SNV and deletion
        ("nonm", p - 2, [(M, 30)], None, None),                         # no NM tag
        ("shows", p - 6, [(M, 7), (I, 3), (M, 20)], INS_LETTERS, 3),    # shows the listed insertion already
        ("eq", p - 4, [(EQ, 30)], None, 0),                             # a = operation is split and keeps its type
        ("dlastno", pd + DEL_LEN + 1 - 30, [(M, 30)], None, 0),         # ends on the deletion's last deleted position
        ("dlastok", pd + DEL_LEN + 2 - 30, [(M, 30)], None, 0),         # one aligned base behind the deletion
        ("flip", pf - 5, [(M, 30)], None, 1),                           # one mismatch elsewhere: the shorter l_seq flips the bit
    ]
    recs = []
    for name, pos, cigar, own, nm in shapes:
        for b in range(N_BC):
            seq, x = [], pos
            for op, l in cigar:
                if op in (M, EQ):
                    seq.append(ref[x:x + l]); x += l
                elif op == D:
                    x += l
                elif op == I:
                    seq.append(own)
                else:
                    seq.append("".join(rng.choice(list("ACGT"), size=l)))
            seq = list("".join(seq))
            if name == "flip":
                seq[2] = other(seq[2])                                   # (the mismatch its NM of 1 stands for)
            qual = rng.choice([25, 30, 37, 40], size=len(seq)).astype(np.uint8)
            recs.append(dict(tid=0, pos=pos, qname="r%s%d:tag:%s%02d:x" % (name, b, name.upper(), b), flag=0x41, mapq=60, cigar=cigar,
                             seq="".join(seq), qual=qual.tolist(), nm=nm))
    recs.sort(key=lambda r: r["pos"])
    bam = os.path.join(tmp, "spike_indel.bam")
    bamio.write_bam(bam, [(CASE_CHROM, len(ref))], recs, block=8000)
    bamio.write_bai(bam)
    loci = [(CASE_CHROM, q) for q in range(P_INS - 4, P_FLIP + FLIP_LEN + 4)]
    return bam, fa, loci, VcParams(mtDepth=N_BC * len(shapes), rpb=1.0, hpLen=8), variants


def pick_variants(bam_path, fa_path, loci, n=4, gap=24):
    """Listed variants for a fixture: the `n` deepest loci at least `gap` apart whose reference letters are out of ACGT - in turn an
    insertion of GA, a deletion of 3, an SNV, an insertion of one letter - sorted by position."""
    from smcounter_amd import fasta
    genome = fasta.FastaFile(fa_path)
    pb = SR.R.pileups(bam_path, fa_path, loci)
    depth = np.diff(pb.read_off)
    out = []
    for l in np.argsort(-depth, kind="stable").tolist():
        c, p = loci[l]
        letters = genome.fetch(c, p - 1, p + 4).upper()
        if depth[l] <= 0 or len(letters) < 5 or any(x not in "ACGT" for x in letters) or any(v.chrom == c and abs(v.pos - p) < gap for v in out):
            continue
        kind = len(out) % 4
        nxt = "ACGT"[("ACGT".index(letters[0]) + 1) % 4]
        out.append(variant(c, p, letters[0], letters[0] + "GA") if kind == 0 else variant(c, p, letters[:4], letters[0]) if kind == 1 else
                   variant(c, p, letters[0], nxt) if kind == 2 else variant(c, p, letters[0], letters[0] + nxt))
        if len(out) == n:
            break
    return sorted(out, key=lambda v: (v.chrom, v.pos))
