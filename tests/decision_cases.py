"""Loci built on purpose for the stage between the barcode posteriors and the output row: the ranking of a locus's allele keys by
prediction index, the order exact ties fall back on (the slot order of a Python 2 dict, smCounter.py:534), the choice of ALT and
`biallelic` (:541, :553-555), which candidates go to filterVariants (:549, :563) and its integer and ratio gates (:187-266).

Plain and deterministic, in the manner of fisher_exact_ref.sb_pileup: a locus is a list of barcodes, a barcode a list of fragments, a
fragment one or two reads; barcode u is umi u and its fragment j read id j, the reads in the order written.  One function per family
returns (PileupBatch, fake FASTA, VcParams, labels, designs): `labels[l]` names locus l, `designs[l]` is None or, for a locus of `gates`,
(the FILTER column the reference must print, the number of Fisher tests it must run) - the design the fixture generator
(tests/golden/make_decision_golden.py) holds the reference to.

What makes a designed tie EXACT in the reference's doubles (the generator asserts it, nothing here relies on it silently):
  * a barcode that shows one base pads the other three keys with the same product (smCounter.py:49-54, :88-91): bit-equal by construction;
  * two barcodes of equal shape, one per tied base, give (own + pad) and (pad + own): equal when they are the FIRST two barcodes of the
    pileup (the sums start at 0.0 and one addition commutes); every later barcode adds the same number to both.  "Equal shape" is
    not enough by itself: calProb sums its likelihoods in the key order of a set (:83-93), which differs from base to base, and a
    barcode of two or of four paired fragments of C comes out 2e-13 away from the same barcode of A, T or G.  Barcodes of one and of
    three paired fragments come out bit-equal for every pair of bases: the tied barcodes here have those sizes;
  * a barcode that carries the minority keys (N, DEL, an indel key) shows the tied bases as its first two fragments - one unpaired read
    each -, so their products differ only in the order of the first two factors."""
import numpy as np

from smcounter_amd import pileup
from smcounter_amd.params import VcParams

BASES = "ATGC"
CHROM = "c"
SPACING = 40
FIRST_POS = 60


def rd(a, bq=30, r2=False, rev=None, qpos=50):
    """One read: allele text, quality, READ2?, reverse strand? (default: READ2 reads are), query position (of 100 aligned bases)."""
    return (a, bq, r2, r2 if rev is None else rev, qpos)


def pair(a, bq=30):
    """A fragment of two concordant mates."""
    return [rd(a, bq), rd(a, bq, r2=True)]


def lone(a, bq=30, r2=False, rev=None, qpos=50):
    """A fragment of one read (calProb gives it an error probability of 0.1 whatever its quality, :67-68)."""
    return [rd(a, bq, r2, rev, qpos)]


def bc(a, n=1):
    """A barcode of n paired fragments of one allele: prediction index 2.57 (n = 1), 3.34, 3.82, 4.14, ... 4.80 (n = 8)."""
    return [pair(a) for _ in range(n)]


class Locus(object):
    def __init__(self, label, ref, barcodes, design=None, homopolymer=False):
        self.label, self.ref, self.barcodes, self.design, self.homopolymer = label, ref, barcodes, design, homopolymer


def ins_key(ref, text):
    return "INS|%s|%s%s" % (ref, ref, text)


def del_key(n):
    """Resolved against the FASTA by build(): 'DEL|<ref><the n bases after the locus>|<ref>' (smCounter.py:394-396)."""
    return ("del", n)


def build(loci, params):
    """-> (PileupBatch, {chrom: sequence}, params, labels, designs).  Locus l sits at FIRST_POS + SPACING * l of a chromosome that
    repeats ACGT (no homopolymer, no low-complexity window) except for the locus's own reference base - and, for a locus marked
    `homopolymer`, ten A before it (isHPorLowComp then says homopolymer, :133; the locus's reference base is not A)."""
    n_pos = FIRST_POS + SPACING * (len(loci) + 1)
    seq = ["ACGT"[i % 4] for i in range(n_pos)]
    pos = [FIRST_POS + SPACING * l for l in range(len(loci))]
    for L, p in zip(loci, pos):
        seq[p - 1] = L.ref
        if L.homopolymer:
            assert L.ref != "A"
            seq[p - 11:p - 1] = "A" * 10
    seq = "".join(seq)
    cols = {k: [] for k in ("umi", "frag", "flag", "n_indel", "qpos", "indel", "is_del", "allele", "bq")}
    off, tables = [0], []
    for L, p in zip(loci, pos):
        table = list(pileup.BASE_ALLELES)
        for u, barcode in enumerate(L.barcodes):
            for j, fragment in enumerate(barcode):
                assert 1 <= len(fragment) <= 2
                for (a, bq, r2, rev, qpos) in fragment:
                    if isinstance(a, tuple):
                        a = "DEL|%s%s|%s" % (L.ref, seq[p:p + a[1]], L.ref)
                    if a not in table:
                        table.append(a)
                    n_ind = indel = 0
                    if a.startswith("INS|"):
                        n_ind = indel = len(a.split("|")[2]) - 1
                    elif a.startswith("DEL|"):
                        n_ind = len(a.split("|")[1]) - 1
                        indel = -n_ind
                    elif a == "DEL":
                        n_ind = 1
                    cols["umi"].append(u); cols["frag"].append(j)
                    cols["flag"].append((pileup.F_READ2 if r2 else pileup.F_READ1) | (pileup.F_REVERSE if rev else 0))
                    cols["n_indel"].append(n_ind); cols["qpos"].append(qpos); cols["indel"].append(indel)
                    cols["is_del"].append(a == "DEL"); cols["allele"].append(table.index(a)); cols["bq"].append(bq)
        assert len(table) <= pileup.MAX_ALLELES
        tables.append(table)
        off.append(len(cols["umi"]))
    n, nl = off[-1], len(loci)
    z = lambda dt, v=0: np.full(n, v, dt)
    dt = dict(umi=np.uint32, frag=np.uint32, flag=np.uint8, n_indel=np.uint32, qpos=np.int32, indel=np.int32, is_del=bool,
              allele=np.uint8, bq=np.uint8)
    pb = pileup.PileupBatch(
        chrom=[CHROM] * nl, pos=np.array(pos, np.int64), ref=[L.ref for L in loci], alleles=tables, read_off=np.array(off, np.int64),
        mq=z(np.uint8, 60), nm=z(np.uint32), left_sp=z(np.uint32), qlen=z(np.uint32, 100), qalen=z(np.uint32, 100),
        **{k: np.array(v, dt[k]) for k, v in cols.items()})
    labels = [L.label for L in loci]
    assert len(set(labels)) == nl, "labels must be unique"
    return pb, {CHROM: seq}, params, labels, [L.design for L in loci]


# ---- ties -----------------------------------------------------------------------------------------------------------------------

P_TIES = VcParams(mtDepth=1000, rpb=2.0)


def carrier(first_two, major, others, extras):
    """The barcode that brings the minority keys `extras` into a locus without breaking a tie between the bases `first_two`: one
    unpaired read per allele, the two tied bases first (their products then differ in the order of the first two factors only),
    three reads of the base `major` next - the barcode's consensus, by a wide margin: no barcode here has a maximum that hangs on
    rounding -, the other shown bases and the extras last.  With four or more alleles nothing is padded (smCounter.py:49)."""
    frs = [lone(b) for b in first_two] + [lone(major)] * 3 + [lone(b) for b in others] + [lone(x) for x in extras]
    assert len(set(first_two) | {major} | set(others) | set(extras)) >= 4
    return frs


def tie_loci(prefix, extras=(), extras_first=False):
    """The tie set of one table: for each reference base a clean locus, one and two other bases shown, each pair of other bases tied
    behind the reference and - without the reference's barcodes - for first place, and the reference tied with one other base for
    first.  `extras`: minority keys every locus also carries (the carrier barcode above; last in the pileup, or first)."""
    out = []

    def add(label, ref, tied, barcodes, shown):
        """`tied`: the two bases the carrier must treat alike (the first two of its fragments); `shown`: the bases the locus shows"""
        if extras:
            two = list(tied) if tied else [b for b in BASES if b != ref][:2]
            major = ref if ref not in two else [b for b in BASES if b not in two][0]
            c = carrier(two, major, [b for b in BASES if b not in two and b != major], extras)
            barcodes = [c] + barcodes if extras_first else barcodes + [c]
        out.append(Locus("%s:%s:%s" % (prefix, ref, label), ref, barcodes))

    for ref in BASES:
        oth = [b for b in BASES if b != ref]
        add("clean", ref, None, [bc(ref, 2), bc(ref, 1), bc(ref, 1)], ref)
        for o in oth:                                          # one other base shown: it is second, the two padded bases tie for third
            add("one-%s" % o, ref, [b for b in oth if b != o], [bc(ref, 2), bc(ref, 1), bc(o, 1)], ref + o)
        for o in oth:                                          # two shown, of different weight: all but `o`
            s = [b for b in oth if b != o]
            add("two-%s%s" % (s[0], s[1]), ref, None, [bc(ref, 3), bc(s[0], 2), bc(s[1], 1)], ref + s[0] + s[1])
        for o in oth:                                          # a pair tied for second behind the reference ...
            x, y = [b for b in oth if b != o]
            add("pair-%s%s" % (x, y), ref, (x, y), [bc(x, 1), bc(y, 1), bc(ref, 2), bc(ref, 2), bc(ref, 1)], ref + x + y)
        for o in oth:                                          # ... and for FIRST: ALT, the second candidate and biallelic hang on it
            x, y = [b for b in oth if b != o]
            add("first-%s%s" % (x, y), ref, (x, y), [bc(x, 3), bc(y, 3)], x + y)
        for o in oth:                                          # the reference tied with one other base for first
            add("ref-%s" % o, ref, (ref, o), [bc(ref, 3), bc(o, 3)], ref + o)
    return out


def ties8():
    """At most five keys: the 8-slot order A, C, T, G (N after them).  The second half carries an N read."""
    return build(tie_loci("t8") + tie_loci("t8n", extras=("N",)), P_TIES)


def ties32():
    """Six keys or more through minority N and DEL reads: the 32-slot order A, C, G, N, DEL, T."""
    return build(tie_loci("t32", extras=("N", "DEL")), P_TIES)


N_KEYS_AROUND_GROWTH = (21, 22, 23, 30)


def many_keys_locus(n_keys, ref="C"):
    """A locus of n_keys allele keys - the six fixed ones and insertions after the reference base - whose bases A and T tie for second:
    a Python 2 dict grows to 128 slots with its 22nd key."""
    texts = [a + b for a in "ACGT" for b in ("", "A", "C", "G", "T")] + ["AAA", "CCC", "GGG", "TTT"]
    extras = ["N", "DEL"] + [ins_key(ref, t) for t in texts[:n_keys - 6]]
    assert len(extras) == n_keys - 4
    return Locus("ti:keys%d" % n_keys, ref, [bc("A", 1), bc("T", 1), bc(ref, 2), bc(ref, 2), carrier(["A", "T"], ref, ["G"], extras)])


def ties_indel():
    """The pair ties of both tables with one and with two indel keys, the carrier barcode last in the pileup and first, and loci of 21
    to 30 keys around the growth of the emulated dict to 128 slots."""
    loci = []
    for tag, base in (("8", ()), ("32", ("N", "DEL"))):
        for ref in BASES:
            for n_indel, keys in ((1, [ins_key(ref, "T")]), (2, [ins_key(ref, "GG"), del_key(2)])):
                for first in (False, True):
                    tl = tie_loci("ti%s.%d%s" % (tag, n_indel, "f" if first else "l"), extras=tuple(base) + tuple(keys), extras_first=first)
                    loci += [L for L in tl if L.ref == ref and L.label.split(":")[2].startswith(("pair-", "first-"))]
    loci += [many_keys_locus(n) for n in N_KEYS_AROUND_GROWTH]
    return build(loci, P_TIES)


# ---- gates ----------------------------------------------------------------------------------------------------------------------

# rpb 2.0: a barcode is strong above a prediction index of 3 (smCounter.py:303-308): two paired fragments are (3.34), one is not (2.57)
P_GATES = VcParams(mtDepth=1000, rpb=2.0)
STRONG, WEAK = 2, 1


def _dp_locus(concordant, discordant):
    """ALT T with `concordant` fragments of two T mates and `discordant` fragments of an A mate followed by a T mate (:472-479: the
    second mate's allele is charged, the fragment leaves the barcode), in five barcodes; both strands alike for either allele; 600
    reads of A below minBQ keep T under 60 % of the coverage, so the strand-bias test runs wherever DP does not fire."""
    barcodes = [[] for _ in range(5)]
    for i in range(concordant):
        barcodes[i % 5].append(pair("T"))
    for i in range(discordant):
        sw = bool(i & 1)
        barcodes[i % 5].append([rd("A", rev=sw), rd("T", r2=True, rev=not sw)])
    barcodes += [bc("A", STRONG) for _ in range(3)]
    barcodes.append([lone("A", bq=5, rev=bool(i & 1)) for i in range(600)])
    return barcodes


def gates():
    """Every integer and ratio gate of filterVariants and of the candidate choice from both sides, and exactly on it where the ratio is
    a representable quotient.  design = (FILTER column of the reference, Fisher tests it runs): an SNP that reaches filterVariants runs
    four (three when DP fires or ALT is above 60 % of the coverage), an indel one (none), a candidate that is not filtered none."""
    L = []
    ref3 = [bc("A", STRONG) for _ in range(3)]
    # usedMT < 5 (:187)
    L.append(Locus("g:used_mt-4", "A", [bc("T", STRONG), bc("T", STRONG), bc("A", STRONG), bc("A", STRONG)], (";LM;", 4)))
    L.append(Locus("g:used_mt-5", "A", [bc("T", STRONG), bc("T", STRONG)] + ref3, (";", 4)))
    # strongMTCnt < 2 (:191)
    L.append(Locus("g:vsm-1", "A", [bc("T", STRONG), bc("T", WEAK)] + ref3, (";LSM;", 4)))
    L.append(Locus("g:vsm-2", "A", [bc("T", STRONG), bc("T", STRONG), bc("T", WEAK)] + ref3, (";", 4)))
    # MTCnt / usedMT < 0.99 (:198): seen in a homopolymer only; one-read barcodes (none strong: LSM), ALT above 60 %: three tests
    for vmt, used in ((98, 100), (99, 100), (989, 1000), (990, 1000)):
        hp = 1.0 * vmt / used < 0.99
        L.append(Locus("g:vmf-%d/%d" % (vmt, used), "C", [[lone("T")] for _ in range(vmt)] + [[lone("C")] for _ in range(used - vmt)],
                       (";LSM;HP;" if hp else ";LSM;", 3), homopolymer=True))
    # pairs >= 1000 and discordant / pairs >= 0.5 (:207-209)
    for conc, disc in ((499, 500), (500, 500), (501, 500), (501, 499), (499, 501)):
        fires = conc + disc >= 1000 and 1.0 * disc / (conc + disc) >= 0.5
        L.append(Locus("g:dp-%d+%d" % (conc, disc), "A", _dp_locus(conc, disc), (";DP;", 3) if fires else (";", 4)))
    # af_alt <= 60.0 (:210, :241, :251): ALT on the reverse strand and near the barcode end of READ1, the reference on neither - SB and
    # R1CP fire at 60 % and cannot at 61 %, where the strand-bias test is not even made
    L.append(Locus("g:af-3/5", "A", [[pair("T")], [lone("T")], [pair("A")]], (";LM;LSM;", 4)))
    for n_alt in (60, 61):
        alt = [[lone("T", rev=True, qpos=90) for _ in range(10)] for _ in range(6)]
        if n_alt == 61:
            alt[0].append(lone("T", rev=True, qpos=90))
        refb = [[lone("A") for _ in range(10)] for _ in range(4)]
        if n_alt == 61:
            refb[0].pop()
        L.append(Locus("g:af-%d/100" % n_alt, "A", alt + refb, (";SB;R1CP;", 4) if n_alt == 60 else (";", 3)))
    # lowQReads / alleleCnt > 0.4 (:222-227): an SNP's, never an indel's
    for low in (2, 3):
        for kind, a in (("snp", "T"), ("ins", ins_key("A", "T"))):
            alt = [[lone(a, bq=10 if i < low else 30)] for i in range(5)]
            L.append(Locus("g:bq-%s-%d/5" % (kind, low), "A", alt + ref3,
                           (";LSM;LowQ;" if kind == "snp" and low == 3 else ";LSM;", 4 if kind == "snp" else 1)))
    # altLeEnd / (altLeEnd + altGtEnd) >= 0.98 (:264-265): READ2 on the forward strand, the primer end at the query position; the
    # reference's READ2 are all near the primer end too, so the Fisher half of the test stays silent
    for le in (48, 49, 50):
        alt = [[lone("T", r2=True, rev=False, qpos=1 if 10 * u + i < le else 50) for i in range(10)] for u in range(5)]
        refb = [[lone("A", r2=True, rev=False, qpos=1) for i in range(10)] for u in range(6)]
        L.append(Locus("g:primer-%d/50" % le, "A", alt + refb, (";PrimerCP;" if le >= 49 else ";", 4)))
    L.append(Locus("g:primer-0/0", "A", [[lone("T") for i in range(10)] for u in range(5)] +
                   [[lone("A", r2=True, rev=False, qpos=1) for i in range(10)] for u in range(6)], (";", 4)))
    # bi-allelic: both of the top two are not the reference and hold 45 % of the barcodes each (:553-555); both pass the filters
    L.append(Locus("g:biallelic-9+9", "A", [bc("T", 3) for _ in range(9)] + [bc("G", STRONG) for _ in range(9)] + [bc("A", WEAK)] * 2, (";", 8)))
    L.append(Locus("g:biallelic-9+8", "A", [bc("T", 3) for _ in range(9)] + [bc("G", STRONG) for _ in range(8)] + [bc("A", WEAK)] * 3, (";", 4)))
    L.append(Locus("g:biallelic-8+9", "A", [bc("T", 3) for _ in range(8)] + [bc("G", STRONG) for _ in range(9)] + [bc("A", WEAK)] * 3, (";", 4)))
    L.append(Locus("g:biallelic-ref", "A", [bc("A", 3) for _ in range(9)] + [bc("T", STRONG) for _ in range(9)] + [bc("G", WEAK)] * 2, (";", 4)))
    # the candidate's PI >= 5 (:549), by the number and the size of its barcodes: ONE barcode of paired fragments reaches 4.80 with 8,
    # 4.97 with 10 and 5.03 with 11; two of one fragment 5.13.  Below 5 filterVariants is not called (LM and LSM would show: three
    # barcodes, at most one strong one of T)
    for tag, alt, over in (("1x4", [bc("T", 4)], False), ("1x8", [bc("T", 8)], False), ("1x10", [bc("T", 10)], False),
                           ("1x11", [bc("T", 11)], True), ("1x12", [bc("T", 12)], True), ("2x1", [bc("T", 1), bc("T", 1)], True),
                           ("1x1+lone", [bc("T", 1), [lone("T")]], True), ("1x3+mixed", [bc("T", 3), [lone("T"), lone("G")]], False)):
        L.append(Locus("g:pi-%s" % tag, "A", alt + [bc("A", 12), bc("A", 12)], (";LM;LSM;", 4) if over else (";", 0)))
    # the gap allele as the candidate is not filtered (:549: vtype SDEL), an SNP and an indel beside it are
    for kind, a, design in (("gap", "DEL", (";", 0)), ("snp", "T", (";LM;", 4)), ("ins", ins_key("A", "T"), (";LM;", 1)),
                            ("del", del_key(2), (";LM;", 1))):
        L.append(Locus("g:candidate-%s" % kind, "A", [bc(a, STRONG), bc(a, STRONG), bc("A", STRONG), bc("A", STRONG)], design))
    return build(L, P_GATES)


FAMILIES = ("ties8", "ties32", "ties_indel", "gates")
LIGHT_READS = 400       # gate loci above it (vmf at 1000 barcodes, DP) stay out of the long filter worklist


# ---- what the reference's own numbers say of a locus -----------------------------------------------------------------------------

FIXED_KEYS = ("A", "T", "G", "C", "N", "DEL")
REL = 1e-6               # the project's PI tolerance


def reference_top_two(final):
    """(maxBase, secondMaxBase) of smCounter.py:534-537 from `final`: a stable sort by PI, descending, of the items in dict order."""
    srt = sorted(final, key=lambda kv: -kv[1])
    return srt[0][0], srt[1][0]


def order_class(final):
    if len(final) < 2:
        return "unpinned"
    val = dict((k, v) for k, v in final)
    top = reference_top_two(final)
    for k in top:
        for j in val:
            if j == k:
                continue
            if val[j] == val[k]:
                if j not in BASES or k not in BASES:
                    return "unpinned"
            elif abs(val[j] - val[k]) <= REL * max(abs(val[j]), abs(val[k])):
                return "unpinned"
    return "pinned" if all(k in FIXED_KEYS for k in val) else "pinned_indel"


def has_tie_at_top(final):
    """One of the top two keys shares its PI, bit for bit, with another key."""
    val = dict((k, v) for k, v in final)
    return any(val[j] == val[k] for k in reference_top_two(final) for j in val if j != k)


def designed_tie(label):
    """(the bases a tie locus is built to tie, the place - 0 first, 1 second) or None, from the label `family:ref:kind`."""
    _, ref, kind = label.split(":")
    if kind.startswith("pair-"):
        return tuple(kind[5:]), 1
    if kind.startswith("first-"):
        return tuple(kind[6:]), 0
    if kind.startswith("ref-"):
        return (ref, kind[4:]), 0
    return None


def check_fixture(name, extra):
    """The conditions the generator asserts on a family and tests/test_decision_ref.py repeats on the stored file."""
    exp, labels, designs, classes = extra["expected"], extra["labels"], extra["designs"], extra["order_class"]
    assert len(exp) == len(labels) == len(designs) == len(classes)
    assert classes == [order_class(e["final"]) for e in exp]
    if name == "ties_indel":
        assert 2 * classes.count("pinned_indel") >= len(classes), classes
    else:
        # (a gate locus whose candidate IS an indel cannot but hold an indel key: pinned_indel, and then with no tie in it at all)
        want = ["pinned_indel" if name == "gates" and lab.split(":")[1].split("-")[1] in ("ins", "del") else "pinned" for lab in labels]
        assert classes == want, [(l, c) for l, c, w in zip(labels, classes, want) if c != w]
    for e, lab, design in zip(exp, labels, designs):
        val = dict((k, v) for k, v in e["final"])
        tie = designed_tie(lab) if name in ("ties8", "ties32") else None
        if tie is not None:                                   # the designed tie is there, bit for bit, at the designed place
            (x, y), place = tie
            assert val[x] == val[y] and set(reference_top_two(e["final"])[place:place + 1]) <= {x, y}, (lab, e["final"])
            assert sorted(val.values(), reverse=True)[place] == val[x], (lab, e["final"])
        if name in ("ties8", "ties32") and lab.endswith(":clean"):
            second = sorted(val.values(), reverse=True)[1]
            assert sum(v == second for v in val.values()) >= 2, (lab, e["final"])
        if name == "ties8":
            assert len(val) == (5 if lab.startswith("t8n") else 4), (lab, sorted(val))
        if name == "ties32":
            assert len(val) == 6, (lab, sorted(val))
        if name == "gates":
            if classes[labels.index(lab)] == "pinned_indel":
                assert len(set(val.values())) == len(val) or not has_tie_at_top(e["final"]), lab
            flt, n_fisher = design
            assert e["row"].split("\t")[-1] == flt and len(e["fisher"]) == n_fisher, (lab, design, e["row"].split("\t")[-1], len(e["fisher"]))
            # the side of the PI gate does not hang on the device's own log10: 100 times the PI tolerance away from it
            assert abs(e["pi_raw"][4] - 5.0) >= 1e-4, (lab, e["pi_raw"])


# ---- the stored fixtures (tests/golden/decision/<family>.npz) ---------------------------------------------------------------------

class Family(object):
    """A stored family: the pileup and its device batch, the parameters, the reference provider, and per locus what the reference
    returned (`expected`), the label, the design and the order class.  Nothing outside the repository is read."""

    def __init__(self, name):
        import os
        from conftest import GOLDEN, load_golden
        path = os.path.join(GOLDEN, "decision", name + ".npz")
        self.name = name
        self.pb, self.db, self.P, self.refp, self.expected = load_golden(path)
        self.extra = pileup.load_npz(path)[1]
        self.labels, self.designs, self.classes = self.extra["labels"], self.extra["designs"], self.extra["order_class"]

    def allele_text(self, l, a):
        return self.db.alleles[l][a] if a >= 0 else None

    def reference_choice(self, l):
        return reference_top_two(self.expected[l]["final"])


_FAMILY = {}


def family(name):
    if name not in _FAMILY:
        _FAMILY[name] = Family(name)
    return _FAMILY[name]


def subset(F, idx, reps=1):
    """Family F restricted to the loci `idx`, `reps` times over in one batch (labels, classes and expectations repeat)."""
    from smcounter_amd import features
    S = object.__new__(Family)
    idx = list(idx)
    S.name, S.P, S.refp, S.extra = F.name, F.P, F.refp, F.extra
    one = F.pb.select(idx)
    S.pb = one if reps == 1 else pileup.concat([one] * reps)
    S.db = features.extract_features(S.pb, F.P)
    for k in ("expected", "labels", "designs", "classes"):
        setattr(S, k, [getattr(F, k)[i] for i in idx] * reps)
    return S
