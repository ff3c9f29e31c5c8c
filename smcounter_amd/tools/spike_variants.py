"""Plant listed SNVs in a BAM at a target allele fraction: whole molecular barcodes get the ALT letter at the listed position.

The opposite of tools/ds_allele_fraction.py, which only removes material: "would the caller see a 0.5 % variant at this position, at
this sample's depth, barcode sizes, base qualities and read errors?" - for any position of the panel, in a sample that need not carry
anything there.  The semantics are DESIGN.md's ("--spikeAF"), this file is the specification in code; a run's `--spikeAF` writes, for
every target, the files of a plain run on the BAM this writes.

  1. listed variants: the file format of --dsAFVariants (ds_allele_fraction.parse_variants), SNVs only - REF and ALT one letter each out
     of A, C, G, T; one variant per position; with --refGenome REF must be the genome's (upper-cased) letter.
  2. one draw per barcode b (field -2 of the read name) and variant v at 1-based position P: u_v(b) = word 0 of Philox4x32-10(counter =
     (ident lo, ident hi, 0x73704146 "spAF", P mod 2^32), key = seed lo, hi), ident = the 64-bit FNV-1a of the barcode text.  b is
     spiked at v for target t when u_v(b) < floor(t 2^32).  Neighbouring variants draw independently; the spiked sets are nested over t.
     --phased: the members of a PHASE SET - the SNVs of one MNV line, or the lines that share a PS=<name> entry - all draw with P0,
     the smallest position of the set, in place of their own P: a barcode is spiked at every member or at none, and a read that
     showed REF at two members gets NM + 2.  A variant of no set is a set of one: its draw is the one above.
  3. rewrite: every record of a spiked barcode in the pileup of P (pos <= p < end) whose allele key there is a single letter - a base,
     not inside a deletion, with no insertion or deletion starting behind it (smCounter.py:371-460) - gets ALT at that query position.
     Qualities, CIGAR and flags stay.  NM moves with the base, because the caller's incCond reads it (smCounter.py:329-356): + 1 when
     the old letter was REF, unchanged otherwise (ALT already, another letter, N); an absent NM counts as 0 and the tag is added when
     an increment is due (rewritten with a wider type when the value no longer fits).  MD is not read by the caller and left as it is.
  4. reported per variant: N covering barcodes, V0 carriers before (ds_allele_fraction's rule: more than half of the barcode's reads at
     the locus show ALT), S covering barcodes spiked, READS records rewritten (one that showed ALT already counts), V1 carriers after,
     AF = V1 / N.  Where the variant is present already the achieved fraction exceeds t: reported, not corrected.

--indels (a run's --spikeIndels): the file may hold insertions (REF = X, ALT = XS) and deletions (REF = XD, ALT = X) too, 1 to 255
letters S / D out of ACGT, REF the genome's letters.
  footprint  the reference interval a variant needs: [P, P] (SNV), [P, P + 1] (insertion), [P, P + d + 1] (deletion of d).  A file whose
             footprints overlap is refused by line.
  draw       as above, with the variant's own P.
  eligible   a record of a spiked barcode is rewritten at an insertion / a deletion when the whole footprint lies inside ONE M / = / X
             operation of the record's ORIGINAL CIGAR (so the anchor is a base, nothing starts behind it and an aligned base follows
             the indel) and inside its l_seq bases, and l_seq (+ |S|) and n_cig + 2 stay <= 65535 - counted over the variants taken
             before it, in ascending position.  Every other record is left alone: one that ends inside the footprint, one in a
             deletion there, one with an indel of its own there.  (A real molecule would give such a read a clip or mismatches: not
             modelled.)  SNVs keep rule 3, on the original CIGAR.
  rewrite    insertion: S behind the anchor's base, every letter with the anchor's quality; M(n) -> M(a) I(s) M(n - a).  Deletion:
             the d bases behind the anchor go; M(n) -> M(a) D(d) M(n - a - d).  A = or X operation is split the same way.  pos, the
             reference span (so the bin), flags and mapq stay; NM grows by s / d; MD is left as it is.
  reported   V0 / V1 by the variant's INS|X|XS / DEL|XD|X key (ds_allele_fraction.read_key; a rewritten read whose anchor holds
             another letter than X shows another key and is no carrier), READS the records rewritten.

--phased --indels (a run's --spikeIndelPhase): PS=<name> may stand on an insertion's or a deletion's line too, so a phase set may
hold SNVs, an MNV line's members, insertions and deletions together (at most 8 members; the footprints of ALL listed variants
disjoint).  The leader is the member with the smallest position - an SNV's or an anchor's -, every member draws with the leader's P0,
and each is then applied under its OWN rule above, on the record's original CIGAR: a barcode is spiked at every member or at none,
but a record may take some members and not others (one that ends inside a deletion's footprint takes the SNV in front of it only).
NM accumulates per record: a 3-letter deletion and an SNV that showed REF give NM + 4.  A variant of no set draws as ever.
"""
from __future__ import annotations

import argparse
import bisect
import collections
import os
import struct

import numpy as np

from .. import bamio
from . import ds_allele_fraction as af

SPIKE_DOMAIN = 0x73704146       # counter word 2 of the draw ("spAF")
LETTERS = "ACGT"
_NIBBLE = {c: i for i, c in enumerate("=ACMGRSVTWYHKDBN")}
_NM_FMT = {ord("c"): "<b", ord("C"): "<B", ord("s"): "<h", ord("S"): "<H", ord("i"): "<i", ord("I"): "<I"}
_FIXED = {ord("A"): 1, ord("c"): 1, ord("C"): 1, ord("s"): 2, ord("S"): 2, ord("i"): 4, ord("I"): 4, ord("f"): 4}


PHASE_MAX_MEMBERS = 8           # SMC_SPIKE_PHASE_MAX_MEMBERS: members of a phase set, and letters of an MNV line
PhaseSet = collections.namedtuple("PhaseSet", "name chrom members")     # members: indexes into the variant list, ascending by position


class PhasedVariants(list):
    """parse_variants(phased=True): the member SNVs in file order (an MNV line's members where the line stands), with `sets` - the
    PhaseSets listed, those of one member too, in the order their first line stands in the file - and `mnvs`, per MNV line (chrom,
    pos, REF, line number) for check_reference."""

    def __init__(self, variants=(), sets=(), mnvs=()):
        list.__init__(self, variants)
        self.sets, self.mnvs = list(sets), list(mnvs)


def leaders(variants):
    """Per variant the 1-based position of its phase set's leader (the member with the smallest position) - counter word 3 of its
    draw.  A variant of no listed set is a set of one: its own position, today's draw."""
    out = [v.pos for v in variants]
    for s in getattr(variants, "sets", ()):
        for k in s.members:
            out[k] = variants[s.members[0]].pos
    return out


def phase_sets(variants):
    """The listed sets with two members or more: what the phase pages report."""
    return [s for s in getattr(variants, "sets", ()) if len(s.members) >= 2]


def _parse_phased(path: str, flag: str, indels: bool = False):
    """--spikePhase's reading of the file: ds_allele_fraction.parse_variants' line shapes and refusals, and
      an MNV line   REF and ALT of one length L, 2 <= L <= PHASE_MAX_MEMBERS, letters out of ACGT: one member SNV per offset where they
                    differ (at least one), all in one set named chrom:pos;
      PS=<name>     a `;`-separated entry of column 8 of a VCF-shaped line: the lines of one chromosome with one name are one set (an
                    MNV line with the entry joins it with all its members).
    One variant per position over all members; at most PHASE_MAX_MEMBERS members per set; a name on one chromosome only.
    `indels` (--spikeIndelPhase / --phased --indels): a line may be an insertion X / XS or a deletion XD / X of 1 to MAX_INS letters
    out of ACGT too, and its PS= entry makes it a member like any other; the footprints (footprint()) of ALL listed variants, members
    or not, must be disjoint - refused by line, with parse_variants(indels=True)'s message."""
    out, seen, mnvs = [], set(), []
    line_of = {}                                                 # (chrom, pos) of a listed variant -> its line number
    sets, order = {}, []                                         # set key -> [name, chrom, members], and the keys in file order
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith("#"):
                continue
            f = line.split("\t")
            where = "%s line %d" % (path, n)
            if len(f) >= 5:
                chrom, pos, ref, alt = f[0], f[1], f[3], f[4]
            elif len(f) == 4:
                chrom, pos, ref, alt = f
            else:
                raise ValueError("%s: %d tab-separated columns; VCF (CHROM POS ID REF ALT ...) or `chrom pos ref alt` expected" % (where, len(f)))
            try:
                pos = int(pos)
            except ValueError:
                raise ValueError("%s: position %r is not an integer" % (where, pos))
            if pos < 1:
                raise ValueError("%s: position %d, 1-based positions expected" % (where, pos))
            ref, alt = ref.upper(), alt.upper()
            if "," in alt:
                raise ValueError("%s: ALT %r lists more than one allele (multi-allelic lines are not taken)" % (where, alt))
            ps = [x[3:] for x in f[7].split(";") if x.startswith("PS=")] if len(f) >= 8 else []
            if len(ps) > 1 or (ps and not ps[0]):
                raise ValueError("%s: one PS=<name> entry with a name expected, got %r" % (where, f[7]))
            if len(ref) == len(alt) and len(ref) >= 2:
                if len(ref) > PHASE_MAX_MEMBERS:
                    raise ValueError("%s: %s: an MNV of %d letters, at most %d are taken" % (flag, where, len(ref), PHASE_MAX_MEMBERS))
                if any(c not in LETTERS for c in ref + alt):
                    raise ValueError("%s: %s: %s:%d %s>%s: REF and ALT must be made of A, C, G, T" % (flag, where, chrom, pos, ref, alt))
                members = [(pos + o, r, a) for o, (r, a) in enumerate(zip(ref, alt)) if r != a]
                if not members:
                    raise ValueError("%s: %s: %s:%d %s>%s: REF and ALT of the MNV do not differ in any letter" % (flag, where, chrom, pos, ref, alt))
                mnvs.append((chrom, pos, ref, n))
                key = ("PS", ps[0]) if ps else ("MNV", chrom, pos)
                name = ps[0] if ps else "%s:%d" % (chrom, pos)
            else:
                ka = af.allele_key(ref, alt)
                if ka is None:
                    if len(ref) != len(alt):
                        raise ValueError("%s: %s: REF %r / ALT %r have different lengths and are neither an insertion (X / XS) nor a "
                                         "deletion (XD / X)" % (flag, where, ref, alt))
                    raise ValueError("%s: REF %r / ALT %r is neither a substitution of one letter, an insertion (X / XS) nor a "
                                     "deletion (XD / X)" % (where, ref, alt))
                if ka[1] != af.SNV and not indels:
                    raise ValueError("%s: %s:%d %s>%s is an insertion or a deletion; only one-letter substitutions can be spiked (an indel "
                                     "means rewriting CIGARs)" % (flag, chrom, pos, ref, alt))
                if ka[1] == af.SNV:
                    if ref not in LETTERS or alt not in LETTERS:
                        raise ValueError("%s: %s:%d %s>%s: REF and ALT must be one of A, C, G, T" % (flag, chrom, pos, ref, alt))
                else:                                            # (parse_variants(indels=True)'s refusals of an indel line)
                    if ka[1] == af.INS and len(alt) - 1 > af.MAX_INS:
                        raise ValueError("%s: an insertion of %d letters, at most %d are taken" % (where, len(alt) - 1, af.MAX_INS))
                    if any(c not in LETTERS for c in ref + alt):
                        raise ValueError("%s: %s:%d %s>%s: REF and ALT must be made of A, C, G, T" % (flag, chrom, pos, ref, alt))
                    if ka[1] == af.DEL and len(ref) - 1 > af.MAX_INS:
                        raise ValueError("%s: %s:%d: a deletion of %d letters, at most %d are taken" % (flag, chrom, pos, len(ref) - 1, af.MAX_INS))
                members = [(pos, ref, alt)]
                key, name = (("PS", ps[0]), ps[0]) if ps else (None, None)
            for q, r, a in members:
                if (chrom, q) in seen:
                    raise ValueError("%s: %s:%d is listed twice (one variant per position)" % (where, chrom, q))
                seen.add((chrom, q))
                line_of[(chrom, q)] = n
            if key is not None:
                if key not in sets:
                    sets[key] = [name, chrom, []]
                    order.append(key)
                if sets[key][1] != chrom:
                    raise ValueError("%s: %s: the phase set PS=%s is listed on %s and on %s (a set lies on one chromosome)" %
                                     (flag, where, name, sets[key][1], chrom))
                sets[key][2] += list(range(len(out), len(out) + len(members)))
                if len(sets[key][2]) > PHASE_MAX_MEMBERS:
                    raise ValueError("%s: %s: the phase set %s has %d members, at most %d" % (flag, where, name, len(sets[key][2]), PHASE_MAX_MEMBERS))
            out += [af.Variant(chrom, q, r, a, *af.allele_key(r, a)) for q, r, a in members]
    if not out:
        raise ValueError("%s lists no variant" % path)
    if indels:
        _check_footprints(out, flag, path, line_of)
    return PhasedVariants(out, [PhaseSet(sets[k][0], sets[k][1], tuple(sorted(sets[k][2], key=lambda i: out[i].pos))) for k in order], mnvs)


def footprint(v):
    """The reference interval variant `v` needs, 1-based and closed: [P, P] (SNV), [P, P + 1] (insertion), [P, P + d + 1] (deletion)."""
    return v.pos, v.pos + (0 if v.kind == af.SNV else 1 if v.kind == af.INS else len(v.ref))


def _lines_of(path: str):
    """(chrom, pos) -> line number of the file's variant lines (ds_allele_fraction.parse_variants has taken every one)."""
    out = {}
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            if line.strip() and not line.startswith("#"):
                f = line.split("\t")
                out[(f[0], int(f[1]))] = n
    return out


def _check_footprints(variants, flag: str, path: str, lines) -> None:
    """ValueError, by line, when the footprints of two listed variants of one chromosome overlap.  lines[(chrom, pos)]: line numbers."""
    order = sorted(variants, key=lambda v: (v.chrom, v.pos))
    for u, v in zip(order, order[1:]):
        if u.chrom == v.chrom and footprint(u)[1] >= v.pos:
            raise ValueError("%s: %s line %d: %s:%d %s>%s lies in the footprint %d-%d of %s:%d %s>%s (line %d)" % (
                flag, path, lines[(v.chrom, v.pos)], v.chrom, v.pos, v.ref, v.alt, footprint(u)[0], footprint(u)[1], u.chrom, u.pos,
                u.ref, u.alt, lines[(u.chrom, u.pos)]))


def parse_variants(path: str, flag: str = "--variants", phased: bool = False, indels: bool = False):
    """The variants of a spike-in file, in file order: ds_allele_fraction.parse_variants' format and refusals, and only one-letter
    substitutions out of A, C, G, T (an insertion or a deletion would mean rewriting CIGARs).  ValueError names the variant refused.
    `phased` (--spikePhase / --phased): MNV lines and PS= entries make phase sets (_parse_phased) -> PhasedVariants; without it an
    MNV line is refused as ever and PS= entries are not read.
    `indels` (--spikeIndels / --indels): insertions X / XS and deletions XD / X of 1 to MAX_INS letters out of A, C, G, T are taken
    too; footprints (footprint()) that overlap are refused by line.
    Both (--spikeIndelPhase / --phased --indels): phase sets whose members may be insertions and deletions -> PhasedVariants."""
    if phased:
        return _parse_phased(path, flag, indels)
    out = af.parse_variants(path)
    for v in out:
        if v.kind != af.SNV and not indels:
            raise ValueError("%s: %s:%d %s>%s is an insertion or a deletion; only one-letter substitutions can be spiked (an indel "
                             "means rewriting CIGARs)" % (flag, v.chrom, v.pos, v.ref, v.alt))
        if any(c not in LETTERS for c in v.ref + v.alt):
            raise ValueError("%s: %s:%d %s>%s: REF and ALT must be %s A, C, G, T" % (flag, v.chrom, v.pos, v.ref, v.alt,
                                                                                  "one of" if v.kind == af.SNV else "made of"))
        if v.kind == af.DEL and len(v.ref) - 1 > af.MAX_INS:
            raise ValueError("%s: %s:%d: a deletion of %d letters, at most %d are taken" % (flag, v.chrom, v.pos, len(v.ref) - 1, af.MAX_INS))
    if indels:
        _check_footprints(out, flag, path, _lines_of(path))
    return out


def check_reference(variants, fasta, flag: str = "--variants") -> None:
    """REF of every variant must be the genome's upper-cased letter(s) at its position."""
    for v in variants:
        letter = fasta.fetch(v.chrom, v.pos - 1, v.pos - 1 + len(v.ref)).upper()
        if letter != v.ref:
            raise ValueError("%s: %s:%d %s>%s: the reference genome has %r there, not %s" % (flag, v.chrom, v.pos, v.ref, v.alt, letter, v.ref))
    for chrom, pos, ref, n in getattr(variants, "mnvs", ()):     # (an MNV line: its letters that do not change too)
        letters = fasta.fetch(chrom, pos - 1, pos - 1 + len(ref)).upper()
        if letters != ref:
            raise ValueError("%s: line %d: %s:%d REF %s: the reference genome has %r there" % (flag, n, chrom, pos, ref, letters))


def threshold(t: float) -> int:
    return int(np.floor(float(t) * 4294967296.0))


def draw(idents, seed: int, pos1: int) -> np.ndarray:
    """u_v(b) of every identity for the variant at 1-based pos1: word 0 of Philox4x32-10(counter = (ident lo, ident hi, SPIKE_DOMAIN,
    pos1 mod 2^32), key = (seed lo, seed hi))."""
    idents = np.asarray(idents, np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    n = len(idents)
    c = [idents & m32, idents >> np.uint64(32), np.full(n, SPIKE_DOMAIN, np.uint64), np.full(n, int(pos1) & 0xFFFFFFFF, np.uint64)]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c[0].astype(np.uint64)


def spiked(ident: int, seed: int, pos1: int, thr: int) -> bool:
    return int(draw([ident], seed, pos1)[0]) < thr


def base_at(a, pos1: int):
    """The query position of the base alignment `a` shows at 1-based pos1 when its allele key there is a single letter, else None."""
    col = bamio._column(a, pos1 - 1)
    if col is None:
        return None
    qpos, is_del, indel = col
    return None if is_del or indel != 0 or qpos >= a.l_seq else qpos


def _nm_tag(aux: bytes):
    """-> (offset of the first integer NM tag in the record's tag bytes, its type byte) or None."""
    i, n = 0, len(aux)
    while i + 3 <= n:
        tag, typ = aux[i:i + 2], aux[i + 2]
        if typ in _FIXED:
            if tag == b"NM" and typ in _NM_FMT:
                return i, typ
            i += 3 + _FIXED[typ]
        elif typ in (ord("Z"), ord("H")):
            i = aux.index(b"\x00", i + 3) + 1
        elif typ == ord("B"):
            i += 3 + 5 + struct.unpack_from("<I", aux, i + 4)[0] * _FIXED[aux[i + 3]]
        else:
            raise bamio.BamError("unknown aux type %r" % chr(typ))
    return None


def rewrite_record(raw: bytes, edits, nm_new) -> bytes:
    """A raw record (with its block_size) with the letters of `edits` [(query position, letter)] written into its nibbles and, `nm_new`
    not None, its NM set to that value: in place where the tag is there and the value fits its type, else the tag is taken out and
    added at the end with the smallest unsigned type that holds it."""
    body = bytearray(raw[4:])
    l_name, n_cig, l_seq = body[8], struct.unpack_from("<H", body, 12)[0], struct.unpack_from("<i", body, 16)[0]
    o_seq = 32 + l_name + 4 * n_cig
    for qpos, letter in edits:
        k = o_seq + (qpos >> 1)
        code = _NIBBLE[letter]
        body[k] = (body[k] & 0x0F) | (code << 4) if qpos % 2 == 0 else (body[k] & 0xF0) | code
    if nm_new is not None:
        o_aux = o_seq + (l_seq + 1) // 2 + l_seq
        aux = bytes(body[o_aux:])
        at = _nm_tag(aux)
        done = False
        if at is not None:
            i, typ = at
            try:
                struct.pack_into(_NM_FMT[typ], body, o_aux + i + 3, nm_new)
                done = True
            except struct.error:
                del body[o_aux + i:o_aux + i + 3 + _FIXED[typ]]
        if not done:
            body += b"NM" + (b"C" + struct.pack("<B", nm_new) if nm_new < 256 else b"S" + struct.pack("<H", nm_new) if nm_new < 65536
                             else b"I" + struct.pack("<I", nm_new))
    return struct.pack("<i", len(body)) + bytes(body)


class Plan(object):
    """The listed variants by chromosome, sorted by position, with the seed and the target's threshold: which of them a record spans.
    A member of a phase set (parse_variants(phased=True)) draws with its leader's position."""

    def __init__(self, variants, t: float, seed: int):
        self.lead_pos = leaders(variants)
        self.variants, self.t, self.seed, self.thr = list(variants), float(t), int(seed), threshold(t)
        self.by_chrom = collections.defaultdict(list)
        for k, v in enumerate(self.variants):
            self.by_chrom[v.chrom].append((v.pos, k))
        for c in self.by_chrom:
            self.by_chrom[c].sort()
        self._pos = {c: [p for p, _ in l] for c, l in self.by_chrom.items()}
        self._u = {}

    def spanned(self, chrom: str, pos0: int, end0: int):
        """Indexes of the variants with pos0 < P <= end0 (1-based P inside the 0-based span [pos0, end0)), ascending by position."""
        ps = self._pos.get(chrom)
        if not ps:
            return []
        return [self.by_chrom[chrom][j][1] for j in range(bisect.bisect_left(ps, pos0 + 1), bisect.bisect_right(ps, end0))]

    def is_spiked(self, k: int, ident: int) -> bool:
        key = (k, ident)
        if key not in self._u:
            self._u[key] = spiked(ident, self.seed, self.lead_pos[k], self.thr)
        return self._u[key]


def spike_record(plan: Plan, a, chrom: str, ident: int, counts=None):
    """What the rewrite does to alignment `a` (bamio.Alignment) of the barcode with identity `ident` -> (edits [(qpos, ALT)], NM
    increments).  `counts` (per variant a dict barcode identity -> [reads, alt before, alt after, rewritten]) is added to."""
    edits, inc = [], 0
    for k in plan.spanned(chrom, a.pos, a.end):
        v = plan.variants[k]
        q = base_at(a, v.pos)
        hit = plan.is_spiked(k, ident)
        shows = q is not None and a.seq[q] == v.alt
        if counts is not None:
            c = counts[k].setdefault(ident, [0, 0, 0, 0])
            c[0] += 1
            c[1] += shows
            c[2] += (q is not None) if hit else shows
            c[3] += hit and q is not None
        if hit and q is not None:
            edits.append((q, v.alt))
            inc += a.seq[q] == v.ref
    return edits, inc


MAX16 = 65535                   # l_seq and n_cig of a record are 16-bit fields of the device's records (and n_cig of the BAM's)


def anchor_in_match(a, pos0: int, fp: int):
    """-> (operation index, the anchor's offset in it, its query position) when the 0-based positions pos0 .. pos0 + fp all lie in ONE
    M / = / X operation of alignment `a` and their bases inside its l_seq, else None."""
    x, y = a.pos, 0
    for ci, (op, l) in enumerate(a.cigar):
        if op in (0, 7, 8):
            if x <= pos0 < x + l:
                d0 = pos0 - x
                return (ci, d0, y + d0) if d0 + fp < l and y + d0 + fp < a.l_seq else None
            x += l
            y += l
        elif op in (1, 4):
            y += l
        elif op in (2, 3):
            if x <= pos0 < x + l:
                return None
            x += l
    return None


def spike_record_indels(plan: Plan, a, chrom: str, ident: int, counts=None, fasta=None):
    """spike_record() for a list that holds insertions / deletions -> (actions, NM increments, relocated).  actions, ascending by
    position: ("snv", query position, ALT) | ("ins", operation index, offset of the anchor in it, its query position, S) | ("del",
    ..., d); every one resolved against the ORIGINAL CIGAR.  `relocated`: the record takes an insertion or a deletion."""
    actions, inc, n_cig, l_seq = [], 0, len(a.cigar), a.l_seq
    for k in plan.spanned(chrom, a.pos, a.end):
        v = plan.variants[k]
        hit = plan.is_spiked(k, ident)
        if v.kind == af.SNV:
            q = base_at(a, v.pos)
            shows, ok = q is not None and a.seq[q] == v.alt, q is not None
        else:
            n = len(v.alt) - 1 if v.kind == af.INS else len(v.ref) - 1
            at = anchor_in_match(a, v.pos - 1, 1 if v.kind == af.INS else n + 1)
            ok = at is not None and n_cig + 2 <= MAX16 and (v.kind != af.INS or l_seq + n <= MAX16)
            shows = af.read_key(a, v.pos, chrom, fasta) == af.variant_key(v, fasta)
        if counts is not None:
            c = counts[k].setdefault(ident, [0, 0, 0, 0])
            c[0] += 1
            c[1] += shows
            # (a read that shows a listed insertion already is not eligible for it; a rewritten read whose anchor holds another letter
            # than X shows another key than the variant's)
            c[2] += (ok and (v.kind == af.SNV or a.seq[at[2]] == v.ref[0])) or shows if hit else shows
            c[3] += hit and ok
        if not (hit and ok):
            continue
        if v.kind == af.SNV:
            actions.append(("snv", q, v.alt))
            inc += a.seq[q] == v.ref
        else:
            actions.append(("ins", at[0], at[1], at[2], v.alt[1:]) if v.kind == af.INS else ("del", at[0], at[1], at[2], n))
            inc += n
            n_cig += 2
            l_seq += n if v.kind == af.INS else -n
    return actions, inc, any(x[0] != "snv" for x in actions)


def apply_actions(a, actions):
    """The CIGAR [(op, len)], SEQ and QUAL (bytes) of alignment `a` after `actions` (spike_record_indels)."""
    seq, qual = list(a.seq), list(bytes(a.qual))
    cigar = [list(c) for c in a.cigar]
    for act in reversed(actions):                        # from the back: what stands in front keeps its indexes
        if act[0] == "snv":
            seq[act[1]] = act[2]
            continue
        kind, ci, d0, qa, x = act
        op, l = cigar[ci]
        if kind == "ins":
            cigar[ci:ci + 1] = [[op, d0 + 1], [1, len(x)], [op, l - d0 - 1]]
            seq[qa + 1:qa + 1] = list(x)
            qual[qa + 1:qa + 1] = [qual[qa]] * len(x)
        else:
            cigar[ci:ci + 1] = [[op, d0 + 1], [2, x], [op, l - d0 - 1 - x]]
            del seq[qa + 1:qa + 1 + x]
            del qual[qa + 1:qa + 1 + x]
    return [tuple(c) for c in cigar], "".join(seq), bytes(qual)


def _set_nm(body: bytearray, o_aux: int, nm_new: int) -> None:
    """NM of the record `body` (tags from o_aux) set to nm_new: in place where the tag is there and the value fits its type, else the
    tag is taken out and added at the end with the smallest unsigned type that holds it."""
    at = _nm_tag(bytes(body[o_aux:]))
    if at is not None:
        i, typ = at
        try:
            struct.pack_into(_NM_FMT[typ], body, o_aux + i + 3, nm_new)
            return
        except struct.error:
            del body[o_aux + i:o_aux + i + 3 + _FIXED[typ]]
    body += b"NM" + (b"C" + struct.pack("<B", nm_new) if nm_new < 256 else b"S" + struct.pack("<H", nm_new) if nm_new < 65536
                     else b"I" + struct.pack("<I", nm_new))


def rebuild_record(raw: bytes, cigar, seq: str, qual: bytes, nm_new: int) -> bytes:
    """A raw record with its CIGAR, SEQ, QUAL, l_seq and n_cig replaced and NM set; the fixed fields (the bin too: the reference span
    has not moved), the name and the other tags stay."""
    body = raw[4:]
    l_name, n_cig, l_seq = body[8], struct.unpack_from("<H", body, 12)[0], struct.unpack_from("<i", body, 16)[0]
    o_aux = 32 + l_name + 4 * n_cig + (l_seq + 1) // 2 + l_seq
    packed = bytearray((len(seq) + 1) // 2)
    for i, ch in enumerate(seq):
        packed[i >> 1] |= _NIBBLE[ch] << (4 if i % 2 == 0 else 0)
    head = bytearray(body[:32 + l_name])
    struct.pack_into("<H", head, 12, len(cigar))
    struct.pack_into("<i", head, 16, len(seq))
    out = head + b"".join(struct.pack("<I", (l << 4) | op) for op, l in cigar) + packed + bytearray(qual)
    o_new = len(out)
    out += body[o_aux:]
    _set_nm(out, o_new, nm_new)
    return struct.pack("<i", len(out)) + bytes(out)


def report_rows(plan: Plan, counts):
    """Step 4 from the counters of spike_record -> per variant dict(N, V0, S, READS, V1)."""
    rows = []
    for k, per in enumerate(counts):
        rows.append(dict(N=len(per), V0=sum(2 * c[1] > c[0] for c in per.values()), S=sum(plan.is_spiked(k, b) for b in per),
                         READS=sum(c[3] for c in per.values()), V1=sum(2 * c[2] > c[0] for c in per.values())))
    return rows


def report_line(v, t: float, row) -> str:
    return "--spikeAF %g: %s:%d %s>%s N %d, V0 %d, S %d, READS %d, V1 %d, AF %.6g" % (
        t, v.chrom, v.pos, v.ref, v.alt, row["N"], row["V0"], row["S"], row["READS"], row["V1"], float(row["V1"]) / row["N"] if row["N"] else 0.0)


def spike_file(in_bam: str, out_bam: str, variants, t: float, seed: int, fasta=None):
    """Steps 2-4 over a file -> per variant dict(N, V0, S, READS, V1); writes out_bam (None: only the numbers).  `fasta`: names a
    read's deleted letters when a deletion is listed (without one a deletion is compared by its length)."""
    ids = af.unique_idents(bamio.placed_barcodes(in_bam), in_bam)
    plan = Plan(variants, t, seed)
    counts = [dict() for _ in variants]
    probe = bamio.BamFile(in_bam)
    refs = [name for name, _ in probe.refs]
    probe.close()
    header, recs = bamio.iter_raw_records(in_bam)
    with_indels = any(v.kind != af.SNV for v in variants)

    def out():
        for tid, q, raw in recs:
            if tid >= 0 and refs[tid] in plan.by_chrom:
                a = bamio._parse_record(raw[4:])
                bc = af.barcode_of(q)
                if not (a.flag & 0x4) and a.cigar and bc is not None and plan.spanned(refs[tid], a.pos, a.end):
                    ident = ids.get(bc, af.fnv64(bc))
                    relocated = False
                    if with_indels:
                        actions, inc, relocated = spike_record_indels(plan, a, refs[tid], ident, counts, fasta)
                        edits = [(x[1], x[2]) for x in actions]
                    else:
                        edits, inc = spike_record(plan, a, refs[tid], ident, counts)
                    if relocated:
                        raw = rebuild_record(raw, *apply_actions(a, actions), nm_new=a.nm + inc)
                    elif edits:
                        raw = rewrite_record(raw, edits, a.nm + inc if inc else None)
            yield raw
    if out_bam is None:
        for _ in out():
            pass
    else:
        bamio.write_raw(out_bam, header, out())
    return report_rows(plan, counts)


def main(args):
    if args.runPath:
        os.chdir(args.runPath)
    try:
        variants = parse_variants(args.variants, phased=bool(getattr(args, "phased", False)), indels=bool(getattr(args, "indels", False)))
        targets = af.parse_targets(args.af)
        if len(targets) != 1:
            raise ValueError("--af: one target allele fraction per output BAM, got %r" % args.af)
        genome = None
        if args.refGenome:
            from .. import fasta as _fasta
            genome = _fasta.FastaFile(args.refGenome)
            check_reference(variants, genome)
    except ValueError as e:
        raise SystemExit(str(e))
    rows = spike_file(args.inBam, args.outBam, variants, targets[0], args.seed, genome)
    for v, row in zip(variants, rows):
        print(report_line(v, targets[0], row))
    return rows


def build_parser():
    parser = argparse.ArgumentParser(description="Plant listed SNVs at a target allele fraction by rewriting whole barcodes' bases")
    parser.add_argument("--runPath", default=None, help="path to working directory")
    parser.add_argument("--inBam", default=None, required=True, help="Input BAM file (coordinate-sorted)")
    parser.add_argument("--outBam", default=None, required=True, help="Output BAM file")
    parser.add_argument("--variants", default=None, required=True, help="SNVs: VCF lines, or `chrom pos ref alt` (tab-separated)")
    parser.add_argument("--af", default=None, required=True, help="target allele fraction in (0, 1)")
    parser.add_argument("--seed", type=int, default=1234567, help="Seed of the barcode draws")
    parser.add_argument("--refGenome", default=None, help="indexed FASTA: REF of every listed variant must be its letter there")
    parser.add_argument("--phased", action="store_true", help="read MNV lines (REF and ALT of one length, 2 to 8 letters) and PS=<name> "
                        "entries of VCF column 8 as phase sets: the members of a set are planted on the same barcodes")
    parser.add_argument("--indels", action="store_true", help="take insertions (REF X, ALT XS) and deletions (REF XD, ALT X) of 1 to 255 "
                        "letters too: the records that hold the whole footprint in one aligned operation get the new SEQ, QUAL and CIGAR")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
