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


def _parse_phased(path: str, flag: str):
    """--spikePhase's reading of the file: ds_allele_fraction.parse_variants' line shapes and refusals, and
      an MNV line   REF and ALT of one length L, 2 <= L <= PHASE_MAX_MEMBERS, letters out of ACGT: one member SNV per offset where they
                    differ (at least one), all in one set named chrom:pos;
      PS=<name>     a `;`-separated entry of column 8 of a VCF-shaped line: the lines of one chromosome with one name are one set (an
                    MNV line with the entry joins it with all its members).
    One variant per position over all members; at most PHASE_MAX_MEMBERS members per set; a name on one chromosome only."""
    out, seen, mnvs = [], set(), []
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
                if ka[1] != af.SNV:
                    raise ValueError("%s: %s:%d %s>%s is an insertion or a deletion; only one-letter substitutions can be spiked (an indel "
                                     "means rewriting CIGARs)" % (flag, chrom, pos, ref, alt))
                if ref not in LETTERS or alt not in LETTERS:
                    raise ValueError("%s: %s:%d %s>%s: REF and ALT must be one of A, C, G, T" % (flag, chrom, pos, ref, alt))
                members = [(pos, ref, alt)]
                key, name = (("PS", ps[0]), ps[0]) if ps else (None, None)
            for q, r, a in members:
                if (chrom, q) in seen:
                    raise ValueError("%s: %s:%d is listed twice (one variant per position)" % (where, chrom, q))
                seen.add((chrom, q))
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
            out += [af.Variant(chrom, q, r, a, a, af.SNV) for q, r, a in members]
    if not out:
        raise ValueError("%s lists no variant" % path)
    return PhasedVariants(out, [PhaseSet(sets[k][0], sets[k][1], tuple(sorted(sets[k][2], key=lambda i: out[i].pos))) for k in order], mnvs)


def parse_variants(path: str, flag: str = "--variants", phased: bool = False):
    """The variants of a spike-in file, in file order: ds_allele_fraction.parse_variants' format and refusals, and only one-letter
    substitutions out of A, C, G, T (an insertion or a deletion would mean rewriting CIGARs).  ValueError names the variant refused.
    `phased` (--spikePhase / --phased): MNV lines and PS= entries make phase sets (_parse_phased) -> PhasedVariants; without it an
    MNV line is refused as ever and PS= entries are not read."""
    if phased:
        return _parse_phased(path, flag)
    out = af.parse_variants(path)
    for v in out:
        if v.kind != af.SNV:
            raise ValueError("%s: %s:%d %s>%s is an insertion or a deletion; only one-letter substitutions can be spiked (an indel "
                             "means rewriting CIGARs)" % (flag, v.chrom, v.pos, v.ref, v.alt))
        if v.ref not in LETTERS or v.alt not in LETTERS:
            raise ValueError("%s: %s:%d %s>%s: REF and ALT must be one of A, C, G, T" % (flag, v.chrom, v.pos, v.ref, v.alt))
    return out


def check_reference(variants, fasta, flag: str = "--variants") -> None:
    """REF of every variant must be the genome's upper-cased letter at its position."""
    for v in variants:
        letter = fasta.fetch(v.chrom, v.pos - 1, v.pos).upper()
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


def spike_file(in_bam: str, out_bam: str, variants, t: float, seed: int):
    """Steps 2-4 over a file -> per variant dict(N, V0, S, READS, V1); writes out_bam (None: only the numbers)."""
    ids = af.unique_idents(bamio.placed_barcodes(in_bam), in_bam)
    plan = Plan(variants, t, seed)
    counts = [dict() for _ in variants]
    probe = bamio.BamFile(in_bam)
    refs = [name for name, _ in probe.refs]
    probe.close()
    header, recs = bamio.iter_raw_records(in_bam)

    def out():
        for tid, q, raw in recs:
            if tid >= 0 and refs[tid] in plan.by_chrom:
                a = bamio._parse_record(raw[4:])
                bc = af.barcode_of(q)
                if not (a.flag & 0x4) and a.cigar and bc is not None and plan.spanned(refs[tid], a.pos, a.end):
                    edits, inc = spike_record(plan, a, refs[tid], ids.get(bc, af.fnv64(bc)), counts)
                    if edits:
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
        variants = parse_variants(args.variants, phased=bool(getattr(args, "phased", False)))
        targets = af.parse_targets(args.af)
        if len(targets) != 1:
            raise ValueError("--af: one target allele fraction per output BAM, got %r" % args.af)
        if args.refGenome:
            from .. import fasta as _fasta
            check_reference(variants, _fasta.FastaFile(args.refGenome))
    except ValueError as e:
        raise SystemExit(str(e))
    rows = spike_file(args.inBam, args.outBam, variants, targets[0], args.seed)
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
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
