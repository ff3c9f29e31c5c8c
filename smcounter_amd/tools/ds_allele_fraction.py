"""Dilute listed variants to target allele fractions: drop whole molecular barcodes that carry a listed allele.

The reference's titration kit names a third helper beside ds.mt.py and ds.reads.withinMT.py - `ds.allele.fraction.py`, "reducing the
variant allele fraction at given variant loci" - but does not ship it.  This is that tool with the semantics DESIGN.md fixes
("--dsAF"), the specification in code; a run's `--dsAF` writes, for every target, the files of a plain run on the BAM this writes.

  1. counts, file-wide, at full depth: for a listed variant v and a barcode b (field -2 of the read name), reads(b, v) = the records
     of b in the pileup of v's locus (no filter), alt(b, v) = those whose allele key there (smCounter.py:371-460) is v's.  b covers v
     when reads > 0, carries v when 2 alt > reads.  N_v covering barcodes, V_v carriers, a_v = V_v / N_v.
  2. keep probability k_v(t) = min(1, t (N_v - V_v) / (V_v (1 - t))); 1 when a_v <= t, when V_v = 0 and when V_v = N_v.
     thr_v(t) = floor(k_v(t) 2^32).
  3. one draw per barcode: u(b) = word 0 of Philox4x32-10(counter = (ident lo, ident hi, 0x64734146, 0), key = seed lo, hi), ident =
     the 64-bit FNV-1a of the barcode text.  b is dropped at t when it carries at least one listed v with u(b) >= thr_v(t); all its
     records go, nothing else changes.  The kept sets are nested over t.
  4. achieved N'_v(t), V'_v(t): recounted over the kept barcodes from the sets of step 1.
"""
from __future__ import annotations

import argparse
import collections
import os

import numpy as np

from .. import bamio

AF_DOMAIN = 0x64734146          # counter word 2 of the draw ("dsAF")
MAX_INS = 255                   # inserted letters of a listed insertion (the kernel's pool entry: SMC_AF_MAX_INS)
SNV, INS, DEL, NONE = 0, 1, 2, 3    # SMC_AF_*

Variant = collections.namedtuple("Variant", "chrom pos ref alt key kind")


def allele_key(ref: str, alt: str):
    """(allele key, kind) of a REF / ALT pair by the keys the caller uses (smCounter.py:371-460, convertToVcf :103-117), or None
    when the pair is none of the three shapes."""
    if len(ref) == 1 and len(alt) == 1 and ref != alt:
        return alt, SNV
    if len(ref) == 1 and len(alt) > 1 and alt[0] == ref:
        return "INS|%s|%s" % (ref, alt), INS
    if len(alt) == 1 and len(ref) > 1 and ref[0] == alt:
        return "DEL|%s|%s" % (ref, alt), DEL
    return None


def parse_variants(path: str):
    """The variants of a --dsAFVariants file, in file order.  `#` lines are skipped; five or more tab-separated columns are VCF
    (CHROM POS ID REF ALT), exactly four are chrom pos ref alt; pos is 1-based.  ValueError names the line that is refused."""
    out, seen = [], set()
    with open(path) as fh:
        for n, line in enumerate(fh, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith("#"):
                continue
            f = line.split("\t")
            if len(f) >= 5:
                chrom, pos, ref, alt = f[0], f[1], f[3], f[4]
            elif len(f) == 4:
                chrom, pos, ref, alt = f
            else:
                raise ValueError("%s line %d: %d tab-separated columns; VCF (CHROM POS ID REF ALT ...) or `chrom pos ref alt` expected"
                                 % (path, n, len(f)))
            try:
                pos = int(pos)
            except ValueError:
                raise ValueError("%s line %d: position %r is not an integer" % (path, n, pos))
            if pos < 1:
                raise ValueError("%s line %d: position %d, 1-based positions expected" % (path, n, pos))
            ref, alt = ref.upper(), alt.upper()
            if "," in alt:
                raise ValueError("%s line %d: ALT %r lists more than one allele (multi-allelic lines are not taken)" % (path, n, alt))
            ka = allele_key(ref, alt)
            if ka is None:
                raise ValueError("%s line %d: REF %r / ALT %r is neither a substitution of one letter, an insertion (X / XS) nor a "
                                 "deletion (XD / X)" % (path, n, ref, alt))
            if ka[1] == INS and len(alt) - 1 > MAX_INS:
                raise ValueError("%s line %d: an insertion of %d letters, at most %d are taken" % (path, n, len(alt) - 1, MAX_INS))
            if (chrom, pos) in seen:
                raise ValueError("%s line %d: %s:%d is listed twice (one variant per position)" % (path, n, chrom, pos))
            seen.add((chrom, pos))
            out.append(Variant(chrom, pos, ref, alt, ka[0], ka[1]))
    if not out:
        raise ValueError("%s lists no variant" % path)
    return out


def parse_targets(text, flag="--af"):
    """Comma-separated target allele fractions, each in (0, 1); ValueError otherwise."""
    try:
        ts = [float(x) for x in str(text).split(",") if x.strip()]
    except ValueError:
        raise ValueError("%s: comma-separated allele fractions in (0, 1) expected, got %r" % (flag, text))
    if not ts or any(not (0.0 < t < 1.0) for t in ts):
        raise ValueError("%s: every target allele fraction must lie in (0, 1), got %r" % (flag, text))
    return ts


def barcode_of(qname: str):
    """Field -2 of the stripped read name (ds.mt.py:43-45); None for a name without one."""
    f = qname.strip().split(":")
    return f[-2] if len(f) >= 2 else None


def fnv64(text: str) -> int:
    x = 1469598103934665603
    for c in text.encode():
        x = ((x ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return x


def philox_word0(idents, seed: int) -> np.ndarray:
    """u(b): word 0 of Philox4x32-10(counter = (ident lo, ident hi, AF_DOMAIN, 0), key = (seed lo, seed hi)) for every ident."""
    idents = np.asarray(idents, np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    c = [idents & m32, idents >> np.uint64(32), np.full(len(idents), AF_DOMAIN, np.uint64), np.zeros(len(idents), np.uint64)]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c[0].astype(np.uint64)


def keep_probability(n: int, v: int, t: float) -> float:
    """Step 2: k_v(t).  1 for an absent variant, one every covering barcode carries, and one at or below the target already."""
    if v == 0 or v == n or float(v) / float(n) <= t:
        return 1.0
    return min(1.0, t * float(n - v) / (float(v) * (1.0 - t)))


def threshold(k: float) -> int:
    return 1 << 32 if k >= 1.0 else int(np.floor(k * 4294967296.0))


def read_key(a, pos1: int, chrom: str, fasta=None):
    """The allele key alignment `a` shows at 1-based pos1 (bamio's host pileup rules), None when it is not in the pileup.  A deletion
    start's deleted letters are the reference's (`fasta`); without one they are written as their count, "DEL|X<n>|X"."""
    col = bamio._column(a, pos1 - 1)
    if col is None:
        return None
    qpos, is_del, indel = col
    if is_del and indel == 0:
        return "DEL"
    site = a.seq[qpos]
    if indel > 0:
        return "INS|" + site + "|" + site + a.seq[qpos + 1:qpos + 1 + indel]
    if indel < 0:
        deleted = fasta.fetch(chrom, pos1, pos1 - indel).upper() if fasta is not None else "<%d>" % -indel
        return "DEL|" + site + deleted + "|" + site
    return site


def variant_key(v: Variant, fasta=None) -> str:
    """The key read_key() gives a read that shows `v` (without a reference a deletion is compared by its length)."""
    if v.kind == DEL and fasta is None:
        return "DEL|%s<%d>|%s" % (v.alt, len(v.ref) - 1, v.alt)
    return v.key


def count_file(path: str, variants, fasta=None):
    """Step 1 -> per variant (cover, carry): the barcode texts that cover it, in first-appearance order, and the set that carries it."""
    bam = bamio.BamFile(path)
    out = []
    try:
        for v in variants:
            reads, alt = collections.OrderedDict(), collections.Counter()
            want = variant_key(v, fasta)
            for a in bam.fetch(v.chrom, v.pos - 1, v.pos):
                key = read_key(a, v.pos, v.chrom, fasta)
                if key is None:
                    continue
                parts = a.qname.split(":")
                if len(parts) < 3:
                    raise bamio.BamError("read name %r has fewer than 3 ':' fields; the reference needs "
                                         "<readid>:<tag>:<UMI>:<x> (smCounter.py:320-325)" % a.qname)
                bc = parts[-2]
                reads[bc] = reads.get(bc, 0) + 1
                if key == want:
                    alt[bc] += 1
            out.append((list(reads), {bc for bc in reads if 2 * alt[bc] > reads[bc]}))
    finally:
        bam.close()
    return out


def titrate(covers, carries, targets, seed: int):
    """Steps 2-4 on identities.  covers[v] / carries[v]: uint64 arrays of the barcode identities that cover / carry variant v.
    -> per target dict(dropped = sorted uint64 array, rows = per variant dict(N, V, a, k, thr, N2, V2))."""
    covers = [np.unique(np.asarray(c, np.uint64)) for c in covers]
    carries = [np.unique(np.asarray(c, np.uint64)) for c in carries]
    draws = [philox_word0(c, seed) for c in carries]
    out = []
    for t in targets:
        ks = [keep_probability(len(n), len(v), t) for n, v in zip(covers, carries)]
        thr = [threshold(k) for k in ks]
        gone = [c[u >= np.uint64(h)] if h < (1 << 32) else c[:0] for c, u, h in zip(carries, draws, thr)]
        dropped = np.unique(np.concatenate(gone)) if gone else np.zeros(0, np.uint64)
        rows = []
        for n, v, k, h in zip(covers, carries, ks, thr):
            rows.append(dict(N=len(n), V=len(v), a=float(len(v)) / len(n) if len(n) else 0.0, k=k, thr=h,
                             N2=int(len(n) - np.isin(n, dropped).sum()), V2=int(len(v) - np.isin(v, dropped).sum())))
        out.append(dict(target=t, dropped=dropped, rows=rows))
    return out


def variant_state(row) -> str:
    """Why a variant is left alone, or "" (step 2)."""
    if row["V"] == 0:
        return "absent"
    if row["V"] == row["N"]:
        return "every covering barcode carries it: cannot be diluted"
    return "at or below the target already" if row["k"] >= 1.0 else ""


def report_line(v: Variant, t: float, row) -> str:
    a2 = float(row["V2"]) / row["N2"] if row["N2"] else 0.0
    state = variant_state(row)
    return "--dsAF %g: %s:%d %s>%s N %d, V %d, a %.6g, k %.6g, N' %d, V' %d, a' %.6g%s" % (
        t, v.chrom, v.pos, v.ref, v.alt, row["N"], row["V"], row["a"], row["k"], row["N2"], row["V2"], a2, " (%s)" % state if state else "")


def unique_idents(texts, what: str):
    """text -> identity of every barcode text; ValueError when two texts share one (the drop is by identity in a run)."""
    ids = {t: fnv64(t) for t in texts}
    if len(set(ids.values())) != len(ids):
        raise ValueError("--dsAF: two barcodes of %s share a 64-bit identity (FNV-1a of the text): the file is refused" % what)
    return ids


def plan_file(path: str, variants, targets, seed: int, fasta=None):
    """Steps 1-4 of a file -> (ident of every placed barcode text, titrate()'s result)."""
    ids = unique_idents(bamio.placed_barcodes(path), path)
    counted = count_file(path, variants, fasta)
    arr = lambda texts: np.array([ids[t] for t in texts], np.uint64)
    return ids, titrate([arr(c) for c, _ in counted], [arr(sorted(k)) for _, k in counted], targets, seed)


def main(args) -> int:
    if args.runPath:
        os.chdir(args.runPath)
    variants = parse_variants(args.variants)
    targets = parse_targets(args.af)
    if len(targets) != 1:
        raise SystemExit("--af: one target allele fraction per output BAM, got %r" % args.af)
    fasta = None
    if args.refGenome:
        from .. import fasta as _fasta
        fasta = _fasta.FastaFile(args.refGenome)
    ids, (res,) = plan_file(args.inBam, variants, targets, args.seed, fasta)
    for v, row in zip(variants, res["rows"]):
        print(report_line(v, targets[0], row))
    dropped = set(int(x) for x in res["dropped"])
    header, recs = bamio.iter_raw_records(args.inBam)
    n = [0]

    def chosen():
        for tid, q, raw in recs:
            bc = barcode_of(q)
            if bc is None or ids.get(bc, fnv64(bc)) not in dropped:
                n[0] += 1
                yield raw
    bamio.write_raw(args.outBam, header, chosen())
    return n[0]


def build_parser():
    parser = argparse.ArgumentParser(description="Dilute listed variants to a target allele fraction by dropping barcodes that carry them")
    parser.add_argument("--runPath", default=None, help="path to working directory")
    parser.add_argument("--inBam", default=None, required=True, help="Input BAM file (coordinate-sorted)")
    parser.add_argument("--outBam", default=None, required=True, help="Output BAM file")
    parser.add_argument("--variants", default=None, required=True, help="variants: VCF lines, or `chrom pos ref alt` (tab-separated)")
    parser.add_argument("--af", default=None, required=True, help="target allele fraction in (0, 1)")
    parser.add_argument("--seed", type=int, default=1234567, help="Seed of the barcode draw")
    parser.add_argument("--refGenome", default=None, help="indexed FASTA: a listed deletion is then compared by its deleted letters as "
                                                          "the caller writes them (the reference's), not by their count")
    return parser


if __name__ == "__main__":
    main(build_parser().parse_args())
