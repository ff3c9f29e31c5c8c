"""Host restatement of --dsAF (DESIGN.md "--dsAF") from HOST-BUILT pileups: per read its barcode, its allele id and the locus's
allele table, as bamio's readable decoder and pileup.PileupBatch give them - not through tools/ds_allele_fraction.py's own counting,
drawing or arithmetic.  Shared by tests/test_ds_af.py and tests/test_gpu_ds_af.py."""
import collections
import dataclasses
import math
import os
import sys

import numpy as np

from smcounter_amd import bamio, fasta, pileup, synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ds_rpb_philox_restate as rp  # noqa: E402

AF_DOMAIN = 0x64734146
V = collections.namedtuple("V", "chrom pos ref alt key")


def key_of(ref, alt):
    if len(ref) == 1 and len(alt) == 1:
        return alt
    return ("INS|%s|%s" if len(alt) > 1 else "DEL|%s|%s") % (ref, alt)


def variant_of_key(chrom, pos, ref_letter, key):
    """An allele key of a pileup's table -> V (REF / ALT as convertToVcf writes them)."""
    if len(key) == 1:
        return V(chrom, pos, ref_letter, key, key)
    kind, ref, alt = key.split("|")
    return V(chrom, pos, ref, alt, key)


def pileups(bam_path, fa_path, positions):
    """[(chrom, pos)] -> PileupBatch of exactly those loci (the readable decoder)."""
    bam = bamio.BamFile(bam_path)
    try:
        parts = [pb for _, pb in bamio.iter_pileup_batches(bam, fasta.FastaFile(fa_path), [(c, str(p)) for c, p in positions])]
    finally:
        bam.close()
    return pileup.concat(parts)


def counts(pb, l, key):
    """Step 1 at locus l of the batch -> (barcode texts in first-appearance order, reads per barcode, alt per barcode)."""
    sl = pb.locus_slice(l)
    names = pb.umi_names[l]
    umi, allele = pb.umi[sl].astype(np.int64), pb.allele[sl]
    reads = np.bincount(umi, minlength=len(names))
    aid = pb.alleles[l].index(key) if key in pb.alleles[l] else -1
    alt = np.bincount(umi[allele == aid], minlength=len(names)) if aid >= 0 else np.zeros(len(names), np.int64)
    return names, reads, alt


def draw(texts, seed):
    """u(b) of every barcode text."""
    from smcounter_amd import devplanes
    x = devplanes.fnv64_array(list(texts))
    return rp.philox4x32_10(x & np.uint64(0xFFFFFFFF), x >> np.uint64(32), AF_DOMAIN, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)[0]


def restate(bam_path, fa_path, variants, targets, seed):
    """Steps 1-4 -> (per variant (cover texts, carrier set), per target dict(dropped: set of texts, rows: per variant dict))."""
    pb = pileups(bam_path, fa_path, [(v.chrom, v.pos) for v in variants])
    sets = []
    for l, v in enumerate(variants):
        names, reads, alt = counts(pb, l, v.key)
        sets.append(([n for n, r in zip(names, reads) if r > 0], {n for n, r, a in zip(names, reads, alt) if 2 * a > r}))
    every = sorted(set(n for _, car in sets for n in car))
    u = dict(zip(every, (int(x) for x in draw(every, seed)))) if every else {}
    out = []
    for t in targets:
        ks = []
        for cov, car in sets:
            n, v = len(cov), len(car)
            if v == 0 or v == n or v / n <= t:
                ks.append(1.0)
            else:
                ks.append(min(1.0, t * (n - v) / (v * (1.0 - t))))
        thr = [1 << 32 if k >= 1.0 else int(math.floor(k * 4294967296.0)) for k in ks]
        dropped = {b for (cov, car), h in zip(sets, thr) for b in car if u[b] >= h}
        rows = [dict(N=len(cov), V=len(car), k=k, N2=sum(b not in dropped for b in cov), V2=sum(b not in dropped for b in car))
                for (cov, car), k in zip(sets, ks)]
        out.append(dict(target=t, dropped=dropped, rows=rows))
    return sets, out


def pick_variants(bam_path, fa_path, loci, absent=True):
    """Variants the pileups of `loci` really hold: an SNV, an insertion and a deletion where there is one - of each kind the allele
    that the most barcodes carry (then the most reads show), each at a locus of its own - plus, `absent`, an allele nobody carries at
    one more locus."""
    pb = pileups(bam_path, fa_path, loci)
    best = {}
    for l, (c, p) in enumerate(loci):
        for key in pb.alleles[l]:
            if key in ("N", "DEL") or key == pb.ref[l] or (len(key) == 1 and key not in "ATGC"):
                continue
            names, reads, alt = counts(pb, l, key)
            if not alt.sum():
                continue
            score = (int((2 * alt > reads).sum()), int(alt.sum()))
            kind = "SNV" if len(key) == 1 else key[:3]
            if kind not in best or score > best[kind][0]:
                best[kind] = (score, l, key)
    out, used = [], set()
    for kind in ("SNV", "INS", "DEL"):
        if kind in best and best[kind][1] not in used:
            _, l, key = best[kind]
            used.add(l)
            out.append(variant_of_key(loci[l][0], loci[l][1], pb.ref[l], key))
    if absent:
        for l, (c, p) in enumerate(loci):
            if l not in used and pb.ref[l] in "ATGC":
                out.append(V(c, p, pb.ref[l], pb.ref[l] + "GATTACAGATTACA", "INS|%s|%sGATTACAGATTACA" % (pb.ref[l], pb.ref[l])))
                break
    return out


def write_variants(path, variants, vcf=False):
    with open(path, "w") as fh:
        fh.write("# listed variants\n")
        for v in variants:
            fh.write(("%s\t%d\t.\t%s\t%s\t.\t.\t.\n" if vcf else "%s\t%d\t%s\t%s\n") % (v.chrom, v.pos, v.ref, v.alt))
    return path


SYNTH_CFG = synth.SynthConfig("AF", 64, 150, 6, 20170501, alt_locus_frac=0.3, alt_af=0.2)


def synth_bam(tmp, cfg=SYNTH_CFG, n_loci=64):
    """A synthetic BAM whose planted per-molecule variants lie well above the targets -> (bam, fasta, loci, VcParams, A)."""
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, n_loci, P, nthreads=2)
    bam, fa = os.path.join(tmp, "synth.bam"), os.path.join(tmp, "synth.fa")
    chrom, p0, p1 = synth.alignments_to_bam(A, bam, 0, n_loci, fa)
    return bam, fa, [(chrom, p) for p in range(p0, p1 + 1)], P, A


def planted(bam_path, fa_path, loci, min_frac=0.1, limit=6):
    """The planted transitions of a synthetic BAM: loci where a non-reference letter holds at least `min_frac` of the reads."""
    pb = pileups(bam_path, fa_path, loci)
    out = []
    for l, (c, p) in enumerate(loci):
        sl = pb.locus_slice(l)
        cnt = np.bincount(pb.allele[sl], minlength=len(pb.alleles[l]))
        for aid in np.argsort(-cnt).tolist():
            key = pb.alleles[l][aid]
            if len(key) == 1 and key in "ATGC" and key != pb.ref[l] and cnt[aid] >= min_frac * max(1, cnt.sum()):
                out.append(V(c, p, pb.ref[l], key, key))
                break
        if len(out) >= limit:
            break
    return out


def raw_records(path):
    _, recs = bamio.iter_raw_records(path)
    return [(q, raw) for _, q, raw in recs]
