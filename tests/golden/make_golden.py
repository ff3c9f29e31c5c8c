"""Generate the golden input/output vectors under tests/golden/ (BUILD CONTAINER ONLY).

Runs the reference implementation itself (/root/reference/smCounter.py, imported through
oracle/ref_harness.py) on seeded synthetic pileups and stores, per fixture file:
  inputs   - the primary pileup records (smcounter_amd.pileup.PileupBatch) + the fake FASTA,
  params   - the numeric arguments passed to vc(),
  expected - per locus: the exact string vc_wrapper() returned, the unrounded prediction indices
             (PI_A, PI_T, PI_G, PI_C, PI_alt), every (table, oddsratio, pvalue) scipy's fisher_exact
             produced, and whether the allele choice hinged on an unpinnable py2 dict tie.
Usage:  PYTHONHASHSEED=0 python tests/golden/make_golden.py
"""
import dataclasses
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import ref_harness  # noqa: E402
from smcounter_amd import pileup, synth  # noqa: E402
from smcounter_amd.params import VcParams  # noqa: E402


def emit(name, pb, params, chroms):
    res = [{k: v for k, v in r.items() if k != "pileup"} for r in ref_harness.run_reference(pb, params, chroms)]
    assert not any(r["row"].startswith("Exception thrown!") for r in res), name
    pileup.save_npz(os.path.join(HERE, name + ".npz"), pb, params=dataclasses.asdict(params),
                    chroms=chroms, expected=res)
    n_amb = sum(r["tie_ambiguous"] for r in res)
    print("%-14s %4d loci %7d reads  %d tie-ambiguous  %d down-sampled" % (name, pb.n_loci, pb.n_reads, n_amb,
                                                                          sum(r.get("sampled", False) for r in res)))


def with_names(pb, seed):
    """Attach barcode texts (random 12-mers, unique per locus): the reference's down-sampling depends on them."""
    import numpy as np
    rng = np.random.RandomState(seed)
    names = []
    for l in range(pb.n_loci):
        s = pb.locus_slice(l)
        nu = int(pb.umi[s].max()) + 1 if s.stop > s.start else 0
        seen = set()
        while len(seen) < nu:
            seen.add("".join(rng.choice(list("ACGT"), 12)))
        names.append(sorted(seen, key=lambda t: rng.rand()))
    return dataclasses.replace(pb, umi_names=names)


def main_downsampled():
    """Loci with more barcodes than the cap: `random.seed(pos); random.sample(bcDict.keys(), ds)` (smCounter.py:
    496-498) runs inside the reference, through the CPython-2.7 emulation of seed(str) / sample / dict order
    that oracle/ref_harness.py binds (py2compat.Py2Random) - unpinned against a real py2 (none available)."""
    for name, seed, n, params in (("stress_ds1", 7, 60, VcParams(mtDepth=3, rpb=8.6, hpLen=8, mtDrop=0)),
                                  ("stress_ds2", 8, 40, VcParams(mtDepth=500, rpb=2.0, hpLen=8, maxMT=5))):
        pb, chroms = synth.generate_stress(n, seed)
        emit(name, with_names(pb, seed), params, chroms)


def main():
    stress = ((1, VcParams(mtDepth=200, rpb=8.6, hpLen=8, mtDrop=1), {}),
              (2, VcParams(mtDepth=100, rpb=2.0, hpLen=6, mtDrop=0, primerDist=2), {}),
              (3, VcParams(mtDepth=1000, rpb=1.2, hpLen=10, minBQ=25, minMQ=20, mismatchThr=4.0), {}),
              (4, VcParams(mtDepth=1000, rpb=5, hpLen=8),
               dict(deep=True, scenarios=("snp", "discord", "snp_sb", "het_ins", "biallelic",
                                          "snp_endcluster"))))
    for seed, params, kw in stress:
        n = 12 if kw else 170
        pb, chroms = synth.generate_stress(n, seed, **kw)
        emit("stress%d" % seed, pb, params, chroms)
    for name, n in (("C2", 64), ("C3", 6), ("C5", 3)):
        cfg = synth.CONFIGS[name]
        pb = synth.generate(cfg, 0, n)
        # only the stretch of the periodic reference the loci can touch
        lo = cfg.start_pos - 64
        seq = "N" * lo + synth.CyclicRef().fetch(cfg.chrom, lo, cfg.start_pos + n + 64)
        emit("synth_" + name, pb, synth.params_for(cfg), {cfg.chrom: seq})


def main_giant():
    """Barcodes with thousands of unpaired fragments: calProb's products (rightP = 0.9^n, smCounter.py:62-77) leave the double
    range near n = 6,700 and the reference's own arithmetic decides what survives - one locus each with a barcode of 4,200
    (above the per-count table, below the underflow), 6,600, 6,800 and 7,400 unpaired reference-allele fragments, a few of
    another allele among them, next to ordinary barcodes."""
    import numpy as np
    from smcounter_amd.pileup import BASE_ALLELES, F_HAS_NM, F_READ1, F_READ2, F_REVERSE, PileupBatch
    chroms = synth.stress_reference()
    seq = chroms["chrT"]
    rng = np.random.Generator(np.random.PCG64(4242))
    cols = {k: [] for k in ("umi", "frag", "flag", "mq", "nm", "n_indel", "left_sp", "qlen", "qalen", "qpos", "indel", "is_del",
                            "allele", "bq")}
    chrom, pos, ref, alleles, off = [], [], [], [], [0]
    for l, giant in enumerate((4200, 6600, 6800, 7400)):
        p = 100 + 37 * l
        r = seq[p - 1]
        rid = BASE_ALLELES.index(r)
        alt = BASE_ALLELES.index([c for c in "ATGC" if c != r][l % 3])
        reads = []
        for f in range(giant):                                    # barcode 0: unpaired fragments, mostly the reference allele
            reads.append((0, f, rid if rng.random() > 0.001 else alt, int(rng.choice([25, 30, 37])), rng.random() < 0.5))
        for u in range(1, 25):                                    # ordinary barcodes, some carrying the other allele
            a = alt if u % 4 == 0 else rid
            for f in range(int(rng.integers(1, 6))):
                pair = rng.random() < 0.5
                reads.append((u, f, a, int(rng.choice([25, 30, 37])), False))
                if pair:
                    reads.append((u, f, a, int(rng.choice([25, 30, 37])), True))
        order = rng.permutation(len(reads))
        umap, fmap = {}, {}
        for i in order:
            u, f, a, q, r2 = reads[int(i)]
            f = fmap.setdefault(u, {}).setdefault(f, len(fmap[u]))       # ids by first appearance in the pileup
            u = umap.setdefault(u, len(umap))
            cols["umi"].append(u); cols["frag"].append(f)
            cols["flag"].append((F_READ2 if r2 else F_READ1) | (F_REVERSE if r2 else 0) | F_HAS_NM)
            cols["mq"].append(60); cols["nm"].append(0); cols["n_indel"].append(0); cols["left_sp"].append(0)
            cols["qlen"].append(120); cols["qalen"].append(120); cols["qpos"].append(int(rng.integers(25, 100)))
            cols["indel"].append(0); cols["is_del"].append(False); cols["allele"].append(a); cols["bq"].append(q)
        chrom.append("chrT"); pos.append(p); ref.append(r); alleles.append(list(BASE_ALLELES)); off.append(len(cols["umi"]))
    dt = dict(umi=np.uint32, frag=np.uint32, flag=np.uint8, mq=np.uint8, nm=np.uint32, n_indel=np.uint32, left_sp=np.uint32,
              qlen=np.uint32, qalen=np.uint32, qpos=np.int32, indel=np.int32, is_del=bool, allele=np.uint8, bq=np.uint8)
    pb = PileupBatch(chrom=chrom, pos=np.array(pos, np.int64), ref=ref, alleles=alleles, read_off=np.array(off, np.int64),
                     **{k: np.array(v, dt[k]) for k, v in cols.items()})
    emit("stress_giant", pb, VcParams(mtDepth=20000, rpb=8.6, hpLen=8, mtDrop=0), chroms)


if __name__ == "__main__":
    if sys.argv[1:] == ["giant"]:
        main_giant()
        sys.exit(0)
    if sys.argv[1:] == ["downsampled"]:
        main_downsampled()
    else:
        main()
        main_downsampled()
