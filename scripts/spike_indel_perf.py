"""Cost of --spikeIndels (dev tool, GPU box).

On scripts/spike_perf.py's synthetic BAM (128 loci, `n_umi` barcodes x `rpb` reads per locus: 20,000x) with two listed insertions and
two listed deletions, eight loci apart, and three targets:
(1) the pre-pass alone (devplanes.spike_rules over a list with indels: per run decode, upload, smc_allele_carriers, and per target
    smc_spike_indels, the host's restatement of the rewritten records and smc_allele_carriers on the copy), and the time of one
    smc_spike_indels call (devplanes.spike_indel_run: its uploads, the copies of the two pools, count, scan and scatter, the
    statistics, totals, NM' and n_indel' back) over the run that holds all the listed positions, the device synchronised around the loop;
(2) wall time in process, medians of 5 alternating repetitions after a warm-up: the run with the flag and the three targets against the
    run without the flags; and, once, the offline workflow the flags replace - a plain run, then for every target tools.spike_variants --indels and a plain run on the BAM it
    wrote; the targets' .all.txt / .cut.txt compared.

usage: spike_indel_perf.py [n_loci] [n_umi] [rpb] [out.json]   -> one JSON line (also written to out.json when given)"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ds_af_restate  # noqa: E402
import ds_restate  # noqa: E402
from smcounter_amd import bamio, cli, devplanes, fasta, synth  # noqa: E402
from smcounter_amd.engine import Engine  # noqa: E402
from smcounter_amd.tools import spike_variants as sv  # noqa: E402

TARGETS = (0.05, 0.02, 0.01)
SEED = 1234567
REPETITIONS = 5


def prepass(eng, bam, fa, variants, P, reps=20):
    ref = fasta.FastaFile(fa)
    devplanes.spike_rules(bam, ref, variants, list(TARGETS), [P] * len(TARGETS), SEED, eng)          # (warm-up)
    t0 = time.perf_counter()
    rules, res = devplanes.spike_rules(bam, ref, variants, list(TARGETS), [P] * len(TARGETS), SEED, eng)
    out = {"prepass_s": round(time.perf_counter() - t0, 4), "rows": [r["rows"] for r in res]}
    chrom = variants[0].chrom
    lo, hi = min(v.pos for v in variants) - 1, max(v.pos for v in variants)
    b = bamio.NativeBam(bam)
    A = b.alignments_run(chrom, lo, hi, 1 << 40, P, 0)
    spikes = rules[0].spike
    var, _ = spikes.chrom_variants(chrom, TARGETS[0])
    idents = b.barcode_idents(A["n_bc"])
    nm, n_indel = b.run_mismatches(len(A["aln"]))
    up = devplanes.upload_run(eng, A, "A" * A["nl"])
    seen = {}

    def once():
        got = devplanes.spike_indel_run(eng, up, A, var, spikes.ins[chrom], idents, SEED, P.mismatchThr, nm, n_indel)
        seen["totals"], seen["stats"] = got[2], got[1]
        devplanes.free_spiked(got[0], up)
    once()
    eng.L.smc_device_sync(eng.ctx)
    t0 = time.perf_counter()
    for _ in range(reps):
        once()                                                                                       # (returns after its copies back)
    out["spike_indels_call_ms"] = round((time.perf_counter() - t0) * 1e3 / reps, 4)
    caps = devplanes.spike_indel_caps(A, var)
    out["run"] = {"loci": int(A["nl"]), "alignments": len(A["aln"]), "barcodes": int(A["n_bc"]), "pool_bytes": int(len(A["bq"])),
                  "cigar_words": int(len(A["cig"])), "variants": len(variants), "records_rewritten": [int(x) for x in seen["stats"][:, 0]],
                  "pairs_used": int(seen["totals"][0]), "cigar_words_used": int(seen["totals"][1]), "cap_pairs": int(caps[0]),
                  "cap_cigar_words": int(caps[1])}
    up.free()
    b.close()
    return out


def wall(tmp, bam, fa, bed, vfile, P):
    base = ["--bedTarget=%s" % bed, "--mtDepth=%d" % P.mtDepth, "--rpb=%g" % P.rpb, "--refGenome=%s" % fa]
    parser = cli.build_parser()

    def run(prefix, src, *extra):
        t0 = time.perf_counter()
        cli.main(parser.parse_args(base + ["--bamFile=%s" % src, "--outPrefix=%s" % os.path.join(tmp, prefix)] + list(extra)))
        return round(time.perf_counter() - t0, 3)
    run("warm", bam)
    full, flag = [], []
    for _ in range(REPETITIONS):                                     # (alternating, medians)
        full.append(run("full", bam))
        flag.append(run("sp", bam, "--spikeIndels", "--spikeAF=" + ",".join("%g" % t for t in TARGETS), "--spikeVariants=%s" % vfile,
                        "--dsSeed=%d" % SEED))
    res = {"repetitions": REPETITIONS, "full_s": sorted(full)[REPETITIONS // 2], "spikeIndels_3_targets_s": sorted(flag)[REPETITIONS // 2],
           "full_all_s": full, "spikeIndels_3_targets_all_s": flag}
    t_tool = t_cli = 0.0
    same = True
    for t in TARGETS:
        out = os.path.join(tmp, "sp%g.bam" % t)
        t0 = time.perf_counter()
        sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=SEED, refGenome=fa, indels=True))
        bamio.write_bai(out)
        t_tool += time.perf_counter() - t0
        t_cli += run("wf.spikeAF%g" % t, out)
        for s in (".smCounter.all.txt", ".smCounter.cut.txt"):
            same &= open(os.path.join(tmp, "sp.spikeAF%g%s" % (t, s)), "rb").read() == \
                open(os.path.join(tmp, "wf.spikeAF%g%s" % (t, s)), "rb").read()
    res.update(tool_s=round(t_tool, 3), cli_on_written_bams_s=round(t_cli, 3), workflow_s=round(res["full_s"] + t_tool + t_cli, 3),
               targets_equal_the_workflow=bool(same))
    return res


def pick(fa, loci, first):
    """Two insertions and two deletions, eight loci apart from locus `first` on: GA behind the anchor, three letters gone, one letter
    behind the anchor, two letters gone."""
    genome = fasta.FastaFile(fa)
    out = []
    for k, (ins, n) in enumerate((("GA", 0), (None, 3), ("T", 0), (None, 2))):
        c, p = loci[first + 8 * k]
        letters = genome.fetch(c, p - 1, p + n).upper()
        out.append((c, p, letters[0], letters[0] + ins) if ins else (c, p, letters, letters[0]))
    return out


def main():
    a = sys.argv[1:]
    n_loci = int(a[0]) if a else 128
    n_umi = int(a[1]) if len(a) > 1 else 2000
    rpb = int(a[2]) if len(a) > 2 else 10
    cfg = synth.SynthConfig("SPK", n_loci, n_umi, rpb, 20170502, alt_locus_frac=0.3, alt_af=0.1)
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    bam, fa, loci, P, A = ds_af_restate.synth_bam(tmp, cfg, n_loci)
    bed = ds_restate.write_bed(os.path.join(tmp, "t.bed"), loci)
    vfile = os.path.join(tmp, "v.txt")
    with open(vfile, "w") as fh:
        for c, p, ref, alt in pick(fa, loci, n_loci // 2 - 16):
            fh.write("%s\t%d\t%s\t%s\n" % (c, p, ref, alt))
    variants = sv.parse_variants(vfile, indels=True)
    res = {"targets": list(TARGETS), "file": {"loci": n_loci, "barcodes_per_locus": n_umi, "reads_per_barcode": rpb, "records": len(A["aln"]),
                                              "variants": ["%s:%d %s>%s" % (v.chrom, v.pos, v.ref, v.alt) for v in variants],
                                              "make_s": round(time.perf_counter() - t0, 1)}}
    eng = Engine(0)
    res["prepass"] = prepass(eng, bam, fa, variants, P)
    eng.close()
    res["wall"] = wall(tmp, bam, fa, bed, vfile, P)
    line = json.dumps(res)
    print(line)
    if len(a) > 3:
        with open(a[3], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
