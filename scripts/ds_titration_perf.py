"""Cost of in-run molecule down-sampling (--dsMT; dev tool, GPU box).

(1) smc_select_alignments against smc_build_planes_w16 on one synthetic C3-shaped run (synth.generate_alignments): mean device time
    of each over repeated calls (the device synchronised around each loop), and the bytes the selection moves per alignment.
(2) wall time in process on a synthetic 2000-locus file at 58,000x (the example run's depth): the command line with --dsMT and three
    fractions, against the full run plus, per fraction, tools.ds_mt (the BAM rewrite) and the command line on the BAM it wrote.

usage: ds_titration_perf.py [c3_loci] [n_loci] [depth] [out.json]   -> one JSON line (also written to out.json when given)"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from smcounter_amd import _lib, abi, bamio, cli, devplanes, synth  # noqa: E402
from smcounter_amd.engine import DevBuf, Engine  # noqa: E402
from smcounter_amd.py2compat import py2_round  # noqa: E402
from smcounter_amd.tools import ds_mt  # noqa: E402


def kernel_costs(eng, c3_loci, reps=20):
    L = eng.L
    cfg = synth.CONFIGS["C3"]
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, c3_loci, P)
    n, nl, lo = len(A["aln"]), int(A["nl"]), int(A["start0"])
    up = devplanes.upload_run(eng, A, "A" * nl)
    mask = np.random.default_rng(1).random(int(A["n_bc"])) < 0.5
    ids = devplanes.fnv64_array(["B%d" % g for g in range(int(A["n_bc"]))])
    out = {"c3_loci": nl, "alignments": n}
    for tag, kw in (("mask", dict(mask=mask)), ("philox", dict(idents=ids, frac=0.5, seed=3))):
        sel, counts, d_orig = devplanes.select_run(eng, up, A, lo, **kw)          # (warm: scratch, buffers)
        words = np.packbits(mask, bitorder="little")
        d_rule = DevBuf(eng, 8 * max(1, len(ids)) + 256).upload(ids if tag == "philox" else
                                                               np.concatenate([words, np.zeros((-len(words)) % 4 + 4, np.uint8)]).view(np.uint32))
        d_sum = DevBuf(eng, 256)
        m_ptr, i_ptr = (None, d_rule.data_ptr()) if tag == "philox" else (d_rule.data_ptr(), None)
        L.smc_device_sync(eng.ctx)
        t0 = time.perf_counter()
        for _ in range(reps):
            _lib.check(L.smc_select_alignments(eng.ctx, up.aln.data_ptr(), n, None, nl, lo, m_ptr, i_ptr, int(A["n_bc"]), ctypes.c_uint64(3),
                                               0.5, sel.aln.data_ptr(), d_orig.data_ptr(), sel.loc.data_ptr(), d_sum.data_ptr(), None),
                       "smc_select_alignments")
        L.smc_device_sync(eng.ctx)
        ms = (time.perf_counter() - t0) * 1e3 / reps
        k = sel.n_aln
        out[tag] = {"ms": round(ms, 4), "kept": k,
                    "bytes_per_aln": round((2 * 36 * n + 40 * k + 16 * nl + 12 * nl) / max(1, n), 1),   # two reads of the records, the kept ones + index written, the descriptors
                    "GBps": round((2 * 36 * n + 40 * k) / (ms * 1e-3) / 1e9, 1)}
        sel.free(shared=False); d_orig.free(); d_rule.free(); d_sum.free()
    # the builder on the full run (16-bit words, what the command line runs)
    cap = int(A["n_slots"]) + 64
    words = DevBuf(eng, 2 * cap, walk_output=True)
    uaux = [DevBuf(eng, 4 * (cap + nl + 8192)) for _ in range(3)]
    d_loci = DevBuf(eng, 32 * nl + 256)
    xcap = 4 * nl + 4096
    d_x, d_cnt = DevBuf(eng, 20 * xcap), DevBuf(eng, 8)
    cp = abi.c_params(P)
    bi = abi.SmcBuildIn(up.aln.data_ptr(), up.cig.data_ptr(), up.bq.data_ptr(), up.loc.data_ptr(), up.ref.data_ptr(), lo, nl, A["n_bc"],
                        A["n_pair"], int(A["loc"]["n"].max()), n, up.loc_host.ctypes.data)
    call = lambda: _lib.check(L.smc_build_planes_w16(eng.ctx, ctypes.byref(cp), ctypes.byref(bi), 0, 0, words.data_ptr(), uaux[0].data_ptr(),
                                                      uaux[1].data_ptr(), uaux[2].data_ptr(), d_loci.data_ptr(), d_x.data_ptr(), xcap,
                                                      d_cnt.data_ptr(), None), "smc_build_planes_w16")
    call()
    L.smc_device_sync(eng.ctx)
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    L.smc_device_sync(eng.ctx)
    out["build_w16_ms"] = round((time.perf_counter() - t0) * 1e3 / reps, 4)
    up.free()
    return out


def make_file(tmp, n_loci, depth, rpu=60, RL=120):
    """A coordinate-sorted amplicon-like BAM: barcodes of `rpu` reads around random centres (as scripts/e2e_perf.py makes)."""
    rng = np.random.Generator(np.random.PCG64(11))
    span = n_loci + 2 * RL
    Lr = span + 2000
    ref = "".join(rng.choice(list("ACGT"), size=Lr))
    fa = os.path.join(tmp, "ref.fa")
    with open(fa, "w") as fh:
        fh.write(">chrE\n" + "".join(ref[i:i + 60] + "\n" for i in range(0, Lr, 60)))
    n_umi = max(1, depth * span // RL // rpu)
    recs = []
    for u in range(n_umi):
        c = int(rng.integers(1000 - RL, 1000 + n_loci))
        umi = "".join(rng.choice(list("ACGT"), size=12))
        for f in range(rpu // 2):
            start = max(0, c + int(rng.integers(-20, 20)))
            for mate in (0, 1):
                pos = start + (0 if mate == 0 else int(rng.integers(0, 30)))
                recs.append(dict(tid=0, pos=pos, qname="i:1:r%d_%d:NN:%s:x" % (u, f, umi), flag=(0x40 if mate == 0 else 0x90) | 1,
                                 mapq=60, cigar=[(0, RL)], seq=ref[pos:pos + RL], qual=[37] * RL, nm=0))
    recs.sort(key=lambda r: r["pos"])
    bam = os.path.join(tmp, "big.bam")
    bamio.write_bam(bam, [("chrE", Lr)], recs)
    bamio.write_bai(bam)
    bed = os.path.join(tmp, "t.bed")
    with open(bed, "w") as fh:
        fh.write("chrE\t1000\t%d\n" % (1000 + n_loci))
    return bam, fa, bed, len(recs)


def wall(tmp, bam, fa, bed, depth, fracs):
    base = dict(bamFile=bam, bedTarget=bed, mtDepth=depth, rpb=8.6, refGenome=fa)
    run = lambda prefix, **kw: cli.main(dict(base, outPrefix=os.path.join(tmp, prefix), **kw))
    run("warm")
    t0 = time.perf_counter()
    run("ds", dsMT=",".join("%g" % f for f in fracs))
    t_ds = time.perf_counter() - t0
    t0 = time.perf_counter()
    run("full")
    t_full = time.perf_counter() - t0
    t_tool = t_cli = 0.0
    for f in fracs:
        out = os.path.join(tmp, "ds%g.bam" % f)
        t0 = time.perf_counter()
        ds_mt.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, pct=f, seed=1234567))
        bamio.write_bai(out)
        t1 = time.perf_counter()
        cli.main(dict(base, bamFile=out, mtDepth=max(1, int(py2_round(f * depth))), outPrefix=os.path.join(tmp, "ref%g" % f)))
        t_tool += t1 - t0
        t_cli += time.perf_counter() - t1
    same = all(open(os.path.join(tmp, "ds.dsMT%g.smCounter.all.txt" % f), "rb").read() ==
               open(os.path.join(tmp, "ref%g.smCounter.all.txt" % f), "rb").read() for f in fracs)
    return {"dsMT_s": round(t_ds, 3), "full_s": round(t_full, 3), "ds_mt_tool_s": round(t_tool, 3), "cli_on_ds_bams_s": round(t_cli, 3),
            "workflow_s": round(t_full + t_tool + t_cli, 3), "files_equal_the_workflow": same}


def main():
    a = sys.argv[1:]
    c3_loci = int(a[0]) if a else 190000
    n_loci = int(a[1]) if len(a) > 1 else 2000
    depth = int(a[2]) if len(a) > 2 else 58000
    res = {}
    eng = Engine(0)
    res["kernel"] = kernel_costs(eng, c3_loci)
    eng.close()
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    bam, fa, bed, n_rec = make_file(tmp, n_loci, depth)
    res["file"] = {"loci": n_loci, "depth": depth, "records": n_rec, "bytes": os.path.getsize(bam), "make_s": round(time.perf_counter() - t0, 1)}
    depth_mt = max(1, depth // 60)            # (barcodes per locus: the file's reads / rpu)
    res["wall"] = wall(tmp, bam, fa, bed, depth_mt, (0.5, 0.25, 0.125))
    line = json.dumps(res)
    print(line)
    if len(a) > 3:
        with open(a[3], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
