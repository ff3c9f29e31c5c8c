"""Cost of in-run read down-sampling within barcodes (--dsRpb; dev tool, GPU box).

(1) host: devplanes.reference_read_rules on a synthetic 2000-locus file at 58,000x (scripts/ds_titration_perf.make_file) - the pass
    over the whole file's read names (inflate + names, grouping, probKeep, the identities) and one draw per target (one Python 2
    random() per non-first name of a barcode), timed part by part.
(2) device: smc_select_alignments_keyed at the read level (a host mask over read-name ids, the kept ids renumbered) on one synthetic
    C3-shaped run, next to the barcode-level rule and smc_build_planes_w16 on the same run (scripts/ds_titration_perf.kernel_costs).
(3) wall time in process on the same file: the command line with --dsRpb and three targets, against the full run plus, per target,
    tools.ds_reads_within_mt (the BAM rewrite) and the command line with --rpb r on the BAM it wrote.

usage: ds_rpb_perf.py [c3_loci] [n_loci] [depth] [out.json]   -> one JSON line (also written to out.json when given)"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import ds_titration_perf  # noqa: E402
from smcounter_amd import _lib, bamio, cli, devplanes, synth  # noqa: E402
from smcounter_amd.engine import DevBuf, Engine  # noqa: E402
from smcounter_amd.py2compat import py2_dict_order  # noqa: E402
from smcounter_amd.tools import ds_reads_within_mt as rw  # noqa: E402

TARGETS = (2.0, 5.0, 10.0)
SEED = 1234567


def host_costs(bam, targets):
    out = {}
    t0 = time.perf_counter()
    qn = bamio.placed_qnames(bam)
    t1 = time.perf_counter()
    per_bc, order = rw.group_reads(qn)
    t2 = time.perf_counter()
    names = [q for bc in order for q in per_bc[bc]]
    idents = devplanes.fnv64_array(names)
    t3 = time.perf_counter()
    py2 = py2_dict_order(order)
    draws = []
    for r in targets:
        t = time.perf_counter()
        rw.draw_reads(per_bc, py2, rw.prob_keep(per_bc, r), SEED)
        draws.append(round(time.perf_counter() - t, 3))
    t4 = time.perf_counter()
    rules = devplanes.reference_read_rules(bam, targets, [None] * len(targets), SEED)
    t5 = time.perf_counter()
    out.update(records=len(qn), read_names=len(names), barcodes=len(order), names_s=round(t1 - t0, 3), group_s=round(t2 - t1, 3),
               idents_s=round(t3 - t2, 3), draw_s_per_target=draws, parts_s=round(t4 - t0, 3), reference_read_rules_s=round(t5 - t4, 3),
               prob_keep=[round(r.prob_keep, 6) for r in rules], kept_names=[len(r.kept) for r in rules])
    assert len(idents) == len(names)
    return out


def read_level_costs(eng, c3_loci, reps=20):
    L = eng.L
    cfg = synth.CONFIGS["C3"]
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, c3_loci, P)
    n, nl, lo, npr = len(A["aln"]), int(A["nl"]), int(A["start0"]), int(A["n_pair"])
    up = devplanes.upload_run(eng, A, "A" * nl)
    mask = np.random.default_rng(1).random(npr) < 0.5
    sel, counts, d_orig = devplanes.select_run(eng, up, A, lo, mask=mask, level="read")         # (warm: scratch, buffers)
    words = np.packbits(mask, bitorder="little")
    words = np.concatenate([words, np.zeros((-len(words)) % 4 + 4, np.uint8)]).view(np.uint32)
    d_rule = DevBuf(eng, words.nbytes + 256).upload(words)
    d_sum = DevBuf(eng, 256)
    L.smc_device_sync(eng.ctx)
    t0 = time.perf_counter()
    for _ in range(reps):
        _lib.check(L.smc_select_alignments_keyed(eng.ctx, up.aln.data_ptr(), n, None, nl, lo, 1, int(A["n_bc"]), npr, d_rule.data_ptr(), None, npr,
                                                 ctypes.c_uint64(0), 1.0, sel.aln.data_ptr(), d_orig.data_ptr(), sel.loc.data_ptr(),
                                                 d_sum.data_ptr(), None), "smc_select_alignments_keyed")
    L.smc_device_sync(eng.ctx)
    ms = (time.perf_counter() - t0) * 1e3 / reps
    k = sel.n_aln
    out = {"c3_loci": nl, "alignments": n, "read_ids": npr, "ms": round(ms, 4), "kept": k,
           "GBps": round((2 * 36 * n + 40 * k) / (ms * 1e-3) / 1e9, 1)}
    sel.free(shared=False); d_orig.free(); d_rule.free(); d_sum.free(); up.free()
    return out


def wall(tmp, bam, fa, bed, depth, targets):
    base = dict(bamFile=bam, bedTarget=bed, mtDepth=depth, rpb=8.6, refGenome=fa)
    run = lambda prefix, **kw: cli.main(dict(base, outPrefix=os.path.join(tmp, prefix), **kw))
    run("warm")
    t0 = time.perf_counter()
    run("ds", dsRpb=",".join("%g" % r for r in targets))
    t_ds = time.perf_counter() - t0
    t0 = time.perf_counter()
    run("full")
    t_full = time.perf_counter() - t0
    t_tool = t_cli = 0.0
    for r in targets:
        out = os.path.join(tmp, "rpb%g.bam" % r)
        t0 = time.perf_counter()
        rw.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, rpb=r, seed=SEED))
        bamio.write_bai(out)
        t1 = time.perf_counter()
        cli.main(dict(base, bamFile=out, rpb=r, outPrefix=os.path.join(tmp, "ref%g" % r)))
        t_tool += t1 - t0
        t_cli += time.perf_counter() - t1
    same = all(open(os.path.join(tmp, "ds.dsRpb%g.smCounter.all.txt" % r), "rb").read() ==
               open(os.path.join(tmp, "ref%g.smCounter.all.txt" % r), "rb").read() for r in targets)
    return {"dsRpb_s": round(t_ds, 3), "full_s": round(t_full, 3), "ds_reads_within_mt_tool_s": round(t_tool, 3),
            "cli_on_ds_bams_s": round(t_cli, 3), "workflow_s": round(t_full + t_tool + t_cli, 3), "all_txt_equal_the_workflow": same}


def main():
    a = sys.argv[1:]
    c3_loci = int(a[0]) if a else 190000
    n_loci = int(a[1]) if len(a) > 1 else 2000
    depth = int(a[2]) if len(a) > 2 else 58000
    res = {}
    eng = Engine(0)
    res["kernel_barcode_level_and_builder"] = ds_titration_perf.kernel_costs(eng, c3_loci)
    res["kernel_read_level"] = read_level_costs(eng, c3_loci)
    eng.close()
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    bam, fa, bed, n_rec = ds_titration_perf.make_file(tmp, n_loci, depth)
    res["file"] = {"loci": n_loci, "depth": depth, "records": n_rec, "bytes": os.path.getsize(bam), "make_s": round(time.perf_counter() - t0, 1)}
    res["host"] = host_costs(bam, TARGETS)
    res["wall"] = wall(tmp, bam, fa, bed, max(1, depth // 60), TARGETS)
    line = json.dumps(res)
    print(line)
    if len(a) > 3:
        with open(a[3], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
