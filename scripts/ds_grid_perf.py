"""Cost of --dsGrid (dev tool, GPU box).

(1) the synthetic 2000-locus file at 58,000x (scripts/ds_titration_perf.make_file): the file-wide table (devplanes.philox_read_rules),
    then the device time of smc_read_groups_counts_frac (three fractions) and of one smc_read_groups_masks_grid launch (the 3 x 3
    cells) over every read-name identity of the file, the device synchronised around each loop.
(2) C3-sized: the same two over the keys of a synthetic C3 run's records (the keys ds_rpb_philox_perf.c3_costs feeds the table).
(3) wall time in process on the file of (1): a 3 x 3 --dsGrid run with each pair of samplers and the same run without --dsGrid, against
    the full run plus the nine three-step workflows (tools.ds_mt, tools.ds_reads_within_mt on its BAM, the command line on that BAM);
    the cells' .all.txt / .cut.txt compared with the workflows'.
(4) the device memory a cell adds: the arrays of one _DsBatch at the smallest batch capacity the command line sizes (16-bit read words,
    no raw-field planes, as the command line builds), and per read slot.

usage: ds_grid_perf.py [c3_loci] [n_loci] [depth] [out.json]   -> one JSON line (also written to out.json when given)"""
import argparse
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
from smcounter_amd import bamio, cli, devplanes, synth  # noqa: E402
from smcounter_amd.engine import DevBuf, Engine  # noqa: E402
from smcounter_amd.py2compat import py2_round  # noqa: E402
from smcounter_amd.tools import ds_mt, ds_reads_within_mt  # noqa: E402

FRACS = (0.5, 0.25, 0.125)
TARGETS = (2.0, 5.0, 10.0)
SEED = 1234567


def _dev_ms(eng, fn, reps):
    """Mean time of fn() over `reps` calls, the device synchronised before and after the loop (one call first: warm-up)."""
    fn()
    eng.L.smc_device_sync(eng.ctx)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    eng.L.smc_device_sync(eng.ctx)
    return round((time.perf_counter() - t0) * 1e3 / reps, 4)


def grid_costs(eng, groups, name_ids, reps=20):
    """counts_frac and one masks_grid launch over `name_ids` (uint64, distinct names of the table) for the 3 x 3 cells."""
    fthr = [devplanes.frac_threshold(f) for f in FRACS]
    fc = groups.counts_frac(SEED, fthr)
    cells = [(k, r) for k in range(len(FRACS)) for r in TARGETS]
    probs = [1.0 * (r - 1.0) * (fc[k]["one"] + fc[k]["multi"]) / (fc[k]["multi_names"] - fc[k]["multi"]) for k, r in cells]
    bc = [fthr[k] for k, _ in cells]
    rd = [devplanes.read_threshold(p) for p in probs]
    out = {"frac_counts": dict(zip(("%g" % f for f in FRACS), fc)), "prob_keep": [round(p, 6) for p in probs]}
    out["counts_frac_ms"] = _dev_ms(eng, lambda: groups.counts_frac(SEED, fthr), reps)      # (returns after its copy back: synchronous)
    n = len(name_ids)
    n_words = (n + 31) // 32
    d_id = DevBuf(eng, 8 * n + 256).upload(np.ascontiguousarray(name_ids, np.uint64))
    d_m = DevBuf(eng, 4 * n_words * len(cells) + 256)
    out["masks_grid_ms"] = _dev_ms(eng, lambda: groups.masks_grid(d_id.data_ptr(), n, SEED, bc, rd, d_m.data_ptr()), reps)
    m = d_m.download(np.uint32, n_words * len(cells)).reshape(len(cells), -1)
    out["mask_kept_ids"] = [int(np.unpackbits(w.view(np.uint8), bitorder="little")[:n].sum()) for w in m]
    out["kept_grid"] = groups.kept_grid(SEED, bc, rd)
    out["kept_grid_ms"] = _dev_ms(eng, lambda: groups.kept_grid(SEED, bc, rd), reps)
    out["status"] = groups.status()
    out["ids"] = n
    d_id.free(); d_m.free()
    return out


def file_costs(eng, bam):
    rules = devplanes.philox_read_rules(bam, TARGETS, [None] * len(TARGETS), SEED, eng)
    try:
        b = bamio.NativeBam(bam)
        ids = np.unique(np.concatenate([k[:, 0].copy() for _, k in b.name_keys(devplanes.NAME_KEY_CHUNK)]))
        b.close()
        out = grid_costs(eng, rules[0].groups, ids)
        out["counts"] = rules[0].groups.counts
    finally:
        devplanes.close_rules(rules)
    return out


def c3_costs(eng, c3_loci):
    cfg = synth.CONFIGS["C3"]
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, c3_loci, P)
    aln = A["aln"]
    npr = int(A["n_pair"])
    name_id = devplanes.fnv64_array(["p%d" % g for g in range(npr)])
    bc_id = devplanes.fnv64_array(["b%d" % g for g in range(int(A["n_bc"]))])
    keys = np.stack([name_id[aln["pair_gid"]], bc_id[aln["bc_gid"]],
                     (aln["pair_gid"].astype(np.uint64) & np.uint64(0xFFFFFFFF)) | (aln["bc_gid"].astype(np.uint64) << np.uint64(32))], 1)
    g = devplanes.ReadGroups(eng)
    try:
        g.add(keys, 0)
        c = g.finish()
        out = {"c3_loci": int(A["nl"]), "records": len(aln), "read_ids": npr, "barcodes": int(A["n_bc"]), "counts": c}
        out.update(grid_costs(eng, g, name_id))
    finally:
        g.close()
    return out


def wall(tmp, bam, fa, bed, depth):
    base = ["--bamFile=%s" % bam, "--bedTarget=%s" % bed, "--mtDepth=%d" % depth, "--rpb=8.6", "--refGenome=%s" % fa]
    parser = cli.build_parser()

    def run(prefix, *extra):
        t0 = time.perf_counter()
        cli.main(parser.parse_args(base + ["--outPrefix=%s" % os.path.join(tmp, prefix)] + list(extra)))
        return round(time.perf_counter() - t0, 3)
    ds = ["--dsMT=" + ",".join("%g" % f for f in FRACS), "--dsRpb=" + ",".join("%g" % r for r in TARGETS), "--dsSeed=%d" % SEED]
    run("warm")
    res = {"full_s": run("full"), "dsMT_dsRpb_s": run("nogrid", *ds), "grid_reference_s": run("grid", "--dsGrid", *ds),
           "grid_philox_s": run("gridp", "--dsGrid", "--dsSampler=philox", "--dsRpbSampler=philox", *ds)}
    t_mt = t_rpb = t_cli = 0.0
    same = True
    for f in FRACS:
        out_f = os.path.join(tmp, "ds%g.bam" % f)
        t0 = time.perf_counter()
        ds_mt.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out_f, pct=f, seed=SEED))
        bamio.write_bai(out_f)
        t_mt += time.perf_counter() - t0
        d = max(1, int(py2_round(f * depth)))
        for r in TARGETS:
            out_r = os.path.join(tmp, "ds%g_rpb%g.bam" % (f, r))
            t0 = time.perf_counter()
            ds_reads_within_mt.main(argparse.Namespace(runPath=None, inBam=out_f, outBam=out_r, rpb=r, seed=SEED))
            bamio.write_bai(out_r)
            t1 = time.perf_counter()
            t_rpb += t1 - t0
            wf = "wf.dsMT%g.dsRpb%g" % (f, r)
            cli.main(parser.parse_args(["--bamFile=%s" % out_r, "--bedTarget=%s" % bed, "--mtDepth=%d" % d, "--rpb=%g" % r,
                                        "--refGenome=%s" % fa, "--outPrefix=%s" % os.path.join(tmp, wf)]))
            t_cli += time.perf_counter() - t1
            for s in (".smCounter.all.txt", ".smCounter.cut.txt"):
                same &= open(os.path.join(tmp, "grid.dsMT%g.dsRpb%g%s" % (f, r, s)), "rb").read() == open(os.path.join(tmp, wf + s), "rb").read()
    res.update(ds_mt_tool_s=round(t_mt, 3), ds_reads_tool_s=round(t_rpb, 3), cli_on_written_bams_s=round(t_cli, 3),
               workflow_s=round(res["full_s"] + t_mt + t_rpb + t_cli, 3), cells_equal_the_workflows=bool(same))
    return res


def cell_memory(eng):
    """One cell's _DsBatch at the smallest capacity iter_resident_batches sizes a batch for (4 M reads), 16-bit words, no planes."""
    max_reads = 4_000_000
    cap = max_reads + (max_reads >> 3) + 65536
    d = devplanes._DsBatch(eng, cap, 16, False)
    b = sum(x.nbytes for x in [d.words] + d.uaux)
    d.free()
    return {"cap_slots": cap, "bytes": b, "bytes_per_slot": round(b / cap, 3)}


def main():
    a = sys.argv[1:]
    c3_loci = int(a[0]) if a else 190000
    n_loci = int(a[1]) if len(a) > 1 else 2000
    depth = int(a[2]) if len(a) > 2 else 58000
    res = {"fracs": list(FRACS), "targets": list(TARGETS)}
    eng = Engine(0)
    res["cell_memory"] = cell_memory(eng)
    res["c3"] = c3_costs(eng, c3_loci)
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    bam, fa, bed, n_rec = ds_titration_perf.make_file(tmp, n_loci, depth)
    res["file"] = {"loci": n_loci, "depth": depth, "records": n_rec, "make_s": round(time.perf_counter() - t0, 1)}
    res["file_costs"] = file_costs(eng, bam)
    eng.close()
    res["wall"] = wall(tmp, bam, fa, bed, max(1, depth // 60))
    line = json.dumps(res)
    print(line)
    if len(a) > 3:
        with open(a[3], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
