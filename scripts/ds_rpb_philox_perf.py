"""Cost of the read-level philox sampler (--dsRpb --dsRpbSampler philox; dev tool, GPU box).

(1) the synthetic 2000-locus file at 58,000x (scripts/ds_titration_perf.make_file): the native file pass (bamio.NativeBam.name_keys,
    inflate + record walk + hashes), the device grouping (smc_read_groups_add of the chunks + _finish), the kept counts
    (smc_read_groups_kept), devplanes.philox_read_rules end to end, against devplanes.reference_read_rules on the same file.
(2) C3-sized: the table fed with the keys of a synthetic C3 run's records (synth.generate_alignments: its read-name and barcode ids
    hashed), grouped, and one per-run mask launch (smc_read_groups_masks, three targets) over the run's read-name identities.
(3) wall time in process on the file of (1): the command line with --dsRpb 2,5,10 and each sampler, and without it.

usage: ds_rpb_philox_perf.py [c3_loci] [n_loci] [depth] [out.json]   -> one JSON line (also written to out.json when given)"""
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

TARGETS = (2.0, 5.0, 10.0)
SEED = 1234567


def _ms(t0):
    return round((time.perf_counter() - t0) * 1e3, 3)


def file_costs(eng, bam, reps=3):
    L = eng.L
    out = {}
    best = None
    for _ in range(reps):                       # (the first pass pages the file in)
        t0 = time.perf_counter()
        b = bamio.NativeBam(bam)
        chunks = [(f, k.copy()) for f, k in b.name_keys(devplanes.NAME_KEY_CHUNK)]
        b.close()
        t = _ms(t0)
        best = t if best is None else min(best, t)
    out["file_pass_ms"] = best
    out["records"] = int(sum(len(k) for _, k in chunks))
    for _ in range(2):
        g = devplanes.ReadGroups(eng)
        L.smc_device_sync(eng.ctx)
        t0 = time.perf_counter()
        for f, k in chunks:
            g.add(k, f)
        t_add = _ms(t0)
        t1 = time.perf_counter()
        c = g.finish()
        t_fin = _ms(t1)
        st = g.status()
        probs = [1.0 * (r - 1.0) * (c["one"] + c["multi"]) / (c["multi_names"] - c["multi"]) for r in TARGETS]
        thr = [devplanes.read_threshold(p) for p in probs]
        t2 = time.perf_counter()
        kept = g.kept(SEED, thr)
        t_kept = _ms(t2)
        g.close()
    out.update(add_ms=t_add, finish_ms=t_fin, kept_ms=t_kept, status=st, counts=c, prob_keep=[round(p, 6) for p in probs], kept_names=kept)
    t0 = time.perf_counter()
    rules = devplanes.philox_read_rules(bam, TARGETS, [None] * len(TARGETS), SEED, eng)
    out["philox_read_rules_ms"] = _ms(t0)
    devplanes.close_rules(rules)
    t0 = time.perf_counter()
    devplanes.reference_read_rules(bam, TARGETS, [None] * len(TARGETS), SEED)
    out["reference_read_rules_ms"] = _ms(t0)
    return out


def c3_costs(eng, c3_loci, reps=20):
    L = eng.L
    cfg = synth.CONFIGS["C3"]
    P = synth.params_for(cfg)
    A = synth.generate_alignments(cfg, c3_loci, P)
    aln = A["aln"]
    n, npr = len(aln), int(A["n_pair"])
    # the records' keys: identities of "read name" pair_gid and "barcode" bc_gid (distinct texts: distinct ids), check words to match
    name_id = devplanes.fnv64_array(["p%d" % g for g in range(npr)])
    bc_id = devplanes.fnv64_array(["b%d" % g for g in range(int(A["n_bc"]))])
    keys = np.stack([name_id[aln["pair_gid"]], bc_id[aln["bc_gid"]],
                     (aln["pair_gid"].astype(np.uint64) & np.uint64(0xFFFFFFFF)) | (aln["bc_gid"].astype(np.uint64) << np.uint64(32))], 1)
    # (the check word of a name then only has to be a function of its identity: pair_gid, bc_gid below 2^32)
    out = {"c3_loci": int(A["nl"]), "records": n, "read_ids": npr, "barcodes": int(A["n_bc"])}
    for _ in range(2):
        g = devplanes.ReadGroups(eng)
        L.smc_device_sync(eng.ctx)
        t0 = time.perf_counter()
        g.add(keys, 0)
        t_add = _ms(t0)
        t1 = time.perf_counter()
        c = g.finish()
        t_fin = _ms(t1)
        if _ == 0:
            g.close()
    out.update(add_ms=t_add, finish_ms=t_fin, status=g.status(), counts=c)
    probs = [1.0 * (r - 1.0) * (c["one"] + c["multi"]) / (c["multi_names"] - c["multi"]) for r in TARGETS]
    thr = [devplanes.read_threshold(p) for p in probs]
    d_id = DevBuf(eng, 8 * npr + 256).upload(name_id)
    n_words = (npr + 31) // 32
    d_m = DevBuf(eng, 4 * n_words * len(thr) + 256)
    g.masks(d_id.data_ptr(), npr, SEED, thr, d_m.data_ptr())
    L.smc_device_sync(eng.ctx)
    t0 = time.perf_counter()
    for _ in range(reps):
        g.masks(d_id.data_ptr(), npr, SEED, thr, d_m.data_ptr())
    L.smc_device_sync(eng.ctx)
    out["masks_ms"] = round((time.perf_counter() - t0) * 1e3 / reps, 4)
    m = d_m.download(np.uint32, n_words * len(thr)).reshape(len(thr), -1)
    out["mask_kept_ids"] = [int(np.unpackbits(w.view(np.uint8))[:npr].sum()) for w in m]
    out["status_after_masks"] = g.status()
    d_id.free(); d_m.free(); g.close()
    return out


def wall(tmp, bam, fa, bed, depth):
    base = dict(bamFile=bam, bedTarget=bed, mtDepth=depth, rpb=8.6, refGenome=fa)
    run = lambda prefix, **kw: cli.main(dict(base, outPrefix=os.path.join(tmp, prefix), **kw))
    run("warm")
    res = {}
    t0 = time.perf_counter()
    run("full")
    res["full_s"] = round(time.perf_counter() - t0, 3)
    for s in ("reference", "philox"):
        t0 = time.perf_counter()
        run("ds_" + s, dsRpb=",".join("%g" % r for r in TARGETS), dsRpbSampler=s, dsSeed=SEED)
        res["dsRpb_%s_s" % s] = round(time.perf_counter() - t0, 3)
    return res


def main():
    a = sys.argv[1:]
    c3_loci = int(a[0]) if a else 190000
    n_loci = int(a[1]) if len(a) > 1 else 2000
    depth = int(a[2]) if len(a) > 2 else 58000
    res = {"targets": list(TARGETS)}
    eng = Engine(0)
    res["c3"] = c3_costs(eng, c3_loci)
    tmp = tempfile.mkdtemp()
    t0 = time.perf_counter()
    bam, fa, bed, n_rec = ds_titration_perf.make_file(tmp, n_loci, depth)
    res["file"] = {"loci": n_loci, "depth": depth, "records": n_rec, "bytes": os.path.getsize(bam), "make_s": round(time.perf_counter() - t0, 1)}
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
