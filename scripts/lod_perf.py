"""Cost of --lod (dev tool, GPU box).

(1) smc_lod_table (Engine.lod_table: launch + copy back, synchronous) for `needed` 6, 8, 17, 32 over depth 0 .. 2 x the matching
    mtDepth (450, 1000, 3612, 8000) against tools.mt_depths_lod.find_lod over the same depths on the host (scipy's CDF through the
    restated zeroin): each side after a warm-up, min / median / max over its repetitions.  Also the largest iteration count of each
    table, the rounded mismatches against the tool (every depth) and max |device root - restated root| unrounded, the restatement
    being tests/lod_restate.py (the kernel's formulation in Python floats).
(2) wall time in process of the command line on the synthetic 2000-locus file at 58,000x (scripts/ds_titration_perf.make_file), with
    and without --lod, alternating: a plain run, and --dsMT 0.5,0.25 --dsRpb 2,4 --dsGrid (nine outputs).  Inside the --lod runs the
    time of lod.run_lods (columns -> tables on the GPU -> per-locus LODs) and of the file writing (lod.write_lod, lod.write_summary)
    is taken apart.

usage: lod_perf.py [n_loci] [depth] [out.json] [host_reps]   -> one JSON line (also written to out.json when given)"""
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ds_titration_perf  # noqa: E402
import lod_restate  # noqa: E402
from smcounter_amd import cli, lod  # noqa: E402
from smcounter_amd.engine import Engine  # noqa: E402
from smcounter_amd.tools import mt_depths_lod as tool  # noqa: E402

MT_DEPTHS = (450, 1000, 3612, 8000)


def _stats(xs, digits):
    return {"min": round(min(xs), digits), "median": round(statistics.median(xs), digits), "max": round(max(xs), digits), "reps": len(xs)}


def table_costs(eng, host_reps, dev_reps=20):
    out = []
    for mt in MT_DEPTHS:
        needed, top = tool.barcodes_needed(mt), 2 * mt
        for _ in range(3):
            roots, iters = eng.lod_table(needed, top)                       # warm-up (the first call also sizes the scratch)
        dev = []
        for _ in range(dev_reps):
            t0 = time.perf_counter()
            eng.lod_table(needed, top)                                      # (returns with the values: the copy back ends it)
            dev.append((time.perf_counter() - t0) * 1e3)
        for d in range(0, top + 1, 50):
            tool.find_lod(d, needed)                                        # warm-up (scipy's first calls)
        host, want = [], None
        for _ in range(host_reps):
            t0 = time.perf_counter()
            want = [tool.find_lod(d, needed) for d in range(top + 1)]
            host.append(time.perf_counter() - t0)
        restated = [lod_restate.find_root(d, needed) for d in range(top + 1)]
        got = [round(float(r), 4) for r in roots]
        out.append({"mtDepth": mt, "needed": needed, "depths": top + 1, "device_ms": _stats(dev, 4), "host_tool_s": _stats(host, 3),
                    "host_over_device": round(statistics.median(host) * 1e3 / statistics.median(dev), 1),
                    "largest_iteration_count": int(iters.max()),
                    "rounded_mismatches_against_the_tool": sum(1 for a, b in zip(got, want) if a != b),
                    "iteration_counts_differing_from_the_restatement": sum(1 for k, (_, i) in zip(iters.tolist(), restated) if k != i),
                    "max_abs_device_root_minus_restated_root": max(abs(float(a) - b) for a, (b, _) in zip(roots, restated))})
    return out


class _Timed(object):
    """Wraps a function of smcounter_amd.lod and adds up the time spent in it."""

    def __init__(self, name):
        self.name, self.fn, self.s = name, getattr(lod, name), 0.0
        setattr(lod, name, self)

    def __call__(self, *a, **kw):
        t0 = time.perf_counter()
        try:
            return self.fn(*a, **kw)
        finally:
            self.s += time.perf_counter() - t0


def wall(tmp, bam, fa, bed, mt_depth, reps):
    base = ["--bamFile=%s" % bam, "--bedTarget=%s" % bed, "--mtDepth=%d" % mt_depth, "--rpb=8.6", "--refGenome=%s" % fa]
    parser = cli.build_parser()
    timers = [_Timed(n) for n in ("run_lods", "write_lod", "write_summary")]

    def run(prefix, *extra):
        for t in timers:
            t.s = 0.0
        t0 = time.perf_counter()
        cli.main(parser.parse_args(base + ["--outPrefix=%s" % os.path.join(tmp, prefix)] + list(extra)))
        return time.perf_counter() - t0, timers[0].s, timers[1].s + timers[2].s
    res = {}
    for tag, extra, n in (("plain", [], reps), ("grid", ["--dsMT=0.5,0.25", "--dsRpb=2,4", "--dsGrid"], max(3, reps // 2))):
        run(tag + "_warm", *extra)
        run(tag + "_warm", "--lod", *extra)
        off, on, tables, writing = [], [], [], []
        for _ in range(n):                                                  # alternating: the two sides share the host's noise
            off.append(run(tag + "_off", *extra)[0])
            w, t, f = run(tag + "_on", "--lod", *extra)
            on.append(w); tables.append(t); writing.append(f)
        same = all(open(os.path.join(tmp, tag + "_off" + s), "rb").read() == open(os.path.join(tmp, tag + "_on" + s), "rb").read()
                   for s in (".smCounter.all.txt", ".smCounter.cut.txt"))
        res[tag] = {"without_lod_s": _stats(off, 4), "with_lod_s": _stats(on, 4),
                    "added_s_median": round(statistics.median(on) - statistics.median(off), 4),
                    "of_it_tables_and_lookup_s": _stats(tables, 4), "of_it_file_writing_s": _stats(writing, 4),
                    "outputs": len(open(os.path.join(tmp, tag + "_on.lod.summary.txt")).read().splitlines()) - 1,
                    "all_and_cut_files_same_with_and_without": bool(same)}
    return res


def main():
    a = sys.argv[1:]
    n_loci = int(a[0]) if a else 2000
    depth = int(a[1]) if len(a) > 1 else 58000
    host_reps = int(a[3]) if len(a) > 3 else 3
    eng = Engine(0)
    res = {"tables": table_costs(eng, host_reps)}
    eng.close()
    tmp = tempfile.mkdtemp()
    bam, fa, bed, n_rec = ds_titration_perf.make_file(tmp, n_loci, depth)
    res["file"] = {"loci": n_loci, "depth": depth, "records": n_rec, "mtDepth": max(1, depth // 60)}
    res["wall"] = wall(tmp, bam, fa, bed, max(1, depth // 60), 7)
    line = json.dumps(res)
    print(line)
    if len(a) > 2:
        with open(a[2], "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
