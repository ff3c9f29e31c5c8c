"""Host-side pieces (no GPU): py2 emulation, feature extraction, HP/LowC, row formatting against
the reference's own example output, locus sharding, the C ABI's exported symbols."""
import ctypes
import os
import re

import dataclasses

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden_files, load_golden
from smcounter_amd import _lib, abi, dist, features, hpregion, py2compat, rows, synth
from smcounter_amd.params import VcParams


def test_py2_round_and_str():
    assert py2compat.py2_round(0.03125, 4) == 0.0313 and round(0.03125, 4) == 0.0312
    assert py2compat.py2_round(0.5) == 1.0 and py2compat.py2_round(1.5) == 2.0 and py2compat.py2_round(2.5) == 3.0
    assert py2compat.py2_round(2.675, 2) == 2.67          # binary value is below the tie
    assert py2compat.py2_str_float(10892.58) == "10892.58"
    assert py2compat.py2_str_float(0.0) == "0.0" and py2compat.py2_str_float(1e-05) == "1e-05"
    assert py2compat.py2_str_float(123456789.123456) == "123456789.123"
    assert py2compat.py2_str(7) == "7"


def test_py2_dict_order_of_allele_keys():
    # slots under the unrandomised py2 string hash
    assert py2compat.py2_dict_order(["A", "T", "G", "C"]) == ["A", "C", "T", "G"]
    assert py2compat.py2_dict_order(["T", "G", "C", "A", "N"]) == ["A", "C", "T", "G", "N"]
    assert py2compat.py2_dict_order(["A", "T", "G", "C", "N", "DEL"]) == ["A", "C", "G", "N", "DEL", "T"]
    assert py2compat.py2_str_hash("A") & 7 == 0 and py2compat.py2_str_hash("T") & 31 == 21


def test_threshold_and_smt_and_ds():
    P = VcParams(mtDepth=3612, rpb=8.6)
    assert P.ds == 7224 and P.smt == 4.0
    assert VcParams(rpb=1.2).smt == 2.0 and VcParams(rpb=2.9).smt == 3.0
    assert VcParams(mtDepth=10, maxMT=7).ds == 7


def _check_layout(db, l, P_LAYOUT):
    """Reads of a locus: sorted barcode-major, fragment slots contiguous per barcode, umi_start consistent, read
    classes consistent with the raw fields."""
    o, n = db.read_off(l), int(db.loci["n_reads"][l])
    u, f = db.umi[o:o + n].astype(np.int64), (db.frag[o:o + n] & features.FRAG_SLOT_MASK).astype(np.int64)
    assert (np.diff(u) >= 0).all() and (np.diff(f) >= 0).all()
    # read class (frag bits 27-31) = smc_read_class of the raw fields under the run's parameters
    m, d = db.meta[o:o + n], db.dist[o:o + n]
    fl, bq, mq = (m >> 16) & 0xff, (m >> 8) & 0xff, m >> 24
    kind = (fl >> 3) & 3
    bq_ok = bq >= P_LAYOUT.minBQ
    inc = (bq_ok | (kind == 1)) & (mq >= P_LAYOUT.minMQ) & ((fl & 4) != 0)
    want = features.read_class(kind, (fl & 2) != 0, (fl & 1) != 0, inc, bq_ok, (d & 0xffff) <= 20,
                               (d >> 16) <= P_LAYOUT.primerDist)
    assert np.array_equal(db.frag[o:o + n] >> features.FRAG_CLASS_SHIFT, want)
    nu = int(db.loci["n_umi"][l])
    us = db.umi_start[int(db.loci["umi_off"][l]):int(db.loci["umi_off"][l]) + nu + 1]
    assert us[0] == 0 and us[-1] == n
    tot = 0
    for uu in range(nu):
        run = f[us[uu]:us[uu + 1]]
        assert (u[us[uu]:us[uu + 1]] == uu).all() and len(run) > 0
        assert run.min() == tot and np.array_equal(np.unique(run), np.arange(tot, run.max() + 1))
        tot = int(run.max()) + 1
    assert tot == db.loci["n_frag"][l]


def test_layout_of_native_generator_and_feature_extraction():
    cfg = synth.CONFIGS["C2"]
    db = synth.generate_native(cfg, 0, 50)
    assert (db.loci["n_reads"] == cfg.depth).all() and (db.loci["n_umi"] == cfg.n_umi).all()
    for l in range(db.n_loci):
        _check_layout(db, l, synth.params_for(cfg))
    pb = synth.generate(cfg, 0, 20)
    db2 = features.extract_features(pb, synth.params_for(cfg))
    assert (db2.loci["n_umi"] == cfg.n_umi).all() and db2.n_reads == 20 * cfg.depth
    for l in range(db2.n_loci):
        _check_layout(db2, l, synth.params_for(cfg))
        # the sort is stable: reads of one fragment keep their pileup order
        s_ = pb.locus_slice(l)
        o, n = db2.read_off(l), int(db2.loci["n_reads"][l])
        key = pb.umi[s_].astype(np.int64) * 100000 + pb.frag[s_]
        order = np.argsort(key, kind="stable")
        assert np.array_equal(db2.meta[o:o + n] & 0xff, pb.allele[s_][order])
    pbs, _ = synth.generate_stress(40, 5)
    Ps = VcParams(mtDepth=100, rpb=2, minBQ=25, minMQ=20, primerDist=7)
    dbs = features.extract_features(pbs, Ps)
    for l in range(dbs.n_loci):
        if dbs.loci["n_reads"][l]:
            _check_layout(dbs, l, Ps)


def test_unflagged_first_read_is_an_error():
    pb, _ = synth.generate_stress(3, 11, scenarios=("plain",))
    pb.flag[int(pb.read_off[1])] &= ~np.uint8(3)
    with pytest.raises(features.PileupError):
        features.extract_features(pb, VcParams(mtDepth=10, rpb=2))


def test_hp_and_lowcomp():
    seq = "ACGTTGCA" * 4 + "A" * 10 + "CGTACGTA" * 4
    ref = synth.StringRef({"c": seq})
    p = 32 + 5     # inside the homopolymer
    assert hpregion.is_hp_or_lowcomp("c", p, 8, "A", "G", ref)[0] is True
    assert hpregion.is_hp_or_lowcomp("c", 10, 8, seq[9], "G", ref) == (False, False)
    lc = "ACGTTGCATGCA" * 3 + "AC" * 16 + "GTCAGTCATTGA" * 3
    r2 = synth.StringRef({"c": lc})
    assert hpregion.is_hp_or_lowcomp("c", 36 + 16, 8, lc[36 + 15], "G", r2)[1] is True


def test_convert_to_vcf():
    assert rows.convert_to_vcf("A", "G") == ("A", "G", "SNP")
    assert rows.convert_to_vcf("A", "DEL") == ("A", "DEL", "SDEL")
    assert rows.convert_to_vcf("A", "INS|A|AGG") == ("A", "AGG", "INDEL")
    assert rows.convert_to_vcf("A", "DEL|ACT|A") == ("ACT", "A", "INDEL")


def test_example_all_txt_invariants():
    """The reference's shipped example output pins the arithmetic of the derived columns and the
    number formatting: rebuild them from the integer columns of every row with
    this repo's rounding / printing and compare as strings.  (The file is the copy stored under
    tests/golden/example.)"""
    path = os.path.join(GOLDEN, "example", "example.smCounter.all.txt")
    hdr = None
    n = 0
    for line in open(path):
        f = line.rstrip("\n").split("\t")
        if hdr is None:
            hdr = f
            assert tuple(hdr) == rows.HEADER_ALL
            continue
        if f[-1] == "Zero_Coverage":
            continue
        g = dict(zip(hdr, f))
        dp, umt = int(g["DP"]), int(g["UMT"])
        for b in "ATGC":
            assert py2compat.py2_str(py2compat.py2_round(1.0 * int(g["DP_" + b]) / dp, 4)) == g["AF_" + b]
            assert py2compat.py2_str(py2compat.py2_round(1.0 * int(g["UMT_" + b]) / umt, 4)) == g["UMF_" + b]
        assert py2compat.py2_str(py2compat.py2_round(1.0 * int(g["VDP"]) / dp, 4)) == g["VAF"]
        assert py2compat.py2_str(py2compat.py2_round(1.0 * int(g["VMT"]) / umt, 4)) == g["VMF"]
        n += 1
    assert n == 2000


def test_shard_ranges():
    for n, w in ((10, 3), (200000, 8), (7, 8), (0, 2)):
        spans = [dist.shard_range(n, r, w) for r in range(w)]
        assert spans[0][0] == 0 and spans[-1][1] == n
        assert all(spans[i][1] == spans[i + 1][0] for i in range(w - 1))
        sizes = [b - a for a, b in spans]
        assert max(sizes) - min(sizes) <= 1
    cuts = dist.shard_by_reads([100, 1, 1, 1, 100, 1, 1, 100], 3)
    assert cuts[0] == 0 and cuts[-1] == 8 and cuts == sorted(cuts)


def test_abi_library_loads_and_exports_every_declared_symbol():
    L = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    declared = set(re.findall(r"\b(smc_[a-z_0-9]+)\s*\(", hdr))
    declared -= {"smc_ctx", "smc_plan", "smc_read_class", "smc_class_bits", "smc_param_fingerprint", "smc_class16", "smc_class16_inv",
                 "smc_read_word16", "smc_read_word32"}                                                      # (static inline helpers)
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for name in declared:
        assert getattr(L, name) is not None
    assert L.smc_row_size() == abi.ROW_DTYPE.itemsize == 432
    assert L.smc_locus_size() == features.LOCUS_DTYPE.itemsize == 32
    assert ctypes.sizeof(abi.SmcParams) == 40
    assert L.smc_device_count() >= 0      # counting devices does not initialise the GPU


def test_param_fingerprint_python_matches_the_header():
    """smc_locus.flags bits 1-15 (ABI 2): every producer of a batch states the parameters its planes bake in; the
    Python mirror must equal the header's static inline (compiled here with gcc) on every parameter set."""
    import subprocess
    import tempfile
    from smcounter_amd.params import VcParams
    cases = [(20, 30, 6.0, 2), (25, 30, 6.0, 2), (20, 31, 6.0, 2), (20, 30, 6.5, 2), (20, 30, 6.0, 3), (0, 0, 0.0, 0),
             (93, 255, 100.0, 65535), (-1, 7, 1e-9, -3)]
    src = '#include <stdio.h>\n#include "smcounter_hip.h"\nint main(void){' + "".join(
        'printf("%%d\\n", (int)smc_param_fingerprint(%d, %d, %r, %d));' % c for c in cases) + "return 0;}"
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "fp.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I" + os.path.join(ROOT, "include"), "-o", os.path.join(d, "fp"), os.path.join(d, "fp.c")])
        want = [int(x) for x in subprocess.check_output([os.path.join(d, "fp")]).split()]
    got = [features.param_fingerprint(VcParams(minBQ=a, minMQ=b, mismatchThr=c, primerDist=e)) for a, b, c, e in cases]
    assert got == want and all(0 < x < 32768 for x in got) and len(set(got)) == len(got)
    # every producer writes it: numpy feature extraction, native generator (native decoder: tests/test_bamio.py)
    from smcounter_amd import synth
    cfg = synth.CONFIGS["C2"]
    P = synth.params_for(cfg)
    db = synth.generate_native(cfg, 0, 8, P)
    assert (db.loci["flags"] >> 1 == features.param_fingerprint(P)).all()
    db2 = features.extract_features(synth.generate(cfg, 0, 8), P)
    assert (db2.loci["flags"] >> 1 == features.param_fingerprint(P)).all()


def test_no_gpu_fails_loudly():
    L = _lib.load()
    if L.smc_device_count() > 0:
        pytest.skip("a GPU is present")
    from smcounter_amd import engine
    with pytest.raises(_lib.SmcError):
        engine.Engine(0)


def test_oracle_multithread_wrapper_matches_single_thread():
    import oracle_lib
    from smcounter_amd import synth, abi
    cfg = synth.CONFIGS["C2"]
    P = synth.params_for(cfg)
    db = synth.generate_native(cfg, 0, 300, P)
    a = oracle_lib.call_batch(db, abi.c_params(P), abi.ROW_DTYPE)
    b = oracle_lib.call_batch_mt(db, abi.c_params(P), abi.ROW_DTYPE, 5)
    assert a.tobytes() == b.tobytes()


def test_py2_random_and_downsampling_emulation():
    """CPython-2.7 seed(str) / sample / dict-order emulation.  Pins available without a py2:
    the 64-bit string hash of 'a' (12416037344), the MT19937 stream of an int seed (identical in py2 and py3),
    the pool-vs-set switch of sample(), and self-consistency of the kept set."""
    from smcounter_amd import py2compat as p
    assert p.py2_str_hash("a") == 12416037344 and p.py2_str_hash("") == 0
    assert p.Py2Random(1).random() == 0.13436424411240122
    # a str seeds with its unsigned 64-bit hash, low word first == seeding with that integer
    h = p.py2_str_hash("115256529") & ((1 << 64) - 1)
    assert p.Py2Random("115256529").random() == p.Py2Random(h).random()
    # pool branch (n <= 21): draws int(random() * (n - i)) with swaps
    r1, r2 = p.Py2Random(5), p.Py2Random(5)
    pop = list(range(20))
    got = r1.sample(pop, 3)
    pool, exp = list(pop), []
    for i in range(3):
        j = int(r2.random() * (20 - i)); exp.append(pool[j]); pool[j] = pool[20 - i - 1]
    assert got == exp
    # set branch (n > setsize): rejection on indices
    r1, r2 = p.Py2Random(6), p.Py2Random(6)
    pop = list(range(100))
    got = r1.sample(pop, 4)
    sel, exp = set(), []
    for i in range(4):
        j = int(r2.random() * 100)
        while j in sel:
            j = int(r2.random() * 100)
        sel.add(j); exp.append(pop[j])
    assert got == exp
    names = ["ACGTACGTAC%02d" % i for i in range(40)]
    kept = p.py2_downsample_barcodes("1000", names, 10)
    assert len(kept) == len(set(kept)) == 10 and set(kept) <= set(names)
    assert p.py2_downsample_barcodes("1000", names, 10) == kept            # deterministic
    assert p.py2_downsample_barcodes("1001", names, 10) != kept            # seeded by the position text
    assert p.py2_downsample_barcodes("1000", names[:8], 10) == p.py2_dict_order(names[:8])


def test_downsampled_golden_fixtures_exercise_the_sample():
    import conftest
    from smcounter_amd import abi
    import oracle_lib
    n = 0
    for path in conftest.golden_files():
        if "stress_ds" not in path:
            continue
        pb, db, P, refp, expected = conftest.load_golden(path)
        sampled = np.array([e["sampled"] for e in expected])
        assert sampled.sum() >= 30
        assert ((db.loci["flags"] & 1) != 0).tolist() == sampled.tolist()
        R = oracle_lib.call_batch(db, abi.c_params(P), abi.ROW_DTYPE)
        assert ((R["status"] & abi.ST_DOWNSAMPLED) != 0).tolist() == sampled.tolist()
        assert (R["used_mt"][sampled] == P.ds).all()
        # marks that do not keep exactly ds keys are a contract violation
        bad = dataclasses.replace(db, umi_start=db.umi_start.copy())
        l = int(np.nonzero(sampled)[0][0])
        o = int(db.loci["umi_off"][l])
        k = int(np.nonzero(bad.umi_start[o:o + int(db.loci["n_umi"][l])] >> 31)[0][0])
        bad.umi_start[o + k] &= 0x7fffffff
        R2 = oracle_lib.call_batch(bad, abi.c_params(P), abi.ROW_DTYPE)
        assert R2["status"][l] & abi.ST_BAD_INPUT
        n += 1
    assert n == 2


def test_batch_row_formatter_equals_the_per_row_one():
    import oracle_lib
    n = n_known = 0
    for path in golden_files():
        pb, db, P, refp, expected = load_golden(path)
        R = oracle_lib.call_batch(db, abi.c_params(P), abi.ROW_DTYPE)
        fast = rows.format_rows(R, db, P, refp)                      # numeric columns from libsmc_rowfmt.so
        py = rows.format_rows(R, db, P, refp, native=False)
        slow = [rows.format_row(R[l], db.chrom[l], db.pos[l], db.ref[l], db.alleles[l], P, refp) for l in range(len(R))]
        assert fast == slow
        assert py == slow
        n += len(R)
        # the printer's side band: int(float(PI column)) of the rows it vouches for (raw FILTER ';', numeric POS / VMF) ...
        i_pi = rows.HEADER_ALL.index("PI")
        assert isinstance(fast, rows.RowLines) and len(fast.pred) == len(fast)
        known = 0
        for l, line in enumerate(fast):
            if fast.pred[l] != rows.PRED_NONE:
                f = line.split("\t")
                assert f[-1] == ";" and int(float(f[i_pi])) == fast.pred[l]
                float(f[rows.HEADER_ALL.index("VMF")]); int(f[1])
                known += 1
        n_known += known
        # ... lets the post-filter and the writers skip those rows without changing a byte of what they produce
        from smcounter_amd import postfilter, writers
        import tempfile, os
        chrom = db.chrom[0]
        trf = {chrom: [(int(db.pos[0]) - 1, int(db.pos[len(R) // 2]), "RepT;")]}
        rm = {chrom: [(int(db.pos[len(R) // 3]), int(db.pos[-1]), "RepS;LowC;")]}
        plain = postfilter.apply_repeat_filters(list(fast), trf, rm)
        quick = postfilter.apply_repeat_filters(fast, trf, rm, pred=fast.pred)
        assert quick == plain
        d = tempfile.mkdtemp()
        for thr in (1, 5, 14, 60):
            writers.write_outputs(os.path.join(d, "a"), plain, thr)
            writers.write_outputs(os.path.join(d, "b"), quick, thr, pred=fast.pred)
            for ext in (".smCounter.all.txt", ".smCounter.cut.txt"):
                assert open(os.path.join(d, "a" + ext)).read() == open(os.path.join(d, "b" + ext)).read()
            va = [l for l in open(os.path.join(d, "a.smCounter.cut.vcf")) if not l.startswith("#")]
            vb = [l for l in open(os.path.join(d, "b.smCounter.cut.vcf")) if not l.startswith("#")]
            assert va == vb
    assert n > 600 and n_known > 300


def test_native_number_printer_equals_py2_rounding_and_str():
    """smc_format_tails against py2_round + py2_str on random rows, with the values that separate CPython 2's round
    from this interpreter's: exact ties (odd / 2^(n+1)), values one ulp either side of a tie, negative zero, huge and
    non-finite values (left to the caller), zero denominators."""
    import math
    from smcounter_amd.py2compat import py2_round, py2_str, _py2_round_exact
    rng = np.random.default_rng(77)
    n = 4000
    R = np.zeros(n, abi.ROW_DTYPE)
    for k in ("cvg", "used_mt"):
        R[k] = rng.integers(1, 5000, n)
    for k in ("all_frag", "all_mt", "used_frag", "mt3", "mt5", "mt7", "mt10"):
        R[k] = rng.integers(0, 100000, n)
    for k in ("dp", "umt", "vsm"):
        R[k] = rng.integers(0, 5000, (n, 4))
    # power-of-two denominators make exact quarter / eighth ... fractions: ties of the 4-decimal columns
    R["cvg"][:600] = 2 ** rng.integers(0, 12, 600)
    R["used_mt"][:600] = 2 ** rng.integers(0, 12, 600)
    pi = rng.normal(0, 50, (n, 4))
    ties2 = (2 * rng.integers(-4000, 4000, (n, 4)) + 1) / 8.0                 # odd / 2^3: ties at 2 decimals
    pick = rng.random((n, 4))
    pi = np.where(pick < 0.3, ties2, pi)
    pi = np.where((pick >= 0.3) & (pick < 0.4), np.nextafter(ties2, np.inf), pi)
    pi = np.where((pick >= 0.4) & (pick < 0.5), np.nextafter(ties2, -np.inf), pi)
    pi = np.where((pick >= 0.5) & (pick < 0.55), rng.integers(-3, 3, (n, 4)) / 100.0 * 1.0000000001, pi)
    R["pi"] = pi
    R["pi"][5] = [-0.0, -0.004, 0.005, -0.005]
    R["pi"][6] = [99999999.994, 1e8, -1e9, 12345678.125]
    R["pi"][7] = [np.inf, -np.inf, np.nan, 1.0]
    for c in (0, 1):
        R["cand"]["pi"][:, c] = rng.permuted(pi[:, c])
        for k in ("vdp", "vmt", "vsm"):
            R["cand"][k][:, c] = rng.integers(0, 5000, n)
    R["status"][10] = abi.ST_ZERO_COVERAGE
    R["status"][11] = abi.ST_BAD_INPUT
    R["status"][12] = abi.ST_DOWNSAMPLED                               # still printed
    R["cvg"][13] = 0
    chosen = rng.integers(0, 2, n).astype(np.int8)
    chosen[14] = -1
    tails = rows.format_tails(R, chosen)
    assert len(tails) == n

    def want(l):
        r, c = R[l], R["cand"][l][int(chosen[l])]
        cvg, used = int(r["cvg"]), int(r["used_mt"])
        v = [cvg, int(r["all_frag"]), int(r["all_mt"]), int(r["used_frag"]), used, py2_round(float(c["pi"]), 2),
             int(c["vdp"]), py2_round(1.0 * int(c["vdp"]) / cvg, 4), int(c["vmt"]), py2_round(1.0 * int(c["vmt"]) / used, 4),
             int(c["vsm"])]
        v += [int(x) for x in r["dp"]] + [py2_round(1.0 * int(x) / cvg, 4) for x in r["dp"]]
        v += [int(r["mt3"]), int(r["mt5"]), int(r["mt7"]), int(r["mt10"])]
        v += [int(x) for x in r["umt"]] + [py2_round(1.0 * int(x) / used, 4) for x in r["umt"]]
        v += [int(x) for x in r["vsm"]] + [py2_round(float(x), 2) for x in r["pi"]]
        return "\t".join(py2_str(x) for x in v)

    n_cmp = 0
    for l in range(n):
        if l in (10, 11, 13, 14):
            assert tails[l] == ""
            continue
        if l == 6:
            assert tails[l] == ""                                      # |value| >= 1e8: left to the Python formatter
            continue
        assert tails[l] == want(l), l
        n_cmp += 1
    assert n_cmp == n - 5
    assert tails[5].endswith("-0.0\t-0.0\t0.01\t-0.01")
    assert tails[7].endswith("inf\t-inf\tnan\t1.0")
    # the fast rounding itself against the exact decimal model, on the separating values
    for x in list(ties2[:200].ravel()) + list(np.nextafter(ties2[:200], np.inf).ravel()):
        assert py2_round(float(x), 2) == _py2_round_exact(float(x), 2)


def test_host_libraries_export_every_symbol_of_the_host_header():
    from smcounter_amd import build
    hdr = open(os.path.join(ROOT, "include", "smcounter_host.h")).read()
    declared = set(re.findall(r"\b(smc_[a-z_0-9]+)\s*\(", hdr)) - {"smc_planes_alloc"}
    bam, fmt = ctypes.CDLL(build.build_bam()), ctypes.CDLL(build.build_rowfmt())
    assert len(declared) >= 14
    for name in declared:
        lib = fmt if name in ("smc_rowfmt_stride", "smc_format_tails", "smc_rowfmt_line_stride", "smc_format_lines") else bam
        assert getattr(lib, name) is not None, name


def test_read_class_table_matches_the_definition():
    """The table the kernel uses (built on the host by the library) against a direct evaluation of what a read adds to
    its allele's tallies (smCounter.py:379-459) for every combination of the seven predicates."""
    L = _lib.load()
    tab = (ctypes.c_uint32 * 64)()
    L.smc_class_table(tab)
    tab = np.array(list(tab), np.uint32).reshape(32, 2)
    seen = set()
    for kind in range(4):
        for bits in range(64):
            rev, r2, inc, bq_ok, le20, prle = [(bits >> b) & 1 for b in range(6)]
            if kind == 0 and inc and not bq_ok:
                continue
            c = int(features.read_class(kind, rev, r2, inc, bq_ok, le20, prle))
            assert 0 <= c < 22
            seen.add(c)
            f = [0] * 9
            f[0] = 1
            if kind != 1:
                f[2 if rev else 1] = 1
            if kind == 0:
                f[3] = int(not bq_ok)
                if inc and not r2:
                    f[4], f[5] = 1, le20
                if inc and r2:
                    f[6], f[7], f[8] = 1, le20, prle
            lo, hi = int(tab[c, 0]), int(tab[c, 1])
            got = [(lo >> (5 * t)) & 31 for t in range(6)] + [(hi >> (5 * t)) & 31 for t in range(3)]
            assert got == f, (kind, bits, c)
            assert (hi >> 31) == inc
    assert seen == set(range(22)) and not tab[22:].any()


def test_compare_rows_recognises_ties_with_alleles_outside_the_row():
    """Order flips between PI-tied alleles are unpinned (the reference's own order depends on its dict iteration);
    when the tied allele is a non-candidate indel key its PI is not in the row - the CPU restatement's full PI table
    settles it."""
    a = np.zeros(2, abi.ROW_DTYPE)
    a["max_allele"], a["second_allele"] = 6, 3
    a["pi"][:, 3] = 4.799311822
    a["cand"]["allele"] = -1
    a["cand"]["allele"][:, 0] = 6
    a["cand"]["pi"][:, 0] = 4.96
    for f in ("p_sb", "p_r1", "p_r2", "p_pr"):
        a["cand"][f] = np.nan
    b = a.copy()
    b["second_allele"][0] = 7
    assert abi.compare_rows(a, b) != []                                     # unknown PI of allele 7: reported
    pi_all = np.full((2, 64), np.nan)
    pi_all[:, 3], pi_all[:, 6], pi_all[:, 7] = 4.799311822, 4.96, 4.799311822 + 3e-13
    assert abi.compare_rows(a, b, pi_all=pi_all) == []                      # tie within 1e-9: order not pinned
    pi_all[:, 7] = 4.7
    assert abi.compare_rows(a, b, pi_all=pi_all) != []                      # a real difference is still reported


def _py2_pin_lib():
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle")])
    L = ctypes.CDLL(os.path.join(ROOT, "oracle", "libpy2_pin.so"))
    L.py2pin_str_hash.restype = ctypes.c_int64
    L.py2pin_str_hash.argtypes = [ctypes.c_char_p, ctypes.c_int64]
    return L


def test_py2_emulation_against_the_independent_c_restatement():
    """smcounter_amd/py2compat.py (what the product AND the harnessed reference use for
    `random.seed(pos); random.sample(bcDict.keys(), ds)`, smCounter.py:496-498) against oracle/py2_pin.c, a second
    restatement of CPython 2.7's string hash, dict insertion / resize / key order, MT19937 seeding from a str and
    random.sample, written separately from the published interpreter sources (its own MT19937 too - py2compat leans on this
    interpreter's).  10^4 random barcode sets, sizes concentrated around the resize boundaries of the table (5 -> 6,
    21 -> 22, 85 -> 86, 341 -> 342, 1365 -> 1366 keys) and both branches of sample() (pool swaps up to `setsize`,
    index rejection above)."""
    from smcounter_amd import py2compat as p
    L = _py2_pin_lib()
    rng = np.random.RandomState(20170410)

    def c_strings(strs):
        bs = [s.encode("latin-1") for s in strs]
        arr = (ctypes.c_char_p * len(bs))(*bs)
        lens = (ctypes.c_int64 * len(bs))(*[len(b) for b in bs])
        return arr, lens

    # string hash incl. the empty string and high bytes
    for s in ["", "a", "ACGTACGTAC", "x" * 300, "\xff\xfe", "AAAAAAAAAAAA", "chr17:41243700"] + \
             ["".join(rng.choice(list("ACGT"), int(rng.randint(1, 20)))) for _ in range(300)]:
        b = s.encode("latin-1")
        assert L.py2pin_str_hash(b, len(b)) == p.py2_str_hash(s), s
    # the generator after seed(str): the stream itself
    for s in ["41243700", "1", "", "999999999", "chrS:12"]:
        out = (ctypes.c_double * 50)()
        b = s.encode()
        L.py2pin_random_after_seed(b, len(b), 50, out)
        r = p.Py2Random(s)
        assert list(out) == [r.random() for _ in range(50)], s
    sizes = [1, 2, 4, 5, 6, 7, 20, 21, 22, 23, 84, 85, 86, 87, 340, 341, 342, 343, 1364, 1365, 1366, 1367]
    n_sets = 0
    branch = {"pool": 0, "reject": 0}
    for it in range(10000):
        n = int(rng.choice(sizes)) if it % 4 else int(rng.randint(1, 2500))
        if n > 400 and it % 10:
            n = int(rng.choice(sizes[:14]))                       # keep the bulk small: 10^4 sets in seconds
        L_bc = int(rng.choice([8, 10, 12, 14]))
        seen, names = set(), []
        while len(names) < n:
            s = "".join(rng.choice(list("ACGT"), L_bc))
            if s not in seen:
                seen.add(s)
                names.append(s)
        arr, lens = c_strings(names)
        order = (ctypes.c_int32 * n)()
        assert L.py2pin_dict_order(arr, lens, n, order) == 0
        assert [names[i] for i in order] == p.py2_dict_order(names), (it, n)
        if n >= 2:
            ds = int(rng.randint(1, n))
            pos = str(int(rng.randint(1, 250_000_000)))
            out = (ctypes.c_int32 * ds)()
            pb = pos.encode()
            assert L.py2pin_downsample(pb, len(pb), arr, lens, n, ds, out) == 0
            assert [names[i] for i in out] == p.py2_downsample_barcodes(pos, names, ds), (it, n, ds)
            setsize = 21 + (4 ** np.ceil(np.log(ds * 3) / np.log(4)) if ds > 5 else 0)
            branch["pool" if n <= setsize else "reject"] += 1
        n_sets += 1
    assert n_sets == 10000 and branch["pool"] > 1000 and branch["reject"] > 1000, branch


def test_native_lines_with_several_chromosomes_and_the_pass_rows_sequence():
    """smc_format_lines with rows of several chromosomes in one call (names by id), and postfilter._PassRows - what
    apply_repeat_filters returns on its fast path - as a sequence: items, slices, iteration, equality, its text."""
    import oracle_lib
    from smcounter_amd import postfilter
    pb, db, P, refp, expected = load_golden(golden_files()[0])
    R = oracle_lib.call_batch(db, abi.c_params(P), abi.ROW_DTYPE)
    n = len(R)
    chrom2 = [("chrA" if l % 3 else "chr_other_%d" % (l % 2)) for l in range(n)]
    db2 = dataclasses.replace(db, chrom=chrom2)
    real = {c2: c for c2, c in zip(chrom2, db.chrom)}

    class Renamed(object):                       # the same sequences under the new names
        def get_reference_length(self, chrom):
            return refp.get_reference_length(real[chrom])

        def fetch(self, chrom, start, end):
            return refp.fetch(real[chrom], start, end)
    refp2 = Renamed()
    fast = rows.format_rows(R, db2, P, refp2)
    slow = [rows.format_row(R[l], chrom2[l], db.pos[l], db.ref[l], db.alleles[l], P, refp2) for l in range(n)]
    assert list(fast) == slow
    plain = postfilter.apply_repeat_filters(list(fast), {}, {})
    quick = postfilter.apply_repeat_filters(fast, {}, {}, pred=fast.pred)
    assert isinstance(quick, postfilter._PassRows) and len(quick) == n
    assert quick == plain and plain == quick and not (quick != plain)
    assert [quick[i] for i in range(n)] == plain and quick[2:7] == plain[2:7] and quick[-1] == plain[-1]
    assert quick.text == "\n".join(plain) + "\n"


def test_loci_at_a_printing_boundary_are_reported():
    """rows.pi_boundary_loci: a PI within 1e-8 of a round(PI, 2) half-way point or of the filter gate 5.0 is reported, values a
    little further away are not, and the golden loci (whose strings the GPU tests compare with the reference's) have none."""
    import glob
    import oracle_lib
    from smcounter_amd import abi, features, pileup, rows
    from smcounter_amd.params import VcParams
    r = np.zeros(8, abi.ROW_DTYPE)
    r["cand"]["allele"] = -1
    r["pi"][:] = 1.0
    r["pi"][0, 1] = 12.345 + 4e-9            # half-way point of the second decimal
    r["pi"][1, 2] = 57.995 - 2e-9            # half-way point where int(float(PI)) changes: the writers' threshold
    r["cand"]["allele"][2, 0] = 1; r["cand"]["pi"][2, 0] = 5.0 - 3e-9     # the filter gate
    r["cand"]["allele"][3, 0] = 1; r["cand"]["pi"][3, 0] = 5.0 + 1e-6     # clear of it
    r["pi"][4, 0] = 12.345 + 1e-6            # clear of the half-way point
    r["cand"]["pi"][5, 0] = 5.0              # no such candidate (allele -1)
    r["status"][6] = 1; r["pi"][6, 0] = 0.005   # Zero_Coverage row: nothing printed
    r["cand"]["allele"][7, 1] = 2; r["cand"]["pi"][7, 1] = 0.125 + 1e-10  # second candidate at a half-way point
    assert rows.pi_boundary_loci(r).tolist() == [0, 1, 2, 7]
    n = 0
    for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "s*.npz"))):
        pb, extra = pileup.load_npz(f)
        P = VcParams(**extra["params"])
        got = oracle_lib.call_batch(features.extract_features(pb, P), abi.c_params(P), abi.ROW_DTYPE)
        assert rows.pi_boundary_loci(got).tolist() == []
        n += len(got)
    assert n > 600


def test_bp_heads_bit_trick_against_a_loop_over_the_rows(tmp_path):
    """csrc/bp_masks.h: bp_heads - "the rows that start a run at this locus" by a segmented prefix OR on 32-bit masks, the centre of
    the plane builder's walks (ranks, fragment starts and barcode numbers are popcounts of what it returns) - compiled for the
    host and compared with the definition, row by row, on random columns, run structures and carries."""
    import ctypes, subprocess
    src = tmp_path / "h.cpp"
    src.write_text('#include "bp_masks.h"\nextern "C" uint32_t heads(uint32_t C, uint32_t S, int carried) { return bp_heads(C, S, carried != 0); }\n')
    lib = tmp_path / "h.so"
    subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "smcounter_amd", "csrc"), "-o", str(lib), str(src)])
    L = ctypes.CDLL(str(lib))
    L.heads.restype = ctypes.c_uint32
    L.heads.argtypes = [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_int]
    rng = np.random.default_rng(5)

    def want(C, S, carried):
        H, seen = 0, bool(carried)                  # seen: a row of the current run has covered the locus already
        for r in range(32):
            if r and not (S >> r) & 1:
                seen = False                        # row r starts a new run
            if (C >> r) & 1:
                if not seen:
                    H |= 1 << r
                seen = True
        return H

    cases = [(0, 0, 0), (0xFFFFFFFF, 0xFFFFFFFE, 0), (0xFFFFFFFF, 0xFFFFFFFE, 1), (0xFFFFFFFF, 0, 1), (0x80000001, 0xFFFFFFFE, 0)]
    for _ in range(20000):
        dens = rng.choice([0.05, 0.3, 0.7, 0.97])
        C = int(rng.integers(0, 1 << 32)) & int(sum(1 << b for b in range(32) if rng.random() < rng.choice([0.3, 0.66, 1.0])))
        S = int(sum(1 << b for b in range(1, 32) if rng.random() < dens))
        cases.append((C, S, int(rng.integers(0, 2))))
    for C, S, c in cases:
        assert L.heads(C, S, c) == want(C, S, c), (hex(C), hex(S), c)


def test_pack_words_host_applies_the_slot_contract():
    """devplanes.pack_words_host flags what k_pack_words.inc flags (class 31 = no read class): a slot stepping by two, a first slot
    that is not 0, a last slot that is not n_frag - 1 - at the offending read of that locus and nowhere else."""
    from smcounter_amd import devplanes
    cfg = synth.CONFIGS["C2"]
    P = synth.params_for(cfg)
    good = synth.generate_native(cfg, 0, 32, P)
    w0 = devplanes.pack_words_host(good.meta, good.frag, good.loci)
    o, n = good.read_off(5), int(good.loci["n_reads"][5])
    assert ((w0 >> 27) != 31).all()
    for case in range(3):
        bad = synth.generate_native(cfg, 0, 32, P)
        slot = bad.frag[o:o + n] & np.uint32(features.FRAG_SLOT_MASK)
        cls = bad.frag[o:o + n] & ~np.uint32(features.FRAG_SLOT_MASK)
        if case == 0:
            slot[n // 2:] += 1
            where = [n // 2, n - 1]                  # (the shifted tail also ends one past n_frag - 1)
        elif case == 1:
            slot += 1
            where = [0, n - 1]
        else:
            bad.loci["n_frag"][5] += 1
            where = [n - 1]
        bad.frag[o:o + n] = cls | slot
        w = devplanes.pack_words_host(bad.meta, bad.frag, bad.loci)
        flagged = np.flatnonzero((w >> 27) == 31)
        assert flagged.tolist() == [o + k for k in where]
        keep = np.ones(len(w), bool)
        keep[flagged] = False
        assert np.array_equal(w[keep] & ~np.uint32(1 << 16), w0[keep] & ~np.uint32(1 << 16))


def test_unpack_shard_gives_every_locus_its_own_allele_list():
    from smcounter_amd.pileup import BASE_ALLELES
    base = list(BASE_ALLELES)
    block = dist.pack_shard(np.zeros(3, abi.WIRE_DTYPE), ["A", "C", "G"], [base, base + ["INS|A|AT"], base])
    _, _, alleles = dist.unpack_shard(block)
    alleles[0].append("x")
    assert alleles[2] == base and alleles[1] == base + ["INS|A|AT"]


def test_the_16_bit_read_word_holds_what_the_32_bit_one_does(tmp_path):
    """include/smcounter_hip.h: smc_read_word16 / smc_read_word32 (what the device builder writes and the locus kernels read since
    ABI 7) against each other over every class, allele < 16, quality < 64 and both fragment bits - compiled from the header with
    gcc - and against devplanes' numpy forms of the same (what the tests unpack device-built words with)."""
    import subprocess
    from smcounter_amd import devplanes
    src = tmp_path / "w16.c"
    src.write_text('#include "smcounter_hip.h"\n'
                   'unsigned w16(unsigned w) { return smc_read_word16(w); }\nunsigned w32(unsigned h) { return smc_read_word32(h); }\n'
                   'unsigned c16(unsigned c) { return smc_class16(c); }\nunsigned c16i(unsigned c) { return smc_class16_inv(c); }\n'
                   'unsigned bits(unsigned c) { return smc_class_bits(c); }\n')
    so = str(tmp_path / "w16.so")
    subprocess.check_call(["gcc", "-O1", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-o", so, str(src)])
    C = ctypes.CDLL(so)
    for f in (C.w16, C.w32, C.c16, C.c16i, C.bits):
        f.restype = ctypes.c_uint32; f.argtypes = [ctypes.c_uint32]
    codes = [C.c16(c) for c in range(22)]
    assert len(set(codes)) == 22 and max(codes) < 31 and all(C.c16i(codes[c]) == c for c in range(22))
    assert all(((codes[c] >> 4) & 1) == ((C.bits(c) >> 17) & 1) for c in range(22))          # bit 4 of the code IS incCond
    assert C.c16(22) == 31 and all(C.c16i(x) == 31 for x in range(32) if x not in codes)
    assert (devplanes.class16_table()[:22] == np.array(codes)).all()
    ws = []
    for c in range(22):
        for a in (0, 1, 5, 6, 15):
            for q in (0, 13, 41, 63):
                for nf in (0, 1):
                    ws.append(a | q << 8 | nf << 16 | C.bits(c) | c << 27)
    ws = np.array(ws, np.uint32)
    hs = np.array([C.w16(int(w)) for w in ws], np.uint32)
    assert (hs < 65536).all()
    assert (np.array([C.w32(int(h)) for h in hs], np.uint32) == ws).all()
    real = hs != 0          # (the word of zero - 'A' inside a deletion, not included, quality 0: no read - is the pad behind a locus's last read)
    assert (devplanes.words16_from_32(ws) == hs).all() and (devplanes.words32_from_16(hs.astype(np.uint16))[real] == ws[real]).all()
    assert int((~real).sum()) == 1
    for bad in (16 | C.bits(6) | 6 << 27, 64 << 8 | C.bits(6) | 6 << 27, 3 | 25 << 27):     # allele 16, quality 64, no class
        assert devplanes.words16_from_32(np.array([bad], np.uint32)) is None


def test_16_bit_builder_refuses_a_min_bq_it_has_no_room_for():
    """smc_build_planes_w16: a read inside a deletion carries minBQ as its quality - six bits (no GPU needed: the argument checks
    come first)."""
    L = _lib.load()
    cp = abi.c_params(VcParams(minBQ=64))
    dummy = ctypes.c_void_p(0x1000)
    rc = L.smc_build_planes_w16(None, ctypes.byref(cp), None, 0, 0, dummy, None, None, None, None, None, 0, None, None)
    assert rc != 0 and b"minBQ 64" in L.smc_last_error()
    assert L.smc_build_planes_w16(None, ctypes.byref(cp), None, 0, 0, None, None, None, None, None, None, 0, None, None) != 0     # no words array


class _CountedBuf(object):
    """A stand-in for a device buffer: what download hands back, and how often it and free were called."""

    def __init__(self, data=None, ptr=0):
        self.data, self.downloads, self.freed, self.ptr = data, 0, 0, ptr

    def data_ptr(self):
        return self.ptr

    def download(self, dtype, count, offset_bytes=0):
        self.downloads += 1
        return np.asarray(self.data, dtype)[:count].copy()

    def free(self):
        self.freed += 1


def _kept_run_case(orig, by_read, copy=None):
    """Eight alignments over three barcodes, `orig` the places of the kept ones -> (the adapter, its buffers, the keys the decoder was
    asked for, A, the decoder's identities)."""
    from smcounter_amd import devplanes
    A = dict(aln=np.zeros(8, abi.DEV_ALN_DTYPE), n_bc=3, bq=np.zeros(2 * 64, np.uint8))
    A["aln"]["bc_gid"] = [0, 1, 2, 0, 1, 2, 2, 1]
    idents = np.array([0xA0, 0xB1, 0xC2], np.uint64)
    asked = []

    def key(ai, qpos, indel):
        asked.append((ai, qpos, indel))
        return "K%d" % ai
    bufs = dict(aln=_CountedBuf(), cig=_CountedBuf(), bq=_CountedBuf(), loc=_CountedBuf(), ref=_CountedBuf(),
                orig=_CountedBuf(np.array(orig, np.uint32)))
    sel = devplanes.RunOnDevice(bufs["aln"], bufs["cig"], bufs["bq"], bufs["loc"], bufs["ref"], len(orig))
    kept = devplanes._KeptRun(sel, dict(nl=1), bufs["orig"], A, key, lambda g: "name%d" % g, lambda n: idents[:n], copy=copy, by_read=by_read)
    return kept, bufs, asked, A, idents


def test_kept_run_maps_a_selections_numbering_back_to_the_decoders():
    """devplanes._KeptRun with stand-in buffers: orig_index comes down once and only when asked for; a key is asked for at the original
    index; a read-level selection's barcode ids are the old ones by first kept appearance - and idents() is what the scatter of
    spike_rules' second count (written out here as it stood) gives; a barcode-level selection keeps the ids; free() frees what the
    selection owns."""
    from smcounter_amd import devplanes
    # read level: the first kept alignment belongs to the highest old barcode id - all three kept, then only two
    for orig, new, old_bc in (([2, 3, 4, 7], [0, 1, 2, 2], [2, 0, 1]), ([5, 6, 0], [0, 0, 1], [2, 0])):
        kept, bufs, asked, A, idents = _kept_run_case(orig, True)
        assert bufs["orig"].downloads == 0                                            # nothing asked for, nothing copied
        assert [kept.allele_key(i, 7 + i, -i) for i in range(len(orig))] == ["K%d" % o for o in orig]
        assert asked == [(o, 7 + i, -i) for i, o in enumerate(orig)] and all(type(a[0]) is int for a in asked)
        assert kept.old_bc().tolist() == old_bc
        assert [kept.barcode_name(g) for g in range(len(old_bc))] == ["name%d" % o for o in old_bc]
        assert kept.barcode_name(np.uint32(0)) == "name2"
        assert kept.barcode_idents(3).tolist() == idents[old_bc].tolist() == kept.idents().tolist()
        assert bufs["orig"].downloads == 1                                            # ... however many were asked for
        # the parent's scatter: every new id gets the identity of the old id of a kept alignment that carries it
        orig_a, new_a = np.array(orig, np.uint32), np.array(new, np.uint32)
        of_new = np.zeros(A["n_bc"], np.uint64)
        of_new[new_a.astype(np.int64)] = idents[A["aln"]["bc_gid"][orig_a].astype(np.int64)]
        n = len(kept.idents())
        assert n == len(old_bc) and of_new[:n].tolist() == kept.idents().tolist() and not of_new[n:].any()
        kept.free()
        assert [bufs[x].freed for x in ("aln", "loc", "orig", "cig", "bq", "ref")] == [1, 1, 1, 0, 0, 0]
    # barcode level: the same kept alignments, the decoder's ids
    kept, bufs, asked, A, idents = _kept_run_case([2, 3, 4, 7], False)
    assert kept.old_bc().tolist() == [0, 1, 2] and kept.barcode_name(2) == "name2"
    assert kept.barcode_idents(3).tolist() == idents.tolist() == kept.idents().tolist()
    assert bufs["orig"].downloads == 0
    assert kept.allele_key(1, 0, 0) == "K3" and kept.allele_key(3, 0, 0) == "K7" and bufs["orig"].downloads == 1
    # no selection (the run itself, or a spiked copy): the decoder's index, nothing to copy and nothing to free
    kept, bufs, asked, A, idents = _kept_run_case([], False)
    kept = devplanes._KeptRun(kept.run, A, None, A, lambda ai, q, i: "K%d" % ai, lambda g: "name%d" % g, lambda n: idents[:n])
    assert kept.allele_key(5, 0, 0) == "K5" and kept.barcode_name(1) == "name1" and kept.idents().tolist() == idents.tolist()
    kept.free()
    assert not any(b.freed or b.downloads for b in bufs.values())
    # a selection of an indel copy: the copy's key, at the kept alignment's index in the copy (a record that was not relocated - its
    # pairs stand in the run's own pool - keeps the decoder's answer)
    copy = devplanes.RunOnDevice(_CountedBuf(np.zeros(8, abi.DEV_ALN_DTYPE)), None, _CountedBuf(), None, None, 8)
    kept, bufs, asked, A, idents = _kept_run_case([6, 1], False, copy=copy)
    assert kept.allele_key(0, 4, 2) == "K6" and kept.allele_key(1, 4, 2) == "K1" and asked == [(6, 4, 2), (1, 4, 2)]
    assert copy.aln.downloads == 1 and copy.bq.downloads == 0 and bufs["orig"].downloads == 1


def _copies_case(monkeypatch, stats=None, totals=None):
    """A kept run of 8 alignments with the listed variants 1 and 0 (records 2 and 0 of three), three seeds, and spike_run_copies /
    spike_indel_run_copies patched to hand back counted stand-ins -> (devplanes, the run, its own buffers, the stand-ins, what the
    patched calls were given, the further arguments of the two calls: svar, var_at, seeds, thr, P, variants)."""
    from types import SimpleNamespace as NS
    from smcounter_amd import devplanes
    own = [_CountedBuf(ptr=0x100 * (k + 1)) for k in range(5)]
    run = devplanes.AfRun("chr1", 100, 140, [1, 0], 40, bam=NS(allele_key=lambda ai, q, i: "K%d" % ai, barcode_name=lambda g: "name%d" % g, close=lambda: None),
                          A=dict(n_bc=3, nl=40, n_slots=100, bq=np.zeros(2 * 64, np.uint8)), up=devplanes.RunOnDevice(*own, 8, "loc on the host"),
                          run_ref="A" * 40, idents=np.arange(3, dtype=np.uint64), mism=("NM", "INDEL"))
    made = dict(aln=_CountedBuf(ptr=0x10000), bq=_CountedBuf(ptr=0x20000), cig=_CountedBuf(ptr=0x30000))
    stats = np.array([[[5, 0], [0, 0], [7, 0]]] * 3, np.uint32) if stats is None else stats          # READS 5 at record 0, 7 at record 2
    totals = np.array([[70, 9, 0], [80, 9, 0], [90, 9, 0]], np.uint64) if totals is None else totals
    given = []
    monkeypatch.setattr(devplanes, "spike_run_copies", lambda *a, **k: (given.append((a, k)), (made["aln"], made["bq"], (512, 256), stats))[1])
    monkeypatch.setattr(devplanes, "spike_indel_run_copies",
                        lambda *a, caps=None: (given.append((a, dict(caps=caps))), dict(made, strides=(512, 256, 768), caps=caps or (99, 33),
                                                                                      stats=stats, totals=totals, nm=None, n_indel=None))[1])
    variants = [NS(chrom="chr1", pos=121, ref="A", alt="T"), NS(chrom="chr1", pos=131, ref="A", alt="T")]
    return devplanes, run, own, made, given, ("svar", [2, 0], [11, 12, 13], 1 << 20, VcParams(), variants)


def test_spiked_copies_are_views_at_the_strides_of_the_buffers_they_own(monkeypatch):
    """devplanes._SpikedCopies with stand-in buffers, B = 3: copy c reads its records and pair pool at c x their strides; an SNV copy
    shares the run's CIGAR pool (the object itself), an indel copy has its own at c x its stride and pairs_used from totals[c, 0]; loc
    and ref are the run's; the rewrite is given the run, every seed and one threshold per seed; free() frees what the call returned,
    once, and nothing of the run."""
    devplanes, run, own, made, given, (svar, var_at, seeds, thr, P, variants) = _copies_case(monkeypatch)
    copies = devplanes._SpikedCopies("eng", run, svar, seeds, thr, P)
    assert given == [(("eng", run.up, run.A, svar, run.idents, seeds, [thr] * 3, P.mismatchThr, "NM", "INDEL"), {})]
    assert copies.stats.shape == (3, 3, 2) and copies.strides == (512, 256) and copies.caps is None and copies.totals is None
    for c, r in enumerate(copies.runs):
        assert (r.aln.data_ptr(), r.bq.data_ptr()) == (0x10000 + 512 * c, 0x20000 + 256 * c) and r.aln.word_bits == 32
        assert r.cig is run.up.cig and r.loc is run.up.loc and r.ref is run.up.ref
        assert (r.n_aln, r.loc_host, r.pairs_used) == (8, "loc on the host", None)
    copies.free()
    assert [made[x].freed for x in ("aln", "bq", "cig")] == [1, 1, 0] and not any(b.freed for b in own)
    # the indel rewrite
    devplanes, run, own, made, given, _ = _copies_case(monkeypatch)
    copies = devplanes._SpikedCopies("eng", run, svar, seeds, thr, P, "ins", (120, 40))
    assert given == [(("eng", run.up, run.A, svar, "ins", run.idents, seeds, [thr] * 3, P.mismatchThr, "NM", "INDEL"), dict(caps=(120, 40)))]
    assert copies.strides == (512, 256, 768) and copies.caps == (120, 40)
    for c, r in enumerate(copies.runs):
        assert (r.aln.data_ptr(), r.bq.data_ptr(), r.cig.data_ptr()) == (0x10000 + 512 * c, 0x20000 + 256 * c, 0x30000 + 768 * c)
        assert r.cig is not run.up.cig and r.loc is run.up.loc and r.ref is run.up.ref and r.pairs_used == [70, 80, 90][c]
    assert copies.addresses() == dict(aln=0x10000, cig=0x30000, bq=0x20000, strides=(512, 256, 768), n_aln=8, cap_pairs=120)
    copies.free()
    assert [made[x].freed for x in ("aln", "bq", "cig")] == [1, 1, 1] and not any(b.freed for b in own)


def test_the_two_spike_calls_free_their_copies_once_on_every_way_out(monkeypatch):
    """_spike_rep_call and _scan_call over devplanes._SpikedCopies with stand-in buffers: a READS or an (N, V1) that is not the counts
    call's raises RuntimeError with the text each stage had before there was one class (written out here); a consumer that answers
    NARROW, and the scan's own refusal of a copy that did not fit the caps it passed, end the call too - and on each way out every buffer
    the rewrite returned is freed exactly once, the run's own never."""
    import functools
    case = functools.partial(_copies_case, monkeypatch)

    def freed_once(made, own, indel):
        return [made[x].freed for x in ("aln", "bq", "cig")] == [1, 1, int(indel)] and not any(b.freed for b in own)
    good = [[7, 5]] * 3                                              # READS per copy of variants 1, 0: records 2, 0
    bad = [[7, 5], [7, 6], [7, 5]]
    listed = np.zeros(2, abi.SCAN_LOCUS_DTYPE)
    # READS: the replicate stage names --spikeReps whichever flag is in force, the scan its own
    devplanes, run, own, made, _, (svar, var_at, seeds, thr, P, variants) = case()
    rep = lambda want, *tail: devplanes._spike_rep_call("eng", run, svar, var_at, seeds, thr, want, P, None, variants, 0, "reference", 0, 32, *tail)
    scan = lambda want, check0, *tail: devplanes._scan_call("eng", run, svar, var_at, listed, seeds, thr, want, P, None, variants, 0, "reference",
                                                            0, 32, 0, (), check0, *tail)
    with pytest.raises(RuntimeError) as e:
        rep(bad, [(0.5, P)])
    assert str(e.value) == "--spikeReps: seed 12 at chr1:121: the rewrite touched 5 records, the counts call says 6"
    assert freed_once(made, own, False)
    devplanes, run, own, made, _, _ = case()
    with pytest.raises(RuntimeError) as e:
        scan(bad, None)
    assert str(e.value) == "--spikeScan: seed 12 at chr1:121: the rewrite touched 5 records, the counts call says 6"
    assert freed_once(made, own, False)
    # (N, V1): smc_allele_carriers on the copy says (2, 1) of both variants
    two_one = (np.array([[1, 1, 0]] * 2, bool), np.array([[0, 1, 0]] * 2, bool), None)
    monkeypatch.setattr(devplanes, "allele_carriers_run", lambda *a, **k: two_one)
    monkeypatch.setattr(devplanes, "af_run_variants", lambda *a: ("var", "ins"))
    want = [[(2, 1), (2, 1)], [(2, 1), (2, 2)], [(2, 1), (2, 1)]]
    devplanes, run, own, made, _, _ = case()
    monkeypatch.setattr(devplanes, "_copy_rows", lambda eng, run, variants, n, kept_runs, *a: [kept.free() for kept in kept_runs])
    with pytest.raises(RuntimeError) as e:
        rep(good, (), dict(ins="ins", want=want, want_cells=[]))
    assert str(e.value) == "--spikeIndelReps: seed 12 at chr1:121: the copy holds (N, V1) = (2, 1), the counts call says (2, 2)"
    assert freed_once(made, own, True)
    devplanes, run, own, made, _, _ = case()
    copies = devplanes._SpikedCopies("eng", run, svar, seeds, thr, P, "ins")
    with pytest.raises(RuntimeError) as e:
        copies.check_carriers(1, copies.runs[1], run.A, want[1], "var", "ins", variants, "--spikeIndelReps", " x fraction 0.5")
    assert str(e.value) == "--spikeIndelReps: seed 12 at chr1:121 x fraction 0.5: the copy holds (N, V1) = (2, 1), the counts call says (2, 2)"
    devplanes, run, own, made, _, _ = case()
    with pytest.raises(RuntimeError) as e:
        scan(good, 1, dict(ins="ins", caps=(120, 40), var="var", var_ins="ins", want=want))
    assert str(e.value) == "--spikeScanIndel: seed 12 at chr1:121: the copy holds (N, V1) = (2, 1), the counts call says (2, 2)"
    assert freed_once(made, own, True)
    # NARROW from the consumer
    devplanes, run, own, made, _, _ = case()
    monkeypatch.setattr(devplanes, "_copy_rows", lambda *a: devplanes.NARROW)
    assert rep(good, (), dict(ins="ins", want=[[(2, 1)] * 2] * 3, want_cells=[])) == devplanes.NARROW and freed_once(made, own, True)
    devplanes, run, own, made, _, _ = case()
    monkeypatch.setattr(devplanes, "_build_copies", lambda *a: devplanes.NARROW)
    assert scan(good, None) == devplanes.NARROW and freed_once(made, own, False)
    # a copy that did not fit the caps the scan passed: its own refusal (spike_indel_run_copies raises only without caps)
    devplanes, run, own, made, given, _ = case(totals=np.array([[70, 9, 0], [800, 9, 1], [90, 9, 0]], np.uint64))
    with pytest.raises(_lib.SmcError) as e:
        scan(good, None, dict(ins="ins", caps=(120, 40), var="var", var_ins="ins", want=want))
    assert str(e.value) == "smc_spike_indels_reps: a copy of chr1:101-140 did not fit spike_indel_caps' bounds"
    assert given[0][1] == dict(caps=(120, 40)) and freed_once(made, own, True)


def test_copy_room_is_the_least_of_its_three_limits(monkeypatch):
    """devplanes._copy_room against its formula - max(1, min(SPIKE_MAX_COPIES, SPIKE_REP_BATCH_BYTES // per copy, AF_REP_BATCH_SLOTS //
    (n_slots + nl))) - on runs where each limit binds in turn, for the SNV rewrite's copies and the indel rewrite's, whose caps it
    hands back."""
    from types import SimpleNamespace as NS
    from smcounter_amd import devplanes
    M, BYTES, SLOTS = devplanes.SPIKE_MAX_COPIES, devplanes.SPIKE_REP_BATCH_BYTES, devplanes.AF_REP_BATCH_SLOTS
    assert (M, BYTES, SLOTS) == (64, 1 << 30, 16 << 20)

    def run_of(n_aln, n_pairs, n_slots, nl=40):
        return NS(up=NS(n_aln=n_aln), A=dict(bq=range(2 * n_pairs), n_slots=n_slots), nl=nl)
    seen = []
    monkeypatch.setattr(devplanes, "spike_indel_caps", lambda A, svar: (seen.append(svar), caps)[1])
    #                    n_aln      n_pairs     n_slots     caps                      the room, and the limit that gives it
    for n, n_pairs, n_slots, caps, room in ((8, 64, 100, None, M),
                                            (1_000_000, 50_000_000, 100, None, BYTES // (36_000_000 + 100_000_000)),
                                            (8, 64, 4_000_000, None, SLOTS // 4_000_040),
                                            (8, 64, 100, (70, 12), M),
                                            (1_000_000, 64, 100, (100_000_000, 10_000_000), BYTES // (36_000_000 + 200_000_256 + 40_000_000 + 8_000_000)),
                                            (8, 64, 4_000_000, (70, 12), SLOTS // 4_000_040),
                                            (8, 64, 100, (1 << 30, 12), 1)):
        four = caps is not None
        per_copy = sum(devplanes.spike_indel_copy_strides(n, *caps)) + 8 * n if four else sum(devplanes.spike_copy_strides(n, n_pairs))
        limits = (M, BYTES // per_copy, SLOTS // (n_slots + 40))
        assert devplanes._copy_room(run_of(n, n_pairs, n_slots), "svar", four) == (max(1, min(limits)), caps)
        assert max(1, min(limits)) == room and sorted(limits)[0] < sorted(limits)[1]          # one limit binds, the one this row is for
    assert 1 < BYTES // (36_000_000 + 100_000_000) < M and 1 < SLOTS // 4_000_040 < M and seen == ["svar"] * 4


def test_listed_spans_cut_as_the_three_loops_did():
    """devplanes._listed_spans against the loop of ds_af_sets, _spike_rules and spike_scan as it stood in each (restated here): two
    chromosomes, a variant AF_RUN_LOCI - 1 positions behind its span's first (inside) and one AF_RUN_LOCI behind (the next span), and
    a consumer that takes fewer variants than it is offered - a run the decoder cut short: the rest starts the next span."""
    from types import SimpleNamespace as NS
    from smcounter_amd import devplanes
    W = devplanes.AF_RUN_LOCI
    variants = [NS(chrom=c, pos=p) for c, p in (("chr2", 60), ("chr1", 100 + W), ("chr1", 100), ("chr2", 50), ("chr1", 99 + W), ("chr2", 70),
                                                ("chr1", 700 + W), ("chr1", 101 + W))]
    order = sorted(range(len(variants)), key=lambda k: (variants[k].chrom, variants[k].pos))
    take = lambda span: max(1, len(span) - 1) if variants[span[0]].chrom == "chr2" else len(span)

    def parents():
        i = 0
        while i < len(order):
            v0 = variants[order[i]]
            j = i
            while j + 1 < len(order) and variants[order[j + 1]].chrom == v0.chrom and variants[order[j + 1]].pos - v0.pos < W:
                j += 1
            lo, hi = v0.pos - 1, variants[order[j]].pos
            group = order[i:j + 1][:take(order[i:j + 1])]
            yield v0.chrom, lo, hi, order[i:j + 1], group
            i += len(group)
    mine = []
    spans = devplanes._listed_spans(variants, order)
    for chrom, lo, hi, span in spans:
        mine.append((chrom, lo, hi, span, span[:take(span)]))
        spans.send(take(span))
    assert mine == list(parents())
    assert [(c, lo, hi, [variants[k].pos for k in g]) for c, lo, hi, _, g in mine] == [
        ("chr1", 99, 99 + W, [100, 99 + W]), ("chr1", 99 + W, 101 + W, [100 + W, 101 + W]), ("chr1", 699 + W, 700 + W, [700 + W]),
        ("chr2", 49, 70, [50, 60]), ("chr2", 69, 70, [70])]
    assert list(devplanes._listed_spans(variants, [])) == []
