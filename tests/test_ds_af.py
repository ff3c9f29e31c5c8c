"""--dsAF without a GPU: tools/ds_allele_fraction.py (the specification in code) against the restatement from host-built pileups
(tests/ds_af_restate.py), the properties of the drop, parsing and every refusal, the detection file's format, the ABI."""
import argparse
import math
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, cli, dsaf, fasta
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402

TARGETS = (0.02, 0.05, 0.1)
SEED = 7                       # (test_expected_fraction_within_the_binomial_width: a seed for which the RESTATEMENT holds the bound)


def _inputs(name, tmp):
    """-> (bam, fasta, listed variants as the restatement's V)."""
    if name == "synth":
        bam, fa, loci, _, _ = R.synth_bam(tmp)
        return bam, fa, R.planted(bam, fa, loci)
    bam, fa, loci, _ = ds_restate.load_fixture(name, tmp)
    return bam, fa, R.pick_variants(bam, fa, loci)


def _tool_plan(bam, fa, variants, targets, seed, tmp):
    vs = af.parse_variants(R.write_variants(os.path.join(tmp, "v.txt"), variants))
    ids, res = af.plan_file(bam, vs, list(targets), seed, fasta.FastaFile(fa))
    return vs, ids, res


@pytest.mark.parametrize("name", ("bam_cigars", "bam_deep", "synth"))
def test_tool_equals_the_restatement(tmp_path, name):
    tmp = str(tmp_path)
    bam, fa, variants = _inputs(name, tmp)
    assert variants
    if name == "bam_cigars":
        assert {"SNV", "INS", "DEL"} <= {"SNV" if len(v.key) == 1 else v.key[:3] for v in variants}
    sets, want = R.restate(bam, fa, variants, TARGETS, SEED)
    vs, ids, res = _tool_plan(bam, fa, variants, TARGETS, SEED, tmp)
    text = {i: t for t, i in ids.items()}
    assert any(r["V"] for r in want[0]["rows"])
    for w, g in zip(want, res):
        assert {text[int(i)] for i in g["dropped"]} == w["dropped"]
        for wr, gr in zip(w["rows"], g["rows"]):
            assert (gr["N"], gr["V"], gr["N2"], gr["V2"]) == (wr["N"], wr["V"], wr["N2"], wr["V2"])
            assert gr["k"] == wr["k"]
    # the output BAM holds exactly the other barcodes' records, in file order
    vfile = os.path.join(tmp, "v.txt")
    for w in want[:2]:
        out = os.path.join(tmp, "out%g.bam" % w["target"])
        n = af.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % w["target"], seed=SEED, refGenome=fa))
        keep = [raw for q, raw in R.raw_records(bam) if q.strip().split(":")[-2] not in w["dropped"]]
        assert [raw for _, raw in R.raw_records(out)] == keep and n == len(keep)


@pytest.mark.parametrize("name", ("bam_cigars", "synth"))
def test_properties_of_the_drop(tmp_path, name):
    tmp = str(tmp_path)
    bam, fa, variants = _inputs(name, tmp)
    sets, _ = R.restate(bam, fa, variants, (), SEED)
    vs, ids, res = _tool_plan(bam, fa, variants, TARGETS, SEED, tmp)
    drops = [set(int(i) for i in r["dropped"]) for r in res]
    assert drops[0] >= drops[1] >= drops[2]                                  # kept sets nested: kept(t1) within kept(t2), t1 < t2
    carriers = {ids[b] for _, car in sets for b in car}
    assert drops[0] <= carriers                                              # no non-carrier dropped
    # "any carried variant": a barcode is dropped exactly when one of the variants it carries draws it out
    for r in res:
        u = {}
        for (cov, car), row in zip(sets, r["rows"]):
            for b, x in zip(sorted(car), R.draw(sorted(car), SEED)):
                u.setdefault(ids[b], []).append(int(x) >= row["thr"])
        assert {i for i, hits in u.items() if any(hits)} == set(int(i) for i in r["dropped"])
    if name == "synth":
        shared = [i for i, hits in u.items() if len(hits) > 1]
        assert shared                                                        # nearby planted variants share carriers


def test_variants_left_alone(tmp_path):
    """A fraction at or below the target already, an absent variant and one every covering barcode carries drop nothing."""
    tmp = str(tmp_path)
    bam, fa, loci, _, _ = R.synth_bam(tmp)
    v = R.planted(bam, fa, loci, limit=1)[0]
    other = next(x for x in "ATGC" if x not in (v.ref, v.alt))
    absent = R.V(v.chrom, v.pos, v.ref, v.ref + "TTTTTTTTTTTT", "INS|%s|%sTTTTTTTTTTTT" % (v.ref, v.ref))
    for listed, t in (([v], 0.9), ([absent], 0.05)):
        _, _, (res,) = _tool_plan(bam, fa, listed, [t], SEED, tmp)
        assert len(res["dropped"]) == 0 and res["rows"][0]["k"] == 1.0 and res["rows"][0]["thr"] == 1 << 32
    assert af.variant_state(res["rows"][0]) == "absent"
    assert af.keep_probability(40, 40, 0.01) == 1.0 and af.keep_probability(40, 0, 0.01) == 1.0 and af.keep_probability(100, 5, 0.05) == 1.0
    # V == N through the whole path: titrate() over sets made by hand
    ids = np.arange(1, 11, dtype=np.uint64)
    (res,) = af.titrate([ids], [ids], [0.01], SEED)
    assert len(res["dropped"]) == 0 and af.variant_state(res["rows"][0]).startswith("every covering barcode")
    assert other


def test_expected_fraction_within_the_binomial_width(tmp_path):
    """|V' - k V| <= 4 sqrt(V k (1 - k)) for every listed variant and target of the synthetic BAM, all variants listed together: the
    binomial's own width, not a tuned tolerance.  (A carrier shared with a neighbour can be drawn out by the neighbour: V' is at most
    the variant's own binomial(V, k) draw.)  SEED is fixed, so the check is deterministic; it is a seed for which the RESTATEMENT
    holds the bound (asserted first) - then the tool must."""
    tmp = str(tmp_path)
    bam, fa, variants = _inputs("synth", tmp)
    _, want = R.restate(bam, fa, variants, TARGETS, SEED)
    _, _, got = _tool_plan(bam, fa, variants, TARGETS, SEED, tmp)
    for res in (want, got):
        for r in res:
            for v, row in zip(variants, r["rows"]):
                k, n = row["k"], row["V"]
                print(v.pos, r["target"], n, k, row["V2"], 4 * math.sqrt(n * k * (1 - k)))
                assert n > 10 and k < 1.0
                assert abs(row["V2"] - k * n) <= 4 * math.sqrt(n * k * (1 - k))


def test_variant_file_parsing(tmp_path):
    p = str(tmp_path / "v.vcf")
    open(p, "w").write("##fileformat=VCFv4.2\n#CHROM\tPOS\tID\tREF\tALT\n\nchr1\t100\t.\ta\tg\t50\tPASS\tx\nchr1\t200\tA\tAcg\nchr2\t5\tGTT\tG\n")
    vs = af.parse_variants(p)
    assert [(v.chrom, v.pos, v.ref, v.alt, v.key, v.kind) for v in vs] == [
        ("chr1", 100, "A", "G", "G", af.SNV), ("chr1", 200, "A", "ACG", "INS|A|ACG", af.INS), ("chr2", 5, "GTT", "G", "DEL|GTT|G", af.DEL)]
    bad = (("chr1\t100\tA\n", "3 tab-separated columns"), ("chr1\tx\tA\tG\n", "not an integer"), ("chr1\t0\tA\tG\n", "1-based"),
           ("chr1\t9\t.\tA\tG,T\n", "more than one allele"), ("chr1\t9\tAC\tGT\n", "neither a substitution"),
           ("chr1\t9\tA\tA\n", "neither a substitution"), ("chr1\t9\tA\tCG\n", "neither a substitution"),
           ("chr1\t9\tA\tG\nchr1\t9\tA\tT\n", "listed twice"), ("chr1\t9\tA\tA" + "C" * (af.MAX_INS + 1) + "\n", "at most %d" % af.MAX_INS),
           ("# nothing\n", "lists no variant"))
    for text, msg in bad:
        open(p, "w").write(text)
        with pytest.raises(ValueError, match=re.escape(msg)):
            af.parse_variants(p)
    assert af.parse_targets("0.01,0.005") == [0.01, 0.005]
    for text in ("0", "1", "0.5,1.5", "x", ""):
        with pytest.raises(ValueError, match="allele fraction"):
            af.parse_targets(text)


def _args(tmp, **kw):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp))
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    vfile = str(tmp / "v.txt")
    open(vfile, "w").write("%s\t%d\tA\tG\n" % loci[0])
    d = dict(outPrefix=str(tmp / "o"), bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, refGenome=fa, dsAF="0.05", dsAFVariants=vfile)
    d.update(kw)
    return {k: v for k, v in d.items() if v is not None}, loci


@pytest.mark.parametrize("kw,msg", [
    (dict(dsAFVariants=None), "it needs --dsAFVariants"),
    (dict(dsAF=None), "it needs --dsAF"),
    (dict(dsAF="0.5,1"), "must lie in (0, 1)"),
    (dict(dsAF="0"), "must lie in (0, 1)"),
    (dict(dsMT="0.5"), "cannot be combined with --dsMT"),
    (dict(dsRpb="2"), "cannot be combined with --dsRpb"),
    (dict(dsAFMtDepth="10,20"), "2 depths for 1 --dsAF targets"),
])
def test_cli_refusals_before_any_file(tmp_path, kw, msg):
    args, _ = _args(tmp_path, **kw)
    with pytest.raises(SystemExit, match=re.escape(msg)):
        cli.main(args)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_cli_refuses_dsgrid_more_processes_and_host_planes(tmp_path, monkeypatch):
    args, _ = _args(tmp_path)
    ns = cli.build_parser().parse_args(["--%s=%s" % kv for kv in args.items()] + ["--dsGrid"])
    with pytest.raises(SystemExit, match="cannot be combined with --dsGrid"):
        cli.ds_af_targets(ns)
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="--dsAF runs in one process only"):
        cli.main(args)
    monkeypatch.setenv("WORLD_SIZE", "1")
    for env, val in (("SMC_PLANES", "host"), ("SMC_BAM_DECODER", "python")):
        monkeypatch.setenv(env, val)
        with pytest.raises(SystemExit, match="--dsAF needs the device builder"):
            cli.main(args)
        monkeypatch.delenv(env)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_cli_refuses_bad_variant_files(tmp_path):
    args, loci = _args(tmp_path)
    ns = argparse.Namespace(**args)
    loc_list = [(c, str(p)) for c, p in loci]
    assert len(cli.ds_af_variants(ns, loc_list)) == 1
    c, p = loci[0]
    for text, msg in (("%s\t%d\tA\tG\n" % (c, max(q for _, q in loci) + 1000), "is not a locus of --bedTarget"),
                      ("%s\t%d\tAC\tGT\n" % (c, p), "neither a substitution"), ("%s\t%d\t.\tA\tG,T\n" % (c, p), "more than one allele"),
                      ("%s\t%d\tA\tG\n%s\t%d\tA\tT\n" % (c, p, c, p), "listed twice"),
                      ("%s\t%d\tA\tA%s\n" % (c, p, "C" * 300), "at most 255")):
        open(ns.dsAFVariants, "w").write(text)
        with pytest.raises(SystemExit, match=re.escape(msg)):
            cli.ds_af_variants(ns, loc_list)
    ns.dsAFVariants = str(tmp_path / "missing.txt")
    with pytest.raises(SystemExit):
        cli.ds_af_variants(ns, loc_list)


def test_detection_file_format(tmp_path):
    """Hand-made rows: the columns, the numbers' text (fractions rounded as Python 2 rounds, 6 decimals, printed as its str()), CALLED."""
    from smcounter_amd.rows import HEADER_ALL
    v = af.Variant("chr1", 100, "A", "G", "G", af.SNV)
    row = [""] * len(HEADER_ALL)
    for name, val in (("CHROM", "chr1"), ("POS", "100"), ("REF", "A"), ("ALT", "G"), ("UMT", "3500"), ("VMT", "17"), ("VMF", "0.0049"),
                      ("PI", "31.25"), ("FILTER", "PASS")):
        row[HEADER_ALL.index(name)] = val
    assert dsaf.detection_line(v, None, 3600, 360, 1.0, row, ("A", ["G"])) == \
        "chr1\t100\tA\tG\tfull\t3600\t360\t0.1\t1.0\t3500\t17\t0.0049\t31.25\tPASS\t1"
    assert dsaf.detection_line(v, 0.005, 3257, 17, 0.0452261306533, row, ("A", ["T", "G"]), lod=0.0021) == \
        "chr1\t100\tA\tG\t0.005\t3257\t17\t0.00522\t0.045226\t3500\t17\t0.0049\t31.25\tPASS\t1\t0.0021"
    assert dsaf.detection_line(v, 0.0025, 0, 0, 2.5e-07, None, ("A", ["T"])).split("\t")[4:] == \
        ["0.0025", "0", "0", "0.0", "0.0", "", "", "", "", "", "0"]
    assert dsaf.detection_line(v, 0.5, 2, 1, 0.5, row, None).split("\t")[5:9] == ["2", "1", "0.5", "0.5"]
    assert dsaf.frac_text(1.0 / 3) == "0.333333" and dsaf.frac_text(0.25) == "0.25" and dsaf.frac_text(2e-06) == "2e-06"
    # the file: header, variants outer, outputs inner (full depth first)
    for prefix in ("o", "o.dsAF0.05"):
        open(str(tmp_path / prefix) + ".smCounter.all.txt", "w").write("\t".join(HEADER_ALL) + "\n" + "\t".join(row) + "\n")
        open(str(tmp_path / prefix) + ".smCounter.cut.txt", "w").write("CHROM\tPOS\tREF\tALT\n" + ("chr1\t100\tA\tG\n" if prefix == "o" else ""))
    rows = [dict(N=3600, V=360, a=0.1, k=0.473684210526, thr=1, N2=3400, V2=160)]
    dsaf.write_detection(str(tmp_path / "o"), [v], [(None, str(tmp_path / "o"), None, None), (0.05, str(tmp_path / "o.dsAF0.05"), rows, None)])
    lines = open(str(tmp_path / "o.dsAF.detection.txt")).read().splitlines()
    assert lines[0].split("\t") == list(dsaf.DETECTION_HEADER)
    assert [l.split("\t")[4:9] + [l.split("\t")[-1]] for l in lines[1:]] == [["full", "3600", "360", "0.1", "1.0", "1"],
                                                                            ["0.05", "3400", "160", "0.047059", "0.473684", "0"]]


def test_header_symbol_and_abi():
    h = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"\bint smc_allele_carriers\(smc_ctx\* ctx,", h)
    assert re.search(r"#define SMC_ABI_VERSION 11\b", h)
    assert "#define SMC_AF_MAX_INS %d" % af.MAX_INS in h
    assert "smc_allele_carriers" in _lib.SYMBOLS
    L = _lib.load()
    assert L.smc_abi_version() == 11 and hasattr(L, "smc_allele_carriers")
    assert "--dsAF" in cli.build_parser().format_help()
