"""--spikeIndelPhase without a GPU: the flag and every refusal (before any file; the pinned --spikePhase messages unchanged), PS= on
indel lines, the parser's set and footprint rules, tools.spike_variants --phased --indels against the restatement (tests/
spike_indel_phase_restate.py) record for record on both listings of the hand-made BAM, the properties of the shared draw, the pages
on hand-made rows with indel members, the header, the symbol and the record's new field."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, cli, devplanes, spike
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import spike_indel_phase_restate as XR  # noqa: E402
import spike_indel_restate as IR  # noqa: E402
import spike_restate as SR  # noqa: E402
import test_spike_indels as TI  # noqa: E402  (its command line on bam_cigars)

SEED = XR.SEED
NS = argparse.Namespace
TARGETS = [(0.01, 100, "o.spikeAF0.01"), (0.05, 100, "o.spikeAF0.05")]


def _write(tmp, text, name="v.vcf"):
    p = os.path.join(str(tmp), name)
    open(p, "w").write(text)
    return p


def _tool(bam, fa, vfile, t, out, seed=SEED, **flags):
    return sv.main(NS(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=seed, refGenome=fa, **flags))


# ---- the flag
def test_the_flag_is_parsed_and_implies_both_readings():
    ns = cli.build_parser().parse_args("--outPrefix o --bamFile b --bedTarget t --mtDepth 3 --rpb 2 --spikeIndelPhase".split())
    assert ns.spikeIndelPhase is True and spike.indel_phase(ns, TARGETS) is True
    assert spike.indel_phase(NS(), TARGETS) is False and spike.indel_phase(NS(spikeIndels=True, spikePhase=True), []) is False
    assert spike.indel_phase(NS(spikeIndelPhase=True, spikeIndelReps=4, spikeIndelDepth="0.5"), TARGETS) is True
    assert "--spikeIndelPhase" in cli.build_parser().format_help()


@pytest.mark.parametrize("kw, tg, msg", (
    (dict(spikeIndels=True), TARGETS, "--spikeIndelPhase implies the rules of --spikeIndels: leave --spikeIndels out"),
    (dict(spikePhase=True), TARGETS, "--spikeIndelPhase reads --spikeVariants as --spikePhase does: leave --spikePhase out"),
    (dict(spikeReps=4), TARGETS, "use --spikeIndelReps R beside it"),
    (dict(spikeDepth="0.5"), TARGETS, "use --spikeIndelDepth beside it"),
    (dict(), [], "it needs --spikeAF and --spikeVariants")))
def test_flag_refusals_name_the_flag_to_use(kw, tg, msg):
    with pytest.raises(SystemExit, match=re.escape(msg)):
        spike.indel_phase(NS(spikeIndelPhase=True, **kw), tg)


def test_refused_before_any_file_is_written(tmp_path):
    """The command line itself; the BAM named here does not exist.  The four --spikePhase messages other tests pin stay as they are."""
    base = dict(outPrefix=str(tmp_path / "o"), bamFile=str(tmp_path / "none.bam"), bedTarget=str(tmp_path / "none.bed"), mtDepth=10, rpb=2.0,
                refGenome=str(tmp_path / "none.fa"))
    sp = dict(spikeAF="0.1", spikeVariants="v")
    for more, msg in ((dict(spikeIndelPhase=True), "it needs --spikeAF and --spikeVariants"),
                      (dict(spikeIndelPhase=True, spikeAF="0.1"), "it needs --spikeVariants"),
                      (dict(sp, spikeIndelPhase=True, spikeIndels=True), "leave --spikeIndels out"),
                      (dict(sp, spikeIndelPhase=True, spikePhase=True), "leave --spikePhase out"),
                      (dict(sp, spikeIndelPhase=True, spikeReps=4), "use --spikeIndelReps R beside it"),
                      (dict(sp, spikeIndelPhase=True, spikeDepth="0.5"), "use --spikeIndelDepth beside it"),
                      (dict(sp, spikeIndelPhase=True, spikeIndelReps=1), "must lie in"),
                      (dict(sp, spikeIndelPhase=True, spikeIndelDepth="2"), "must lie in"),
                      (dict(sp, spikeIndelPhase=True, dsMT="0.5"), "cannot be combined with --dsMT"),
                      (dict(sp, spikeAF="1.5", spikeIndelPhase=True), "--spikeAF"),
                      # today's messages, exactly
                      (dict(sp, spikeIndels=True, spikePhase=True),
                       re.escape("--spikeIndels cannot be combined with --spikePhase in one run (replicates, depths and phase sets of indel "
                                 "spike-ins are not built)")),
                      (dict(sp, spikeIndelReps=4, spikePhase=True),
                       re.escape("--spikeIndelReps cannot be combined with --spikePhase in one run (phase sets of indel spike-ins are not built)")),
                      (dict(sp, spikeIndelDepth="0.5", spikePhase=True),
                       re.escape("--spikeIndelDepth cannot be combined with --spikePhase in one run (phase sets of indel spike-ins are not built)")),
                      (dict(sp, spikeIndelReps=4, spikeIndelDepth="0.5", spikePhase=True),
                       re.escape("--spikeIndelReps cannot be combined with --spikePhase in one run (phase sets of indel spike-ins are not built)"))):
        d = dict(base, **more)
        ns = cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in d.items() if v is not True] + ["--" + k for k, v in d.items() if v is True])
        with pytest.raises(SystemExit, match=msg):
            cli.main(ns)
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("lines,msg", [
    (lambda c, p, s: "%s\t%d\t.\t%sC\t%sGG\t.\t.\tPS=h\n" % (c, p, s[0], s[0]), "neither an insertion (X / XS) nor a deletion"),
    (lambda c, p, s: "%s\t%d\t.\t%s\t%sG\t.\t.\tPS=h\n%s\t%d\t.\t%s\t%s\t.\t.\t.\n" % (c, p, s[0], s[0], c, p + 1, s[1], "ACGT"[("ACGT".index(s[1]) + 1) % 4]),
     "lies in the footprint"),
    (lambda c, p, s: "%s\t%d\t.\t%s%s\t%s\t.\t.\tPS=h\n" % (c, p, s[0], "ACGT"[("ACGT".index(s[1]) + 1) % 4] + s[2], s[0]), "the reference genome has"),
    (lambda c, p, s: "%s\t%d\t.\t%s\t%sG\t.\t.\tPS=h\n" % (c, p + 100000, s[0], s[0]), "is not a locus of --bedTarget|the reference genome has"),
])
def test_what_both_readings_refuse_of_the_variants_file_before_any_file(tmp_path, lines, msg):
    ns = TI._args(tmp_path, lines, spikeIndelPhase=True)
    with pytest.raises(SystemExit, match=msg if "|" in msg else re.escape(msg)):
        cli.main(ns)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


# ---- the parser
def test_ps_on_indel_lines_and_an_mnv_line_that_joins_a_set_with_a_deletion(tmp_path):
    text = ("c1\t300\t.\tACGT\tA\t.\t.\tPS=h1\n"          # a deletion of 3: footprint 300-304
            "c1\t10\t.\tG\tT\t.\t.\t.\n"
            "c1\t90\t.\tAC\tGT\t.\t.\tX=1;PS=h1\n"         # an MNV line joins the set with both members
            "c2\t5\t.\tA\tAGG\t.\t.\tPS=h2\n"              # (another name: a set lies on one chromosome)
            "c1\t95\t.\tT\tTG\t.\t.\tPS=h1\n")
    vs = sv.parse_variants(_write(tmp_path, text), phased=True, indels=True)
    assert isinstance(vs, sv.PhasedVariants)
    assert [(v.chrom, v.pos, v.ref, v.alt, v.kind) for v in vs] == [("c1", 300, "ACGT", "A", af.DEL), ("c1", 10, "G", "T", af.SNV), ("c1", 90, "A", "G", af.SNV),
                                                                    ("c1", 91, "C", "T", af.SNV), ("c2", 5, "A", "AGG", af.INS), ("c1", 95, "T", "TG", af.INS)]
    assert [v.key for v in vs] == ["DEL|ACGT|A", "T", "G", "T", "INS|A|AGG", "INS|T|TG"]
    assert [(s.name, s.chrom, s.members) for s in vs.sets] == [("h1", "c1", (2, 3, 5, 0)), ("h2", "c2", (4,))]
    assert sv.leaders(vs) == [90, 10, 90, 90, 5, 90] and [s.name for s in sv.phase_sets(vs)] == ["h1"]
    assert vs.mnvs == [("c1", 90, "AC", 3)]
    # the records of the device: `lead` per chromosome, in the indel records
    s = devplanes.SpikeSet(vs)
    var, order = s.chrom_variants("c1", 0.25)
    assert s.indels and var.dtype == abi.SPIKE_INDEL_VARIANT_DTYPE
    assert var["pos0"].tolist() == [9, 89, 90, 94, 299] and var["lead"].tolist() == [0, 0, 1, 2, 3] and order == [1, 2, 3, 5, 0]
    assert var["kind"].tolist() == [0, 0, 0, 1, 2] and var["len"].tolist() == [0, 0, 0, 1, 3] and (var["thr"] == sv.threshold(0.25)).all()
    assert s.chrom_variants("c2", 0.25)[0]["lead"].tolist() == [0] and s.lead_pos == [90, 10, 90, 90, 5, 90]
    # without sets (a plain list, --spikeIndels): today's records, `lead` 0 throughout
    assert not devplanes.SpikeSet(list(vs)).chrom_variants("c1", 0.25)[0]["lead"].any()
    # the combination is refused without either flag as ever
    with pytest.raises(ValueError, match="only one-letter substitutions"):
        sv.parse_variants(_write(tmp_path, text), phased=True)
    with pytest.raises(ValueError, match="neither a substitution"):
        sv.parse_variants(_write(tmp_path, text), indels=True)         # (the MNV line)


def test_parser_refusals(tmp_path):
    ps = lambda c, p, r, a, name=None: "%s\t%d\t.\t%s\t%s\t.\t.\t%s\n" % (c, p, r, a, "PS=" + name if name else ".")
    nine = "".join(ps("c1", 10 + 4 * k, "A", "AT" if k % 2 else "G", "h") for k in range(9))
    for text, msg in ((nine, "the phase set h has 9 members, at most 8"),
                      # a member and a non-member: by line, with --spikeIndels' message
                      (ps("c1", 9, "ACGT", "A", "h") + ps("c1", 20, "A", "G", "h") + ps("c1", 13, "G", "T"), "line 3: c1:13 G>T lies in the footprint 9-13 of c1:9 ACGT>A (line 1)"),
                      (ps("c1", 9, "A", "AC", "h") + ps("c1", 10, "G", "T", "h"), "line 2: c1:10 G>T lies in the footprint 9-10"),
                      # an MNV line's member inside a deletion's footprint
                      (ps("c1", 9, "ACGT", "A", "h") + ps("c1", 12, "AC", "GT", "h"), "line 2: c1:12 A>G lies in the footprint 9-13"),
                      (ps("c1", 9, "A", "ANG", "h"), "made of A, C, G, T"), (ps("c1", 9, "GNT", "G", "h"), "made of A, C, G, T"),
                      (ps("c1", 9, "A", "A" + "C" * 256, "h"), "at most 255"), (ps("c1", 9, "A" + "C" * 256, "A", "h"), "at most 255"),
                      (ps("c1", 9, "AC", "GTT", "h"), "neither an insertion (X / XS) nor a deletion (XD / X)"),
                      (ps("c1", 9, "A", "G", "h") + ps("c1", 9, "A", "AT", "h"), "listed twice"),
                      (ps("c1", 9, "A", "AT", "h") + ps("c2", 9, "ACG", "A", "h"), "the phase set PS=h is listed on c1 and on c2"),
                      (ps("c1", 9, "A", "AT").replace("\t.\n", "\tPS=a;PS=b\n"), "one PS=<name> entry")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            sv.parse_variants(_write(tmp_path, text), "--spikeVariants", phased=True, indels=True)
    # footprints that touch nothing, members and non-members alike: 9-10, 11, 12-16, 17-18
    ok = ps("c1", 9, "A", "AC", "h") + ps("c1", 11, "G", "T") + ps("c2", 10, "G", "T") + ps("c1", 12, "ACGT", "A", "h") + ps("c1", 17, "C", "CA")
    assert len(sv.parse_variants(_write(tmp_path, ok), phased=True, indels=True)) == 5


def test_check_reference_covers_the_letters_of_an_indel_member(tmp_path):
    bam, fa, loci, P, variants = IR.make_case(str(tmp_path))
    from smcounter_amd import fasta
    genome = fasta.FastaFile(fa)
    good = sv.parse_variants(XR.write_listing(str(tmp_path / "a.vcf"), variants, XR.LISTING_A), phased=True, indels=True)
    sv.check_reference(good, genome)
    d = variants[2]
    wrong = d.ref[:2] + "ACGT"[("ACGT".index(d.ref[2]) + 1) % 4] + d.ref[3:]
    bad = [variants[0], variants[1], IR.variant(d.chrom, d.pos, wrong, d.alt), variants[3]]
    with pytest.raises(ValueError, match="the reference genome has"):
        sv.check_reference(sv.parse_variants(XR.write_listing(str(tmp_path / "b.vcf"), bad, XR.LISTING_A), phased=True, indels=True), genome)


# ---- the tool against the restatement
@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """The hand-made BAM, both listings' files, the restatement at 2^31 and the tool's BAM of each, made once."""
    tmp = str(tmp_path_factory.mktemp("indel_phase"))
    bam, fa, loci, P, variants = IR.make_case(tmp)
    out = dict(tmp=tmp, bam=bam, fa=fa, loci=loci, P=P, variants=variants, before=IR.file_records(bam))
    for name, sets in XR.LISTINGS.items():
        vfile = XR.write_listing(os.path.join(tmp, "%s.vcf" % name), variants, sets)
        records, stats = XR.restate(bam, variants, sets, XR.HALF, SEED, P.mismatchThr, fa)
        tool_bam = os.path.join(tmp, "%s.bam" % name)
        rows = _tool(bam, fa, vfile, 0.5, tool_bam, phased=True, indels=True)
        out[name] = dict(sets=sets, vfile=vfile, records=records, stats=stats, tool=tool_bam, rows=rows)
    return out


def _spiked_of(stats, members):
    return set().union(*(stats[k]["spiked"] for k in members))


def test_the_seed_leaves_nothing_vacuous(case):
    """On the restatement alone: at 2^31 every one of the shapes `all`, `snvins` and `behind` has a spiked and an unspiked barcode, and
    0 < S_ALL < N_ALL for the set - in both listings."""
    for name, sets in XR.LISTINGS.items():
        stats = case[name]["stats"]
        spiked = _spiked_of(stats, sets[0])
        for shape in ("all", "snvins", "behind"):
            mine = ["%s%02d" % (shape.upper(), b) for b in range(IR.N_BC)]
            assert 0 < sum(b in spiked for b in mine) < IR.N_BC, (name, shape)
        counts, joint = XR.restate_counts(case["bam"], case["fa"], case["variants"], sets, [0.5], [1.0], SEED, 1)
        n_all, _, s_all, _ = (int(x) for x in counts[0, 0, 0, 0])
        assert 0 < s_all < n_all == len(joint[0][0]), (name, s_all, n_all)
        assert s_all == len(set(joint[0][0]) & set.intersection(*(stats[k]["spiked"] for k in sets[0])))


@pytest.mark.parametrize("name", ("A", "B"))
def test_tool_equals_the_restatement_record_for_record(case, name):
    c = case[name]
    got, want = IR.file_records(c["tool"]), IR.expected_records(case["bam"], c["records"])
    assert len(got) == len(want) and all(g == w for g, w in zip(got, want))
    for row, s in zip(c["rows"], c["stats"]):
        assert row == {k: s[k] for k in ("N", "V0", "S", "READS", "V1")}
    assert sum(r["relocated"] for r in c["records"].values()) > 0
    # the unphased restatement is another file: the members' own positions draw differently
    loose, _ = IR.restate(case["bam"], case["variants"], XR.HALF, SEED, case["P"].mismatchThr, case["fa"])
    assert {k: r["applied"] for k, r in loose.items()} != {k: r["applied"] for k, r in c["records"].items()}


def test_members_are_spiked_on_the_same_barcodes_and_the_sets_are_nested(case):
    bam, fa, P, variants = case["bam"], case["fa"], case["P"], case["variants"]
    cover = [set(names) for names, _ in XR.QR.host_counters(bam, variants, fa)[0]]
    for name, sets in XR.LISTINGS.items():
        members = sets[0]
        last = None
        for t in (0.05, 0.2, 0.5, 0.9):
            _, stats = XR.restate(bam, variants, sets, sv.threshold(t), SEED, P.mismatchThr, fa)
            joint = set.intersection(*(cover[k] for k in members))
            spiked = [stats[k]["spiked"] & joint for k in members]
            assert all(s == spiked[0] for s in spiked), (name, t)                       # set equality among the barcodes that cover all
            # ... and on every pair's common cover: a barcode is spiked at every member it covers or at none
            for a in members:
                for b in members:
                    both = cover[a] & cover[b]
                    assert stats[a]["spiked"] & both == stats[b]["spiked"] & both
            every = [stats[k]["spiked"] for k in range(len(variants))]
            if last is not None:
                assert all(x <= y for x, y in zip(last, every))                         # nested over the targets
            last = every
            if name == "B" and t == 0.5:
                # 105 is no member: it draws on its own, between the two members
                both = cover[0] & cover[1]
                assert stats[1]["spiked"] & both != stats[0]["spiked"] & both
                _, own = IR.restate(bam, variants, sv.threshold(t), SEED, P.mismatchThr, fa)
                assert stats[1]["spiked"] == own[1]["spiked"] and stats[3]["spiked"] == own[3]["spiked"]
        assert any(last)


def test_what_the_shapes_take(case):
    variants, before = case["variants"], {(r[0], r[1], r[2]): r for r in case["before"]}
    c = case["A"]
    spiked = _spiked_of(c["stats"], (0, 1, 2))
    got = {(r[0], r[1], r[2]): r for r in IR.file_records(c["tool"])}
    seen = {"all": 0, "snvins": 0, "behind": 0, "same": 0}
    for key, r in c["records"].items():
        bc = af.barcode_of(key[0])
        shape = XR.shape_of(bc)
        kinds = sorted(variants[k].kind for k in r["applied"] if k != 3)
        if bc not in spiked:
            assert not [k for k in r["applied"] if k != 3]
            continue
        if shape == "all":
            # the insertion of 3, the SNV (the read showed REF at 105) and the deletion of 3: NM + 3 + 1 + 3
            assert kinds == [af.SNV, af.INS, af.DEL] and r["nm_inc"] == 3 + 3 + 1 and r["indel_inc"] == 6
            assert got[key][6] == before[key][6] + 7 and got[key][3] != before[key][3]
            seen["all"] += 1
        elif shape == "snvins":
            # the read ends on the deletion's anchor: it takes the insertion and the SNV, not the deletion ("not modelled")
            assert kinds == [af.SNV, af.INS] and r["nm_inc"] == 4
            seen["snvins"] += 1
        elif shape == "behind":
            # the leader's anchor lies in front of the read: the members behind it are taken all the same
            assert kinds == [af.SNV, af.DEL] and r["nm_inc"] == 4
            seen["behind"] += 1
    assert all(seen[s] > 0 for s in ("all", "snvins", "behind")), seen
    # unspiked barcodes are byte-identical (but for the singleton at 150, which draws on its own)
    every = spiked | c["stats"][3]["spiked"]
    for key, r in got.items():
        if af.barcode_of(key[0]) not in every:
            assert r == before[key]
            seen["same"] += 1
    assert seen["same"] > 0


def test_without_sets_and_without_indels_the_tool_writes_what_it_wrote(case, tmp_path):
    tmp, bam, fa, variants = str(tmp_path), case["bam"], case["fa"], case["variants"]
    # no set: --phased --indels == --indels, byte for byte
    plain = XR.write_listing(os.path.join(tmp, "plain.vcf"), variants, [])
    a, b = os.path.join(tmp, "a.bam"), os.path.join(tmp, "b.bam")
    assert _tool(bam, fa, plain, 0.5, a, phased=True, indels=True) == _tool(bam, fa, plain, 0.5, b, indels=True)
    assert open(a, "rb").read() == open(b, "rb").read()
    # no indel: --phased --indels == --phased, byte for byte (the hand-made BAM of --spikeAF, two SNVs one set)
    sbam, sfa, _, _, snvs = SR.make_case(tmp)
    import spike_phase_restate as PH
    listed = _write(tmp, PH.snv_line(snvs[1], "hap") + PH.snv_line(snvs[2]) + PH.snv_line(snvs[0], "hap"), "snv.vcf")
    a, b = os.path.join(tmp, "c.bam"), os.path.join(tmp, "d.bam")
    assert _tool(sbam, sfa, listed, 0.5, a, phased=True, indels=True) == _tool(sbam, sfa, listed, 0.5, b, phased=True)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert open(a, "rb").read() != open(sbam, "rb").read()


# ---- the pages
def _set():
    vs = [IR.variant("chr1", 100, "A", "AGAT"), IR.variant("chr1", 104, "C", "T"), IR.variant("chr1", 109, "GTTA", "G"), IR.variant("chr1", 50, "G", "A")]
    return vs, sv.PhaseSet("hap", "chr1", (0, 1, 2))


def test_phase_lines_with_indel_members():
    vs, ps = _set()
    r = dict(N_ALL=3000, V0_ALL=1, S_ALL=14, V1_ALL=15)
    assert spike.phase_line(ps, vs, 0.005, 0.5, 1750, r, 1) == \
        "hap\tchr1\t100,104,109\tA,C,GTTA\tAGAT,T,G\t0.005\t0.5\t1750\t3000\t1\t14\t15\t0.005\t1"
    assert spike.phase_replicate_line(ps, vs, 0.005, None, 3500, 2, 99, r, 0).split("\t")[:12] == \
        ["hap", "chr1", "100,104,109", "A,C,GTTA", "AGAT,T,G", "0.005", "full", "3500", "2", "99", "3000", "1"]
    assert spike.phase_sensitivity_line(ps, vs, 0.05, None, 50, [(r, 1), (r, 0)]).split("\t")[:11] == \
        ["hap", "chr1", "100,104,109", "A,C,GTTA", "AGAT,T,G", "0.05", "full", "50", "2", "1", "0.5"]
    # CALLED_ALL: per member the comparison of the detection page's CALLED, at the anchor for an indel
    cut = {("chr1", "100"): ("A", ["AGAT"]), ("chr1", "104"): ("C", ["A", "T"]), ("chr1", "109"): ("GTTA", ["G"])}
    assert spike.called_all(ps, vs, cut) == 1
    det = lambda m, c: spike.detection_line(m, 0.1, dict(N=1, V0=0, S=0, READS=0, V1=0), None, c.get((m.chrom, "%d" % m.pos))).split("\t")[16]
    assert [det(m, cut) for m in vs[:3]] == ["1", "1", "1"]
    other = {**cut, ("chr1", "109"): ("GTT", ["G"])}
    assert [det(m, other) for m in vs[:3]] == ["1", "1", "0"] and spike.called_all(ps, vs, other) == 0
    assert spike.called_all(ps, vs, {**cut, ("chr1", "109"): ("GTT", ["G"])}) == 0                 # another deletion at the anchor
    assert spike.called_all(ps, vs, {**cut, ("chr1", "100"): ("A", ["AGA"])}) == 0                 # another insertion
    assert spike.called_all(ps, vs, {k: v for k, v in cut.items() if k != ("chr1", "104")}) == 0      # a member not cut


def test_phase_files_with_indel_members(tmp_path):
    from smcounter_amd.rows import HEADER_ALL
    vs, ps = _set()
    prefixes = [str(tmp_path / p) for p in ("o", "o.spikeAF0.1", "o.spikeAF0.1.dsMT0.5")]
    for k, prefix in enumerate(prefixes):
        open(prefix + ".smCounter.all.txt", "w").write("\t".join(HEADER_ALL) + "\n")
        open(prefix + ".smCounter.cut.txt", "w").write("CHROM\tPOS\tREF\tALT\n" + ("chr1\t100\tA\tAGAT\nchr1\t104\tC\tT\n" if k else "") +
                                                       ("chr1\t109\tGTTA\tG\n" if k == 1 else ""))
    r = dict(N_ALL=40, V0_ALL=0, S_ALL=5, V1_ALL=4)
    outs = [(None, None, 80, prefixes[0], [dict(r, S_ALL=0, V1_ALL=0)]), (0.1, None, 80, prefixes[1], [r]),
            (0.1, 0.5, 40, prefixes[2], [dict(r, N_ALL=20, S_ALL=2, V1_ALL=2)])]
    spike.write_phase(prefixes[0], vs, [ps], outs)
    lines = [l.split("\t") for l in open(prefixes[0] + ".spikeAF.phase.txt").read().splitlines()]
    assert lines[0] == list(spike.PHASE_HEADER) and len(lines) == 4
    assert all(l[:5] == ["hap", "chr1", "100,104,109", "A,C,GTTA", "AGAT,T,G"] for l in lines[1:])
    assert [l[5:] for l in lines[1:]] == [["full", "full", "80", "40", "0", "0", "0", "0.0", "0"], ["0.1", "full", "80", "40", "0", "5", "4", "0.1", "1"],
                                         ["0.1", "0.5", "40", "20", "0", "2", "2", "0.1", "0"]]
    entries = {(0, 0): [(r, 1), (dict(r, S_ALL=3, V1_ALL=3), 0)], (0, 1): [(dict(r, N_ALL=20), 0), (dict(r, N_ALL=25), 0)]}
    spike.write_phase_replicates(prefixes[0], vs, [ps], [(0.1, None, 80), (0.1, 0.5, 40)], [7, 8], entries)
    reps = [l.split("\t") for l in open(prefixes[0] + ".spikeAF.phase.replicates.txt").read().splitlines()]
    assert reps[0] == list(spike.PHASE_REPLICATES_HEADER) and [l[3:10] for l in reps[1:]] == \
        [["A,C,GTTA", "AGAT,T,G", "0.1", "full", "80", "0", "7"], ["A,C,GTTA", "AGAT,T,G", "0.1", "full", "80", "1", "8"],
         ["A,C,GTTA", "AGAT,T,G", "0.1", "0.5", "40", "0", "7"], ["A,C,GTTA", "AGAT,T,G", "0.1", "0.5", "40", "1", "8"]]
    spike.write_phase_sensitivity(prefixes[0], vs, [ps], [(0.1, None, 80), (0.1, 0.5, 40)], entries)
    sens = [l.split("\t") for l in open(prefixes[0] + ".spikeAF.phase.sensitivity.txt").read().splitlines()]
    assert sens[0] == list(spike.PHASE_SENSITIVITY_HEADER) and len(sens) == 3 and sens[1][8:11] == ["2", "1", "0.5"]


def test_joint_rows_of_four_counters():
    """devplanes.spike_joint on four counters per covering barcode: the barcodes that cover every member, each member's row."""
    ids = [np.array([5, 9, 2, 7], np.uint64), np.array([7, 2, 11], np.uint64)]
    cnt = [np.arange(16, dtype=np.uint32).reshape(4, 4), 100 + np.arange(12, dtype=np.uint32).reshape(3, 4)]
    (both, rows), = devplanes.spike_joint([sv.PhaseSet("h", "c", (0, 1))], ids, cnt)
    assert both.tolist() == [2, 7] and rows.shape == (2, 2, 4)
    assert rows[0].tolist() == [[8, 9, 10, 11], [104, 105, 106, 107]] and rows[1].tolist() == [[12, 13, 14, 15], [100, 101, 102, 103]]
    (_, three), = devplanes.spike_joint([sv.PhaseSet("h", "c", (0, 1))], ids, [c[:, :3] for c in cnt])
    assert three.shape == (2, 2, 3) and three[0].tolist() == [[8, 9, 10], [104, 105, 106]]              # (--spikePhase's rows as ever)


def test_a_leader_beyond_the_fields_range_is_refused():
    """65,536 records between a member and its leader do not fit the 16-bit `lead` (a run's entries take at most 4,096 variants: only a
    list handed to SpikeSet directly gets here)."""
    n = 0x10000
    vs = [IR.variant("c", 10 + 2 * k, "A", "G") for k in range(n + 1)]
    ok = sv.PhasedVariants(vs[:n], [sv.PhaseSet("h", "c", (0, n - 1))])
    assert int(devplanes.SpikeSet(ok, indels=True).chrom_variants("c", 0.5)[0]["lead"][-1]) == n - 1 == 0xFFFF
    far = sv.PhasedVariants(vs, [sv.PhaseSet("h", "c", (0, n))])
    for indels in (True, False):
        with pytest.raises(ValueError, match="c:%d: its phase set's leader stands 65536 records in front" % vs[n].pos):
            devplanes.SpikeSet(far, indels=indels)


# ---- the header
def test_the_entry_and_the_field_are_declared():
    h = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"#define SMC_ABI_VERSION 11\b", h)
    assert re.search(r"\bint smc_spike_indel_phase_counts\(smc_ctx\* ctx, const uint64_t\* d_joint_ident, const uint32_t\* d_joint_cnt,", h)
    body = h[h.index("typedef struct smc_spike_indel_variant"):h.index("} smc_spike_indel_variant;")]
    assert re.search(r"uint16_t len;", body) and re.search(r"uint16_t lead;", body) and "uint32_t len" not in body
    assert "smc_spike_indel_phase_counts" in _lib.SYMBOLS
    d = abi.SPIKE_INDEL_VARIANT_DTYPE
    assert d.itemsize == 24 and d.fields["len"][1] == 8 and d.fields["lead"][1] == 10 and d.fields["lead"][0] == np.dtype("<u2")
    assert d.fields["ins_off"][1] == 12 and d.fields["thr"][1] == 16
    # a record of today's callers - `len` up to 255 in what was a 32-bit field - has the same bytes
    old = np.dtype([("pos0", "<i4"), ("kind", "u1"), ("ref", "u1"), ("alt", "u1"), ("pad", "u1"), ("len", "<u4"), ("ins_off", "<u4"), ("thr", "<u8")])
    a, b = np.zeros(1, old), np.zeros(1, d)
    for f, x in (("pos0", 77), ("kind", 2), ("ref", 65), ("alt", 65), ("len", 255), ("ins_off", 9), ("thr", 1 << 32)):
        a[f], b[f] = x, x
    assert a.tobytes() == b.tobytes()
    L = _lib.load()
    assert L.smc_abi_version() == 11 and hasattr(L, "smc_spike_indel_phase_counts")
    assert L.smc_spike_indel_phase_counts.argtypes == L.smc_spike_phase_counts.argtypes
