"""--spikePhase without a GPU: the flag, MNV and PS= parsing with every refusal before any file, the shared draw (set equality, not
a statistic), tools.spike_variants --phased against the restatement (tests/spike_phase_restate.py) record for record on the hand-made
BAM, the three pages on hand-made rows, and the ABI entry's declaration."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, cli, dsaf, fasta, spike
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import spike_phase_restate as PH  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402

SEED = 20240607
NS = lambda **kw: argparse.Namespace(**kw)
TARGETS = [(0.01, 100, "o.spikeAF0.01")]


def _write(tmp, text, name="v.vcf"):
    path = os.path.join(str(tmp), name)
    open(path, "w").write(text)
    return path


def test_the_flag_is_parsed():
    ns = cli.build_parser().parse_args("--outPrefix o --bamFile b --bedTarget t --mtDepth 3 --rpb 2 --spikePhase".split())
    assert ns.spikePhase is True
    assert cli.build_parser().parse_args("--outPrefix o --bamFile b --bedTarget t --mtDepth 3 --rpb 2".split()).spikePhase is False
    assert spike.phase(ns, TARGETS) is True and spike.phase(NS(), TARGETS) is False and spike.phase(NS(spikePhase=False), []) is False
    with pytest.raises(SystemExit, match="it needs --spikeAF"):
        spike.phase(ns, [])
    tool = sv.build_parser().parse_args("--inBam a --outBam b --variants v --af 0.1 --phased".split())
    assert tool.phased is True and sv.build_parser().parse_args("--inBam a --outBam b --variants v --af 0.1".split()).phased is False


def test_spike_phase_without_spike_af_is_refused_before_any_file(tmp_path):
    base = dict(outPrefix=str(tmp_path / "o"), bamFile=str(tmp_path / "none.bam"), bedTarget=str(tmp_path / "none.bed"), mtDepth=10, rpb=2.0,
                refGenome=str(tmp_path / "none.fa"))
    with pytest.raises(SystemExit, match="--spikePhase .* it needs --spikeAF"):
        cli.main(cli.build_parser().parse_args(["--%s=%s" % kv for kv in base.items()] + ["--spikePhase"]))
    assert os.listdir(str(tmp_path)) == []


def test_mnv_lines_expand_and_equal_letters_in_the_middle_are_skipped(tmp_path):
    path = _write(tmp_path, "#c\nc1\t100\t.\tACGT\tTCGA\t.\t.\t.\nc1\t50\tG\tT\nc1\t200\tAC\tGT\n")
    vs = sv.parse_variants(path, phased=True)
    assert [tuple(v) for v in vs] == [("c1", 100, "A", "T", "T", af.SNV), ("c1", 103, "T", "A", "A", af.SNV), ("c1", 50, "G", "T", "T", af.SNV),
                                      ("c1", 200, "A", "G", "G", af.SNV), ("c1", 201, "C", "T", "T", af.SNV)]
    assert vs.sets == [sv.PhaseSet("c1:100", "c1", (0, 1)), sv.PhaseSet("c1:200", "c1", (3, 4))]
    assert sv.leaders(vs) == [100, 100, 50, 200, 200] and sv.phase_sets(vs) == vs.sets
    assert vs.mnvs == [("c1", 100, "ACGT", 2), ("c1", 200, "AC", 4)]
    # an MNV with one differing letter is a set of one: its draw is a singleton's, and no page reports it
    one = sv.parse_variants(_write(tmp_path, "c1\t100\tACG\tATG\n", "one.txt"), phased=True)
    assert [tuple(v)[:4] for v in one] == [("c1", 101, "C", "T")] and sv.leaders(one) == [101] and sv.phase_sets(one) == []
    # lower case is upper-cased, as for SNVs
    assert [v.alt for v in sv.parse_variants(_write(tmp_path, "c1\t7\tac\tgt\n", "low.txt"), phased=True)] == ["G", "T"]


def test_ps_sets_and_an_mnv_that_joins_one(tmp_path):
    text = ("c1\t300\t.\tA\tC\t.\t.\tDP=3;PS=h1\n" "c1\t10\t.\tG\tT\t.\t.\tPS=h2\n" "c1\t90\t.\tAC\tGT\t.\t.\tPS=h1;X\n" "c2\t5\t.\tA\tC\t.\t.\tPS=h3\n"
            "c1\t500\t.\tT\tG\t.\t.\tXPS=h1\n" "c1\t20\t.\tC\tA\t.\t.\tPS=h2\n" "c1\t400\tA\tT\n")
    vs = sv.parse_variants(_write(tmp_path, text), phased=True)
    assert [(v.chrom, v.pos) for v in vs] == [("c1", 300), ("c1", 10), ("c1", 90), ("c1", 91), ("c2", 5), ("c1", 500), ("c1", 20), ("c1", 400)]
    # members ascending by position; the leader is the smallest position, not the first line
    assert vs.sets == [sv.PhaseSet("h1", "c1", (2, 3, 0)), sv.PhaseSet("h2", "c1", (1, 6)), sv.PhaseSet("h3", "c2", (4,))]
    assert sv.leaders(vs) == [90, 10, 90, 90, 5, 500, 10, 400]
    assert [s.name for s in sv.phase_sets(vs)] == ["h1", "h2"]
    # PS= on a four-column line is not read (there is no eighth column); without the flag PS= is ignored altogether
    plain = sv.parse_variants(_write(tmp_path, "c1\t300\t.\tA\tC\t.\t.\tPS=h1\nc1\t310\t.\tA\tC\t.\t.\tPS=h1\n", "p.vcf"))
    assert type(plain) is list and sv.leaders(plain) == [300, 310]


def _refusals():
    nine = "ACGTACGTA"
    return (("c1\t10\tACG\tAC\n", "different lengths"), ("c1\t10\tAC\tACGG\n", "different lengths"),
            ("c1\t10\t%s\t%s\n" % (nine, nine[::-1]), "an MNV of 9 letters, at most 8"), ("c1\t10\tACG\tACG\n", "do not differ in any letter"),
            ("c1\t10\tANG\tTNC\n", "must be made of A, C, G, T"),
            ("".join("c1\t%d\t.\tA\tC\t.\t.\tPS=big\n" % (10 * k) for k in range(1, 10)), "the phase set big has 9 members, at most 8"),
            ("c1\t10\t.\tACGTA\tTGCAT\t.\t.\tPS=big\nc1\t30\t.\tACGT\tTGCA\t.\t.\tPS=big\n", "has 9 members"),
            ("c1\t10\t.\tA\tC\t.\t.\tPS=h\nc2\t10\t.\tA\tC\t.\t.\tPS=h\n", "PS=h is listed on c1 and on c2"),
            ("c1\t10\tAC\tGT\nc1\t11\tC\tA\n", "c1:11 is listed twice"), ("c1\t11\tC\tA\nc1\t10\tAC\tGT\n", "c1:11 is listed twice"),
            ("c1\t10\tA\tAGG\n", "only one-letter substitutions"), ("c1\t10\tAGG\tA\n", "only one-letter substitutions"),
            ("c1\t10\tA\tN\n", "must be one of A, C, G, T"), ("c1\t10\tA\tC,G\n", "more than one allele"), ("c1\tx\tA\tC\n", "not an integer"),
            ("c1\t0\tA\tC\n", "1-based"), ("c1\t10\tA\n", "3 tab-separated columns"), ("# nothing\n", "lists no variant"),
            ("c1\t10\tA\tA\n", "neither a substitution"))


def test_every_refusal_names_its_line_and_comes_before_any_file(tmp_path):
    bam, fa, loci, P = ds_restate.load_fixture("bam_cigars", str(tmp_path))
    before = sorted(os.listdir(str(tmp_path)))
    ns = NS(spikeVariants=str(tmp_path / "bad.vcf"), spikePhase=True, outPrefix=str(tmp_path / "o"))
    ref = fasta.FastaFile(fa)
    loc_list = [(c, str(p)) for c, p in loci]
    for k, (text, msg) in enumerate(_refusals()):
        _write(tmp_path, text, "bad.vcf")
        with pytest.raises(ValueError, match=re.escape(msg)) as e:
            sv.parse_variants(ns.spikeVariants, "--spikeVariants", phased=True)
        if k < 10:                                  # (the new refusals name the file and the line; the others keep today's text)
            assert re.search(r"bad\.vcf line \d+", str(e.value)), str(e.value)
        with pytest.raises(SystemExit, match=re.escape(msg)):
            spike.variants(ns, loc_list, ref)
    # with the genome: an MNV whose unchanged middle letter is not the genome's is refused too
    c, p = loci[0]
    letters = ref.fetch(c, p - 1, p + 2).upper()
    other = lambda x: "ACGT"[("ACGT".index(x) + 1) % 4]
    _write(tmp_path, "%s\t%d\t%s\t%s\n" % (c, p, letters[0] + other(letters[1]) + letters[2], other(letters[0]) + other(letters[1]) + other(letters[2])),
           "bad.vcf")
    with pytest.raises(SystemExit, match="the reference genome has"):
        spike.variants(ns, loc_list, ref)
    _write(tmp_path, "%s\t%d\t%s\t%s\n" % (c, p, letters, other(letters[0]) + letters[1] + other(letters[2])), "bad.vcf")
    good = spike.variants(ns, loc_list, ref)
    assert [v.pos for v in good] == [p, p + 2] and len(good.sets) == 1
    assert sorted(set(os.listdir(str(tmp_path))) - set(before)) == ["bad.vcf"]


def test_without_the_flag_an_mnv_file_fails_with_the_old_text(tmp_path):
    path = _write(tmp_path, "c1\t100\tAC\tGT\n")
    old = "REF 'AC' / ALT 'GT' is neither a substitution of one letter, an insertion (X / XS) nor a deletion (XD / X)"
    for call in (lambda: sv.parse_variants(path), lambda: sv.parse_variants(path, "--spikeVariants", phased=False), lambda: af.parse_variants(path)):
        with pytest.raises(ValueError, match=re.escape(old)):
            call()
    with pytest.raises(SystemExit, match=re.escape(old)):
        spike.variants(NS(spikeVariants=path), [], None)
    with pytest.raises(SystemExit, match=re.escape(old)):
        sv.main(NS(runPath=None, inBam="none.bam", outBam=str(tmp_path / "o.bam"), variants=path, af="0.1", seed=1, refGenome=None))
    assert os.listdir(str(tmp_path)) == ["v.vcf"]


def test_draws_a_singleton_is_todays_members_share_neighbours_do_not_and_sets_are_nested(tmp_path):
    texts = ["ACGTACGT%04d" % k for k in range(600)]
    ids = PR.idents(texts)
    path = _write(tmp_path, "c1\t100\tACGT\tTCGA\nc1\t110\tA\tC\nc1\t111\tC\tG\n")
    vs = sv.parse_variants(path, phased=True)
    last = None
    for t in (0.05, 0.3, 0.7):
        plan = sv.Plan(vs, t, SEED)
        hit = [{b for b in ids.tolist() if plan.is_spiked(k, b)} for k in range(len(vs))]
        # a singleton's draw is sv.draw at its own position; the tool's draw is the restatement's
        for k in (2, 3):
            assert hit[k] == set(ids[sv.draw(ids, SEED, vs[k].pos) < np.uint64(sv.threshold(t))].tolist())
        assert np.array_equal(sv.draw(ids, SEED, 100), SR.draw(texts, SEED, 100))
        # the members of a set: exactly the same barcodes, those of the leader's position
        assert hit[0] == hit[1] == set(ids[sv.draw(ids, SEED, 100) < np.uint64(sv.threshold(t))].tolist()) and hit[0]
        assert hit[1] != set(ids[sv.draw(ids, SEED, 103) < np.uint64(sv.threshold(t))].tolist())
        # two unphased neighbours are not
        assert hit[2] != hit[3]
        unphased = sv.Plan(list(vs), t, SEED)
        assert {b for b in ids.tolist() if unphased.is_spiked(1, b)} != hit[0]
        if last is not None:
            assert all(a <= b for a, b in zip(last, hit))
        last = hit


def _case(tmp):
    """The hand-made BAM with (P1, P1 + 7) as one MNV line - both inside the `first` shape's reads, as the two_positions pair is, which
    lies 10 letters apart and so cannot be one MNV line of at most 8 - and P3 as a singleton -> (bam, fa, loci, P, variants, sets,
    the variants file)."""
    bam, fa, loci, P, given = SR.make_case(tmp)
    ref = fasta.FastaFile(fa).fetch(SR.CASE_CHROM, SR.P1 - 1, SR.P1 + 7).upper()
    other = lambda c: "ACGT"[("ACGT".index(c) + 1) % 4]
    variants = [SR.V(SR.CASE_CHROM, SR.P1, ref[0], other(ref[0]), other(ref[0])), SR.V(SR.CASE_CHROM, SR.P1 + 7, ref[7], other(ref[7]), other(ref[7])),
                given[2]]
    vfile = _write(tmp, PH.mnv_line(SR.CASE_CHROM, SR.P1, ref, {0: variants[0].alt, 7: variants[1].alt}, vcf=False) +
                   "%s\t%d\t%s\t%s\n" % (SR.CASE_CHROM, given[2].pos, given[2].ref, given[2].alt), "mnv.txt")
    return bam, fa, loci, P, variants, [(0, 1)], vfile


def _tool(bam, fa, vfile, t, out, phased=True):
    return sv.main(NS(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=SEED, refGenome=fa, phased=phased))


@pytest.mark.parametrize("t", (0.5, 0.15))
def test_tool_phased_equals_the_restatement_record_for_record(tmp_path, t):
    tmp = str(tmp_path)
    bam, fa, loci, P, variants, sets, vfile = _case(tmp)
    records, stats = PH.restate(bam, fa, variants, sets, t, SEED, P.mismatchThr)
    out = os.path.join(tmp, "out.bam")
    rows = _tool(bam, fa, vfile, t, out)
    got, want = SR.file_records(out), SR.expected_records(bam, records)
    assert len(got) == len(want) and all(g == w for g, w in zip(got, want))
    for row, s in zip(rows, stats):
        assert row == {k: s[k] for k in ("N", "V0", "S", "READS", "V1")}
    # the members are spiked on the same barcodes (among those that cover both), the singleton on others
    both = stats[0]["spiked"] & stats[1]["spiked"]
    joint = PH.host_joint(bam, fa, variants, sets)[0][0]
    assert {b for b in stats[0]["spiked"] if b in joint} == {b for b in stats[1]["spiked"] if b in joint} == both & set(joint) and both
    # NM + 2 on exactly the records that showed REF at both positions and belong to a spiked barcode
    before = {(r[0], r[1], r[2]): r for r in SR.file_records(bam)}
    plus2 = 0
    for g in got:
        b = before[(g[0], g[1], g[2])]
        r = records.get((g[0], g[1], g[2]))
        if r is not None and r["inc"] == 2:
            assert g[6] == b[6] + 2 and sorted(r["old"].values()) == sorted(v.ref for v in variants[:2])
            plus2 += 1
        if af.barcode_of(g[0]) not in set().union(*(s["spiked"] for s in stats)):
            assert g == b                                                        # an unspiked barcode's records are untouched
    assert plus2 > 0
    # a record that spans both members (the `first` shape: P1 its query position 0, P1 + 7 its 7) is rewritten at both or at neither
    spans = [r for key, r in records.items() if key[0].startswith("mfirst")]
    assert spans and all(len([q for q in r["edits"] if q in (0, 7)]) in (0, 2) for r in spans)
    assert any(len(r["edits"]) == 2 for r in spans) and any(not r["edits"] for r in spans)
    # unphased, the same two positions land on different barcodes: the restatement without sets is another file
    _, loose = PH.restate(bam, fa, variants, [], t, SEED, P.mismatchThr)
    assert loose[1]["spiked"] != stats[1]["spiked"] and loose[0]["spiked"] == stats[0]["spiked"]


def test_tool_phased_on_the_two_positions_pair_as_a_ps_set_and_equal_to_unphased_without_sets(tmp_path):
    tmp = str(tmp_path)
    bam, fa, loci, P, variants = SR.make_case(tmp)
    vfile = _write(tmp, PH.snv_line(variants[1], "hap") + PH.snv_line(variants[2]) + PH.snv_line(variants[0], "hap"))
    order = [variants[1], variants[2], variants[0]]
    records, stats = PH.restate(bam, fa, order, [(0, 2)], 0.5, SEED, P.mismatchThr)
    out = os.path.join(tmp, "ps.bam")
    rows = _tool(bam, fa, vfile, 0.5, out)
    assert SR.file_records(out) == SR.expected_records(bam, records)
    assert [r["S"] for r in rows] == [s["S"] for s in stats]
    assert any(r["inc"] == 2 for r in records.values() if "two_positions" in r["notes"])
    # no set listed: --phased writes byte for byte what the tool writes without it
    plain = _write(tmp, "".join(PH.snv_line(v) for v in variants), "plain.vcf")
    a, b = os.path.join(tmp, "a.bam"), os.path.join(tmp, "b.bam")
    assert _tool(bam, fa, plain, 0.5, a, phased=True) == _tool(bam, fa, plain, 0.5, b, phased=False)
    assert open(a, "rb").read() == open(b, "rb").read()


def test_joint_counts_of_the_restatement_are_consistent(tmp_path):
    """The restatement's own two ways: the joint counts from the counters and the draws equal those counted on restate()'s spiked
    sets, and M = 1 gives spike_depth_restate's columns."""
    import spike_depth_restate as DS
    tmp = str(tmp_path)
    bam, fa, loci, P, variants, sets, _ = _case(tmp)
    targets, fracs = (0.15, 0.5), (0.4, 1.0)
    counts, joint = PH.restate_counts(bam, fa, variants, sets + [(2,)], targets, fracs, SEED, 2)
    assert counts.shape == (2, 2, 2, 2, 4)
    for j, s in enumerate(PR.seeds(SEED, 2)):
        for t, target in enumerate(targets):
            _, stats = PH.restate(bam, fa, variants, sets, target, s, P.mismatchThr)
            names = joint[0][0]
            assert counts[0, j, t, 1, 0] == len(names) and counts[0, j, t, 1, 2] == len(set(names) & stats[0]["spiked"] & stats[1]["spiked"])
    single, _ = DS.restate_counts(bam, fa, variants[2:], targets, fracs, SEED, 2)
    assert np.array_equal(counts[1], single[0][..., [0, 1, 2, 4]])
    assert (counts[0, :, :, 0, 0] <= counts[0, :, :, 1, 0]).all() and (counts[..., 3] <= counts[..., 0]).all()


def _set():
    vs = [R.V("chr1", 100, "A", "G", "G"), R.V("chr1", 103, "C", "T", "T"), R.V("chr1", 50, "G", "A", "A")]
    return vs, sv.PhaseSet("chr1:100", "chr1", (0, 1))


def test_phase_lines_on_hand_made_rows():
    vs, ps = _set()
    assert spike.PHASE_HEADER == ("SET", "CHROM", "POSITIONS", "REFS", "ALTS", "TARGET", "FRACTION", "MTDEPTH", "N_ALL", "V0_ALL", "S_ALL", "V1_ALL",
                                  "AF_ALL", "CALLED_ALL")
    assert spike.PHASE_REPLICATES_HEADER == spike.PHASE_HEADER[:8] + ("REP", "SEED") + spike.PHASE_HEADER[8:]
    r = dict(N_ALL=3000, V0_ALL=1, S_ALL=14, V1_ALL=15)
    assert spike.phase_line(ps, vs, None, None, 3500, dict(r, S_ALL=0, V1_ALL=1), 0) == \
        "chr1:100\tchr1\t100,103\tA,C\tG,T\tfull\tfull\t3500\t3000\t1\t0\t1\t0.000333\t0"
    assert spike.phase_line(ps, vs, 0.005, 0.5, 1750, r, 1) == "chr1:100\tchr1\t100,103\tA,C\tG,T\t0.005\t0.5\t1750\t3000\t1\t14\t15\t0.005\t1"
    assert spike.phase_line(ps, vs, 0.005, None, 10, dict(N_ALL=0, V0_ALL=0, S_ALL=0, V1_ALL=0), 0).split("\t")[8:] == ["0", "0", "0", "0", "0.0", "0"]
    assert spike.phase_replicate_line(ps, vs, 0.005, None, 3500, 2, 99, r, 1).split("\t")[5:12] == ["0.005", "full", "3500", "2", "99", "3000", "1"]
    cut = {("chr1", "100"): ("A", ["G"]), ("chr1", "103"): ("C", ["A", "T"]), ("chr1", "50"): ("G", ["A"])}
    assert spike.called_all(ps, vs, cut) == 1
    assert spike.called_all(ps, vs, {**cut, ("chr1", "103"): ("C", ["A"])}) == 0                  # another ALT
    assert spike.called_all(ps, vs, {k: v for k, v in cut.items() if k != ("chr1", "100")}) == 0      # a member not cut


def test_phase_sensitivity_line_against_wilson():
    vs, ps = _set()
    per = [(dict(N_ALL=100, V0_ALL=0, S_ALL=4, V1_ALL=4), 1), (dict(N_ALL=100, V0_ALL=0, S_ALL=7, V1_ALL=6), 0),
           (dict(N_ALL=90, V0_ALL=0, S_ALL=9, V1_ALL=9), 1), (dict(N_ALL=0, V0_ALL=0, S_ALL=0, V1_ALL=0), 0)]
    f = spike.phase_sensitivity_line(ps, vs, 0.05, 0.5, 50, per).split("\t")
    assert tuple(spike.PHASE_SENSITIVITY_HEADER[8:]) == ("REPS", "CALLED_ALL", "RATE", "LO95", "HI95", "AF_MEAN", "AF_MIN", "AF_MAX")
    lo, hi = dsaf.wilson(2, 4)
    assert (lo, hi) == pytest.approx(PR.wilson(2, 4))
    assert f[:8] == ["chr1:100", "chr1", "100,103", "A,C", "G,T", "0.05", "0.5", "50"]
    assert f[8:] == ["4", "2", "0.5", dsaf.frac_text(lo), dsaf.frac_text(hi), dsaf.frac_text((0.04 + 0.06 + 0.1 + 0.0) / 4), "0.0", "0.1"]


def test_phase_files_on_hand_made_rows(tmp_path):
    from smcounter_amd.rows import HEADER_ALL
    vs, ps = _set()
    prefixes = [str(tmp_path / p) for p in ("o", "o.spikeAF0.1", "o.spikeAF0.1.dsMT0.5")]
    for k, prefix in enumerate(prefixes):
        open(prefix + ".smCounter.all.txt", "w").write("\t".join(HEADER_ALL) + "\n")
        open(prefix + ".smCounter.cut.txt", "w").write("CHROM\tPOS\tREF\tALT\n" + ("chr1\t100\tA\tG\n" if k else "") + ("chr1\t103\tC\tT\n" if k == 1 else ""))
    r = dict(N_ALL=40, V0_ALL=0, S_ALL=5, V1_ALL=5)
    outs = [(None, None, 80, prefixes[0], [dict(r, S_ALL=0, V1_ALL=0)]), (0.1, None, 80, prefixes[1], [r]),
            (0.1, 0.5, 40, prefixes[2], [dict(r, N_ALL=20, S_ALL=2, V1_ALL=2)])]
    spike.write_phase(prefixes[0], vs, [ps], outs)
    lines = [l.split("\t") for l in open(prefixes[0] + ".spikeAF.phase.txt").read().splitlines()]
    assert lines[0] == list(spike.PHASE_HEADER) and len(lines) == 4
    assert [l[5:] for l in lines[1:]] == [["full", "full", "80", "40", "0", "0", "0", "0.0", "0"], ["0.1", "full", "80", "40", "0", "5", "5", "0.125", "1"],
                                         ["0.1", "0.5", "40", "20", "0", "2", "2", "0.1", "0"]]
    entries = {(0, 0): [(r, 1), (dict(r, S_ALL=3, V1_ALL=3), 0)], (0, 1): [(dict(r, N_ALL=20), 0), (dict(r, N_ALL=25), 0)]}
    spike.write_phase_replicates(prefixes[0], vs, [ps], [(0.1, None, 80), (0.1, 0.5, 40)], [7, 8], entries)
    reps = [l.split("\t") for l in open(prefixes[0] + ".spikeAF.phase.replicates.txt").read().splitlines()]
    assert reps[0] == list(spike.PHASE_REPLICATES_HEADER) and [l[5:10] for l in reps[1:]] == \
        [["0.1", "full", "80", "0", "7"], ["0.1", "full", "80", "1", "8"], ["0.1", "0.5", "40", "0", "7"], ["0.1", "0.5", "40", "1", "8"]]
    spike.write_phase_sensitivity(prefixes[0], vs, [ps], [(0.1, None, 80), (0.1, 0.5, 40)], entries)
    sens = [l.split("\t") for l in open(prefixes[0] + ".spikeAF.phase.sensitivity.txt").read().splitlines()]
    assert sens[0] == list(spike.PHASE_SENSITIVITY_HEADER) and len(sens) == 3
    assert sens[1] == spike.phase_sensitivity_line(ps, vs, 0.1, None, 80, entries[(0, 0)]).split("\t") and sens[1][8:11] == ["2", "1", "0.5"]


def test_the_entry_is_declared():
    h = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"#define SMC_ABI_VERSION 11\b", h) and re.search(r"#define SMC_SPIKE_PHASE_MAX_MEMBERS 8\b", h)
    assert re.search(r"\bint smc_spike_phase_counts\(smc_ctx\* ctx, const uint64_t\* d_joint_ident, const uint32_t\* d_joint_cnt,", h)
    assert re.search(r"uint16_t lead;", h) and "uint8_t pad[2]" not in h[h.index("typedef struct smc_spike_variant"):h.index("} smc_spike_variant;")]
    assert "smc_spike_phase_counts" in _lib.SYMBOLS
    assert abi.SPIKE_VARIANT_DTYPE.itemsize == 16 and abi.SPIKE_VARIANT_DTYPE.fields["lead"][1] == 6 and abi.SPIKE_VARIANT_DTYPE.fields["thr"][1] == 8
    assert abi.SPIKE_PHASE_MAX_MEMBERS == sv.PHASE_MAX_MEMBERS == 8
    L = _lib.load()
    assert L.smc_abi_version() == 11 and hasattr(L, "smc_spike_phase_counts")


def test_spike_set_fills_lead_per_chromosome(tmp_path):
    from smcounter_amd import devplanes
    text = ("c1\t300\t.\tA\tC\t.\t.\tPS=h1\n" "c1\t10\t.\tG\tT\t.\t.\t.\n" "c1\t90\t.\tAC\tGT\t.\t.\tPS=h1\n" "c2\t5\t.\tAC\tCA\t.\t.\t.\n" "c1\t95\t.\tT\tG\t.\t.\t.\n")
    vs = sv.parse_variants(_write(tmp_path, text), phased=True)
    s = devplanes.SpikeSet(vs)
    var, order = s.chrom_variants("c1", 0.25)
    assert var["pos0"].tolist() == [9, 89, 90, 94, 299] and var["lead"].tolist() == [0, 0, 1, 0, 3] and order == [1, 2, 3, 6, 0]
    assert (var["thr"] == sv.threshold(0.25)).all()
    assert s.chrom_variants("c2", 0.25)[0]["lead"].tolist() == [0, 1]
    assert s.lead_pos == [90, 10, 90, 90, 5, 5, 95]
    assert not devplanes.SpikeSet(list(vs)).chrom_variants("c1", 0.25)[0]["lead"].any()     # (a plain list: no sets, today's records)
