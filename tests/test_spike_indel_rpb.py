"""--spikeIndelRpb without a GPU: the flag's parsing and every refusal (before any file), --spikeRpb's refusals of the indel flags as
they were, the two ABI entries' declarations, and the restatement's own properties (tests/spike_indel_rpb_restate.py) - on an SNV-only
list it is the --spikeRpb restatement word for word, at the full read threshold the --spikeIndelReps restatement, the kept sets are
nested in r and the hit sets in t - and the conditions on the GPU tests' synthetic input: every case that makes four bits necessary
occurs at a listed indel, and thinning bites on an indel."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, cli, devplanes, spike
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import spike_indel_reps_restate as QR  # noqa: E402
import spike_indel_restate as IR  # noqa: E402
import spike_indel_rpb_restate as XR  # noqa: E402
import spike_restate as SR  # noqa: E402
import spike_rpb_restate as RR  # noqa: E402
import test_spike_indels as TI  # noqa: E402  (its command line on bam_cigars)

SEED = XR.SEED
ONE = 1 << 32
TARGETS = (0.05, 0.3, 0.7)
NS = lambda **kw: argparse.Namespace(**kw)
CLI_TARGETS = [(0.01, 100, "o.spikeAF0.01"), (0.05, 25, "o.spikeAF0.05")]


# ---- the command line
def test_flag_is_parsed_into_cells():
    ns = cli.build_parser().parse_args("--outPrefix o --bamFile b --bedTarget t --mtDepth 3 --rpb 2 --spikeIndelRpb 1.5,3 --spikeIndelReps 4".split())
    assert ns.spikeIndelRpb == "1.5,3" and ns.spikeRpb is None
    assert spike.indel_flags(ns, CLI_TARGETS) == (4, None)                              # (the flag is checked there; its text is the cells')
    assert spike.indel_flags(NS(spikeIndelRpb="2"), CLI_TARGETS) == (None, None)
    rs, cells = spike.indel_rpb_cells(ns, CLI_TARGETS)
    assert rs == [1.5, 3.0]
    assert cells == [(0, 0.01, 1.5, 100, "o.spikeAF0.01.dsRpb1.5"), (0, 0.01, 3.0, 100, "o.spikeAF0.01.dsRpb3"),
                     (1, 0.05, 1.5, 25, "o.spikeAF0.05.dsRpb1.5"), (1, 0.05, 3.0, 25, "o.spikeAF0.05.dsRpb3")]
    assert (rs, cells) == spike.rpb_cells(NS(spikeRpb="1.5,3"), CLI_TARGETS)            # (--spikeRpb's cells: one output kind, one set of writers)
    assert spike.indel_rpb_cells(NS(), CLI_TARGETS) == (None, []) and spike.rpb_cells(ns, CLI_TARGETS) == (None, [])


@pytest.mark.parametrize("kw, tg, msg", (
    (dict(spikeIndelRpb="2"), [], "--spikeIndelRpb thins the reads of the --spikeAF spike-ins, insertions and deletions among them: it needs --spikeAF"),
    (dict(spikeIndelRpb="2", spikeRpb="2"), CLI_TARGETS, "--spikeIndelRpb takes the targets"),
    (dict(spikeIndelRpb="2", spikeIndels=True), CLI_TARGETS, "--spikeIndelRpb implies the rules of --spikeIndels: leave --spikeIndels out"),
    (dict(spikeIndelRpb="2", spikeReps=4), CLI_TARGETS, "--spikeIndelRpb cannot be combined with --spikeReps in one run: --spikeIndelReps R replicates"),
    (dict(spikeIndelRpb="2", spikeDepth="0.5"), CLI_TARGETS, "--spikeIndelRpb cannot be combined with --spikeDepth in one run: --spikeIndelDepth takes"),
    (dict(spikeIndelRpb="2", spikePhase=True), CLI_TARGETS, "--spikeIndelRpb cannot be combined with --spikePhase in one run"),
    (dict(spikeIndelRpb="2", spikeIndelDepth="0.5"), CLI_TARGETS, "--spikeIndelRpb cannot be combined with --spikeIndelDepth in one run .the combination is not built"),
    (dict(spikeIndelRpb="2", spikeIndelReps=4, spikeIndelDepth="0.5"), CLI_TARGETS, "--spikeIndelDepth in one run .the combination is not built"),
    (dict(spikeIndelRpb="2", spikeIndelPhase=True), CLI_TARGETS, "--spikeIndelRpb cannot be combined with --spikeIndelPhase in one run .the combination is not built"),
    (dict(spikeIndelRpb="2", spikeIndelReps=1), CLI_TARGETS, r"--spikeIndelReps: the number of replicates must lie in 2 \.\. 1000, got 1")))
def test_flag_refusals(kw, tg, msg):
    with pytest.raises(SystemExit, match=msg):
        spike.indel_flags(NS(**kw), tg)


@pytest.mark.parametrize("text, tg, msg", (
    ("2", [], "it needs --spikeAF"), ("a,b", CLI_TARGETS, "--spikeIndelRpb: comma-separated reads-per-barcode targets > 0 expected"),
    ("2;3", CLI_TARGETS, "--spikeIndelRpb: comma-separated reads-per-barcode targets"), ("0", CLI_TARGETS, "--spikeIndelRpb: every target must be a number > 0"),
    ("2,-1", CLI_TARGETS, "must be a number > 0"), (",", CLI_TARGETS, "must be a number > 0"), ("nan", CLI_TARGETS, "must be a number > 0"),
    ("inf", CLI_TARGETS, "must be a number > 0"), ("2,2.0", CLI_TARGETS, "--spikeIndelRpb: a target is listed twice"),
    (",".join("%g" % (1 + 0.1 * k) for k in range(17)), CLI_TARGETS, "--spikeIndelRpb: 2 targets x 17 reads-per-barcode targets = 34 cells, at most 32")))
def test_target_refusals(text, tg, msg):
    with pytest.raises(SystemExit, match=msg):
        spike.indel_rpb_cells(NS(spikeIndelRpb=text), tg)


def test_refused_before_any_file_is_written(tmp_path):
    """The command line itself ends the run before it opens anything (the BAM named here does not exist)."""
    base = dict(outPrefix=str(tmp_path / "o"), bamFile=str(tmp_path / "none.bam"), bedTarget=str(tmp_path / "none.bed"), mtDepth=10, rpb=2.0,
                refGenome=str(tmp_path / "none.fa"))
    sp = dict(spikeAF="0.1", spikeVariants="v")
    for more, msg in ((dict(spikeIndelRpb="2"), "it needs --spikeAF"), (dict(spikeAF="0.1", spikeIndelRpb="2"), "it needs --spikeVariants"),
                      (dict(sp, spikeIndelRpb="2", spikeRpb="2"), "--spikeIndelRpb takes the targets"),
                      (dict(sp, spikeIndelRpb="2", spikeIndels=""), "leave --spikeIndels out"),
                      (dict(sp, spikeIndelRpb="2", spikeReps=4), "--spikeIndelReps R replicates the spike-ins itself"),
                      (dict(sp, spikeIndelRpb="2", spikeDepth="0.5"), "--spikeIndelDepth takes the barcode fractions"),
                      (dict(sp, spikeIndelRpb="2", spikePhase=""), "cannot be combined with --spikePhase"),
                      (dict(sp, spikeIndelRpb="2", spikeIndelDepth="0.5"), "--spikeIndelRpb cannot be combined with --spikeIndelDepth"),
                      (dict(sp, spikeIndelRpb="2", spikeIndelPhase=""), "--spikeIndelRpb cannot be combined with --spikeIndelPhase"),
                      (dict(sp, spikeIndelRpb="x"), "comma-separated reads-per-barcode targets"), (dict(sp, spikeIndelRpb="2,0"), "must be a number > 0"),
                      (dict(sp, spikeIndelRpb="2,2"), "listed twice"),
                      (dict(sp, spikeIndelRpb=",".join("%g" % (1 + 0.1 * k) for k in range(33))), "at most 32"),
                      (dict(sp, spikeIndelRpb="2", spikeIndelReps=1), "must lie in"),
                      # what --spikeAF refuses
                      (dict(sp, spikeIndelRpb="2", spikeAF="1.5"), "--spikeAF"), (dict(sp, spikeIndelRpb="2", spikeAF="0.1,0.10"), "listed twice"),
                      (dict(sp, spikeIndelRpb="2", dsRpb="2"), r"--spikeAF cannot be combined with --dsRpb in one run \(spike-ins on a down-sampled file are not built\)"),
                      (dict(sp, spikeIndelRpb="2", dsMT="0.5"), "cannot be combined with --dsMT"),
                      # --spikeRpb beside the indel flags: today's messages
                      (dict(sp, spikeRpb="2", spikeIndels=""), "--spikeRpb cannot be combined with --spikeIndels in one run .the combination is not built"),
                      (dict(sp, spikeRpb="2", spikeIndelReps=3), "--spikeRpb cannot be combined with --spikeIndelReps in one run .the combination is not built"),
                      (dict(sp, spikeRpb="2", spikeIndelDepth="0.5"), "--spikeRpb cannot be combined with --spikeIndelDepth in one run"),
                      (dict(sp, spikeRpb="2", spikeIndelPhase=""), "--spikeRpb cannot be combined with --spikeIndelPhase in one run")):
        given = dict(base, **more)
        ns = cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in given.items() if v != ""] + ["--" + k for k, v in given.items() if v == ""])
        with pytest.raises(SystemExit, match=msg):
            cli.main(ns)
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("kw,lines,msg", [
    (dict(spikeIndelRpb="2"), lambda c, p, s: "%s\t%d\t%sC\t%sGG\n" % (c, p, s[0], s[0]), "neither a substitution"),
    (dict(spikeIndelRpb="2"), lambda c, p, s: "%s\t%d\t%s\t%sG\n%s\t%d\t%s\t%s\n" % (c, p, s[0], s[0], c, p + 1, s[1], "ACGT"[("ACGT".index(s[1]) + 1) % 4]),
     "lies in the footprint"),
    (dict(spikeIndelRpb="2", spikeIndelReps="3"), lambda c, p, s: "%s\t%d\t%s%s\t%s\n" % (c, p, s[0], "ACGT"[("ACGT".index(s[1]) + 1) % 4] + s[2], s[0]),
     "the reference genome has"),
    (dict(spikeIndelRpb="2"), lambda c, p, s: "%s\t%d\t%s\t%sG\n" % (c, p + 100000, s[0], s[0]), "is not a locus of --bedTarget|the reference genome has"),
    # --spikeRpb does not take the indel line --spikeIndelRpb takes: its refusal, as it was
    (dict(spikeRpb="2"), None, "only one-letter substitutions"),
])
def test_what_spike_indels_refuses_of_the_variants_file_before_any_file(tmp_path, kw, lines, msg):
    ns = TI._args(tmp_path, lines, **kw)
    with pytest.raises(SystemExit, match=msg if "|" in msg else re.escape(msg)):
        cli.main(ns)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def test_the_pre_pass_refuses_what_it_refused_and_names_the_flag(tmp_path):
    bam, fa, loci, P, variants = IR.make_case(str(tmp_path))
    assert any(v.kind != af.SNV for v in variants)
    rpb = dict(targets=[2.0], params=[P])
    not_built = "^--spikeRpb: cells of barcode depths, phase sets or indel spike-ins are not built$"
    # (raised before the engine is touched: None stands for it)
    with pytest.raises(ValueError, match=not_built):                                     # --spikeRpb with an indel in the list: as it was
        devplanes.spike_rules(bam, None, variants, [0.5], [P], SEED, None, rpb=dict(rpb))
    with pytest.raises(ValueError, match=not_built):                                     # cells of barcode depths stay refused under the new flag
        devplanes.spike_rules(bam, None, variants, [0.5], [P], SEED, None, rpb=dict(rpb), indel_counters=True, depth=dict(fracs=[0.5], params=[P]))
    with pytest.raises(ValueError, match=not_built):                                     # phase sets too
        devplanes.spike_rules(bam, None, variants, [0.5], [P], SEED, None, rpb=dict(rpb), indel_counters=True, phase=dict(sets=[]))
    spikes = devplanes.SpikeSet(variants, indels=True)
    cell = devplanes.DsRule(1.0, None, seed=7, level="read", target=1.5, prob_keep=0.25, groups=object(), thr=1 << 30, af=0.05, spike=spikes)
    assert cell.spike_rpb_cell and cell.flag == "--spikeIndelRpb" and cell.label == "spiked allele fraction 0.05 x target 1.5"
    snvs = devplanes.SpikeSet([v for v in variants if v.kind == af.SNV])
    assert devplanes.DsRule(1.0, None, level="read", target=1.5, groups=object(), thr=1, af=0.05, spike=snvs).flag == "--spikeRpb"


def test_the_entries_are_declared():
    text = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"#define SMC_ABI_VERSION 11\b", text)
    assert re.search(r"\bint smc_spike_indel_read_bits\(smc_ctx\* ctx, const smc_dev_aln\* d_aln,", text)
    assert re.search(r"\bint smc_spike_indel_rpb_counts\(smc_ctx\* ctx, const uint64_t\* d_cov_ident,", text)
    assert "smc_spike_indel_read_bits" in _lib.SYMBOLS and "smc_spike_indel_rpb_counts" in _lib.SYMBOLS
    L = _lib.load()
    assert L.smc_abi_version() == 11
    assert len(L.smc_spike_indel_read_bits.argtypes) == 17 and len(L.smc_spike_indel_rpb_counts.argtypes) == 19
    assert len(L.smc_spike_read_bits.argtypes) == 15 and len(L.smc_spike_rpb_counts.argtypes) == 19
    kernels = open(os.path.join(ROOT, "smcounter_amd", "csrc", "k_spike_rpb.inc")).read()
    # ONE counts kernel body for both entries; the touch bit from the rewrite's own walk
    assert len(re.findall(r"void k_spr_counts\(", kernels)) == 1 and "spi_walk<false, SPI_TOUCH_ONE>" in kernels and "asm" not in kernels
    assert (devplanes.SPB_COVERS, devplanes.SPB_ALT, devplanes.SPB_ALT1, devplanes.SPB_TOUCH) == (XR.COVERS, XR.ALT0, XR.ALT1, XR.TOUCH)


# ---- the restatement's own properties
@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """The GPU tests' synthetic input, its covering records and its read thresholds (computed once, only read)."""
    bam, fa, P, variants = XR.synth_inputs(str(tmp_path_factory.mktemp("irpb")))
    groups = XR.file_groups(bam)
    return bam, fa, variants, XR.records(bam, fa, variants, groups), XR.read_thresholds(groups, XR.RPB_TARGETS)


def test_on_snvs_it_is_the_spike_rpb_restatement_word_for_word(tmp_path):
    bam, fa, P, snvs = RR.synth_inputs(str(tmp_path))
    variants = [IR.variant(v.chrom, v.pos, v.ref, v.alt) for v in snvs]
    theirs, their_recs, rthr = RR.restate_counts(bam, fa, snvs, TARGETS, RR.RPB_TARGETS, SEED, 3)
    mine, recs, my_rthr = XR.restate_counts(bam, fa, variants, TARGETS, RR.RPB_TARGETS, SEED, 3)
    assert my_rthr == rthr and mine.shape == theirs.shape and mine.dtype == theirs.dtype == np.uint32
    assert np.array_equal(mine, theirs) and mine[..., 2].any() and mine[..., 4].any()
    for rows, old in zip(recs, their_recs):
        assert [(r.barcode, r.name, r.first, r.alt0, r.alt1, r.touch) for r in rows] == [(o.barcode, o.name, o.first, o.alt, o.single, o.single) for o in old]
        assert all(r.case is None for r in rows)
    # and on the hand-made records (inside deletions, indels behind the base, soft clips)
    os.makedirs(str(tmp_path / "case"))
    bam, fa, loci, P, given = SR.make_case(str(tmp_path / "case"))
    variants = [IR.variant(v.chrom, v.pos, v.ref, v.alt) for v in given]
    theirs, _, rthr = RR.restate_counts(bam, fa, given, TARGETS, (1.5, 20), SEED, 2)
    mine, recs, _ = XR.restate_counts(bam, fa, variants, TARGETS, (1.5, 20), SEED, 2)
    assert np.array_equal(mine, theirs) and any(not r.touch for rows in recs for r in rows)


def _ties_to_the_reps_restatement(bam, fa, variants, recs, reps=3):
    seeds, thr = XR.seeds(SEED, reps), [XR.threshold(t) for t in TARGETS]
    pos = [v.pos for v in variants]
    counters, _ = QR.host_counters(bam, variants, fa)
    for (names, cnt), rows in zip(counters, recs):
        mine = XR.barcode_counters(rows)
        assert list(names) == mine[0] and np.array_equal(cnt, mine[1])                  # (per barcode the four bits sum to the four counters)
    mine = XR.counts_from(recs, pos, thr, [ONE], seeds)
    theirs = QR.counts_from(counters, pos, thr, seeds, [ONE])
    assert mine.shape == theirs.shape == (len(variants), reps, len(thr), 1, 5) and mine.dtype == theirs.dtype == np.uint32
    assert np.array_equal(mine, theirs) and mine[..., 2].any()
    return counters


def test_full_read_threshold_is_the_indel_reps_restatement(synth, tmp_path):
    bam, fa, variants, recs, _ = synth
    _ties_to_the_reps_restatement(bam, fa, variants, recs)
    bam, fa, loci, P, given = IR.make_case(str(tmp_path))
    counters = _ties_to_the_reps_restatement(bam, fa, given, XR.records(bam, fa, given))
    assert any((cnt[:, 2] != cnt[:, 3]).any() for (_, cnt), v in zip(counters, given) if v.kind != af.SNV)     # (alt1 and touch are two numbers)


def test_kept_sets_are_nested_in_r_and_hits_in_t(synth):
    bam, fa, variants, recs, rthr = synth
    assert 0 < rthr[0] < rthr[1] < rthr[2] == ONE
    for rows, v in zip(recs, variants):
        full = XR.barcode_counters(rows)[1].astype(np.int64)
        last = None
        for q in [0] + rthr:
            texts, cnt = XR.kept_counters(rows, q, SEED)
            assert (cnt <= full).all() and (last is None or (last <= cnt).all())
            last = cnt
        assert np.array_equal(last, full)
        _, zero = XR.kept_counters(rows, 0, SEED)
        assert np.array_equal(zero[:, 0], np.array([sum(r.first for r in rows if r.barcode == b) for b in texts]))
    thr = [XR.threshold(t) for t in (0.0, 0.05, 0.3, 0.7, 1.0)]
    got = XR.counts_from(recs, [v.pos for v in variants], thr, rthr, [SEED]).astype(np.int64)
    assert (np.diff(got[:, 0, :, :, 2], axis=1) >= 0).all() and (np.diff(got[:, 0, :, :, 3], axis=1) >= 0).all()      # S', READS' grow with t
    assert (np.diff(got[:, 0, :, :, 0], axis=2) >= 0).all() and (np.diff(got[:, 0, :, :, 2], axis=2) >= 0).all()      # N', S' grow with r
    assert not got[:, 0, 0, :, 2].any() and np.array_equal(got[:, 0, 4, :, 2], got[:, 0, 4, :, 0])                  # t = 0: nobody; t = 1: everybody
    assert np.array_equal(got[:, 0, 0, :, 4], got[:, 0, 0, :, 1])                                                  # nothing spiked: V1' = V0'
    assert (got[:, 0, :, :, 0] == got[:, 0, :1, :, 0]).all() and (got[:, 0, :, :, 1] == got[:, 0, :1, :, 1]).all()  # N', V0' do not depend on t


def test_the_gpu_tests_input_holds_every_case_and_thinning_bites_on_an_indel(synth):
    """Conditions on the inputs, checked on the restatement alone.  At a listed indel the file has a touched record whose anchor letter
    is not REF's, an untouched one that shows the indel already and one that ends inside the footprint; and at the smallest
    reads-per-barcode target, with the tests' seed, a covering barcode of an INDEL leaves the locus, one that stays changes its majority,
    and READS falls below its unthinned value."""
    bam, fa, variants, recs, rthr = synth
    assert {v.kind for v in variants} == {af.SNV, af.INS, af.DEL}
    indel = [k for k, v in enumerate(variants) if v.kind != af.SNV]
    seen = {c: sum(XR.cases(recs[k])[c] for k in indel) for c in XR.CASES}
    assert all(seen[c] >= 1 for c in XR.CASES), seen
    assert min(len(recs[k]) for k in indel) > 256                                       # (a locus window wider than one workgroup)
    gone = flipped = 0
    for k in indel:
        _, full = XR.kept_counters(recs[k], ONE, SEED)
        _, thin = XR.kept_counters(recs[k], rthr[0], SEED)
        there = thin[:, 0] > 0
        gone += int((~there).sum())
        flipped += int((((2 * full[:, 2] > full[:, 0]) != (2 * thin[:, 2] > thin[:, 0])) & there).sum())      # car1, by alt1
    assert gone >= 1 and flipped >= 1
    counts = XR.counts_from([recs[k] for k in indel], [variants[k].pos for k in indel], [XR.threshold(0.7)], [rthr[0], ONE], [SEED])
    assert (counts[:, 0, 0, 0, 0] < counts[:, 0, 0, 1, 0]).all() and (counts[:, 0, 0, 0, 3] < counts[:, 0, 0, 1, 3]).all()      # N' < N, READS' < READS
    # four bits are needed: at some indel the kept alt1 and touch differ
    assert any((XR.kept_counters(recs[k], rthr[0], SEED)[1][:, 2] != XR.kept_counters(recs[k], rthr[0], SEED)[1][:, 3]).any() for k in indel)
    # bam_cigars with the listed indels of its GPU tests: records that span them, of both kinds
    bam2, fa2, loci2, P2 = ds_restate.load_fixture("bam_cigars", os.path.dirname(bam))
    vs2 = IR.pick_variants(bam2, fa2, loci2, 4, gap=8)
    recs2 = XR.records(bam2, fa2, vs2)
    assert {v.kind for v in vs2} == {af.SNV, af.INS, af.DEL} and all(len(rows) for rows in recs2)
