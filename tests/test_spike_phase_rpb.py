"""--spikePhaseRpb without a GPU: the flag's parsing and every refusal (before any file), the pinned refusals of --spikeRpb and
--spikeIndelRpb beside the phase flags as they were, the entry's declaration and export, the phase writers with the RPB axis, the host's
spike_joint_records against the restatement, and the restatement's own properties (tests/spike_phase_rpb_restate.py): at one member it
is the --spikeIndelRpb restatement's columns, at the full read threshold the --spikeIndelPhase restatement, N_ALL' and S_ALL' are nested
in r and in t - and the conditions on the GPU tests' synthetic input that make a joint count more than a minimum over its members."""
import argparse
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, cli, devplanes, dsaf, spike
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import spike_indel_phase_restate as JR  # noqa: E402
import spike_indel_restate as IR  # noqa: E402
import spike_phase_rpb_restate as ZR  # noqa: E402

XR, PR = ZR.XR, ZR.PR
SEED, ONE = ZR.SEED, ZR.ONE
TARGETS = (0.05, 0.3, 0.7)
NS = lambda **kw: argparse.Namespace(**kw)
CLI_TARGETS = [(0.01, 100, "o.spikeAF0.01"), (0.05, 25, "o.spikeAF0.05")]


# ---- the command line
def test_flag_is_parsed_into_the_cells_of_spike_rpb():
    ns = cli.build_parser().parse_args("--outPrefix o --bamFile b --bedTarget t --mtDepth 3 --rpb 2 --spikePhaseRpb 1.5,3 --spikeIndelReps 4".split())
    assert ns.spikePhaseRpb == "1.5,3" and ns.spikeRpb is None and ns.spikeIndelRpb is None and not ns.spikeIndelPhase
    rs, cells = spike.phase_rpb_cells(ns, CLI_TARGETS)
    assert rs == [1.5, 3.0]
    assert cells == [(0, 0.01, 1.5, 100, "o.spikeAF0.01.dsRpb1.5"), (0, 0.01, 3.0, 100, "o.spikeAF0.01.dsRpb3"),
                     (1, 0.05, 1.5, 25, "o.spikeAF0.05.dsRpb1.5"), (1, 0.05, 3.0, 25, "o.spikeAF0.05.dsRpb3")]
    assert (rs, cells) == spike.indel_rpb_cells(NS(spikeIndelRpb="1.5,3"), CLI_TARGETS)
    assert spike.phase_rpb_cells(NS(), CLI_TARGETS) == (None, [])
    # (the flags it stands beside read nothing of it)
    assert spike.indel_flags(ns, CLI_TARGETS) == (4, None) and spike.rpb_cells(ns, CLI_TARGETS) == (None, []) and not spike.indel_phase(ns, CLI_TARGETS)
    assert "--spikePhaseRpb" in cli.build_parser().format_help()


@pytest.mark.parametrize("kw, tg, msg", (
    (dict(), [], "--spikePhaseRpb thins the reads of the --spikeAF spike-ins, phase sets among them: it needs --spikeAF and --spikeVariants"),
    (dict(spikeRpb="2"), CLI_TARGETS, "--spikePhaseRpb cannot be combined with --spikeRpb in one run: --spikePhaseRpb takes the targets"),
    (dict(spikeIndelRpb="2"), CLI_TARGETS, "--spikePhaseRpb cannot be combined with --spikeIndelRpb in one run: --spikePhaseRpb takes the targets"),
    (dict(spikeIndels=True), CLI_TARGETS, "--spikePhaseRpb implies the rules of --spikeIndels: leave --spikeIndels out"),
    (dict(spikePhase=True), CLI_TARGETS, "--spikePhaseRpb implies the rules of --spikePhase: leave --spikePhase out"),
    (dict(spikeIndelPhase=True), CLI_TARGETS, "--spikePhaseRpb implies the rules of --spikeIndelPhase: leave --spikeIndelPhase out"),
    (dict(spikeReps=4), CLI_TARGETS, "--spikePhaseRpb cannot be combined with --spikeReps in one run: use --spikeIndelReps R beside it"),
    (dict(spikeDepth="0.5"), CLI_TARGETS, "--spikePhaseRpb cannot be combined with --spikeDepth in one run .phase sets in cells of barcode depths"),
    (dict(spikeIndelDepth="0.5"), CLI_TARGETS, "--spikePhaseRpb cannot be combined with --spikeIndelDepth in one run .phase sets in cells")))
def test_flag_refusals(kw, tg, msg):
    with pytest.raises(SystemExit, match=msg):
        spike.phase_rpb_cells(NS(spikePhaseRpb="2", **kw), tg)


@pytest.mark.parametrize("text, msg", (
    ("a,b", "--spikePhaseRpb: comma-separated reads-per-barcode targets > 0 expected"), ("2;3", "--spikePhaseRpb: comma-separated reads-per-barcode targets"),
    ("0", "--spikePhaseRpb: every target must be a number > 0"), ("2,-1", "must be a number > 0"), (",", "must be a number > 0"),
    ("nan", "must be a number > 0"), ("inf", "must be a number > 0"), ("2,2.0", "--spikePhaseRpb: a target is listed twice"),
    (",".join("%g" % (1 + 0.1 * k) for k in range(17)), "--spikePhaseRpb: 2 targets x 17 reads-per-barcode targets = 34 cells, at most 32")))
def test_target_refusals(text, msg):
    with pytest.raises(SystemExit, match=msg):
        spike.phase_rpb_cells(NS(spikePhaseRpb=text), CLI_TARGETS)


def test_refused_before_any_file_is_written(tmp_path):
    """The command line itself ends the run before it opens anything (the BAM named here does not exist)."""
    base = dict(outPrefix=str(tmp_path / "o"), bamFile=str(tmp_path / "none.bam"), bedTarget=str(tmp_path / "none.bed"), mtDepth=10, rpb=2.0,
                refGenome=str(tmp_path / "none.fa"))
    sp = dict(spikeAF="0.1", spikeVariants="v", spikePhaseRpb="2")
    for more, msg in ((dict(spikePhaseRpb="2"), "it needs --spikeAF"), (dict(spikeAF="0.1", spikePhaseRpb="2"), "it needs --spikeVariants"),
                      (dict(sp, spikeRpb="2"), "--spikePhaseRpb takes the targets"), (dict(sp, spikeIndelRpb="2"), "--spikePhaseRpb takes the targets"),
                      (dict(sp, spikeIndels=""), "leave --spikeIndels out"), (dict(sp, spikePhase=""), "leave --spikePhase out"),
                      (dict(sp, spikeIndelPhase=""), "--spikePhaseRpb implies the rules of --spikeIndelPhase"),
                      (dict(sp, spikeReps=4), "use --spikeIndelReps R beside it"),
                      (dict(sp, spikeDepth="0.5"), "--spikePhaseRpb cannot be combined with --spikeDepth"),
                      (dict(sp, spikeIndelDepth="0.5"), "--spikePhaseRpb cannot be combined with --spikeIndelDepth"),
                      (dict(sp, spikePhaseRpb="x"), "comma-separated reads-per-barcode targets"), (dict(sp, spikePhaseRpb="2,0"), "must be a number > 0"),
                      (dict(sp, spikePhaseRpb="2,2"), "listed twice"),
                      (dict(sp, spikePhaseRpb=",".join("%g" % (1 + 0.1 * k) for k in range(33))), "at most 32"),
                      (dict(sp, spikeIndelReps=1), "must lie in"),
                      # what --spikeAF refuses
                      (dict(sp, spikeAF="1.5"), "--spikeAF"), (dict(sp, spikeAF="0.1,0.10"), "listed twice"),
                      (dict(sp, dsRpb="2"), r"--spikeAF cannot be combined with --dsRpb in one run \(spike-ins on a down-sampled file are not built\)"),
                      (dict(sp, dsMT="0.5"), "cannot be combined with --dsMT"),
                      # --spikeRpb and --spikeIndelRpb beside the phase flags: their messages, as they were
                      (dict(spikeAF="0.1", spikeVariants="v", spikeRpb="2", spikePhase=""),
                       "--spikeRpb cannot be combined with --spikePhase in one run .the combination is not built"),
                      (dict(spikeAF="0.1", spikeVariants="v", spikeRpb="2", spikeIndelPhase=""),
                       "--spikeRpb cannot be combined with --spikeIndelPhase in one run .the combination is not built"),
                      (dict(spikeAF="0.1", spikeVariants="v", spikeIndelRpb="2", spikePhase=""),
                       "--spikeIndelRpb cannot be combined with --spikePhase in one run .phase sets of indel spike-ins are not built"),
                      (dict(spikeAF="0.1", spikeVariants="v", spikeIndelRpb="2", spikeIndelPhase=""),
                       "--spikeIndelRpb cannot be combined with --spikeIndelPhase in one run .the combination is not built")):
        given = dict(base, **more)
        ns = cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in given.items() if v != ""] + ["--" + k for k, v in given.items() if v == ""])
        with pytest.raises(SystemExit, match=msg):
            cli.main(ns)
    assert os.listdir(str(tmp_path)) == []


def test_the_pre_pass_lifts_the_refusal_for_this_flag_only(tmp_path):
    bam, fa, loci, P, variants = IR.make_case(str(tmp_path))
    rpb = dict(targets=[2.0], params=[P])
    not_built = "^--spikeRpb: cells of barcode depths, phase sets or indel spike-ins are not built$"
    # (raised before the engine is touched: None stands for it)
    with pytest.raises(ValueError, match=not_built):                                     # --spikeIndelRpb beside phase sets: as it was
        devplanes.spike_rules(bam, None, variants, [0.5], [P], SEED, None, rpb=dict(rpb), indel_counters=True, phase=dict(sets=[]))
    with pytest.raises(ValueError, match=not_built):                                     # the flag without four counters
        devplanes.spike_rules(bam, None, variants, [0.5], [P], SEED, None, rpb=dict(rpb, flag="--spikePhaseRpb"), phase=dict(sets=[]))
    with pytest.raises(ValueError, match=not_built):                                     # cells of barcode depths stay refused under it
        devplanes.spike_rules(bam, None, variants, [0.5], [P], SEED, None, rpb=dict(rpb, flag="--spikePhaseRpb"), indel_counters=True,
                              phase=dict(sets=[]), depth=dict(fracs=[0.5], params=[P]))
    spikes = devplanes.SpikeSet(variants, indels=True)
    cell = devplanes.DsRule(1.0, None, seed=7, level="read", target=1.5, prob_keep=0.25, groups=object(), thr=1 << 30, af=0.05, spike=spikes)
    assert cell.flag == "--spikeIndelRpb"
    spikes.rpb_flag = "--spikePhaseRpb"
    assert cell.spike_rpb_cell and cell.flag == "--spikePhaseRpb" and cell.label == "spiked allele fraction 0.05 x target 1.5"


def test_the_entry_is_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert re.search(r"#define SMC_ABI_VERSION 11\b", text)
    assert re.search(r"\bint smc_spike_phase_rpb_counts\(smc_ctx\* ctx, const uint64_t\* d_joint_ident, const uint32_t\* d_joint_off,", text)
    assert "--spikePhaseRpb" in text and "smc_spike_phase_rpb_counts" in _lib.SYMBOLS
    L = _lib.load()
    assert L.smc_abi_version() == 11 and hasattr(L, "smc_spike_phase_rpb_counts")
    assert len(L.smc_spike_phase_rpb_counts.argtypes) == 23 and len(L.smc_spike_indel_rpb_counts.argtypes) == 19
    kernels = open(os.path.join(ROOT, "smcounter_amd", "csrc", "k_spike_rpb.inc")).read()
    # ONE counts kernel body serves the listed variants and the sets
    assert len(re.findall(r"void k_spr_counts\(", kernels)) == 1 and "k_spr_counts<SMC_RG_MAX_TARGETS, false, true>" in open(
        os.path.join(ROOT, "smcounter_amd", "csrc", "host_abi.inc")).read() and "asm" not in kernels


# ---- the writers with the RPB axis
def test_the_phase_writers_take_the_rpb_axis(tmp_path):
    assert spike.phase_header() == spike.PHASE_HEADER and spike.phase_replicates_header() == spike.PHASE_REPLICATES_HEADER
    assert spike.phase_sensitivity_header() == spike.PHASE_SENSITIVITY_HEADER and "FRACTION" in spike.PHASE_HEADER
    swap = lambda h: tuple("RPB" if x == "FRACTION" else x for x in h)
    assert spike.phase_header(spike.RPB_AXIS) == swap(spike.PHASE_HEADER)
    assert spike.phase_replicates_header(spike.RPB_AXIS) == swap(spike.PHASE_REPLICATES_HEADER)
    assert spike.phase_sensitivity_header(spike.RPB_AXIS) == swap(spike.PHASE_SENSITIVITY_HEADER)
    variants = [IR.variant("chr1", 10, "A", "AGG"), IR.variant("chr1", 14, "C", "T")]
    ps = sv.PhaseSet("hap", "chr1", (0, 1))
    prefix = str(tmp_path / "o")
    cell = prefix + ".spikeAF0.1.dsRpb1.5"
    open(cell + ".smCounter.all.txt", "w").write("CHROM\tPOS\tREF\tALT\n")
    open(cell + ".smCounter.cut.txt", "w").write("CHROM\tPOS\tREF\tALT\nchr1\t10\tA\tAGG\nchr1\t14\tC\tT\n")
    r = dict(N_ALL=40, V0_ALL=1, S_ALL=9, V1_ALL=10)
    spike.write_phase(prefix, variants, [ps], [(0.1, 1.5, 250, cell, [r])], spike.RPB_AXIS)
    lines = open(prefix + ".spikeAF.rpb.phase.txt").read().splitlines()
    assert lines[0].split("\t") == list(spike.phase_header(spike.RPB_AXIS))
    called = spike.called_all(ps, variants, dsaf.read_output(cell)[1])
    assert lines[1].split("\t") == ["hap", "chr1", "10,14", "A,C", "AGG,T", "0.1", "1.5", "250", "40", "1", "9", "10", dsaf.frac_text(0.25), "%d" % called]
    entries = {(0, 0): [(r, 1), (dict(r, V1_ALL=20), 0)]}
    spike.write_phase_replicates(prefix, variants, [ps], [(0.1, 1.5, 250)], [7, 8], entries, spike.RPB_AXIS)
    spike.write_phase_sensitivity(prefix, variants, [ps], [(0.1, 1.5, 250)], entries, spike.RPB_AXIS)
    reps = [l.split("\t") for l in open(prefix + ".spikeAF.rpb.phase.replicates.txt").read().splitlines()]
    assert reps[0] == list(spike.phase_replicates_header(spike.RPB_AXIS)) and reps[2][6:10] == ["1.5", "250", "1", "8"] and reps[2][13] == "20"
    sens = [l.split("\t") for l in open(prefix + ".spikeAF.rpb.phase.sensitivity.txt").read().splitlines()]
    assert sens[0] == list(spike.phase_sensitivity_header(spike.RPB_AXIS)) and sens[1][6:10] == ["1.5", "250", "2", "1"]
    assert sorted(f for f in os.listdir(str(tmp_path)) if "phase" in f) == ["o.spikeAF.rpb.phase.replicates.txt", "o.spikeAF.rpb.phase.sensitivity.txt",
                                                                             "o.spikeAF.rpb.phase.txt"]


# ---- the restatement's own properties
@pytest.fixture(scope="module")
def synth(tmp_path_factory):
    """The GPU tests' synthetic input, its covering records and its read thresholds (computed once, only read)."""
    bam, fa, loci, P, variants, sets = ZR.synth_case(str(tmp_path_factory.mktemp("prpb")))
    groups = XR.file_groups(bam)
    return bam, fa, variants, sets, XR.records(bam, fa, variants, groups), XR.read_thresholds(groups, ZR.RPB_TARGETS)


def test_the_synthetic_case_is_two_sets_and_an_unphased_variant(synth):
    bam, fa, variants, sets, recs, rthr = synth
    assert len(variants) == 5 and len(sets) == 2 and sorted(k for m in sets for k in m) != list(range(5))
    kinds = [tuple(variants[k].kind for k in m) for m in sets]
    assert sorted(kinds) == sorted([(af.SNV, af.DEL), (af.INS, af.SNV)])                  # (an SNV before a deletion; an insertion leads an SNV)
    for m in sets:
        a, b = (variants[k] for k in m)
        assert a.chrom == b.chrom and ZR.NEAR[0] <= b.pos - IR.footprint(a)[1] <= ZR.NEAR[1]
        spans = {r.name for r in recs[m[0]]} & {r.name for r in recs[m[1]]}
        assert len(spans) > 256                                                           # (reads span both members; more than a workgroup of them)
    assert 0 < rthr[0] < rthr[1] < rthr[2] == ONE


def test_one_member_is_the_indel_rpb_restatement(synth):
    bam, fa, variants, sets, recs, rthr = synth
    seeds, thr = PR.seeds(SEED, 3), [PR.threshold(t) for t in TARGETS]
    pos = [v.pos + 3 for v in variants]                                                  # (any position may lead)
    mine = ZR.counts_from([[rows] for rows in recs], pos, thr, rthr, seeds)
    theirs = XR.counts_from(recs, pos, thr, rthr, seeds)
    assert mine.shape == (5, 3, 3, 3, 4) and mine.dtype == np.uint32
    assert np.array_equal(mine, theirs[..., [0, 1, 2, 4]]) and mine[..., 2].any() and mine[..., 3].any()


def test_full_read_threshold_is_the_indel_phase_restatement(synth):
    bam, fa, variants, sets, recs, rthr = synth
    seeds, thr = PR.seeds(SEED, 3), [PR.threshold(t) for t in TARGETS]
    lead = [min(variants[k].pos for k in m) for m in sets]
    mine = ZR.counts_from(ZR.set_rows(recs, sets), lead, thr, [ONE], seeds)
    joint = JR.host_joint(bam, variants, sets, fa)
    theirs = JR.counts_from(joint, lead, thr, [ONE], seeds)
    assert mine.shape == theirs.shape == (2, 3, 3, 1, 4) and np.array_equal(mine, theirs) and mine[..., 3].any()
    assert [names for names, _ in joint] == [ZR.joint_names(rows) for rows in ZR.set_rows(recs, sets)]
    assert JR.lead_positions(variants, sets) == [lead[[g for g, m in enumerate(sets) if k in m][0]] if any(k in m for m in sets) else v.pos
                                                 for k, v in enumerate(variants)]


def test_joint_counts_are_nested_in_r_and_in_t(synth):
    bam, fa, variants, sets, recs, rthr = synth
    lead = [min(variants[k].pos for k in m) for m in sets]
    thr = [PR.threshold(t) for t in (0.0, 0.05, 0.3, 0.7, 1.0)]
    got = ZR.counts_from(ZR.set_rows(recs, sets), lead, thr, [0] + rthr, [SEED]).astype(np.int64)[:, 0]
    assert (np.diff(got[..., 0], axis=2) >= 0).all() and (np.diff(got[..., 2], axis=2) >= 0).all()       # N_ALL', S_ALL' grow with r
    assert (np.diff(got[..., 2], axis=1) >= 0).all()                                                      # S_ALL' grows with t
    assert (got[..., 0] == got[:, :1, :, 0]).all() and (got[..., 1] == got[:, :1, :, 1]).all()            # N_ALL', V0_ALL' do not depend on t
    assert not got[:, 0, :, 2].any() and np.array_equal(got[:, 4, :, 2], got[:, 4, :, 0])                 # t = 0: nobody; t = 1: everybody
    assert np.array_equal(got[:, 0, :, 3], got[:, 0, :, 1])                                               # nothing spiked: V1_ALL' = V0_ALL'
    assert (got[..., 1] <= got[..., 0]).all() and (got[..., 3] <= got[..., 0]).all()


def test_the_gpu_tests_input_makes_the_joint_count_more_than_a_minimum_over_its_members(synth):
    """Conditions on the input, checked on the restatement alone with the tests' seed at the smallest reads-per-barcode target: some
    barcode that is joint unthinned keeps a read at one member and none at another; in some set V1_ALL' lies below every member's V1'
    (a barcode carries one member and not the other after spiking); some set has N_ALL' below its unthinned N_ALL."""
    bam, fa, variants, sets, recs, rthr = synth
    thr = [PR.threshold(t) for t in TARGETS]
    split = below = fewer = 0
    for m in sets:
        rows = [recs[k] for k in m]
        names = ZR.joint_names(rows)
        c = ZR.member_counters(rows, names, rthr[0], SEED)
        there = c[:, :, 0] > 0
        split += int((there.any(axis=1) & ~there.all(axis=1)).sum())
        lead = min(variants[k].pos for k in m)
        joint = ZR.counts_from([rows], [lead], thr, [rthr[0], ONE], [SEED])[0, 0]
        per = XR.counts_from(rows, [lead] * len(m), thr, [rthr[0], ONE], [SEED])[:, 0]
        below += int((joint[:, 0, 3] < per[:, :, 0, 4].min(axis=0)).sum())
        fewer += int(joint[0, 0, 0] < joint[0, 1, 0] == len(names))
        assert (joint[:, 0, 0] <= per[:, :, 0, 0].min(axis=0)).all()
    assert split >= 1 and below >= 1 and fewer >= 1, (split, below, fewer)


# ---- the host's CSR of (joint barcode, member) segments
def test_spike_joint_records_joins_the_members_by_identity(synth):
    """devplanes.spike_joint_records over per-variant covers and CSRs made from the restatement's records (the members of a set in two
    differently ordered cover lists, as two runs of the pre-pass would give them): the joint identities ascending, and per segment
    the records of that barcode at that member - summed per bit they are the restatement's counters at the full read threshold."""
    bam, fa, variants, sets, recs, rthr = synth
    covers, records = [], []
    for k, rows in enumerate(recs):
        texts = sorted({r.barcode for r in rows}, reverse=bool(k % 2))
        per = {b: [r for r in rows if r.barcode == b] for b in texts}
        flat = [r for b in texts for r in per[b]]
        off = np.zeros(len(texts) + 1, np.uint32)
        off[1:] = np.cumsum([len(per[b]) for b in texts])
        flags = np.array([(1 if r.first else 0) | (2 if r.alt0 else 0) | (4 if r.alt1 else 0) | (8 if r.touch else 0) for r in flat], np.uint8)
        covers.append(PR.idents(texts)); records.append((off, XR.rp.fnv64([r.name for r in flat]), flags))
    psets = [sv.PhaseSet("hap%d" % g, variants[m[0]].chrom, m) for g, m in enumerate(sets)]
    joint = devplanes.spike_joint_records(psets, covers, records)
    for (ids, off, names, flags), m in zip(joint, sets):
        rows = [recs[k] for k in m]
        texts = ZR.joint_names(rows)
        order = np.argsort(PR.idents(texts))
        assert np.array_equal(ids, np.asarray(PR.idents(texts), np.uint64)[order]) and (np.diff(ids) > 0).all()
        assert off.dtype == np.uint32 and len(off) == len(ids) * len(m) + 1 and off[0] == 0 and int(off[-1]) == len(names) == len(flags)
        want = ZR.member_counters(rows, texts, ONE, SEED)[order]                          # [n, M, 4] = (reads, alt0, alt1, touch)
        o = off.astype(np.int64)
        got = np.stack([np.diff(o)] + [np.add.reduceat(np.concatenate([(flags >> s) & 1, [0]]).astype(np.int64), o[:-1]) * (np.diff(o) > 0)
                                       for s in (1, 2, 3)], axis=1).reshape(len(ids), len(m), 4)
        assert np.array_equal(got, want)
        for e in (0, len(ids) - 1):
            for x, k in enumerate(m):
                mine = sorted(names[o[e * len(m) + x]:o[e * len(m) + x + 1]].tolist())
                assert mine == sorted(XR.rp.fnv64([r.name for r in recs[k] if r.barcode == texts[order[e]]]).tolist())
