"""--spikeIndelReps / --spikeIndelDepth without a GPU: the flags and every refusal (before any file), the pre-pass's refusal of a record
at which the 16-bit limits could bind, the restated four counters against the offline tool replicate by replicate, the report writers
with indel variants, header and symbols."""
import argparse
import inspect
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT
from smcounter_amd import _lib, abi, cli, devplanes, dsaf, spike
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import spike_indel_reps_restate as QR  # noqa: E402
import spike_indel_restate as IR  # noqa: E402
import test_spike_indels as TI  # noqa: E402  (its command line on bam_cigars)

SEED = 20240607
NS = argparse.Namespace
TARGETS = [(0.01, 100, "o.spikeAF0.01"), (0.05, 100, "o.spikeAF0.05")]


def test_flags_are_parsed():
    ns = cli.build_parser().parse_args("--outPrefix o --bamFile b --bedTarget t --mtDepth 3 --rpb 2 --spikeIndelReps 16 --spikeIndelDepth 0.5,1".split())
    assert ns.spikeIndelReps == 16 and ns.spikeIndelDepth == "0.5,1"
    assert spike.indel_flags(ns, TARGETS) == (16, "0.5,1")
    assert spike.indel_flags(NS(), TARGETS) == (None, None) and spike.indel_flags(NS(spikeReps=4, spikeIndels=True), []) == (None, None)
    assert spike.indel_flags(NS(spikeIndelDepth="0.5"), TARGETS) == (None, "0.5")
    fr, cells = spike.depth_cells(ns, TARGETS, "spikeIndelDepth")
    assert fr == [0.5, 1.0] and [(k, t, f, d) for k, t, f, d, _ in cells] == [(0, 0.01, 0.5, 50), (0, 0.01, 1.0, 100), (1, 0.05, 0.5, 50), (1, 0.05, 1.0, 100)]
    assert cells[0][4] == "o.spikeAF0.01.dsMT0.5"
    assert spike.depth_cells(ns, TARGETS) == (None, [])                              # (--spikeDepth itself is not given)


@pytest.mark.parametrize("kw, tg, msg", (
    (dict(spikeIndelReps=4, spikeIndels=True), TARGETS, "implies the rules of --spikeIndels"),
    (dict(spikeIndelReps=4, spikeReps=4), TARGETS, "--spikeIndelReps R replicates the spike-ins itself"),
    (dict(spikeIndelDepth="0.5", spikeReps=4), TARGETS, "cannot be combined with --spikeReps"),
    (dict(spikeIndelReps=4, spikeDepth="0.5"), TARGETS, "--spikeIndelDepth takes the barcode fractions"),
    (dict(spikeIndelDepth="0.5", spikeDepth="0.5"), TARGETS, "cannot be combined with --spikeDepth"),
    (dict(spikeIndelReps=4, spikePhase=True), TARGETS, "phase sets of indel spike-ins are not built"),
    (dict(spikeIndelDepth="0.5", spikePhase=True), TARGETS, "phase sets of indel spike-ins are not built"),
    (dict(spikeIndelReps=4), [], "it needs --spikeAF and --spikeVariants"),
    (dict(spikeIndelDepth="0.5"), [], "--spikeIndelDepth thins the barcodes of the --spikeAF spike-ins, insertions and deletions among them: it needs --spikeAF"),
    (dict(spikeIndelReps=1), TARGETS, r"--spikeIndelReps: the number of replicates must lie in 2 \.\. 1000, got 1"),
    (dict(spikeIndelReps=1001), TARGETS, r"--spikeIndelReps: the number of replicates must lie in 2 \.\. 1000, got 1001"),
    (dict(spikeIndelReps="x"), TARGETS, r"--spikeIndelReps: an integer in 2 \.\. 1000 expected, got 'x'"),
    (dict(spikeIndelReps=2.5), TARGETS, r"--spikeIndelReps: an integer in 2 \.\. 1000 expected")))
def test_flag_refusals(kw, tg, msg):
    with pytest.raises(SystemExit, match=msg):
        spike.indel_flags(NS(**kw), tg)


@pytest.mark.parametrize("text, msg", (("0", "--spikeIndelDepth: every fraction must lie in (0, 1]"), ("1.5", "every fraction must lie in (0, 1]"),
                                       ("x", "--spikeIndelDepth: comma-separated fractions in (0, 1] expected"),
                                       ("0.5,0.50", "--spikeIndelDepth: a fraction is listed twice"),
                                       (",".join("%g" % (0.01 * k) for k in range(1, 18)), "--spikeIndelDepth: 2 targets x 17 fractions = 34 cells, at most 32")))
def test_fraction_refusals(text, msg):
    with pytest.raises(SystemExit, match=re.escape(msg)):
        spike.depth_cells(NS(spikeIndelDepth=text), TARGETS, "spikeIndelDepth")


def test_refused_before_any_file_is_written(tmp_path):
    """The command line itself; the BAM named here does not exist."""
    base = dict(outPrefix=str(tmp_path / "o"), bamFile=str(tmp_path / "none.bam"), bedTarget=str(tmp_path / "none.bed"), mtDepth=10, rpb=2.0,
                refGenome=str(tmp_path / "none.fa"))
    sp = dict(spikeAF="0.1", spikeVariants="v")
    for more, msg in ((dict(spikeIndelReps=4), "it needs --spikeAF"), (dict(spikeIndelDepth="0.5"), "it needs --spikeAF"),
                      (dict(spikeIndelReps=4, spikeAF="0.1"), "it needs --spikeVariants"),
                      (dict(sp, spikeIndelReps=1), "must lie in"), (dict(sp, spikeIndelReps=4, spikeIndels=True), "leave --spikeIndels out"),
                      (dict(sp, spikeIndelReps=4, spikeReps=4), "cannot be combined with --spikeReps"),
                      (dict(sp, spikeIndelDepth="0.5", spikeDepth="0.5"), "cannot be combined with --spikeDepth"),
                      (dict(sp, spikeIndelReps=4, spikePhase=True), "cannot be combined with --spikePhase"),
                      (dict(sp, spikeIndelDepth="0.5,0.5"), "listed twice"), (dict(sp, spikeIndelDepth="2"), "must lie in"),
                      (dict(sp, spikeIndelReps=4, spikeIndelDepth=",".join("%g" % (0.01 * k) for k in range(1, 34))), "at most 32"),
                      (dict(sp, spikeIndelReps=4, dsMT="0.5"), "cannot be combined with --dsMT"),
                      (dict(sp, spikeAF="1.5", spikeIndelReps=4), "--spikeAF")):
        d = dict(base, **more)
        ns = cli.build_parser().parse_args(["--%s=%s" % (k, v) for k, v in d.items() if v is not True] + ["--" + k for k, v in d.items() if v is True])
        with pytest.raises(SystemExit, match=msg):
            cli.main(ns)
    assert os.listdir(str(tmp_path)) == []


@pytest.mark.parametrize("kw,lines,msg", [
    (dict(spikeIndelReps="3"), lambda c, p, s: "%s\t%d\t%sC\t%sGG\n" % (c, p, s[0], s[0]), "neither a substitution"),
    (dict(spikeIndelDepth="0.5"), lambda c, p, s: "%s\t%d\t%s\t%sG\n%s\t%d\t%s\t%s\n" % (c, p, s[0], s[0], c, p + 1, s[1], "ACGT"[("ACGT".index(s[1]) + 1) % 4]),
     "lies in the footprint"),
    (dict(spikeIndelReps="3"), lambda c, p, s: "%s\t%d\t%s%s\t%s\n" % (c, p, s[0], "ACGT"[("ACGT".index(s[1]) + 1) % 4] + s[2], s[0]),
     "the reference genome has"),
    (dict(spikeIndelReps="3", spikeIndelDepth="0.5"), lambda c, p, s: "%s\t%d\t%s\t%sG\n" % (c, p + 100000, s[0], s[0]),
     "is not a locus of --bedTarget|the reference genome has"),
])
def test_what_spike_indels_refuses_of_the_variants_file_before_any_file(tmp_path, kw, lines, msg):
    ns = TI._args(tmp_path, lines, **kw)
    with pytest.raises(SystemExit, match=msg if "|" in msg else re.escape(msg)):
        cli.main(ns)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("o.")]


def _hand_made(n_cig, l_seq, variants):
    aln = np.zeros(2, abi.DEV_ALN_DTYPE)
    aln["pos"], aln["end"], aln["n_cig"], aln["l_seq"] = [90, 90], [200, 200], [3, n_cig], [100, l_seq]
    var, _, _ = devplanes.spike_indel_variants(variants, 0)
    return dict(aln=aln, bq=np.zeros(8, np.uint8), cig=np.zeros(4, np.uint32)), var


def test_a_record_at_which_the_16_bit_limits_could_bind_is_found():
    ins = IR.variant("c", 101, "A", "AGAT")
    dl = IR.variant("c", 120, "ACGT", "A")
    snv = IR.variant("c", 110, "A", "G")
    # one indel: n_cig + 2 = 65536
    assert devplanes.spike_indel_limits(*_hand_made(65534, 100, [ins])) == 1
    assert devplanes.spike_indel_limits(*_hand_made(65533, 100, [ins])) is None
    # two indels and an SNV between them: the SNV adds nothing, 65531 + 4 = 65535 still fits
    assert devplanes.spike_indel_limits(*_hand_made(65531, 100, [ins, snv, dl])) is None
    assert devplanes.spike_indel_limits(*_hand_made(65532, 100, [ins, snv, dl])) == 1
    # inserted letters: l_seq + 3 > 65535; a deletion adds none
    assert devplanes.spike_indel_limits(*_hand_made(3, 65533, [ins, dl])) == 1
    assert devplanes.spike_indel_limits(*_hand_made(3, 65532, [ins, dl])) is None
    assert devplanes.spike_indel_limits(*_hand_made(3, 65535, [dl, snv])) is None
    # a record that spans none of them
    A, var = _hand_made(65535, 65535, [IR.variant("c", 301, "A", "AG")])
    assert devplanes.spike_indel_limits(A, var) is None
    assert "spike_indel_limits" in inspect.getsource(devplanes.spike_rules)          # (the pre-pass asks, next to spike_indel_caps)


def _tool(bam, fa, vfile, t, seed):
    return sv.main(NS(runPath=None, inBam=bam, outBam=None, variants=vfile, af="%g" % t, seed=seed, refGenome=fa, indels=True))


def test_restated_counts_equal_the_offline_tool_replicate_by_replicate(tmp_path, capsys):
    bam, fa, loci, P, variants = IR.make_case(str(tmp_path))
    vfile = R.write_variants(str(tmp_path / "v.txt"), variants)
    counters, cases = QR.host_counters(bam, variants, fa)
    targets, n_reps = (0.5, 0.25), 4
    got = QR.counts_from(counters, [v.pos for v in variants], [QR.threshold(t) for t in targets], QR.seeds(SEED, n_reps))
    assert got.shape == (len(variants), n_reps, len(targets), 3)
    moved = 0
    for j, s in enumerate(QR.seeds(SEED, n_reps)):
        for t, target in enumerate(targets):
            rows = _tool(bam, fa, vfile, target, s)
            for i, row in enumerate(rows):
                assert got[i, j, t].tolist() == [row["S"], row["READS"], row["V1"]], (i, j, t)
                assert len(counters[i][0]) == row["N"] and int((2 * counters[i][1][:, 1].astype(int) > counters[i][1][:, 0]).sum()) == row["V0"]
            moved += any(got[i, j, t].tolist() != got[i, 0, t].tolist() for i in range(len(variants)))
    assert moved                                                                      # (the replicates differ)
    # three counters do not suffice here: a record that shows the insertion already is counted in alt1 and not in touch
    assert sum(c["shows_it_already"] for c in cases) > 0 and sum(c["ends_in_footprint"] for c in cases) > 0
    assert any((cnt[:, 2] != cnt[:, 3]).any() for (_, cnt), v in zip(counters, variants) if v.kind != af.SNV)
    assert all((cnt[:, 2] == cnt[:, 3]).all() for (_, cnt), v in zip(counters, variants) if v.kind == af.SNV)
    # the cells at one fraction of 2^32 are the replicate counts
    cells = QR.counts_from(counters, [v.pos for v in variants], [QR.threshold(t) for t in targets], QR.seeds(SEED, n_reps), [1 << 32])
    assert np.array_equal(cells[:, :, :, 0, 2:], got) and (cells[:, :, :, 0, 0] == np.array([len(n) for n, _ in counters])[:, None, None]).all()


def test_report_writers_take_indel_variants(tmp_path):
    ins, dl = IR.variant("chr1", 100, "A", "AGAT"), IR.variant("chr1", 200, "ACGT", "A")
    variants, targets, seeds = [ins, dl], [0.05, 0.01], [7, 8]
    row = lambda v, pi: [v.chrom, "%d" % v.pos, v.ref] + ["x"] * (len(dsaf.HEADER_ALL) - 3)
    entries, k = {}, 0
    for i, v in enumerate(variants):
        for t in range(2):
            per = []
            for j in range(2):
                called = (i + t + j) % 2 == 0
                per.append((dict(N=50, V0=1, S=3 + j, READS=9 + k, V1=4 + j), row(v, 1.0), (v.ref, [v.alt]) if called else None))
                k += 1
            entries[(i, t)] = per
    out = str(tmp_path / "o")
    spike.write_replicates(out, variants, targets, seeds, entries)
    spike.write_sensitivity(out, variants, targets, entries)
    spike.write_curve(out, variants, targets, entries)
    rep = [l.split("\t") for l in open(out + ".spikeAF.replicates.txt").read().splitlines()]
    assert rep[0] == list(spike.REPLICATES_HEADER) and len(rep) == 1 + 8
    assert rep[1][:7] == ["chr1", "100", "A", "AGAT", "0.05", "0", "7"] and rep[1][7:12] == ["50", "1", "3", "9", "4"] and rep[1][-1] == "1"
    assert rep[6][:7] == ["chr1", "200", "ACGT", "A", "0.05", "1", "8"] and rep[6][-1] == "1" and rep[5][-1] == "0"
    sens = [l.split("\t") for l in open(out + ".spikeAF.sensitivity.txt").read().splitlines()]
    assert sens[0] == list(spike.SENSITIVITY_HEADER) and [l[:7] for l in sens[1:]] == [
        ["chr1", "100", "A", "AGAT", "0.05", "2", "1"], ["chr1", "100", "A", "AGAT", "0.01", "2", "1"],
        ["chr1", "200", "ACGT", "A", "0.05", "2", "1"], ["chr1", "200", "ACGT", "A", "0.01", "2", "1"]]
    curve = [l.split("\t") for l in open(out + ".spikeAF.curve.txt").read().splitlines()]
    assert curve[0] == list(spike.curve_header(targets)) and curve[1][:5] == ["chr1", "100", "A", "AGAT", "50"] and curve[2][-1] == "NA"
    # a deletion is called by its REF and ALT strings, as the cut file has them
    assert spike._called(dl, [(None, None, ("ACGT", ["A"]))]) == 1 and spike._called(dl, [(None, None, ("A", ["ACGT"]))]) == 0
    cells = [(0, 0.05, 0.5, 25, out + ".c", None)]
    spike.write_depth_replicates(out, variants, cells, seeds, {(i, 0): entries[(i, 0)] for i in range(2)})
    dr = [l.split("\t") for l in open(out + ".spikeAF.depth.replicates.txt").read().splitlines()]
    assert dr[0] == list(spike.DEPTH_REPLICATES_HEADER) and dr[3][:9] == ["chr1", "200", "ACGT", "A", "0.05", "0.5", "25", "0", "7"]


def test_header_symbols_and_abi():
    h = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    for name in ("smc_spike_indels_reps", "smc_spike_indel_touch", "smc_spike_indel_counts"):
        assert re.search(r"\bint %s\(smc_ctx\* ctx," % name, h) and name in _lib.SYMBOLS, name
    assert re.search(r"#define SMC_ABI_VERSION 11\b", h)
    L = _lib.load()
    assert L.smc_abi_version() == 11 and all(hasattr(L, n) for n in ("smc_spike_indels_reps", "smc_spike_indel_touch", "smc_spike_indel_counts"))
    assert len(L.smc_spike_indels_reps.argtypes) == 33 and len(L.smc_spike_indel_counts.argtypes) == 15


def test_smc_spike_rep_counts_is_declared_and_documented_as_before():
    h = open(os.path.join(ROOT, "include", "smcounter_hip.h")).read()
    assert ("int smc_spike_rep_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint32_t* d_cov_cnt, const uint32_t* d_cov_off,\n"
            "                         const uint32_t* cov_off_host, const uint32_t* d_pos1, int32_t n_var, const uint64_t* d_seeds, int32_t n_reps,\n"
            "                         const uint64_t* thr, int32_t n_targets, uint32_t* d_out, void* stream);") in h
    assert ("d_cov_cnt[e][3] uint32 per barcode its pileup reads at the variant's position, those that show ALT before spiking\n"
            " *            and those whose allele key there is a single letter - what the rewrite can touch") in h
    assert "d_out[v][j][t][3] uint32 = (S: covering b with hit, READS: the sum of single[b] over them, V1: the b with" in h
    assert len(_lib.load().smc_spike_rep_counts.argtypes) == 13 and len(_lib.load().smc_spike_depth_counts.argtypes) == 15
    sig = inspect.signature(devplanes.spike_rep_counts)
    assert list(sig.parameters) == ["eng", "positions", "covers", "counters", "seeds", "thresholds"]
