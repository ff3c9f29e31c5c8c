"""The command line with --spikeIndelReps / --spikeIndelDepth on the hand-made BAM of tests/spike_indel_restate.py: the files of the
same run with plain --spikeIndels stay byte for byte; every replicate line is the variant's line in the detection page of a separate
--spikeIndels run with that replicate's seed; a replicate other than 0 and a depth cell against plain runs on the BAM
tools/spike_variants.py --indels writes; the sensitivity and curve pages against the replicates page."""
import argparse
import os
import sys

import pytest

from conftest import ROOT
from smcounter_amd import bamio, dsaf, spike
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import spike_depth_restate as DS  # noqa: E402  (the columns of a cell's replicate line)
import spike_indel_restate as IR  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import test_gpu_lod as TL  # noqa: E402  (its helpers: a run of the command line)

pytestmark = pytest.mark.gpu
SEED = 20240607
REPS, TARGETS, FRACS = 3, (0.5, 0.25), (0.5,)


def _lines(path):
    return [l.split("\t") for l in open(path).read().splitlines()]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The run under test, the plain --spikeIndels run beside it and one --spikeIndels run per replicate seed, made once."""
    tmp = tmp_path_factory.mktemp("indel_reps_cli")
    bam, fa, loci, P, variants = IR.make_case(str(tmp))
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    vfile = R.write_variants(str(tmp / "v.txt"), variants)
    kw = dict(spikeAF=",".join("%g" % t for t in TARGETS), spikeVariants=vfile, dsSeed=SEED)
    # (the same prefix - the VCFs name it: the plain run's files are read before the run under test writes them again)
    TL._run_cli(tmp, "o", bam, fa, bed, P, flags=["--spikeIndels"], **kw)
    plain = {f: open(str(tmp / f), "rb").read() for f in sorted(os.listdir(str(tmp))) if f.startswith("o.")}
    got = TL._run_cli(tmp, "o", bam, fa, bed, P, spikeIndelReps=REPS, spikeIndelDepth=",".join("%g" % f for f in FRACS), **kw)
    seeded = [TL._run_cli(tmp, "s%d" % j, bam, fa, bed, P, flags=["--spikeIndels"], **dict(kw, dsSeed=s)) for j, s in enumerate(PR.seeds(SEED, REPS))]
    return dict(tmp=tmp, bam=bam, fa=fa, bed=bed, P=P, variants=variants, vfile=vfile, plain=plain, got=got, seeded=seeded)


def test_every_file_of_the_plain_spike_indels_run_is_byte_equal(runs):
    tmp, plain = str(runs["tmp"]), runs["plain"]
    names = sorted(f[2:] for f in plain)
    assert len(names) >= 3 * (1 + len(TARGETS)) + 1 and "spikeAF.detection.txt" in names
    for f in names:
        assert open(os.path.join(tmp, "o." + f), "rb").read() == plain["o." + f], f
    more = sorted(set(f[2:] for f in os.listdir(tmp) if f.startswith("o.")) - set(names))
    cells = ["spikeAF%g.dsMT%g%s" % (t, f, s) for t in TARGETS for f in FRACS for s in TL.SUFFIXES]
    pages = ["spikeAF.replicates.txt", "spikeAF.sensitivity.txt", "spikeAF.curve.txt", "spikeAF.depth.detection.txt", "spikeAF.depth.replicates.txt",
             "spikeAF.depth.sensitivity.txt", "spikeAF.depth.curve.txt"]
    assert more == sorted(cells + pages)


def test_replicate_lines_are_the_detection_lines_of_separate_runs(runs):
    variants, T = runs["variants"], len(TARGETS)
    reps = _lines(runs["got"] + ".spikeAF.replicates.txt")
    assert reps[0] == list(spike.REPLICATES_HEADER) and len(reps) == 1 + len(variants) * T * REPS
    compared = 0
    for j, s in enumerate(PR.seeds(SEED, REPS)):
        det = _lines(runs["seeded"][j] + ".spikeAF.detection.txt")
        assert det[0] == list(spike.DETECTION_HEADER) and len(det) == 1 + len(variants) * (1 + T)
        for i in range(len(variants)):
            for t in range(T):
                mine = reps[1 + (i * T + t) * REPS + j]
                assert mine[5:7] == ["%d" % j, "%d" % s]
                assert mine[:5] + mine[7:] == det[1 + i * (1 + T) + 1 + t], (i, t, j)
                compared += 1
    assert compared == len(variants) * T * REPS
    # the replicates differ: S moves with the seed somewhere
    assert any(len({reps[1 + (i * T + t) * REPS + j][PR.S] for j in range(REPS)}) > 1 for i in range(len(variants)) for t in range(T))


def _tool_bam(runs, t, seed, tag):
    out = str(runs["tmp"] / ("tool_%s.bam" % tag))
    sv.main(argparse.Namespace(runPath=None, inBam=runs["bam"], outBam=out, variants=runs["vfile"], af="%g" % t, seed=seed, refGenome=runs["fa"],
                               indels=True))
    bamio.write_bai(out)
    return out


def _called_fields(prefix, v):
    rows, cut = dsaf.read_output(prefix)
    key = (v.chrom, "%d" % v.pos)
    return [rows[key][dsaf._COL[c]] for c in ("UMT", "VMT", "VMF", "PI", "FILTER")] + ["%d" % int(key in cut and cut[key][0] == v.ref and v.alt in cut[key][1])]


def test_a_replicate_and_a_cell_equal_plain_runs_on_the_tools_bam(runs):
    variants, T, P = runs["variants"], len(TARGETS), runs["P"]
    j, t = 2, 1
    s = PR.seeds(SEED, REPS)[j]
    out = _tool_bam(runs, TARGETS[t], s, "rep")
    ref = TL._run_cli(runs["tmp"], "toolrep", out, runs["fa"], runs["bed"], P)
    reps = _lines(runs["got"] + ".spikeAF.replicates.txt")
    for i, v in enumerate(variants):
        assert reps[1 + (i * T + t) * REPS + j][-6:] == _called_fields(ref, v), i
    # one depth cell of the run's own seed: --dsMT 0.5 --dsSampler philox on the BAM the tool writes with that seed
    out = _tool_bam(runs, TARGETS[0], SEED, "cell")
    # (a VCF names its prefix: the plain run writes under the target's own prefix, whose files are put back afterwards)
    target = "%s.spikeAF%g" % (runs["got"], TARGETS[0])
    cell = "%s.dsMT%g" % (target, FRACS[0])
    mine = {x: TL._read(x, TL.SUFFIXES) for x in (target, cell)}
    try:
        ref = TL._run_cli(runs["tmp"], os.path.basename(target), out, runs["fa"], runs["bed"], P, dsMT="%g" % FRACS[0], dsSampler="philox", dsSeed=SEED)
        assert ref == target
        for x in (target, cell):
            for a, b, sfx in zip(mine[x], TL._read(x, TL.SUFFIXES), TL.SUFFIXES):
                assert a == b, (x, sfx)
    finally:
        for x, files in mine.items():
            for sfx, data in zip(TL.SUFFIXES, files):
                open(x + sfx, "wb").write(data)
    det = _lines(runs["got"] + ".spikeAF.depth.detection.txt")
    assert det[0] == list(spike.DEPTH_DETECTION_HEADER) and len(det) == 1 + len(variants) * T * len(FRACS)
    for i, v in enumerate(variants):
        assert det[1 + i * T * len(FRACS)][-6:] == _called_fields("%s.dsMT%g" % (ref, FRACS[0]), v), i
    # ... and the cell of a replicate other than 0
    out = _tool_bam(runs, TARGETS[t], s, "repcell")
    ref = TL._run_cli(runs["tmp"], "toolrepcell", out, runs["fa"], runs["bed"], P, dsMT="%g" % FRACS[0], dsSampler="philox", dsSeed=s)
    dreps = _lines(runs["got"] + ".spikeAF.depth.replicates.txt")
    assert dreps[0] == list(spike.DEPTH_REPLICATES_HEADER) and len(dreps) == 1 + len(variants) * T * len(FRACS) * REPS
    for i, v in enumerate(variants):
        line = dreps[1 + ((i * T + t) * len(FRACS)) * REPS + j]
        assert line[DS.REP] == "%d" % j and line[DS.SEED] == "%d" % s
        assert line[-6:] == _called_fields("%s.dsMT%g" % (ref, FRACS[0]), v), i


def test_sensitivity_and_curve_agree_with_the_replicates_page(runs):
    variants, T = runs["variants"], len(TARGETS)
    reps = _lines(runs["got"] + ".spikeAF.replicates.txt")
    sens, curve = _lines(runs["got"] + ".spikeAF.sensitivity.txt"), _lines(runs["got"] + ".spikeAF.curve.txt")
    assert sens[0] == list(spike.SENSITIVITY_HEADER) and curve[0] == list(spike.curve_header(TARGETS))
    want = PR.sensitivity_from(reps[1:], variants, TARGETS, REPS, dsaf.frac_text)
    assert len(sens) == 1 + len(variants) * T == 1 + len(want) and [l[:19] for l in sens[1:]] == want
    want = PR.curve_from(reps[1:], variants, TARGETS, REPS, dsaf.frac_text)
    assert len(curve) == 1 + len(variants) and [l[:len(want[0])] for l in curve[1:]] == want
