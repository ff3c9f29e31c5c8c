"""The command line with --spikeIndelPhase, every run a fresh child process under a time limit of its own: on the hand-made BAM of
tests/spike_indel_restate.py (listing A) and on bam_cigars, with two targets x two fractions x R = 4 and --lod - each target's files
against a plain run on the BAM tools/spike_variants.py --phased --indels writes, the cells against the two-step --dsMT f --dsSampler
philox workflow on it, the full-depth files, the phase page against the restatement (tests/spike_indel_phase_restate.py) and the
outputs' own .cut.txt, the replicate lines against separate runs with --dsSeed s_j, the sensitivity page against the replicate lines.
Two cross-checks against what exists without the flag: sets without an indel give --spikePhase's tree, indels without a set the tree
of the same run without the flag."""
import argparse
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT
from smcounter_amd import bamio, dsaf, spike
from smcounter_amd.py2compat import py2_round
from smcounter_amd.tools import spike_variants as sv

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_restate  # noqa: E402
import spike_indel_phase_restate as XR  # noqa: E402
import spike_indel_restate as IR  # noqa: E402
import spike_phase_restate as PH  # noqa: E402  (the columns of the phase pages)
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = XR.SEED
SUFFIXES = (".smCounter.all.txt", ".smCounter.cut.txt", ".smCounter.cut.vcf")
LOD_SUFFIXES = (".lod.bedgraph", ".lod.bedgraph.quantiles.txt")
REPS, FRACS = 4, (0.5, 0.25)
LIMIT = 600                      # seconds a child may take


def _start(tmp, tag, bam, fa, bed, P, flags=(), **kw):
    """A run of the command line in a child process of its own -> (prefix, the process)."""
    prefix = str(tmp / tag)
    opts = dict(outPrefix=prefix, bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, hpLen=P.hpLen, minBQ=P.minBQ, minMQ=P.minMQ,
                mismatchThr=P.mismatchThr, mtDrop=P.mtDrop, maxMT=P.maxMT, primerDist=P.primerDist, refGenome=fa, **kw)
    cmd = [sys.executable, "-m", "smcounter_amd.cli"] + ["--%s=%s" % (k, v) for k, v in opts.items()] + list(flags)
    return prefix, subprocess.Popen(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _finish(started):
    """Every child to its end, each under LIMIT; a failure or a child over its limit fails the test with the child's output."""
    bad = []
    for prefix, p in started:
        try:
            out, _ = p.communicate(timeout=LIMIT)
        except subprocess.TimeoutExpired:
            p.kill()
            out, _ = p.communicate()
            bad.append("%s: over %d s\n%s" % (prefix, LIMIT, out[-2000:]))
            continue
        if p.returncode != 0:
            bad.append("%s: exit status %d\n%s" % (prefix, p.returncode, out[-2000:]))
    assert not bad, "\n".join(bad)
    return [prefix for prefix, _ in started]


def _read(prefix, suffixes):
    return [open(prefix + s, "rb").read() for s in suffixes]


def _lines(path):
    return [l.split("\t") for l in open(path).read().splitlines()]


def _tree(tmp, tag):
    """The files of the run with prefix `tag`, by suffix, with the prefix itself (a path in .cut.vcf, a name in the LOD summary) masked."""
    mask = lambda data: re.sub(b"(?m)^" + tag.encode() + b"(?=[.\t])", b"<prefix>", data.replace(str(tmp / tag).encode(), b"<prefix>"))
    return {f[len(tag):]: mask(open(str(tmp / f), "rb").read()) for f in sorted(os.listdir(str(tmp))) if f.startswith(tag + ".")}


def _inputs(name, tmp):
    """-> (bam, fasta, loci, params, variants, the set's members, targets)."""
    if name == "case":
        bam, fa, loci, P, variants = IR.make_case(tmp)
        return bam, fa, loci, P, variants, XR.LISTING_A, (0.5, 0.25)
    bam, fa, loci, P = ds_restate.load_fixture(name, tmp)
    variants = IR.pick_variants(bam, fa, loci, 4, gap=8)
    on = [k for k, v in enumerate(variants) if v.chrom == variants[0].chrom]
    assert len(on) >= 3                                                                  # (a non-member between the two members)
    return bam, fa, loci, P, variants, [(on[0], on[-1])], (0.3, 0.1)


@pytest.fixture(scope="module", params=("case", "bam_cigars"))
def runs(request, tmp_path_factory):
    """The run under test and every run it is compared with, started together (nine processes) and made once per input."""
    tmp = tmp_path_factory.mktemp("indel_phase_cli_" + request.param)
    bam, fa, loci, P, variants, sets, targets = _inputs(request.param, str(tmp))
    bed = ds_restate.write_bed(str(tmp / "t.bed"), loci)
    vfile = XR.write_listing(str(tmp / "v.vcf"), variants, sets)
    depth = ",".join("%g" % f for f in FRACS)
    kw = dict(spikeAF=",".join("%g" % t for t in targets), spikeVariants=vfile)
    started = [_start(tmp, "o", bam, fa, bed, P, flags=["--lod", "--spikeIndelPhase"], spikeIndelReps=REPS, spikeIndelDepth=depth, dsSeed=SEED, **kw),
               _start(tmp, "p", bam, fa, bed, P, flags=["--lod"])]
    for j, s in enumerate(PR.seeds(SEED, REPS)):
        if j:                                                                            # (replicate 0 has the seed of the run itself)
            started.append(_start(tmp, "s%d" % j, bam, fa, bed, P, flags=["--spikeIndelPhase"], spikeIndelDepth=depth, dsSeed=s, **kw))
    for t in targets:
        out = str(tmp / ("tool%g.bam" % t))
        sv.main(argparse.Namespace(runPath=None, inBam=bam, outBam=out, variants=vfile, af="%g" % t, seed=SEED, refGenome=fa, phased=True, indels=True))
        bamio.write_bai(out)
        started.append(_start(tmp, "w.spikeAF%g" % t, out, fa, bed, P, dsMT=depth, dsSampler="philox", dsSeed=SEED))
    assert len(started) <= 16
    done = _finish(started)
    return dict(tmp=tmp, bam=bam, fa=fa, P=P, variants=variants, sets=sets, targets=targets, got=done[0], plain=done[1],
                seeded=dict(zip(range(1, REPS), done[2:2 + REPS - 1])), tool=dict(zip(targets, done[2 + REPS - 1:])))


def test_targets_and_cells_equal_plain_runs_on_the_tools_bam_and_the_full_depth_files_stay(runs):
    got, targets = runs["got"], runs["targets"]
    mine, plain = _tree(runs["tmp"], "o"), _tree(runs["tmp"], "p")
    for s in SUFFIXES + LOD_SUFFIXES:
        assert mine[s] == plain[s], s                                                    # (the full-depth files are those of a run without the flags)
    moved = 0
    for t in targets:
        ref = runs["tool"][t]
        mine = got + ".spikeAF%g" % t
        assert _read(mine, SUFFIXES) == [x.replace(ref.encode(), mine.encode()) for x in _read(ref, SUFFIXES)], "target %g" % t
        moved += _read(mine, SUFFIXES)[0] != _read(got, SUFFIXES)[0]
        for f in FRACS:
            cell, theirs = "%s.dsMT%g" % (mine, f), "%s.dsMT%g" % (ref, f)
            assert _read(cell, SUFFIXES) == [x.replace(theirs.encode(), cell.encode()) for x in _read(theirs, SUFFIXES)], "cell %g x %g" % (t, f)
    assert moved > 0                                                                     # (a spike-in changed a row somewhere)
    names = {f[2:] for f in os.listdir(str(runs["tmp"])) if f.startswith("o.")}
    assert {"spikeAF.detection.txt", "spikeAF.phase.txt", "spikeAF.phase.replicates.txt", "spikeAF.phase.sensitivity.txt", "spikeAF.replicates.txt",
            "spikeAF.depth.detection.txt", "spikeAF.depth.replicates.txt"} <= names


def _want_line(pset_name, members, o, c):
    _, cut = dsaf.read_output(o[3])
    key = lambda v: (v.chrom, "%d" % v.pos)
    called = int(all(key(v) in cut and cut[key(v)][0] == v.ref and v.alt in cut[key(v)][1] for v in members))
    return [pset_name, members[0].chrom, ",".join("%d" % v.pos for v in members), ",".join(v.ref for v in members), ",".join(v.alt for v in members),
            "full" if o[0] is None else "%g" % o[0], "full" if o[1] is None else "%g" % o[1], "%d" % o[2]] + ["%d" % x for x in c] + \
           [dsaf.frac_text(int(c[3]) / int(c[0]) if int(c[0]) else 0.0), "%d" % called]


def test_the_phase_page_is_the_restatement_and_the_outputs_own_cut(runs):
    got, targets, P, variants = runs["got"], list(runs["targets"]), runs["P"], runs["variants"]
    T, F = len(targets), len(FRACS)
    members = sorted((variants[k] for k in runs["sets"][0]), key=lambda v: v.pos)
    counts, joint = XR.restate_counts(runs["bam"], runs["fa"], variants, runs["sets"], targets, [1.0] + list(FRACS), SEED, REPS)
    page = _lines(got + ".spikeAF.phase.txt")
    assert page[0] == list(spike.PHASE_HEADER) and len(page) == 1 + 1 + T + T * F
    outs = [(None, None, P.mtDepth, got)] + [(t, None, P.mtDepth, got + ".spikeAF%g" % t) for t in targets] + \
           [(t, f, max(1, int(py2_round(f * P.mtDepth))), got + ".spikeAF%g.dsMT%g" % (t, f)) for t in targets for f in FRACS]
    for k, o in enumerate(outs):
        if o[0] is None:
            c = [counts[0, 0, 0, 0, 0], counts[0, 0, 0, 0, 1], 0, counts[0, 0, 0, 0, 1]]
        else:
            c = counts[0, 0, targets.index(o[0]), 0 if o[1] is None else 1 + FRACS.index(o[1])]
        assert page[1 + k] == _want_line("hap", members, o, c), k
    assert any(len(v.ref) != len(v.alt) for v in members) and "," in page[1][3]          # (an indel member prints its listed texts)
    assert int(page[1][PH.P_N]) == len(joint[0][0]) > 0 and any(0 < int(l[PH.P_S]) for l in page[2:])
    # the replicate lines: the phase page of a separate run with --dsSeed s_j; replicate 0 the run's own page
    reps = _lines(got + ".spikeAF.phase.replicates.txt")
    assert reps[0] == list(spike.PHASE_REPLICATES_HEADER) and len(reps) == 1 + (T + T * F) * REPS
    for j, seed_j in enumerate(PR.seeds(SEED, REPS)):
        single_page = page if j == 0 else _lines(runs["seeded"][j] + ".spikeAF.phase.txt")
        for c in range(T + T * F):
            line = reps[1 + c * REPS + j]
            assert line[8:10] == ["%d" % j, "%d" % seed_j] and line[:8] + line[10:] == single_page[2 + c], (c, j)
            t, f = (c, 0) if c < T else (divmod(c - T, F)[0], 1 + divmod(c - T, F)[1])
            assert line[10:14] == ["%d" % x for x in counts[0, j, t, f]]
    assert len({tuple(reps[1 + j][10:14]) for j in range(REPS)}) > 1                      # (the replicates differ)
    # the sensitivity table: what the replicate lines say
    sens = _lines(got + ".spikeAF.phase.sensitivity.txt")
    assert sens[0] == list(spike.PHASE_SENSITIVITY_HEADER) and len(sens) == 1 + T + T * F
    for c in range(T + T * F):
        per = reps[1 + c * REPS:1 + (c + 1) * REPS]
        called = sum(int(l[PH.R_CALLED]) for l in per)
        lo, hi = PR.wilson(called, REPS)
        afs = [int(l[PH.R_V1]) / int(l[PH.R_N]) if int(l[PH.R_N]) else 0.0 for l in per]
        assert sens[1 + c] == per[0][:8] + ["%d" % REPS, "%d" % called, dsaf.frac_text(called / REPS), dsaf.frac_text(lo), dsaf.frac_text(hi),
                                            dsaf.frac_text(sum(afs) / REPS), dsaf.frac_text(min(afs)), dsaf.frac_text(max(afs))]


def test_sets_without_an_indel_give_the_tree_of_spike_phase(tmp_path):
    bam, fa, loci, P, snvs = SR.make_case(str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = str(tmp_path / "v.vcf")
    open(vfile, "w").write(PH.snv_line(snvs[1], "hap") + PH.snv_line(snvs[2]) + PH.snv_line(snvs[0], "hap"))
    kw = dict(spikeAF="0.5,0.2", spikeVariants=vfile, dsSeed=SEED)
    _finish([_start(tmp_path, "a", bam, fa, bed, P, flags=["--spikeIndelPhase"], spikeIndelReps=4, spikeIndelDepth="0.5", **kw),
             _start(tmp_path, "b", bam, fa, bed, P, flags=["--spikePhase"], spikeReps=4, spikeDepth="0.5", **kw)])
    mine, theirs = _tree(tmp_path, "a"), _tree(tmp_path, "b")
    assert sorted(mine) == sorted(theirs) and ".spikeAF.phase.replicates.txt" in mine
    for f in sorted(mine):
        assert mine[f] == theirs[f], f


def test_indels_without_a_set_give_the_tree_of_the_run_without_the_flag(tmp_path):
    bam, fa, loci, P, variants = IR.make_case(str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    vfile = XR.write_listing(str(tmp_path / "v.vcf"), variants, [])
    kw = dict(spikeAF="0.5,0.2", spikeVariants=vfile, dsSeed=SEED)
    _finish([_start(tmp_path, "a", bam, fa, bed, P, flags=["--spikeIndelPhase"], spikeIndelReps=4, spikeIndelDepth="0.5", **kw),
             _start(tmp_path, "b", bam, fa, bed, P, spikeIndelReps=4, spikeIndelDepth="0.5", **kw),
             _start(tmp_path, "c", bam, fa, bed, P, flags=["--spikeIndelPhase"], **kw),
             _start(tmp_path, "d", bam, fa, bed, P, flags=["--spikeIndels"], **kw)])
    for x, y in (("a", "b"), ("c", "d")):
        mine, theirs = _tree(tmp_path, x), _tree(tmp_path, y)
        assert sorted(mine) == sorted(theirs) and ".spikeAF.detection.txt" in mine and ".spikeAF.phase.txt" not in mine
        for f in sorted(mine):
            assert mine[f] == theirs[f], (x, f)
