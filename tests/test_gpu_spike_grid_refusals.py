"""--spikeGrid: the refusals that depend on the data.  Its own - a (replicate, fraction) at which no kept barcode has two or more read
names, for the run's seed and for a later replicate's, the message naming the replicate, its seed and f - and what --dsRpbSampler
philox refuses, under this flag: a file without a barcode of two or more names, a run where one read id stands for two names, a hash
collision (status forced).  Each ends the run with its message naming --spikeGrid before any file is written, with the file-wide
table closed and every uploaded run freed, and the same command works afterwards in the same process."""
import os
import sys

import pytest

from conftest import ROOT
from smcounter_amd import cli, devplanes, fasta
from smcounter_amd.tools import ds_allele_fraction as af
from smcounter_amd.tools import ds_reads_within_mt as rw

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_grid_restate as GR  # noqa: E402
import ds_restate  # noqa: E402
import ds_rpb_restate  # noqa: E402
import spike_grid_restate as G  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402
import spike_rpb_restate as RR  # noqa: E402
from test_gpu_spike_rpb_refusals import _released, tracked  # noqa: E402,F401  (its tracking of tables and uploaded runs)

pytestmark = pytest.mark.gpu
SEED = 20240607
FRACS, RPBS = (1.0, 0.5), (1.5, 3.0)
GRID_FILES = ("detection", "replicates", "sensitivity", "budget")


def _inputs(tmp_path):
    bam, fa, loci, P = ds_restate.make_case(str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    variants = SR.pick_positions(bam, fa, loci, 2)
    vfile = R.write_variants(str(tmp_path / "v.txt"), variants)
    return bam, fa, loci, P, bed, variants, vfile


def _run(tmp_path, tag, bam, fa, bed, P, vfile, seed=SEED, reps=None):
    prefix = str(tmp_path / tag)
    argv = ["--%s=%s" % kv for kv in dict(outPrefix=prefix, bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, hpLen=P.hpLen, refGenome=fa,
                                          spikeAF="0.3", spikeVariants=vfile, spikeDepth="1,0.5", spikeRpb="1.5,3", dsSeed=seed).items()]
    cli.main(cli.build_parser().parse_args(argv + ["--spikeGrid"] + (["--spikeReps=%d" % reps] if reps else [])))
    return prefix


def _nothing_written(tmp_path, tag):
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith(tag + ".")]


def _works(tmp_path, seen, bam, fa, bed, P, vfile, seed=SEED, reps=2):
    """The same command in the same process, on the good file, replicates included."""
    good = _run(tmp_path, "good", bam, fa, bed, P, vfile, seed=seed, reps=reps)
    assert os.path.exists(good + ".spikeAF0.3.dsMT0.5.dsRpb1.5.smCounter.all.txt")
    assert all(os.path.exists(good + ".spikeAF.grid.%s.txt" % x) for x in GRID_FILES)
    _released(seen)


def _one_multi(tmp_path, bam, reps):
    """A copy of `bam` whose only barcode of two or more names is `multi`, and a base seed - found on the CPU - under which the "dsMT"
    draw keeps `multi` at 0.5 for replicate 0 and drops it for some later replicate -> (the copy, the base seed, the first such
    replicate, a base seed whose replicate 0 drops it)."""
    per_bc, order = rw.group_reads(ds_restate.placed_qnames(bam))
    multi = next(bc for bc in order if len(per_bc[bc]) > 1)
    out = GR.one_multi_barcode_bam(bam, str(tmp_path / "onemulti.bam"), multi)
    groups = RR.file_groups(out)
    assert groups["counts"]["multi"] == 1
    later = first = None
    for s in range(SEED, SEED + 400):
        kept = [bool(G.keeps_a_multi_name_barcode(groups, FRACS, [x])) for x in PR.seeds(s, reps)]
        if later is None and kept[0] and not all(kept):
            later = (s, kept.index(False))
        if first is None and not kept[0]:
            first = s
        if later and first is not None:
            return out, later[0], later[1], first
    raise AssertionError("no seed found")


def test_a_later_replicate_that_keeps_no_multi_name_barcode_is_refused_before_any_file(tmp_path, tracked):
    bam, fa, loci, P, bed, variants, vfile = _inputs(tmp_path)
    reps = 4
    bad, seed, j, _ = _one_multi(tmp_path, bam, reps)
    assert j > 0
    msg = r"^--spikeGrid: replicate %d \(seed %d\), fraction 0\.5: no barcode kept there has more than one read name, so " \
          r"ds\.reads\.withinMT\.py's probKeep \(:58\) is not defined \(it divides by zero\)$" % (j, PR.seeds(seed, reps)[j])
    with pytest.raises(SystemExit, match=msg):
        _run(tmp_path, "bad", bad, fa, bed, P, vfile, seed=seed, reps=reps)
    _nothing_written(tmp_path, "bad")
    _released(tracked)
    # the same file and seed with the replicates before that one: every (replicate, fraction) used is defined, and the run works
    fine = _run(tmp_path, "fine", bad, fa, bed, P, vfile, seed=seed, reps=j if j >= 2 else None)
    assert os.path.exists(fine + ".spikeAF0.3.dsMT0.5.dsRpb3.smCounter.all.txt") and os.path.exists(fine + ".spikeAF.grid.detection.txt")
    _released(tracked)
    _works(tmp_path, tracked, bam, fa, bed, P, vfile, seed=seed, reps=reps)


def test_the_runs_own_seed_that_keeps_no_multi_name_barcode_is_refused_before_any_file(tmp_path, tracked):
    bam, fa, loci, P, bed, variants, vfile = _inputs(tmp_path)
    bad, _, _, seed = _one_multi(tmp_path, bam, 4)
    msg = r"^--spikeGrid: replicate 0 \(seed %d\), fraction 0\.5: no barcode kept there has more than one read name" % seed
    for reps in (None, 3):
        with pytest.raises(SystemExit, match=msg):
            _run(tmp_path, "bad", bad, fa, bed, P, vfile, seed=seed, reps=reps)
        _nothing_written(tmp_path, "bad")
        _released(tracked)
    _works(tmp_path, tracked, bam, fa, bed, P, vfile, seed=seed)


def _refused(tmp_path, seen, bad_bam, msg, reps=None):
    bam, fa, loci, P, bed, variants, vfile = _inputs(tmp_path)
    with pytest.raises(SystemExit, match=msg):
        _run(tmp_path, "bad", bad_bam(bam), fa, bed, P, vfile, reps=reps)
    _nothing_written(tmp_path, "bad")
    _released(seen)
    _works(tmp_path, seen, bam, fa, bed, P, vfile)


def test_a_file_without_a_multi_name_barcode_is_refused(tmp_path, tracked):
    _refused(tmp_path, tracked, lambda bam: ds_rpb_restate.write_one_name_per_barcode(bam, str(tmp_path / "one.bam")),
             r"--spikeGrid 1\.5: .*one\.bam has no barcode with more than one read name")


@pytest.mark.parametrize("reps", (None, 2))
def test_a_read_id_that_stands_for_two_names_is_refused(tmp_path, tracked, reps):
    _refused(tmp_path, tracked, lambda bam: ds_rpb_restate.write_shared_read_ids(bam, str(tmp_path / "shared.bam")),
             r"--spikeGrid: the run \S+ has a read id \(read name without its last field\) shared by two different read names", reps=reps)


def test_a_hash_collision_is_refused(engine0, tmp_path, tracked, monkeypatch):
    """The table's status forced to a name collision: the refusal names the switch, leaves out the advice to use a sampler the cells do
    not have, and closes the table; the pre-pass works once the status is the table's own again."""
    bam, fa, loci, P, bed, variants, vfile = _inputs(tmp_path)
    vs = [af.Variant(v.chrom, v.pos, v.ref, v.alt, v.alt, af.SNV) for v in variants]
    grid = lambda: dict(targets=list(RPBS), fracs=list(FRACS), reps=2, flag="--spikeGrid", params=[P] * 4)
    with monkeypatch.context() as m:
        m.setattr(devplanes.ReadGroups, "status", lambda self: devplanes.RG_NAME_COLLISION)
        with pytest.raises(ValueError, match=r"^--spikeGrid: .*: two read names share a 64-bit name identity; the philox read sampler "
                                             r"refuses the file$"):
            devplanes.spike_rules(bam, fasta.FastaFile(fa), vs, [0.3], [P], SEED, engine0, keep={}, rpb=grid())
        _released(tracked)
        with pytest.raises(SystemExit, match="--spikeGrid: .*two read names share a 64-bit name identity"):
            _run(tmp_path, "bad", bam, fa, bed, P, vfile)
        _nothing_written(tmp_path, "bad")
        _released(tracked)
    keep, rpb = {}, grid()
    try:
        devplanes.spike_rules(bam, fasta.FastaFile(fa), vs, [0.3], [P], SEED, engine0, keep=keep, rpb=rpb)
        assert len(rpb["rules"]) == 4 and all(r.grid and r.flag == "--spikeGrid" for r in rpb["rules"]) and rpb["rep_thr"].shape == (2, 2, 2)
        assert len(rpb["counts"]) == len(vs) and all(len(c) == 4 for c in rpb["counts"]) and all(r is not None for r in keep["records"])
    finally:
        devplanes.free_af_runs(keep.get("runs"))
        devplanes.close_rules(rpb.get("rules"))
    _released(tracked)
