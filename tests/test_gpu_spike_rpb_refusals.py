"""--spikeRpb: what --dsRpbSampler philox refuses, under this flag - a file without a barcode of two or more names, a run where one
read id stands for two names, a hash collision (status forced) - each with its message naming --spikeRpb, no output file written, the
file-wide table closed and every uploaded run freed, and a run in the same process that works afterwards."""
import os
import sys

import pytest

from conftest import ROOT
from smcounter_amd import cli, devplanes, fasta
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.join(ROOT, "tests"))
import ds_af_restate as R  # noqa: E402
import ds_restate  # noqa: E402
import ds_rpb_restate  # noqa: E402
import spike_restate as SR  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = 20240607


@pytest.fixture
def tracked(monkeypatch):
    """Every ReadGroups table made and every run uploaded while the test runs, and which of the runs were freed."""
    seen = dict(tables=[], uploaded=[], freed=set())
    init, upload, free = devplanes.ReadGroups.__init__, devplanes.upload_run, devplanes.RunOnDevice.free

    def new_table(self, eng):
        init(self, eng)
        seen["tables"].append(self)

    def new_upload(eng, A, run_ref):
        up = upload(eng, A, run_ref)
        seen["uploaded"].append(up)
        return up

    def new_free(self, shared=True):
        if shared:
            seen["freed"].add(id(self))
        free(self, shared)
    monkeypatch.setattr(devplanes.ReadGroups, "__init__", new_table)
    monkeypatch.setattr(devplanes, "upload_run", new_upload)
    monkeypatch.setattr(devplanes.RunOnDevice, "free", new_free)
    return seen


def _released(seen):
    assert seen["tables"] and all(t._h is None for t in seen["tables"])                    # (every table closed)
    assert all(id(up) in seen["freed"] for up in seen["uploaded"])                         # (every uploaded run freed)


def _inputs(tmp_path):
    bam, fa, loci, P = ds_restate.make_case(str(tmp_path))
    bed = ds_restate.write_bed(str(tmp_path / "t.bed"), loci)
    variants = SR.pick_positions(bam, fa, loci, 2)
    vfile = R.write_variants(str(tmp_path / "v.txt"), variants)
    return bam, fa, loci, P, bed, variants, vfile


def _run(tmp_path, tag, bam, fa, bed, P, vfile, **kw):
    prefix = str(tmp_path / tag)
    cli.main(dict(outPrefix=prefix, bamFile=bam, bedTarget=bed, mtDepth=P.mtDepth, rpb=P.rpb, hpLen=P.hpLen, refGenome=fa, spikeAF="0.3",
                  spikeVariants=vfile, spikeRpb="1.5,3", dsSeed=SEED, **kw))
    return prefix


def _refused(tmp_path, tracked, bad_bam, msg, **kw):
    """The run on `bad_bam` ends with `msg` before any file; then the same command works on the good file, replicates included."""
    bam, fa, loci, P, bed, variants, vfile = _inputs(tmp_path)
    with pytest.raises(SystemExit, match=msg):
        _run(tmp_path, "bad", bad_bam(bam), fa, bed, P, vfile, **kw)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("bad.")]
    _released(tracked)
    good = _run(tmp_path, "good", bam, fa, bed, P, vfile, spikeReps=2)
    assert os.path.exists(good + ".spikeAF0.3.dsRpb1.5.smCounter.all.txt") and os.path.exists(good + ".spikeAF.rpb.replicates.txt")
    _released(tracked)


def test_a_file_without_a_multi_name_barcode_is_refused(tmp_path, tracked):
    _refused(tmp_path, tracked, lambda bam: ds_rpb_restate.write_one_name_per_barcode(bam, str(tmp_path / "one.bam")),
             r"--spikeRpb 1\.5: .*one\.bam has no barcode with more than one read name")


@pytest.mark.parametrize("reps", (None, 2))
def test_a_read_id_that_stands_for_two_names_is_refused(tmp_path, tracked, reps):
    _refused(tmp_path, tracked, lambda bam: ds_rpb_restate.write_shared_read_ids(bam, str(tmp_path / "shared.bam")),
             r"--spikeRpb: the run \S+ has a read id \(read name without its last field\) shared by two different read names",
             **({"spikeReps": reps} if reps else {}))


def test_a_hash_collision_is_refused(engine0, tmp_path, tracked, monkeypatch):
    """The table's status forced to a name collision: spike_rules(rpb=) refuses with the flag's name and without the advice to use a
    sampler the cells do not have, closes the table, and works once the status is the table's own again."""
    bam, fa, loci, P, bed, variants, vfile = _inputs(tmp_path)
    vs = [af.Variant(v.chrom, v.pos, v.ref, v.alt, v.alt, af.SNV) for v in variants]
    call = lambda keep: devplanes.spike_rules(bam, fasta.FastaFile(fa), vs, [0.3], [P], SEED, engine0, keep=keep,
                                              rpb=dict(targets=[1.5, 3.0], params=[P, P]))
    with monkeypatch.context() as m:
        m.setattr(devplanes.ReadGroups, "status", lambda self: devplanes.RG_NAME_COLLISION)
        with pytest.raises(ValueError, match=r"^--spikeRpb: .*: two read names share a 64-bit name identity; the philox read sampler "
                                             r"refuses the file$"):
            call({})
        _released(tracked)
        with pytest.raises(SystemExit, match="--spikeRpb: .*two read names share a 64-bit name identity"):
            _run(tmp_path, "bad", bam, fa, bed, P, vfile)
        assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("bad.")]
        _released(tracked)
    keep = {}
    rpb = dict(targets=[1.5, 3.0], params=[P, P])
    try:
        devplanes.spike_rules(bam, fasta.FastaFile(fa), vs, [0.3], [P], SEED, engine0, keep=keep, rpb=rpb)
        assert len(rpb["rules"]) == 2 and len(rpb["counts"]) == len(vs) and all(r is not None for r in keep["records"])
    finally:
        devplanes.free_af_runs(keep.get("runs"))
        devplanes.close_rules(rpb.get("rules"))
    _released(tracked)
