"""Host restatement of --spikeIndelPhase (DESIGN.md "--spikeIndelPhase"): a phase set whose members may be insertions and deletions.
Every member is drawn with the position of the set's leader - its smallest, an SNV's or an anchor's - in counter word 3 and then
applied under its own rule.  The records are tests/spike_indel_restate.py's base-by-base rewrite with that one position swapped in
the draw; the joint rows of FOUR counters per member come from tests/spike_indel_reps_restate.py's walk over the records of the
members' pileups, joined over the barcodes that cover every member; the joint counts from those rows and the two numpy Philox draws
(tests/spike_phase_restate.py's rule with car1 from column 2).  Nothing from the kernel, from tools/spike_variants.py's parsing or
drawing, or from smcounter_amd/spike.py's pages.  Shared by tests/test_spike_indel_phase.py, tests/test_gpu_spike_indel_phase.py and
tests/test_gpu_spike_indel_phase_cli.py."""
import contextlib
import os
import sys

import numpy as np

from smcounter_amd import abi
from smcounter_amd.tools import ds_allele_fraction as af

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ds_af_depth_restate as DR  # noqa: E402  (the "dsMT" draw in numpy)
import spike_indel_reps_restate as QR  # noqa: E402
import spike_indel_restate as IR  # noqa: E402
import spike_phase_restate as PH  # noqa: E402
import spike_reps_restate as PR  # noqa: E402
import spike_restate as SR  # noqa: E402

NAMES = PH.NAMES
# the listings of the hand-made BAM (indexes into IR.make_case's variants: P_INS 101, P_SNV 105, P_DEL 110, P_FLIP 150)
LISTING_A = [(0, 1, 2)]            # PS=hap on 101, 105 and 110; 150 a singleton
LISTING_B = [(0, 2)]               # PS=hap on 101 and 110: 105 a non-member between members, `lead` of 110 is 2
LISTINGS = {"A": LISTING_A, "B": LISTING_B}
# A seed at which, with a threshold of 2^31, the leader's draw spikes some and spares some of the 4 barcodes of each of the shapes
# `all`, `snvins` and `behind`, so that 0 < S_ALL < N_ALL - found on the CPU from this restatement alone (tests/test_spike_indel_phase.py
# asserts it).
SEED = 20240607
HALF, ONE = 1 << 31, 1 << 32


def lead_positions(variants, sets):
    return PH.lead_positions(variants, sets)


@contextlib.contextmanager
def leader_draw(variants, sets):
    """Within the block, IR.restate draws every listed position with its leader's (all variants on one chromosome)."""
    assert len({v.chrom for v in variants}) == 1
    lead = {v.pos: p for v, p in zip(variants, lead_positions(variants, sets))}
    real = IR.draws
    IR.draws = lambda idents, seed, pos1: real(idents, seed, lead.get(pos1, pos1))
    try:
        yield
    finally:
        IR.draws = real


def restate(bam_path, variants, sets, thr, seed, mismatch_thr, fa=None):
    """IR.restate with the sets' draws -> (records, stats)."""
    with leader_draw(variants, sets):
        return IR.restate(bam_path, variants, thr, seed, mismatch_thr, fa)


def host_joint(bam_path, variants, sets, fa=None):
    """Per set (the texts of the barcodes that cover every member, sorted; uint32 [n, M, 4] = per member (reads, alt0, alt1, touch)),
    the members ascending by position."""
    per, _ = QR.host_counters(bam_path, variants, fa)
    out = []
    for members in sets:
        members = sorted(members, key=lambda k: variants[k].pos)
        rows = [dict(zip(per[k][0], per[k][1].tolist())) for k in members]
        names = sorted(set.intersection(*[set(r) for r in rows]))
        out.append((names, np.array([[r[b] for r in rows] for b in names], np.uint32).reshape(len(names), len(members), 4)))
    return out


def cell_rule(cnt, u, d, thr, dthr):
    """(N_ALL', V0_ALL', S_ALL', V1_ALL') of one set from its joint barcodes' counters [n, M, 4] and the two draws."""
    c = np.asarray(cnt).astype(np.int64)
    assert c.ndim == 3 and c.shape[2] == 4
    car0 = (2 * c[:, :, 1] > c[:, :, 0]).all(axis=1)
    car1 = (2 * c[:, :, 2] > c[:, :, 0]).all(axis=1)
    hit = np.asarray(u).astype(np.uint64) < np.uint64(thr)
    keep = np.asarray(d).astype(np.uint64) < np.uint64(dthr)
    return [int(keep.sum()), int((keep & car0).sum()), int((keep & hit).sum()), int((keep & np.where(hit, car1, car0)).sum())]


def counts_from(joint, lead_pos, thr, dthr, seed_list):
    """uint32 [G, R, T, F, 4] from per set (barcode texts, uint32 [n, M, 4]), the leaders' 1-based positions and both axes' thresholds."""
    out = np.zeros((len(joint), len(seed_list), len(thr), len(dthr), 4), np.uint32)
    for g, ((names, cnt), pos) in enumerate(zip(joint, lead_pos)):
        for j, s in enumerate(seed_list):
            u = SR.draw(names, s, pos) if len(names) else np.zeros(0, np.uint64)
            d = DR.depth_draw(PR.idents(names), s)
            for t, h in enumerate(thr):
                for f, q in enumerate(dthr):
                    out[g, j, t, f] = cell_rule(cnt, u, d, h, q)
    return out


def restate_counts(bam_path, fa_path, variants, sets, targets, fracs, seed, n_reps):
    """-> (uint32 [G, R, T, F, 4], the host's joint barcodes); fracs: 1.0 stands for the full depth."""
    joint = host_joint(bam_path, variants, sets, fa_path)
    lead = [min(variants[k].pos for k in members) for members in sets]
    return counts_from(joint, lead, [PR.threshold(t) for t in targets], [DR.frac_thr(f) for f in fracs], PR.seeds(seed, n_reps)), joint


def variant_line(v, ps=None):
    return "%s\t%d\t.\t%s\t%s\t.\t.\t%s\n" % (v.chrom, v.pos, v.ref, v.alt, "PS=%s" % ps if ps else ".")


def write_listing(path, variants, sets, names=None):
    """A VCF-shaped variants file in the order given: the members of sets[g] carry PS=<names[g]> (hap, hap1, ...)."""
    names = names or ["hap" + ("%d" % g if g else "") for g in range(len(sets))]
    of = {k: names[g] for g, members in enumerate(sets) for k in members}
    with open(path, "w") as fh:
        for k, v in enumerate(variants):
            fh.write(variant_line(v, of.get(k)))
    return path


def records_with_lead(variants, sets, thr):
    """The records as smc_spike_indels takes them, ascending by position, with `lead` from the sets (indexes into `variants`) ->
    (abi.SPIKE_INDEL_VARIANT_DTYPE array, the pool of inserted letters, the index of each record in `variants`)."""
    lead = lead_positions(variants, sets)
    order = sorted(range(len(variants)), key=lambda k: variants[k].pos)
    var = np.zeros(len(order), abi.SPIKE_INDEL_VARIANT_DTYPE)
    pool = bytearray()
    at = [variants[m].pos for m in order]
    for j, k in enumerate(order):
        v = variants[k]
        var[j]["pos0"], var[j]["kind"], var[j]["thr"], var[j]["lead"] = v.pos - 1, v.kind, thr, j - at.index(lead[k])
        if v.kind == af.SNV:
            var[j]["ref"], var[j]["alt"] = ord(v.ref), ord(v.alt)
        else:
            var[j]["ref"] = var[j]["alt"] = ord(v.ref[0])
            var[j]["len"] = IR.length(v)
            if v.kind == af.INS:
                var[j]["ins_off"] = len(pool)
                pool += v.alt[1:].encode()
    return var, np.frombuffer(bytes(pool) or b"\0", np.uint8).copy(), order


def shape_of(text):
    """The read shape of a barcode text of the hand-made BAM ("ALL02" -> "all")."""
    return text[:-2].lower()
