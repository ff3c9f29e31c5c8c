"""Python mirror of include/smcounter_hip.h: ctypes structs and numpy record dtypes."""
from __future__ import annotations

import ctypes

import numpy as np

from .params import VcParams

SMC_NT = 12
(T_CNT, T_FWD, T_REV, T_LOWQ, T_R1N, T_R1LE, T_R2N, T_R2BCLE, T_R2PRLE, T_CONCORD, T_DISCORD,
 T_PAD) = range(SMC_NT)

ST_OK, ST_ZERO_COVERAGE, ST_DOWNSAMPLED, ST_BAD_INPUT, ST_UNDERFLOW = 0, 1, 0x100, 0x200, 0x400

F_LM, F_LSM, F_HP, F_LOWC, F_DP, F_SB, F_LOWQ, F_R1CP, F_R2CP, F_PRIMERCP = (
    1, 2, 4, 8, 16, 32, 64, 128, 256, 512)
# FILTER names in the order filterVariants appends them (smCounter.py:187-266)
FILTER_NAMES = ((F_LM, "LM"), (F_LSM, "LSM"), (F_HP, "HP"), (F_LOWC, "LowC"), (F_DP, "DP"),
                (F_SB, "SB"), (F_LOWQ, "LowQ"), (F_R1CP, "R1CP"), (F_R2CP, "R2CP"),
                (F_PRIMERCP, "PrimerCP"))


class SmcParams(ctypes.Structure):
    _fields_ = [("min_bq", ctypes.c_int32), ("min_mq", ctypes.c_int32),
                ("mt_drop", ctypes.c_int32), ("primer_dist", ctypes.c_int32),
                ("ds", ctypes.c_int32), ("reserved", ctypes.c_int32), ("smt", ctypes.c_double),
                ("mismatch_thr", ctypes.c_double)]


class SmcBuildIn(ctypes.Structure):
    """smc_build_in (include/smcounter_hip.h): device pointers to a run's alignment arrays."""
    _fields_ = [("aln", ctypes.c_void_p), ("cig", ctypes.c_void_p), ("bq", ctypes.c_void_p),
                ("loc", ctypes.c_void_p), ("refseq", ctypes.c_void_p), ("start0", ctypes.c_int32), ("n_loci", ctypes.c_int32),
                ("n_bc", ctypes.c_int32), ("n_pair", ctypes.c_int32), ("max_depth", ctypes.c_int32), ("n_aln", ctypes.c_int32),
                ("loc_host", ctypes.c_void_p)]


DEV_ALN_DTYPE = np.dtype([("pos", "<i4"), ("end", "<i4"), ("cig_off", "<u4"), ("seq_off", "<u4"), ("n_cig", "<u2"),
                          ("oflag", "u1"), ("mapq", "u1"), ("left_sp", "<u2"), ("qalen", "<u2"), ("l_seq", "<u2"),
                          ("pad", "<u2"), ("bc_gid", "<u4"), ("pair_gid", "<u4")])
DEV_LOCUS_DTYPE = np.dtype([("w0", "<u4"), ("w1", "<u4"), ("slot_off", "<u4"), ("n", "<u4")])
assert DEV_ALN_DTYPE.itemsize == 36 and DEV_LOCUS_DTYPE.itemsize == 16
# smc_af_variant (smc_allele_carriers): a listed variant of a run
AF_VARIANT_DTYPE = np.dtype([("locus", "<u4"), ("kind", "<u4"), ("letter", "<u4"), ("len", "<u4"), ("ins_off", "<u4"), ("pad", "<u4", (3,))])
assert AF_VARIANT_DTYPE.itemsize == 32
# smc_spike_variant (smc_spike_alleles): a listed SNV by reference position, the records back to the leader of its phase set (0: its
# own leader), and its target's threshold
SPIKE_VARIANT_DTYPE = np.dtype([("pos0", "<i4"), ("ref", "u1"), ("alt", "u1"), ("lead", "<u2"), ("thr", "<u8")])
SPIKE_PHASE_MAX_MEMBERS = 8    # SMC_SPIKE_PHASE_MAX_MEMBERS
assert SPIKE_VARIANT_DTYPE.itemsize == 16
# smc_spike_indel_variant (smc_spike_indels): an SNV, an insertion or a deletion by the reference position of its base / anchor
SPIKE_INDEL_VARIANT_DTYPE = np.dtype([("pos0", "<i4"), ("kind", "u1"), ("ref", "u1"), ("alt", "u1"), ("pad", "u1"), ("len", "<u2"),
                                      ("lead", "<u2"), ("ins_off", "<u4"), ("thr", "<u8")])
assert SPIKE_INDEL_VARIANT_DTYPE.itemsize == 24
# smc_scan_locus / smc_scan_verdict (smc_scan_detect): a listed locus of a called batch, and what the kernel says of it per copy - the
# verdict in bits 30 - 31 of mt_verdict above the used MT
SCAN_LOCUS_DTYPE = np.dtype([("offset", "<u4"), ("alt", "<u4")])
SCAN_VERDICT_DTYPE = np.dtype([("pi", "<f8"), ("vmt", "<i4"), ("mt_verdict", "<u4")])
assert SCAN_LOCUS_DTYPE.itemsize == 8 and SCAN_VERDICT_DTYPE.itemsize == 16
SCAN_NOT, SCAN_CALLED, SCAN_HOST, SCAN_MT_MASK = 0, 1, 2, 0x3FFFFFFF
# (smc_scan_detect_sets) a joint word: the joint verdict in bits 31..30, the members CALLED / HOST / NOT by bit in bytes 0 / 1 / 2
SCAN_JOINT_CALLED_SHIFT, SCAN_JOINT_HOST_SHIFT, SCAN_JOINT_NOT_SHIFT = 0, 8, 16


def scan_joint_rule(verdicts, set_off):
    """smc_scan_detect_sets' joint rule in numpy.  verdicts: int [B, G], the member verdicts (SCAN_NOT / SCAN_CALLED / SCAN_HOST);
    set_off: [n_sets + 1], the sets' tiling of the G records -> (uint32 [B, n_sets]: the joint words, the indices c * G + g of the HOST
    members of the sets whose joint verdict is HOST, ascending)."""
    verdicts = np.asarray(verdicts, np.int64)
    B, G = verdicts.shape
    off = np.asarray(set_off, np.int64)
    words, listed = np.zeros((B, len(off) - 1), np.uint32), []
    for c in range(B):
        for s in range(len(off) - 1):
            w = 0
            for m, g in enumerate(range(int(off[s]), int(off[s + 1]))):
                v = int(verdicts[c, g])
                w |= 1 << (m + (SCAN_JOINT_CALLED_SHIFT if v == SCAN_CALLED else SCAN_JOINT_HOST_SHIFT if v == SCAN_HOST else SCAN_JOINT_NOT_SHIFT))
            jv = SCAN_NOT if w & 0xFF0000 else SCAN_HOST if w & 0xFF00 else SCAN_CALLED
            words[c, s] = (jv << 30) | w
            if jv == SCAN_HOST:
                listed += [c * G + g for g in range(int(off[s]), int(off[s + 1])) if int(verdicts[c, g]) == SCAN_HOST]
    return words, np.array(sorted(listed), np.uint32)


# (smc_scan_detect_keys) what d_alt_id holds where no extras entry of the copy shows the listed key / where the host has to look
SCAN_ID_NONE, SCAN_ID_HOST = 0xFFFFFFFF, 0xFFFFFFFE
# (smc_scan_filter) the four names only postfilter adds, behind the ten SMC_F_* bits; the 14 names of a FILTER column in the order of
# their bits; the bit that leaves a row's FILTER to the host
F_REPT, F_REPS, F_SL, F_OTHER_REPEAT = 0x400, 0x800, 0x1000, 0x2000
SCAN_FILTER_NAMES = FILTER_NAMES + ((F_REPT, "RepT"), (F_REPS, "RepS"), (F_SL, "SL"), (F_OTHER_REPEAT, "Other_Repeat"))
SCAN_FLT_DEVICE_MASK, SCAN_FLT_NAMES_MASK, SCAN_FLT_HOST = 0x3FF, 0x3FFF, 0x80000000
# (smc_scan_filter_sets) a joint FILTER word: the OR of the members' name bits, bit 16 + m where member m is not PASS, bit 31 where a
# member's word has it
SCAN_FLT_MEMBER_SHIFT = 16


def scan_filter_joint_rule(member_words, set_off):
    """smc_scan_filter_sets' joint rule in numpy.  member_words: uint32 [B, G], smc_scan_filter's words of the members; set_off:
    [n_sets + 1], the sets' tiling of the G members -> uint32 [B, n_sets]: the joint words."""
    member_words = np.asarray(member_words, np.uint32)
    B, G = member_words.shape
    off = np.asarray(set_off, np.int64)
    words = np.zeros((B, len(off) - 1), np.uint32)
    for c in range(B):
        for s in range(len(off) - 1):
            w = 0
            for m, g in enumerate(range(int(off[s]), int(off[s + 1]))):
                mw = int(member_words[c, g])
                w |= mw & (SCAN_FLT_NAMES_MASK | SCAN_FLT_HOST)
                if mw & SCAN_FLT_NAMES_MASK:
                    w |= 1 << (SCAN_FLT_MEMBER_SHIFT + m)
            words[c, s] = w
    return words


SPIKE_DRAW_DOMAIN, READ_DRAW_DOMAIN = 0x73704146, 0x64735250      # counter word 2 of the spike draw ("spAF") and of the read draw ("dsRP")


def philox_word0(idents, domain: int, word3: int, seed: int) -> np.ndarray:
    """Word 0 of Philox4x32-10(counter = (ident lo, ident hi, domain, word3), key = (seed lo, seed hi)) per identity, in numpy."""
    idents = np.asarray(idents, np.uint64)
    m32, n = np.uint64(0xFFFFFFFF), len(idents)
    c = [idents & m32, idents >> np.uint64(32), np.full(n, int(domain), np.uint64), np.full(n, int(word3) & 0xFFFFFFFF, np.uint64)]
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    k0, k1 = seed & 0xFFFFFFFF, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m32]
        k0, k1 = (k0 + 0x9E3779B9) & 0xFFFFFFFF, (k1 + 0xBB67AE85) & 0xFFFFFFFF
    return c[0].astype(np.uint64)


def scan_phase_rpb_counts_rule(bm_aln, bm_name, bm_first, bc_start, idents, bits, row_off, row_var, joint_off, joint_gid, pos1, seeds, thr,
                               read_thr, detail: list = None) -> np.ndarray:
    """smc_scan_phase_rpb_counts in numpy, on the entry's own arrays -> uint32 [rows, R, T, Rr, 4] = (N_ALL', V0_ALL', S_ALL', V1_ALL').
    bm_aln, bm_name, bm_first, bc_start: the run in barcode-major order; idents: the barcodes' identities; bits: uint8 [n_var, n_aln],
    smc_spike_read_bits' bytes; row_off over row_var: a row's members (indices of bit rows); joint_off over joint_gid: a row's joint
    barcodes (run-wide ids); pos1: the rows' draw positions; seeds, thr, read_thr: the replicates' seeds and the thresholds of both axes.
    detail: a list that gets, per row, int64 [R, n joint barcodes, M, Rr, 3] = (reads, alt0, alt1) of every barcode at every member
    over the records kept at r - what the verdicts are made of."""
    bm_aln, bm_name = np.asarray(bm_aln, np.int64), np.asarray(bm_name, np.uint64)
    bm_first, bc_start = np.asarray(bm_first, np.uint8) != 0, np.asarray(bc_start, np.int64)
    idents, bits = np.asarray(idents, np.uint64), np.asarray(bits, np.uint8)
    n_aln, n_bc = len(bm_aln), len(idents)
    bits = bits.reshape(-1, n_aln) if n_aln else bits.reshape(len(bits), 0)
    row_off, joint_off = np.asarray(row_off, np.int64), np.asarray(joint_off, np.int64)
    row_var, joint_gid = np.asarray(row_var, np.int64), np.asarray(joint_gid, np.int64)
    rthr = np.array([int(q) for q in read_thr], np.uint64)
    n_rows, R, T, Rr = len(row_off) - 1, len(seeds), len(thr), len(rthr)
    out = np.zeros((n_rows, R, T, Rr, 4), np.uint32)
    for g in range(n_rows):
        gids = joint_gid[joint_off[g]:joint_off[g + 1]]
        members = row_var[row_off[g]:row_off[g + 1]]
        n, M = len(gids), len(members)
        ok = gids < n_bc                                            # (an id that is not below n_bc reads nothing)
        safe = np.where(ok, gids, 0)
        ids = np.where(ok, idents[safe] if n_bc else 0, 0).astype(np.uint64)
        r0 = np.where(ok, np.minimum(bc_start[safe], n_aln), 0)
        r1 = np.where(ok, np.minimum(bc_start[safe + 1], n_aln), 0) if n_bc else r0
        length = np.maximum(r1 - r0, 0)
        lane = np.repeat(np.arange(n), length)                      # every record of every joint barcode, barcode after barcode
        k = np.repeat(r0 - (np.cumsum(length) - length), length) + np.arange(int(length.sum()))
        a = bm_aln[k]
        inside = a < n_aln
        lane, k, a = lane[inside], k[inside], a[inside]
        cnt = np.zeros((R, n, M, Rr, 3), np.int64)
        for j, s in enumerate(seeds):
            kept = bm_first[k][:, None] | (philox_word0(bm_name[k], READ_DRAW_DOMAIN, 0, s)[:, None] < rthr[None, :])       # [records, Rr]
            for m, v in enumerate(members):
                byte = bits[v][a]
                mine = (byte & 1) != 0
                for q, bit in enumerate((1, 2, 4)):
                    w = kept[mine] & ((byte[mine] & bit) != 0)[:, None]
                    np.add.at(cnt[j, :, m, :, q], lane[mine], w.astype(np.int64))
            c = cnt[j]
            there = (c[..., 0] > 0).all(axis=1)                     # [n, Rr]
            car0 = (2 * c[..., 1] > c[..., 0]).all(axis=1)
            car1 = (2 * c[..., 2] > c[..., 0]).all(axis=1)
            u = philox_word0(ids, SPIKE_DRAW_DOMAIN, int(pos1[g]), s)
            for t, h in enumerate(thr):
                hit = (u < np.uint64(int(h)))[:, None]
                out[g, j, t, :, 0] = there.sum(axis=0)
                out[g, j, t, :, 1] = (there & car0).sum(axis=0)
                out[g, j, t, :, 2] = (there & hit).sum(axis=0)
                out[g, j, t, :, 3] = (there & np.where(hit, car1, car0)).sum(axis=0)
        if detail is not None:
            detail.append(cnt)
    return out


def c_params(p: VcParams) -> SmcParams:
    return SmcParams(p.minBQ, p.minMQ, p.mtDrop, p.primerDist, p.ds, 0, p.smt, float(p.mismatchThr))


CAND_DTYPE = np.dtype([
    ("allele", "<i4"), ("flt_applied", "<i4"), ("flt", "<u4"), ("vmf_lt_099", "<i4"),
    ("vdp", "<i4"), ("vmt", "<i4"), ("vsm", "<i4"), ("pad", "<i4"),
    ("tal", "<i4", (SMC_NT,)), ("pi", "<f8"),
    ("p_sb", "<f8"), ("p_r1", "<f8"), ("p_r2", "<f8"), ("p_pr", "<f8")])
assert CAND_DTYPE.itemsize == 120

ROW_DTYPE = np.dtype([
    ("status", "<i4"), ("n_touched", "<i4"),
    ("cvg", "<i4"), ("all_frag", "<i4"), ("all_mt", "<i4"), ("used_frag", "<i4"), ("used_mt", "<i4"),
    ("mt3", "<i4"), ("mt5", "<i4"), ("mt7", "<i4"), ("mt10", "<i4"),
    ("max_allele", "<i4"), ("second_allele", "<i4"), ("biallelic", "<i4"),
    ("dp", "<i4", (4,)), ("umt", "<i4", (4,)), ("vsm", "<i4", (4,)),
    ("pi", "<f8", (4,)), ("touched_mask", "<u8"),
    ("ref_tal", "<i4", (SMC_NT,)), ("cand", CAND_DTYPE, (2,))])
assert ROW_DTYPE.itemsize == 432

# smc_wire_row: the printed part of a row, what the multi-GPU gather moves (include/smcounter_hip.h)
WIRE_CAND_DTYPE = np.dtype([("allele", "<i2"), ("flags", "<u2"), ("vdp", "<i4"), ("vmt", "<i4"), ("vsm", "<i4"), ("pi", "<f8")])
WIRE_DTYPE = np.dtype([("status", "<u4"), ("cvg", "<i4"), ("all_frag", "<i4"), ("all_mt", "<i4"), ("used_frag", "<i4"),
                       ("used_mt", "<i4"), ("mt3", "<i4"), ("mt5", "<i4"), ("mt7", "<i4"), ("mt10", "<i4"),
                       ("dp", "<i4", (4,)), ("umt", "<i4", (4,)), ("vsm", "<i4", (4,)), ("pi", "<f8", (4,)),
                       ("cand", WIRE_CAND_DTYPE, (2,))])
assert WIRE_CAND_DTYPE.itemsize == 24 and WIRE_DTYPE.itemsize == 168
WIRE_BIALLELIC, WIRE_FLT_MASK, WIRE_FLT_APPLIED, WIRE_VMF_LT_099 = 0x10000, 0x3FF, 0x400, 0x800


def pack_wire(rows: np.ndarray) -> np.ndarray:
    """numpy mirror of the device's k_pack_rows (csrc/k_pack_rows.inc): ROW_DTYPE -> WIRE_DTYPE.  The GPU test checks
    the kernel against it byte for byte; the CPU (gloo) tests use it in place of the kernel."""
    w = np.zeros(len(rows), WIRE_DTYPE)
    w["status"] = (rows["status"].astype(np.uint32) & 0xFFFF) | np.where(rows["biallelic"] != 0, WIRE_BIALLELIC, 0).astype(np.uint32)
    for f in ("cvg", "all_frag", "all_mt", "used_frag", "used_mt", "mt3", "mt5", "mt7", "mt10", "dp", "umt", "vsm", "pi"):
        w[f] = rows[f]
    c, wc = rows["cand"], w["cand"]
    wc["allele"] = c["allele"].astype(np.int16)
    wc["flags"] = ((c["flt"] & WIRE_FLT_MASK) | np.where(c["flt_applied"] != 0, WIRE_FLT_APPLIED, 0)
                   | np.where(c["vmf_lt_099"] != 0, WIRE_VMF_LT_099, 0)).astype(np.uint16)
    for f in ("vdp", "vmt", "vsm", "pi"):
        wc[f] = c[f]
    return w


def unpack_wire(wire: np.ndarray) -> np.ndarray:
    """WIRE_DTYPE -> ROW_DTYPE through the library's smc_unpack_rows (host code, no GPU): every printed field restored,
    the rest zero / NaN.  rows.format_rows prints the same strings from the result as from the original rows."""
    from . import _lib
    wire = np.ascontiguousarray(wire)
    assert wire.dtype.itemsize == WIRE_DTYPE.itemsize
    out = np.zeros(len(wire), ROW_DTYPE)
    _lib.check(_lib.load().smc_unpack_rows(wire.ctypes.data, len(wire), out.ctypes.data), "smc_unpack_rows")
    return out


INT_FIELDS = ("status", "n_touched", "cvg", "all_frag", "all_mt", "used_frag", "used_mt", "mt3", "mt5",
              "mt7", "mt10", "max_allele", "second_allele", "biallelic", "dp", "umt", "vsm",
              "touched_mask", "ref_tal")
CAND_INT_FIELDS = ("allele", "flt_applied", "flt", "vmf_lt_099", "vdp", "vmt", "vsm", "tal")
CAND_F64_FIELDS = ("pi", "p_sb", "p_r1", "p_r2", "p_pr")


def _pi_of(row, allele):
    """PI of an allele if the row carries it (A,T,G,C and the candidates), else None."""
    if 0 <= allele < 4:
        return float(row["pi"][allele])
    for c in row["cand"]:
        if int(c["allele"]) == allele:
            return float(c["pi"])
    return None


def near_tie_loci(a: np.ndarray, b: np.ndarray, eps=1e-9, pi_all=None):
    """Loci where the two implementations pick maxBase / secondMaxBase differently although the
    prediction indices of the alleles they disagree on are equal to within floating-point summation
    order (|dPI| <= eps): the reference's own choice there depends on the order its dict iterates
    barcodes (smCounter.py:506, :534), so it is not pinned.  `pi_all` ([n_loci, 64], the CPU restatement's PI of
    every allele key) settles alleles the rows do not carry (a non-candidate indel key)."""
    out = set()
    d = np.nonzero((a["max_allele"] != b["max_allele"]) | (a["second_allele"] != b["second_allele"]))[0]
    for i in d:
        ok = True
        for f in ("max_allele", "second_allele"):
            x, y = int(a[f][i]), int(b[f][i])
            if x == y:
                continue
            px, py = _pi_of(a[i], x), _pi_of(a[i], y)
            if px is None:
                px = _pi_of(b[i], x)
            if py is None:
                py = _pi_of(b[i], y)
            if pi_all is not None:
                if px is None and 0 <= x < 64 and pi_all[i][x] == pi_all[i][x]:
                    px = float(pi_all[i][x])
                if py is None and 0 <= y < 64 and pi_all[i][y] == pi_all[i][y]:
                    py = float(pi_all[i][y])
            if px is None or py is None or abs(px - py) > eps * max(1.0, abs(px)):
                ok = False
        if ok:
            out.add(int(i))
    return out


def compare_rows(a: np.ndarray, b: np.ndarray, pi_tol=1e-6, p_tol=1e-6, fragile=None, pi_all=None):
    """Field-wise comparison of two row arrays: integer fields bit-exact, PI and Fisher p-values
    within tolerance.  Returns a list of human-readable mismatches (empty = equal).

    Two kinds of loci are unpinned by the reference algorithm itself and skipped for the fields
    they affect: `near_tie_loci` (order of two PI-tied alleles) and loci where `fragile[l] > 0`
    (oracle/smc_oracle.c: a barcode whose unique-maximum test hinges on rounding)."""
    bad = []
    assert a.shape == b.shape
    # SMC_ST_UNDERFLOW on either side: a barcode whose calProb products left the normal double range - the reference's own
    # numbers there are denormal rounding in its multiplication order.  Such loci are compared on the fields that do not come
    # out of calProb (the read / fragment / barcode counts) and excused on the rest, like the ties below.
    under = ((a["status"] | b["status"]) & ST_UNDERFLOW) != 0
    if under.any():
        a, b = a.copy(), b.copy()
        for r in (a, b):
            r["status"] &= ~np.int32(ST_UNDERFLOW)
        for f in ("pi", "umt", "vsm", "max_allele", "second_allele", "biallelic", "n_touched", "touched_mask", "cand", "ref_tal"):
            a[f][under] = b[f][under]
    ties = near_tie_loci(a, b, pi_all=pi_all)
    keep = np.ones(len(a), bool)
    keep[list(ties)] = False
    firm = np.ones(len(a), bool) if fragile is None else (np.asarray(fragile) == 0)
    order_dep = ("max_allele", "second_allele", "biallelic")
    mt_dep = ("umt", "vsm", "max_allele", "second_allele", "biallelic")
    fr = np.zeros(len(a), np.int64) if fragile is None else np.asarray(fragile, np.int64)
    # The tallies that only filterVariants reads (SMC_T_FWD .. SMC_T_R2PRLE, words 1-8) are part of a row where a candidate
    # goes through the filters (flt_applied); elsewhere a producer may leave them out (the GPU path does, the CPU restatement
    # fills them always).  alleleCnt is compared everywhere; the pair counts (words 9, 10: concordPairCnt / discordPairCnt)
    # everywhere for the candidates - the DP filter reads the candidate's (:207) - and nowhere for the reference allele,
    # whose pair counts nothing ever reads.
    filt_words = np.zeros(a["ref_tal"].shape[1], bool)
    filt_words[1:9] = True
    ref_dead = np.zeros(a["ref_tal"].shape[1], bool)
    ref_dead[9:11] = True
    applied = (a["cand"]["flt_applied"] != 0) & (b["cand"]["flt_applied"] != 0)            # [n, 2]
    any_applied = applied.any(axis=1)
    for f in INT_FIELDS:
        if f == "ref_tal":
            ne = ((a[f] != b[f]) & ~ref_dead[None, :] & (~filt_words[None, :] | any_applied[:, None])).any(axis=1)
        else:
            ne = (a[f] != b[f]).reshape(len(a), -1).any(axis=1)
        if f in order_dep:
            ne &= keep
        if f in ("umt", "vsm"):
            # a fragile barcode moves at most one count
            d = np.abs(a[f].astype(np.int64) - b[f].astype(np.int64)).sum(axis=1)
            ne &= d > 2 * fr
        elif f in mt_dep:
            ne &= firm
        for i in np.nonzero(ne)[0][:5]:
            bad.append("locus %d: %s %r != %r" % (i, f, a[f][i].tolist(), b[f][i].tolist()))
    ok = (a["status"] & 0xff) == ST_OK
    d = np.abs(a["pi"] - b["pi"])[ok]
    if d.size and d.max() > pi_tol:
        bad.append("pi max-abs-diff %g > %g" % (d.max(), pi_tol))
    keep &= firm
    for f in CAND_INT_FIELDS:
        if f == "tal":
            ne = ((a["cand"][f] != b["cand"][f]) & (~filt_words[None, None, :] | applied[:, :, None])).reshape(len(a), -1).any(axis=1) & keep
        else:
            ne = (a["cand"][f] != b["cand"][f]).reshape(len(a), -1).any(axis=1) & keep
        for i in np.nonzero(ne)[0][:5]:
            bad.append("locus %d: cand.%s %r != %r" % (i, f, a["cand"][f][i].tolist(),
                                                        b["cand"][f][i].tolist()))
    for f in CAND_F64_FIELDS:
        x, y = a["cand"][f][keep], b["cand"][f][keep]
        nan_mismatch = np.isnan(x) != np.isnan(y)
        if nan_mismatch.any():
            bad.append("cand.%s NaN pattern differs at %d loci" % (f, int(nan_mismatch.any(axis=1).sum())))
        tol = pi_tol if f == "pi" else p_tol
        dd = np.abs(np.where(np.isnan(x) | np.isnan(y), 0.0, x - y))
        if dd.size and dd.max() > tol:
            bad.append("cand.%s max-abs-diff %g > %g" % (f, dd.max(), tol))
    return bad


def parity_report(a: np.ndarray, b: np.ndarray, fragile=None, pi_all=None, pi_tol=1e-6, p_tol=1e-6) -> dict:
    """compare_rows plus its denominators: how many loci were compared, how many had candidate / consensus fields
    excused because the reference's own result is order-dependent there (`fragile`: a barcode whose unique-maximum
    test hinges on rounding, smCounter.py:514; `near_tie`: two alleles whose PI differ only by summation order,
    :534), and the largest PI difference seen.  "0 mismatches" means nothing without these."""
    bad = compare_rows(a, b, pi_tol, p_tol, fragile, pi_all)
    ok = ((a["status"] & 0xff) == ST_OK) & ((b["status"] & 0xff) == ST_OK)
    d = np.abs(a["pi"] - b["pi"])[ok]
    # the p-value half of the metric: how many loci reached filterVariants, how many Fisher tests ran there (a p-value that is
    # not NaN in the CPU restatement's row), and the largest difference between the two implementations' p-values
    p_max, n_tests = 0.0, 0
    for f in ("p_sb", "p_r1", "p_r2", "p_pr"):
        x, y = a["cand"][f], b["cand"][f]
        both = ~np.isnan(x) & ~np.isnan(y)
        n_tests += int((~np.isnan(y)).sum())
        if both.any():
            p_max = max(p_max, float(np.abs(x[both] - y[both]).max()))
    return {"loci": int(len(a)), "mismatches": len(bad),
            "fragile_skipped": 0 if fragile is None else int((np.asarray(fragile) > 0).sum()),
            "near_tie_skipped": len(near_tie_loci(a, b, pi_all=pi_all)),
            "pi_max_abs_diff": float(d.max()) if d.size else 0.0,
            "underflow_skipped": int((((a["status"] | b["status"]) & ST_UNDERFLOW) != 0).sum()),
            "loci_filtered": int((b["cand"]["flt_applied"] != 0).any(axis=1).sum()),
            "fisher_tests_run": n_tests, "p_max_abs_diff": p_max, "detail": bad[:3]}
