"""Device-resident batches: BAM -> alignments (host decode) -> planes built ON THE GPU (smc_build_planes) -> hot path.

The per-pileup-read half of the reference's feature extraction and barcode bookkeeping (smCounter.py:316-366, :371-452,
:462-471) runs in csrc/k_build_planes.inc; the host keeps the per-alignment half (csrc/smc_bam.cpp: smc_bam_alignments)
and whatever needs strings: the texts of indel alleles, the reference's down-sampling on barcode texts (:496-498, py2
semantics).  A run the device path does not take (a locus deeper than smc_build_max_depth(), an alignment with neither
READ1 nor READ2, an overflow the kernel reports) is built by the host builder (smc_bam_planes) and uploaded into the same
device arrays - the same batch either way up to the numbering of barcodes and fragments within a locus, which the layout
contract leaves to the builder (planecheck.py; tests/test_gpu_devplanes.py compares them).
"""
from __future__ import annotations

import ctypes
import dataclasses
import functools
import os
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib, abi, bamio
from .features import LF_SAMPLED, LOCUS_DTYPE, USTART_DROPPED
from .pileup import BASE_ALLELES

_BASE_TABLE = list(BASE_ALLELES)           # the allele table of a locus that met only the six fixed keys (shared: read-only)


_TIMES = {"decode": 0.0, "upload+launch": 0.0, "kernel (sync)": 0.0}      # SMC_DEVPLANES_TIMING=1: seconds per stage


@dataclasses.dataclass
class ResidentBatch:
    """A batch whose planes live in HBM (engine.DevBuf allocations: no PyTorch in this path); the descriptors and what row
    formatting needs are on the host."""
    planes: list               # [meta, umi, frag, dist, umi_start] device buffers (`data_ptr()`), uint32 words; the four
                               # raw-field planes are None when the batch was built with all_planes=False
    loci: np.ndarray           # LOCUS_DTYPE[n_loci] (host copy; offsets are batch-relative)
    chrom: List[str]
    pos: np.ndarray
    ref: List[str]
    alleles: List[List[str]]
    n_device_runs: int = 0     # runs built by k_build_planes / by the host builder (fallback)
    n_host_runs: int = 0
    n_slots: int = 0
    n_ustart: int = 0
    words: object = None       # the read words (one per read: what the locus kernels read), device buffer; 32 bits each, or 16
                               # (include/smcounter_hip.h: smc_read_word16) when its `word_bits` says so

    @property
    def n_loci(self) -> int:
        return len(self.loci)

    def to_host(self):
        """-> features.DeviceBatch with the planes copied back (tests, the CPU restatement)."""
        from .features import DeviceBatch
        m, u, f, d = (t.download(np.uint32, self.n_slots) for t in self.planes[:4])
        us = self.planes[4].download(np.uint32, self.n_ustart)
        return DeviceBatch(loci=self.loci.copy(), meta=m, umi=u, frag=f, dist=d, umi_start=us, chrom=list(self.chrom),
                           pos=self.pos.copy(), ref=list(self.ref), alleles=[list(t) for t in self.alleles])


FIRST_RUN_WHOLE_BYTES = 48 << 20   # ... unless the whole stretch (up to 65536 loci) is no more than this in the file
FIRST_RUN_LOCI = 64            # loci of a file's first run (iter_resident_batches): enough to learn the depth from
BUILD_ST_NARROW = 32           # smc_build_planes_w16's status bit: the run has no room in 16-bit read words
NARROW = "narrow"              # what build_run answers then


def class16_table() -> np.ndarray:
    """smc_read_class's number -> smc_class16's code (included << 4 | index), 31 where there is no class (include/smcounter_hip.h)."""
    t = np.full(32, 31, np.uint32)
    for c in range(22):
        if c < 2:
            t[c] = (c & 1) << 4
        elif c < 6:
            t[c] = ((c & 1) << 4) | (1 + ((c - 2) >> 1))
        else:
            rev, sub = (c - 6) >> 3, (c - 6) & 7
            t[c] = 3 + 2 * rev + sub if sub < 2 else 16 | (3 + 6 * rev + (sub - 2))
    return t


def words16_from_32(w: np.ndarray):
    """32-bit read words -> 16-bit ones (smc_read_word16), or None when one of them has no room: an allele id beyond 15, a
    quality beyond 63, a class that is none (a word of zero - the pad behind a locus's last read - stays zero)."""
    w = np.asarray(w, np.uint32)
    cls = w >> np.uint32(27)
    c16 = class16_table()[cls]
    real = w != 0
    if bool(((((w & np.uint32(0xFF)) > 15) | (((w >> np.uint32(8)) & np.uint32(0xFF)) > 63) | (c16 == 31)) & real).any()):
        return None
    h = (w & np.uint32(15)) | ((w >> np.uint32(16)) & np.uint32(1)) << np.uint32(4) | ((c16 >> np.uint32(4)) & np.uint32(1)) << np.uint32(5) | \
        (c16 & np.uint32(3)) << np.uint32(6) | ((w >> np.uint32(8)) & np.uint32(63)) << np.uint32(8) | ((c16 >> np.uint32(2)) & np.uint32(3)) << np.uint32(14)
    return np.where(real, h, 0).astype(np.uint16)


def words32_from_16(h: np.ndarray) -> np.ndarray:
    """... and back (smc_read_word32): what tests compare with the host-built words."""
    h = np.asarray(h, np.uint16).astype(np.uint32)
    inv = np.full(32, 31, np.uint32)
    t = class16_table()
    for c in range(22):
        inv[t[c]] = c
    c16 = ((h >> np.uint32(5)) & np.uint32(1)) << np.uint32(4) | ((h >> np.uint32(6)) & np.uint32(3)) | ((h >> np.uint32(14)) & np.uint32(3)) << np.uint32(2)
    cls = inv[c16]
    inc = np.where(cls < 6, cls & 1, ((cls - 6) & 7) >= 2).astype(np.uint32)
    w = (h & np.uint32(15)) | ((h >> np.uint32(8)) & np.uint32(63)) << np.uint32(8) | ((h >> np.uint32(4)) & np.uint32(1)) << np.uint32(16) | \
        inc << np.uint32(17) | np.uint32(1 << 18) | cls << np.uint32(27)
    return np.where(h != 0, w, 0).astype(np.uint32)


def pack_words_host(meta: np.ndarray, frag: np.ndarray, loci: np.ndarray) -> np.ndarray:
    """The read words (include/smcounter_hip.h: smc_read_word) of a host-built batch, as smc_pack_words makes them on the device:
    allele and quality from the meta word, the class from the frag word, "first read of its fragment" from the slots."""
    from .features import FRAG_SLOT_MASK, FRAG_CLASS_SHIFT
    ns = len(meta)
    slot = frag & np.uint32(FRAG_SLOT_MASK)
    nf = np.ones(ns, bool)
    nf[1:] = slot[1:] != slot[:-1]
    start = 4 * loci["read_off4"].astype(np.int64)
    n = loci["n_reads"].astype(np.int64)
    nf[start[n > 0]] = True
    d = np.zeros(ns + 1, np.int64)
    np.add.at(d, start, 1)
    np.add.at(d, start + n, -1)
    valid = np.cumsum(d[:-1]) > 0
    cls = frag >> np.uint32(FRAG_CLASS_SHIFT)
    # the slot contract, checked as k_pack_words.inc checks it: within a locus the slots start at 0, step by 0 or 1 and end at
    # n_frag - 1; a read that breaks it gets class 31 (no read class), which the kernels answer with SMC_ST_BAD_INPUT
    prev = np.empty(ns, np.uint32)
    prev[1:] = slot[:-1]
    prev[:1] = 0
    prev[start[n > 0]] = np.uint32(0xFFFFFFFF)
    step = slot - prev
    bad = step > np.uint32(1)
    last = (start + n - 1)[n > 0]
    bad[last] |= slot[last] != (loci["n_frag"][n > 0].astype(np.int64) - 1).astype(np.uint32)
    nf = step != 0
    cls = np.where(bad, np.uint32(31), cls)
    # bits 17 / 18: the read is included / its class is a known one (include/smcounter_hip.h: smc_class_bits)
    c = np.arange(32)
    inc = np.where(c < 6, c & 1, ((c - 6) & 7) >= 2).astype(np.uint32)
    bits = np.where(c < 22, (np.uint32(4) | inc << np.uint32(1)), np.uint32(0)).astype(np.uint32) << np.uint32(16)
    w = (meta & np.uint32(0xFFFF)) | (nf.astype(np.uint32) << np.uint32(16)) | bits[cls] | (cls << np.uint32(27))
    return np.where(valid, w, np.uint32(0)).astype(np.uint32)


READS_PER_BYTE = 6        # pileup reads a batch is sized for per compressed byte of the file under its targets (typical: ~ 2.5)


def iter_resident_batches(path: str, fasta, loci: Sequence[Tuple[str, str]], params, eng, max_reads: int = 128_000_000,
                          nthreads: int = 0, force_host: bool = False, all_planes: bool = True, sampler: str = "reference",
                          sampler_seed: int = 0, ds_rules: Sequence[DsRule] = None, close_tables: bool = True):
    """BAM -> `ResidentBatch` chunks: same loci per chunk as bamio.iter_device_batches_native, planes built on the GPU.
    `ds_rules` (--dsMT): every run is decoded and uploaded once and built K + 1 times - at full depth and, through
    smc_select_alignments, for the kept barcodes of every rule (called with that rule's params); each item is then
    (first, [full-depth batch, batch of rule 1, ...]), all of the same loci.  Every run must be one the device builder takes.
    (--dsRpb: a rule of level "read" keeps read names, by the run's read-name ids - smc_select_alignments_keyed; the same batches.)
    `all_planes=False`: only what the locus kernels read - the read words and umi_start - is built and kept (a fifth of the
    device memory of a batch, a quarter of the builder's stores); the four raw-field planes (for checks) are then None.
    (Round 5 built and measured decoding run i + 1 on a helper thread - a second decoder handle, the streaming cursor handed
    over - beside the upload, build and call of run i: at the example run's depth a run is 14 ms of decoding against 4 ms of
    everything else, the helper's decodes were 30 % slower than the main thread's and its exit cost 40 ms per file: 13 k loci/s
    against 22-24 k without.  Taken out again; what stayed is the sizing of the runs below.)"""
    from .engine import DevBuf
    L = eng.L
    bam = bamio.NativeBam(path)
    nthreads = nthreads or bamio.host_threads()
    max_depth = L.smc_build_max_depth()
    cp = abi.c_params(params)
    i, n = 0, len(loci)
    # last locus of the stretch of consecutive positions (same chromosome) every locus lies in
    if n:
        pos_all = np.array([p for _, p in loci]).astype(np.int64)
        chrom_all = [c for c, _ in loci]
        brk = pos_all[1:] != pos_all[:-1] + 1
        if chrom_all.count(chrom_all[0]) != n:
            brk |= np.array([chrom_all[k] != chrom_all[k + 1] for k in range(n - 1)], bool)
        ends = np.append(np.flatnonzero(brk), n - 1)
        stretch_end = ends[np.searchsorted(ends, np.arange(n))]
    # The device arrays of a batch are sized for max_reads - but not for more than the FILE can hold (a 2 MB BAM made every
    # batch allocate three 576 MB barcode arrays and a read-word block large enough to send the library through its search among
    # twelve allocations).  The linear index says how many compressed bytes lie under the target stretches; a batch takes at most
    # READS_PER_BYTE pileup reads per byte of them (a 150-base read is 60-100 compressed bytes and at most 150 pileup reads; an estimate
    # that is too low only ends batches earlier - the decoder is handed `max_reads - total` and stops there).
    if n and not _lib.exp_env("SMC_NO_FILE_SIZED_BATCH"):
        try:
            nb, seen = 0, set()
            for e in np.unique(stretch_end).tolist():
                b = int(np.searchsorted(stretch_end, e, side="left"))
                k = bam.span_bytes(chrom_all[b], int(pos_all[b]) - 1, int(pos_all[e]))
                if k < 0:
                    nb = -1
                    break
                nb += int(k)
            if nb >= 0:
                max_reads = int(min(max_reads, max(4_000_000, READS_PER_BYTE * nb)))
        except Exception:
            pass
    cap = max_reads + (max_reads >> 3) + 65536
    per_locus = 0.0          # pileup reads per locus of the previous run: sizes the next run (a run is decoded as a whole)

    def span_of(i, total, per_locus, first):
        """The run that starts at locus i of a batch that holds `total` reads so far: (chrom, lo, hi, reads it may take)."""
        chrom = loci[i][0]
        # (the decoder inflates everything up to the run's end: a run much longer than what max_reads lets through
        # would be decoded again by the next one)
        # (the floor was 1024 loci and the factor 1.15 until round 5: at the example run's 58,000x a batch's first run took 550
        # loci, its second was asked for 1024 - half a 2000-locus file inflated and parsed - to take the 51 the batch still had room for)
        span_cap = 65536 if per_locus <= 0 else int(max(64, min(65536, 1.02 * (max_reads - total) / per_locus)))
        if per_locus <= 0 and i == first:
            # nothing decoded yet: a short first run tells the depth, the runs after it are sized by it.  (Until round 5 the first
            # run was sized from the compressed bytes the linear index gives for the stretch, at 2.5 pileup reads per
            # byte: on the 58,000x fixture that asked for all 2000 loci - 40 ms of decoding - to keep the 550 a batch has room for.)
            # A stretch whose compressed bytes are few (the linear index knows) is taken whole: decoding all of it costs less than a
            # run of its own for the first loci would.
            span_cap = FIRST_RUN_LOCI
            jj = min(int(stretch_end[i]), i + 65536 - 1)
            nb = bam.span_bytes(chrom, int(pos_all[i]) - 1, int(pos_all[jj]))
            if 0 <= nb < FIRST_RUN_WHOLE_BYTES:
                span_cap = 65536
            if _lib.exp_env("SMC_FIRST_RUN_8192"):                                             # (the switch: measurement)
                span_cap = 8192
        j = min(int(stretch_end[i]), i + span_cap - 1)
        return chrom, int(pos_all[i]) - 1, int(pos_all[j]), max_reads - total

    import time
    try:
        while i < n:
            first = i
            planes = [DevBuf(eng, 4 * cap) if all_planes else None for k in range(4)]
            # 16-bit read words where nothing but the words is kept, until a run has no room in them (an allele id beyond 15, a
            # quality beyond 63): that batch is then built again, and the rest of the file, with 32-bit words
            bits = 16 if (not all_planes and eng.word_bits == 16 and 0 <= params.minBQ <= 63) else 32
            words = DevBuf(eng, (bits // 8) * cap, walk_output=True)      # (a large one is chosen by the write-pattern probe: engine.DevBuf)
            words.word_bits = bits
            narrow = False
            uaux = [DevBuf(eng, 4 * (cap + 8192)) for _ in range(3)]      # umi_start, u_gid, u_finc
            # (--dsMT: the same arrays for every rule - a rule's run holds at most the full run's reads)
            ds = [_DsBatch(eng, cap, bits, all_planes) for _ in (ds_rules or ())]
            LC, chroms, poss, refs, tables = [], [], [], [], []
            total = slots = n_loc = 0
            n_dev = n_host = 0
            while i < n and total < max_reads:
                key = span_of(i, total, per_locus, first)
                chrom, lo, hi = key[0], key[1], key[2]
                run_ref = fasta.fetch(chrom, lo, hi).upper()
                umi_base = slots + n_loc
                done = None
                if ds_rules and force_host:
                    raise bamio.BamError(_ds_refused(chrom, lo, hi, "the planes are built on the host", _ds_flag(ds_rules)))
                if not force_host:
                    T = _TIMES if os.environ.get("SMC_DEVPLANES_TIMING") else None
                    t0 = time.perf_counter()
                    A = bam.alignments_run(chrom, lo, hi, key[3], params, nthreads, host_array=eng.pinned)
                    if T is not None:
                        T["decode"] += time.perf_counter() - t0
                    up = upload_run(eng, A, run_ref) if ds_rules and A["nl"] else None
                    done = build_run(A, L, eng, cp, params, chrom, lo, fasta, run_ref, [words] + planes, uaux, slots, umi_base, cap, max_depth,
                                     bam.allele_key, bam.barcode_name, sampler=sampler, sampler_seed=sampler_seed,
                                     barcode_idents=bam.barcode_idents, uploaded=up)
                    if ds_rules and done is None:
                        raise bamio.BamError(_ds_refused(chrom, lo, hi, "the device builder does not take it", _ds_flag(ds_rules)))
                    if ds_rules and done != NARROW:
                        narrow = not _ds_build_run(ds_rules, ds, A, up, eng, chrom, lo, fasta, run_ref, cap, max_depth, bam, sampler,
                                                   sampler_seed, n_loc)
                    if up is not None:
                        up.free()
                    if done == NARROW or narrow:
                        narrow = True
                        break
                if done is None:
                    # host builder (the run is not one the device path takes): same planes, uploaded
                    nl, hp, ustart, lc, tb = bam.planes_run(chrom, lo, hi, max_reads - total, params, run_ref, nthreads, fasta)
                    if sampler == "philox" and params.ds > 0 and bool((lc["n_umi"] > params.ds).any()):
                        import warnings
                        warnings.warn("--sampler philox: the run %s:%d-%d was built on the host (not one the device builder takes): its loci "
                                      "over the UMI cap keep the reference's sample" % (chrom, lo + 1, lo + nl))
                    ns = len(hp[0])
                    if slots + ns > cap or umi_base + len(ustart) > cap + 8192:
                        raise bamio.BamError("run of %d read slots does not fit the device arena" % ns)
                    for k in range(4):
                        if planes[k] is not None:
                            planes[k].upload(hp[k], 4 * slots)
                    hw = pack_words_host(hp[0], hp[2], lc)
                    if bits == 16:
                        hw = words16_from_32(hw)
                        if hw is None:
                            narrow = True
                            break
                    words.upload(hw, (bits // 8) * slots)
                    uaux[0].upload(ustart, 4 * umi_base)
                    lc = lc.copy()
                    lc["read_off4"] += slots // 4
                    lc["umi_off"] += umi_base
                    n_host += 1
                else:
                    nl, ns, lc, tb = done
                    n_dev += 1
                LC.append(lc)
                if nl:
                    per_locus = max(1.0, float(lc["n_reads"].sum()) / nl)
                slots += ns
                n_loc += nl
                total += int(lc["n_reads"].sum())
                chroms += [chrom] * nl
                poss.append(np.arange(lo + 1, lo + 1 + nl, dtype=np.int64))
                refs += list(run_ref[:nl]) + [""] * max(0, nl - len(run_ref))
                tables += tb
                i += nl
            if narrow:
                for b in [words] + uaux + [p for p in planes if p is not None]:
                    b.free()
                for d in ds:
                    d.free()
                eng.word_bits = 32
                eng.drop_spare_tuned()           # (the block chosen for the 16-bit words is of a size nothing asks for again: back to the runtime)
                i = first
                continue
            uaux[1].free(); uaux[2].free()
            rb = ResidentBatch(planes=planes + [uaux[0]], words=words, n_slots=slots, n_ustart=slots + n_loc + 1,
                               loci=_all_loci(LC), chrom=chroms, pos=poss[0] if len(poss) == 1 else np.concatenate(poss) if poss else np.zeros(0, np.int64),
                               ref=refs, alleles=tables,
                               n_device_runs=n_dev, n_host_runs=n_host)
            if ds_rules is None:
                yield first, rb
            else:
                yield first, [rb] + [d.batch(rb) for d in ds]
    finally:
        bam.close()
        # (--dsRpbSampler philox: the file-wide table in HBM - on the last batch, or on an error; `close_tables` False: the caller owns
        # the rules' tables and closes them itself - the command line, whose replicate stage of --spikeRpb reads the table behind the
        # last batch)
        if close_tables:
            close_rules(ds_rules)


def _all_loci(LC):
    """The descriptors of a batch from those of its builds, in order."""
    return LC[0] if len(LC) == 1 else np.concatenate(LC)


class _DsBatch(object):
    """The device arrays and host parts of one --dsMT rule's batch (iter_resident_batches), or of the copies of one kept run that a
    replicate stage calls together (_build_copies)."""

    def __init__(self, eng, cap, bits, all_planes):
        from .engine import DevBuf
        self.planes = [DevBuf(eng, 4 * cap) if all_planes else None for k in range(4)]
        self.words = DevBuf(eng, (bits // 8) * cap, walk_output=True)
        self.words.word_bits = bits
        self.uaux = [DevBuf(eng, 4 * (cap + 8192)) for _ in range(3)]
        self.LC, self.tables, self.slots = [], [], 0

    def free(self):
        for b in [self.words] + self.uaux + [p for p in self.planes if p is not None]:
            b.free()

    def add(self, done):
        """What build_run answered for a build into these arrays at `slots`: the next one stands behind it."""
        _, ns, lc, tb = done
        self.LC.append(lc)
        self.tables += tb
        self.slots += ns

    def loci(self) -> np.ndarray:
        return _all_loci(self.LC)

    def batch(self, full) -> ResidentBatch:
        self.uaux[1].free(); self.uaux[2].free()
        lc = self.loci()
        return ResidentBatch(planes=self.planes + [self.uaux[0]], words=self.words, n_slots=self.slots, n_ustart=self.slots + len(lc) + 1,
                             loci=lc, chrom=full.chrom, pos=full.pos, ref=full.ref, alleles=self.tables, n_device_runs=full.n_device_runs)


def _ds_refused(chrom, lo, hi, why, flag="--dsMT"):
    return "%s needs the device builder: the run %s:%d-%d cannot go through it (%s)" % (flag, chrom, lo + 1, hi, why)


def _ds_flag(rules):
    return " / ".join(sorted({r.flag for r in rules}, reverse=True))


class _KeptRun(object):
    """What build_run needs of one build of a decoded run `A`: the arrays in HBM with their counts - the run's own, a spiked copy's
    (`run`, A, None) or a selection of either (select_run's `sel, counts, d_orig`) - and the three callbacks that take the build's
    numbering back to the decoder's (`key`, `name`, `idents`: its allele_key, barcode_name and barcode_idents).
    A kept alignment's index is not the decoder's: with a selection a key is asked for at orig_index of it.  `copy` (a copy
    smc_spike_indels wrote, or the one a selection was made of): a relocated record's texts come from the copy (copy_allele_key).
    `by_read` (select_run at level "read"): the selection renumbers the barcodes by first kept appearance, so new id g is old id
    old_bc()[g] - the old ids of the kept alignments in order, each at its first appearance; a barcode-level selection keeps the ids.
    idents() is therefore what scattering the decoder's identities of the kept alignments' old ids to their new ids gives
    (tests/test_host_logic.py pins the two against each other).  orig_index comes down once, when first asked for.
    -> allele_key(ai, qpos, indel), barcode_name(g), barcode_idents(n): build_run's callbacks; old_bc(), idents()."""

    def __init__(self, run: RunOnDevice, counts, d_orig, A, key, name, idents, copy: RunOnDevice = None, by_read: bool = False):
        self.run, self.counts, self.A, self.d_orig, self.by_read = run, counts, A, d_orig, by_read
        self._key = key if copy is None else copy_allele_key(copy, A, key)
        self._name, self._idents = name, idents
        self._orig = self._old_bc = None
        # (what build_run is handed: where nothing is renumbered, the decoder's own - no call in between)
        self.allele_key = self._key if d_orig is None else self._kept_key
        self.barcode_name, self.barcode_idents = (self._old_name, lambda n: self.idents()) if by_read else (name, idents)

    def orig_index(self) -> np.ndarray:
        """The place in the run of every kept alignment."""
        if self._orig is None:
            self._orig = self.d_orig.download(np.uint32, self.run.n_aln) if self.run.n_aln else np.zeros(0, np.uint32)
        return self._orig

    def _kept_key(self, ai, qpos, indel):
        # (the builder's alignment index counts the KEPT alignments: the decoder's records, and a copy's, are those of the full run)
        return self._key(int(self.orig_index()[int(ai)]), qpos, indel)

    def old_bc(self) -> np.ndarray:
        """The decoder's barcode id of every barcode id of this build."""
        if self._old_bc is None:
            if self.by_read:
                old = self.A["aln"]["bc_gid"][self.orig_index()]
                self._old_bc = old[np.sort(np.unique(old, return_index=True)[1])]
            else:
                self._old_bc = np.arange(int(self.A["n_bc"]))
        return self._old_bc

    def _old_name(self, g):
        return self._name(int(self.old_bc()[int(g)]))

    def idents(self) -> np.ndarray:
        """The identity of every barcode id of this build."""
        ids = self._idents(self.A["n_bc"])
        return ids[self.old_bc()] if self.by_read else ids

    def free(self):
        """A selection's own arrays; the run's and a copy's stay their owner's."""
        if self.d_orig is not None:
            self.run.free(shared=False)
            self.d_orig.free()


def _ds_build_run(rules, ds, A, up, eng, chrom, lo, fasta, run_ref, cap, max_depth, bam, sampler, sampler_seed, n_loc):
    """The rules' builds of one decoded run (`up`: its arrays in HBM) behind the batch's first `n_loc` loci: select, build into each
    rule's batch.  False: a build has no room in 16-bit read words (the batch is built again with 32-bit ones)."""
    L = eng.L
    nl = A["nl"]
    res = []
    idents = names = p_idents = p_names = mism = None
    d_masks = {}                     # (philox read rules) (id(table), grid) -> (device masks of those rules, words per mask, id(rule) -> index)
    d_cells = None                   # (--dsAFDepth) (device masks of every cell of this run, words per mask)
    # (--spikeAF, --spikeDepth) a target's spiked copy of this run (None: no record spans a listed position) and the builds that still
    # need it - the target's own and those of its cells
    spiked_of = {}
    users = {}
    for rule in rules:
        if rule.spike is not None:
            users[(id(rule.spike), rule.af)] = users.get((id(rule.spike), rule.af), 0) + 1

    def read_idents(rule):
        # (--dsRpb, --spikeRpb: the kept read names, by read-name id - an id must stand for one full name, or the rule cannot be applied)
        nonlocal p_idents
        if p_idents is None:
            p_idents = pair_idents_or_refuse(bam, A, rule.flag if rule.spike_rpb_cell else "--dsRpb", chrom, lo, nl)
        return p_idents

    def read_mask(rule):
        # (--dsRpbSampler philox: the masks of every target from the file-wide table, one launch per run; the --dsGrid cells over
        # the same table: one launch more) -> the device address of the rule's mask
        # (--spikeRpb: the T cells of one r keep the same names - one mask serves them)
        key = (id(rule.groups), rule.grid)
        same = lambda r: (r.thr, r.bc_thr)
        if key not in d_masks:
            first = {}
            for r in rules:
                if r.groups is rule.groups and r.grid == rule.grid:
                    first.setdefault(same(r), r)
            buf, n_words, index = _run_read_masks(eng, rule.groups, list(first.values()), read_idents(rule), chrom, lo, nl)
            d_masks[key] = (buf, n_words, {k: index[id(r)] for k, r in first.items()})
        buf, n_words, index = d_masks[key]
        return buf.data_ptr() + 4 * n_words * index[same(rule)]
    try:
        for rule, d in zip(rules, ds):
            if not nl:
                res.append((0, 0, np.zeros(0, LOCUS_DTYPE), []))
                continue
            spiked = None
            if rule.spike is not None:
                # (--spikeAF: no selection - the run's records and bases copied and the listed SNVs written into the copy; a run none
                # of whose records spans a listed position is built from the run's own arrays)
                key = (id(rule.spike), rule.af)
                if key not in spiked_of:
                    spiked_of[key] = None
                    var = rule.spike.run_variants(chrom, A, rule.af)
                    if len(var):
                        if idents is None:
                            idents = bam.barcode_idents(A["n_bc"])
                        if mism is None:
                            mism = bam.run_mismatches(len(A["aln"]))
                        spiked_of[key], _ = spike_copy(eng, up, A, rule.spike, chrom, var, idents, rule.seed, rule.params.mismatchThr,
                                                       mism[0], mism[1])
                spiked = spiked_of[key]
                if rule.spike_rpb_cell:
                    # (--spikeRpb: the philox read selection at r over the target's copy, or over the run's own arrays where nothing
                    # was spiked - the masks of every cell of the table from one launch: spiking changes no name)
                    sel, counts, d_orig = select_run(eng, spiked or up, A, lo, d_mask=read_mask(rule), level="read")
                elif rule.spike_cell:
                    # (--spikeDepth: the --dsMT philox selection at f over the target's copy - the one spiked above for the target's
                    # own build -, or over the run's own arrays where nothing was spiked)
                    if idents is None:
                        idents = bam.barcode_idents(A["n_bc"])
                    sel, counts, d_orig = select_run(eng, spiked or up, A, lo, idents=idents, frac=rule.frac, seed=rule.seed)
                else:
                    sel, counts, d_orig = spiked or up, A, None
            elif rule.level == "read":
                if rule.groups is not None:
                    sel, counts, d_orig = select_run(eng, up, A, lo, d_mask=read_mask(rule), level="read")
                else:
                    read_idents(rule)
                    if rule.kept_idents is not None:
                        mask = np.isin(p_idents, rule.kept_idents)
                    else:
                        if p_names is None:
                            p_names = [bam.pair_name(g) for g in range(int(A["n_pair"]))]
                        mask = np.array([t in rule.kept for t in p_names], bool)
                    sel, counts, d_orig = select_run(eng, up, A, lo, mask=mask, level="read")
            elif rule.depth is not None:
                # (--dsAFDepth: the masks of every cell from the carrier table and the two draws, one launch per run.  This branch
                # stands BEFORE the dropped_idents one on purpose: a cell's rule also carries `dropped_idents` of t and `bc_thr` of f -
                # what the cell is, for the log and for whoever restates it on the host - but its mask is the table's)
                if idents is None:
                    idents = bam.barcode_idents(A["n_bc"])
                if d_cells is None:
                    d_cells = _run_depth_masks(eng, rule.depth, idents)
                sel, counts, d_orig = select_run(eng, up, A, lo, d_mask=d_cells[0].data_ptr() + 4 * d_cells[1] * rule.cell)
            elif rule.dropped_idents is not None:
                # (--dsAF: every barcode but the dropped carriers)
                if idents is None:
                    idents = bam.barcode_idents(A["n_bc"])
                sel, counts, d_orig = select_run(eng, up, A, lo, mask=~np.isin(idents, rule.dropped_idents))
            elif rule.kept is None:
                if idents is None:
                    idents = bam.barcode_idents(A["n_bc"])
                sel, counts, d_orig = select_run(eng, up, A, lo, idents=idents, frac=rule.frac, seed=rule.seed)
            else:
                if idents is None:
                    idents = bam.barcode_idents(A["n_bc"])
                if rule.kept_idents is not None:
                    mask = np.isin(idents, rule.kept_idents)
                else:
                    if names is None:
                        names = [bam.barcode_name(g) for g in range(int(A["n_bc"]))]
                    mask = np.array([t in rule.kept for t in names], bool)
                sel, counts, d_orig = select_run(eng, up, A, lo, mask=mask)
            # (--spikeAF: every alignment is there; a key beyond the six fixed ones is an insertion's, a deletion's or an odd letter's, and
            # its site is a base the rewrite leaves alone or turns into a fixed key - the decoder's texts hold.  --spikeIndels: a relocated
            # record has another query layout - its texts come from the copy; --spikeIndelDepth: a cell of such a copy - the kept
            # alignment's index in the copy, then the copy's texts)
            # (the read level: the texts the cap samplers need are the decoder's, by the old id of every new one)
            kept = _KeptRun(sel, counts, d_orig, A, bam.allele_key, bam.barcode_name, bam.barcode_idents,
                            copy=spiked if spiked is not None and spiked.cig is not up.cig else None, by_read=rule.level == "read")
            w = d.words
            done = build_run(counts, L, eng, abi.c_params(rule.params), rule.params, chrom, lo, fasta, run_ref, [w] + d.planes, d.uaux,
                             d.slots, d.slots + n_loc, cap, max_depth, kept.allele_key, kept.barcode_name, sampler=sampler,
                             sampler_seed=sampler_seed, barcode_idents=kept.barcode_idents, uploaded=sel)
            kept.free()
            if rule.spike is not None:
                users[key] -= 1
                if not users[key] and spiked is not None:          # (behind the last build of its target)
                    free_spiked(spiked, up)
                    spiked_of[key] = None
            if done is None:
                raise bamio.BamError(_ds_refused(chrom, lo, lo + nl, "%s: the device builder does not take it" % rule.label, rule.flag))
            if done == NARROW:
                return False
            res.append(done)
    finally:
        for buf, _, _ in d_masks.values():
            buf.free()
        if d_cells is not None:
            d_cells[0].free()
        for spiked in spiked_of.values():                          # (a build that ended early: NARROW, or an error)
            if spiked is not None:
                free_spiked(spiked, up)
    for d, done in zip(ds, res):
        d.add(done)
    return True


def pair_idents_or_refuse(bam, A, flag: str, chrom: str, lo: int, nl: int) -> np.ndarray:
    """The identity of every read-name id of the run `A` that `bam` decoded last (bamio.NativeBam.pair_idents).  BamError: a read id
    stands for two different read names - a rule that keeps whole names (`flag`: --dsRpb, --spikeRpb) cannot be applied by id."""
    p_idents, shared = bam.pair_idents(A["n_pair"])
    if shared:
        raise bamio.BamError("%s: the run %s:%d-%d has a read id (read name without its last field) shared by two "
                             "different read names: ds.reads.withinMT.py keeps whole names, the decoder's ids cannot tell "
                             "them apart" % (flag, chrom, lo + 1, lo + nl))
    return p_idents


def _run_read_masks(eng, groups, rules, p_idents, chrom, lo, nl):
    """One launch for a run: the keep masks of every philox read rule of one table over the run's read-name identities ->
    (device buffer, words per mask, {id(rule): index}).  An identity the table does not hold (it cannot happen) ends the run.
    (--dsGrid cells - all of `rules` or none - take the composed rule: ReadGroups.masks_grid.)"""
    from .engine import DevBuf
    n = len(p_idents)
    n_words = (n + 31) // 32
    d_id = DevBuf(eng, 8 * max(1, n) + 256).upload(np.ascontiguousarray(p_idents, np.uint64) if n else np.zeros(1, np.uint64))
    buf = DevBuf(eng, 4 * max(1, n_words * len(rules)) + 256)
    try:
        if rules[0].grid:
            groups.masks_grid(d_id.data_ptr(), n, rules[0].seed, [r.bc_thr for r in rules], [r.thr for r in rules], buf.data_ptr())
        else:
            groups.masks(d_id.data_ptr(), n, rules[0].seed, [r.thr for r in rules], buf.data_ptr())
        st = groups.status()
    except BaseException:
        buf.free()
        raise
    finally:
        d_id.free()
    if st & RG_MISS:
        buf.free()
        raise bamio.BamError("--dsRpbSampler philox: the run %s:%d-%d has a read name the file-wide table does not hold (status %#x)"
                             % (chrom, lo + 1, lo + nl, st))
    return buf, n_words, {id(r): k for k, r in enumerate(rules)}


def _run_depth_masks(eng, table, idents):
    """One launch for a run: the keep masks of every --dsAFDepth cell (the table's one seed) over the run's barcode identities ->
    (device buffer of T x F masks, words per mask)."""
    from .engine import DevBuf
    n = len(idents)
    n_words = mask_words(n)
    d_id = DevBuf(eng, 8 * max(1, n) + 256).upload(np.ascontiguousarray(idents, np.uint64) if n else np.zeros(1, np.uint64))
    buf = DevBuf(eng, 4 * n_words * table.n_targets * table.n_fracs * len(table.seeds) + 256)
    try:
        table.masks(d_id.data_ptr(), n, buf.data_ptr(), n_words)
    except BaseException:
        buf.free()
        raise
    finally:
        d_id.free()
    return buf, n_words


def _build_status(cnt, xcap, w16, chrom, lo, nl):
    """What a build's two counters (extras entries, status bits) say -> True: use it; NARROW: an allele id beyond 15 or a quality beyond
    63 with 16-bit read words - the caller builds with 32-bit words; None: the device builder does not take the run.  PileupError: a
    base quality > 126."""
    if int(cnt[1]) != 0 or int(cnt[0]) > xcap:
        if w16 and (int(cnt[1]) & ~BUILD_ST_NARROW) == 0 and int(cnt[0]) <= xcap:
            return NARROW                     # (an allele id beyond 15 or a quality beyond 63: the caller builds with 32-bit words)
        if int(cnt[1]) & 4:
            from .features import PileupError
            raise PileupError("base quality > 126 at %s:%d-%d" % (chrom, lo + 1, lo + nl))
        return None
    return True


def _philox_marks_over_cap(eng, L, cp, params, d_loci, lc, positions, words, w16, uaux, sampler, sampler_seed, n_bc, barcode_idents, barcode_name):
    """(sampler "philox") smc_philox_marks over the built loci `d_loci` (their descriptors on the host: `lc`; their 1-based positions:
    `positions`) where one is over the barcode cap -> the descriptors as the call leaves them, or `lc`."""
    n = len(lc)
    if not (sampler == "philox" and params.ds > 0 and bool((lc["n_umi"] > params.ds).any())):
        return lc
    from .engine import DevBuf
    # the NON-parity down-sampling of the loci over the barcode cap, on the device (smc_philox_marks: Philox4x32-10 keyed by
    # position): marks in umi_start + SMC_LF_SAMPLED in the descriptors, where the reference-exact sampling leaves its own
    d_pos = DevBuf(eng, 8 * n + 256).upload(np.ascontiguousarray(positions, np.int64))
    d_st = DevBuf(eng, 256).upload(np.zeros(4, np.uint32))
    # (what identifies a barcode is a hash of its TEXT, by the run-wide id the builder left in u_gid at these loci: the sample does
    # not depend on where the runs and batches of the file were cut)
    idents = barcode_idents(n_bc) if barcode_idents is not None else \
        np.array([_fnv64(barcode_name(g)) for g in range(int(n_bc))], np.uint64)
    d_id = DevBuf(eng, 8 * max(1, len(idents)) + 256).upload(idents)
    _lib.check(L.smc_philox_marks(eng.ctx, ctypes.byref(cp), d_loci.data_ptr(), n, d_pos.data_ptr(), words.data_ptr(),
                                  16 if w16 else 32, uaux[0].data_ptr(), d_id.data_ptr(), uaux[1].data_ptr(),
                                  ctypes.c_uint64(int(sampler_seed) & 0xFFFFFFFFFFFFFFFF), d_st.data_ptr(), ctypes.c_void_p(0)), "smc_philox_marks")
    lc = d_loci.download(LOCUS_DTYPE, n)
    d_pos.free(); d_st.free(); d_id.free()
    return lc


def _py2_sample_over_cap(params, lc, pos_text, uaux, barcode_name) -> None:
    """The reference's down-sampling (smCounter.py:496-498) on the loci of `lc` over the barcode cap that no sampler has marked: barcode
    texts by first included read, the dropped ones marked in umi_start (uaux[0]), SMC_LF_SAMPLED set in `lc`.  pos_text(l): the
    locus's 1-based position as text (the sample's seed)."""
    over = np.nonzero((lc["n_umi"] > params.ds) & ((lc["flags"] & LF_SAMPLED) == 0))[0] if params.ds > 0 else []
    if len(over):
        from .py2compat import py2_downsample_barcodes
        for l in over.tolist():
            o, nu = int(lc["umi_off"][l]), int(lc["n_umi"][l])
            us = uaux[0].download(np.uint32, nu, 4 * o)
            gid = uaux[1].download(np.uint32, nu, 4 * o)
            finc = uaux[2].download(np.uint32, nu, 4 * o)
            keys = np.nonzero(finc != 0xFFFFFFFF)[0]
            keys = keys[np.argsort(finc[keys], kind="stable")]
            if len(keys) <= params.ds:
                continue
            names = [barcode_name(int(gid[u])) for u in keys]
            kept = set(py2_downsample_barcodes(pos_text(l), names, params.ds))
            for u, name in zip(keys.tolist(), names):
                if name not in kept:
                    us[u] |= USTART_DROPPED
            uaux[0].upload(us, 4 * o)
            lc["flags"][l] |= LF_SAMPLED


def build_run(A, L, eng, cp, params, chrom, lo, fasta, run_ref, planes, uaux, slot_base, umi_base, cap, max_depth,
              allele_key, barcode_name, stream_sync=True, sampler: str = "reference", sampler_seed: int = 0, barcode_idents=None,
              uploaded=None, extras: "BuildExtras" = None):
    """smc_build_planes over one run's alignments `A` (bamio.NativeBam.alignments_run or synth.generate_alignments) into the
    batch's device arrays (`planes`: [words, meta, umi, frag, dist], any of them None).  `allele_key(ai, qpos, indel)` / `barcode_name(gid)` give the texts the host needs (indel allele
    keys, barcode names for the reference's down-sampling).  `uploaded` (RunOnDevice): the run's arrays are in HBM already (A then
    holds only the counts and "deepest"); they stay the caller's.  `extras` (BuildExtras, off by default): the build's extras list
    and its count stay in the caller's device regions, extras.n gets the count, and no per-locus table is made - the answer's tables
    are [] (extras_table makes the one of a locus when it is asked for)."""
    import time
    from .engine import DevBuf
    T = _TIMES if os.environ.get("SMC_DEVPLANES_TIMING") else None
    t1 = time.perf_counter()
    nl, ns = A["nl"], A["n_slots"]
    if nl == 0:
        return 0, 0, np.zeros(0, LOCUS_DTYPE), []
    deepest = A["deepest"] if "deepest" in A else int(A["loc"]["n"].max()) if len(A["loc"]) else 0
    # (status bit 1 - an alignment flagged neither READ1 nor READ2 - no longer sends the run to the host builder: the walk's
    # exact path takes the previous pileup read's pairOrder, smCounter.py:359-362)
    if (A["status"] & ~1) != 0 or deepest > max_depth or slot_base + ns > cap or \
            umi_base + ns + nl + 1 > cap + 8192:
        return None
    if (A["status"] & 1) and A["aln"] is not None and len(A["aln"]):
        # unflagged alignments: the walk looks back for the previous flagged pileup read of every such (read, locus) - fine for a
        # sprinkle of them, quadratic for single-end data, and a run that BEGINS with one ends in the host builder's error anyway
        unfl = (A["aln"]["oflag"] & 3) == 0
        if bool(unfl[0]) or float(unfl.mean()) > 0.25:
            return None
    if uploaded is None:
        own = upload_run(eng, A, run_ref)
        d_aln, d_cig, d_bq, d_loc, d_ref = own.aln, own.cig, own.bq, own.loc, own.ref
        loc_host, n_aln = own.loc_host, own.n_aln
    else:
        own = None
        d_aln, d_cig, d_bq, d_loc, d_ref = uploaded.aln, uploaded.cig, uploaded.bq, uploaded.loc, uploaded.ref
        loc_host, n_aln = uploaded.loc_host, uploaded.n_aln
    d_loci = DevBuf(eng, nl * LOCUS_DTYPE.itemsize)
    xcap = build_xcap(nl)
    d_x, d_cnt = (DevBuf(eng, 20 * xcap), DevBuf(eng, 8)) if extras is None else (extras.x, extras.cnt)
    bi = abi.SmcBuildIn(d_aln.data_ptr(), d_cig.data_ptr(), d_bq.data_ptr(), d_loc.data_ptr(), d_ref.data_ptr(),
                        lo, nl, A["n_bc"], A["n_pair"], deepest, n_aln, loc_host.ctypes.data if loc_host is not None else None)
    pp = [t.data_ptr() if t is not None else None for t in planes]     # [words, meta, umi, frag, dist]
    w16 = getattr(planes[0], "word_bits", 32) == 16
    if w16:                                                            # (16-bit read words: nothing but the words is written)
        assert all(p is None for p in pp[1:])
        _lib.check(L.smc_build_planes_w16(eng.ctx, ctypes.byref(cp), ctypes.byref(bi), slot_base, umi_base, pp[0], uaux[0].data_ptr(),
                                          uaux[1].data_ptr(), uaux[2].data_ptr(), d_loci.data_ptr(), d_x.data_ptr(), xcap,
                                          d_cnt.data_ptr(), ctypes.c_void_p(0)), "smc_build_planes_w16")
    else:
        _lib.check(L.smc_build_planes(eng.ctx, ctypes.byref(cp), ctypes.byref(bi), slot_base, umi_base, pp[0], pp[1], pp[2], pp[3], pp[4],
                                      uaux[0].data_ptr(),
                                      uaux[1].data_ptr(), uaux[2].data_ptr(), d_loci.data_ptr(), d_x.data_ptr(), xcap,
                                      d_cnt.data_ptr(), ctypes.c_void_p(0)), "smc_build_planes")
    t2 = time.perf_counter()
    cnt = d_cnt.download(np.uint32, 2)        # (a copy on the default stream: behind the kernel)
    t3 = time.perf_counter()
    if T is not None:
        T["upload+launch"] += t2 - t1; T["kernel (sync)"] += t3 - t2
    st = _build_status(cnt, xcap, w16, chrom, lo, nl)
    if st is not True:
        return st
    lc = d_loci.download(LOCUS_DTYPE, nl)
    if sampler == "philox":                   # (the positions are made only where the call may need them)
        lc = _philox_marks_over_cap(eng, L, cp, params, d_loci, lc, np.arange(lo + 1, lo + 1 + nl, dtype=np.int64), planes[0], w16, uaux, sampler,
                                    sampler_seed, A["n_bc"], barcode_idents, barcode_name)
    if own is not None:
        own.free()
    for b in (d_loci,) + ((d_cnt,) if extras is None else ()):
        b.free()                              # (back to the engine's spare list right away, not whenever the collector gets to them)
    nx = int(cnt[0])
    if extras is not None:
        extras.n, tables = nx, []
    else:
        # allele tables: the six fixed keys + what the kernel met, in the order it numbered them
        tables = [_BASE_TABLE] * nl             # (shared, never written: a locus that met more alleles gets its own list)
        if nx:
            _extras_into_tables(tables, d_x.download(np.uint32, 5 * nx).reshape(nx, 5), allele_key, chrom, lo, fasta)
        d_x.free()
    if params.ds > 0:
        _py2_sample_over_cap(params, lc, lambda l: str(lo + l + 1), uaux, barcode_name)
    return nl, ns, lc, tables


def build_xcap(nl: int) -> int:
    """The extras entries build_run gives a build of `nl` loci room for (20 bytes each)."""
    return 4 * int(nl) + 4096


@dataclasses.dataclass
class BuildExtras:
    """Where build_run leaves a build's extras list instead of making tables of it: `x`, a device region of 20 * build_xcap(nl) bytes,
    and `cnt`, one of 8 bytes (the count, then the builder's status word); both stay the caller's.  `n`: the count, once built."""
    x: object
    cnt: object
    n: int = None


def _extras_into_tables(tables, xl: np.ndarray, allele_key, chrom: str, lo: int, fasta) -> None:
    """The extras entries `xl` ([n, 5]: locus, allele id, alignment, query position, indel) appended to the allele tables of their
    loci, in the order the kernel numbered them; a locus that still shares _BASE_TABLE gets a list of its own."""
    xl = xl[np.lexsort((xl[:, 1], xl[:, 0]))]
    for l, aid, ai, qpos, indel in xl.tolist():
        key = allele_key(ai, qpos, np.int32(np.uint32(indel)))
        if key[0] == "D" and len(key) > 1:        # "D<len>|<site>" -> DEL|site+deleted|site (smCounter.py:392-396)
            ln, site = key[1:].split("|")
            pos1 = lo + l + 1
            key = "DEL|" + site + fasta.fetch(chrom, pos1, pos1 + int(ln)).upper() + "|" + site
        if tables[l] is _BASE_TABLE:
            tables[l] = list(BASE_ALLELES)
        assert aid == len(tables[l]), (l, aid, len(tables[l]))
        tables[l].append(key)


def extras_table(xl: np.ndarray, locus: int, allele_key, chrom: str, lo: int, fasta):
    """The allele table of one locus of a build from the build's extras entries `xl` (a BuildExtras region downloaded: [n, 5])."""
    tables = {locus: _BASE_TABLE}
    _extras_into_tables(tables, xl[xl[:, 0] == locus], allele_key, chrom, lo, fasta)
    return tables[locus]


@dataclasses.dataclass
class RunOnDevice:
    """A run's alignment arrays in HBM (what smc_build_planes reads): uploaded once, built from as often as the caller likes."""
    aln: object
    cig: object
    bq: object
    loc: object
    ref: object
    n_aln: int
    loc_host: object = None     # loc[] in host memory (sizes the builder's launches), or None: the library copies it back
    pairs_used: int = None      # (a copy smc_spike_indels wrote) the pairs of its pool: the run's own, then the relocated records'

    def free(self, shared: bool = True):
        for b in ((self.aln, self.cig, self.bq, self.loc, self.ref) if shared else (self.aln, self.loc)):
            b.free()


def _up8(eng, a: np.ndarray):
    """A DevBuf of its own that holds the bytes of the contiguous array `a` (four zero bytes for an empty one)."""
    from .engine import DevBuf
    return DevBuf(eng, a.nbytes + 256).upload(a.view(np.uint8).reshape(-1) if a.nbytes else np.zeros(4, np.uint8))


def upload_run(eng, A, run_ref: str) -> RunOnDevice:
    nl = A["nl"]
    up = functools.partial(_up8, eng)
    d_ref = up(np.frombuffer(run_ref[:nl].encode().ljust(nl, b"\0"), np.uint8).copy())
    # (the windows size the sort and the launch grids: read on the host)
    return RunOnDevice(up(A["aln"]), up(A["cig"]), up(A["bq"]), up(A["loc"]), d_ref, len(A["aln"]), np.ascontiguousarray(A["loc"]))


# ---- in-run molecule down-sampling (--dsMT): ds.mt.py's drop of whole barcodes, done on the run's alignments in HBM
DS_DOMAIN = 0x64734D54         # counter word 2 of the philox draw (k_select_aln.inc: SEL_DOMAIN)


@dataclasses.dataclass
class DsRule:
    """One fraction of --dsMT: which barcodes stay, and the parameters that fraction is called with (its mtDepth: its cap, its
    threshold).  `kept`: the reference's kept set (barcode texts, tools.ds_mt semantics over the whole file); None: the device's
    philox rule with `seed`."""
    frac: float
    params: object
    kept: object = None
    seed: int = 1234567
    kept_idents: object = None  # (sorted FNV-1a idents of `kept` when no two barcodes of the file share one: a run's mask without texts)
    # (--dsRpb) level "read": `kept` holds full read names (ds.reads.withinMT.py), `target` the reads per barcode asked for, `prob_keep`
    # the reference's probKeep, `n_names` the distinct read names of the file
    level: str = "barcode"
    target: float = None
    prob_keep: float = None
    n_names: int = 0
    # (--dsRpbSampler philox) `groups`: the file-wide ReadGroups table in HBM (kept is None), `thr` = floor(probKeep x 2^32) clamped
    # to [0, 2^32], `n_kept` the names it keeps
    groups: object = None
    thr: int = None
    n_kept: int = None
    # (--dsGrid) a cell: level "read", `frac` f and `target` r; `kept` the names of the three-step workflow (reference), or, philox,
    # `bc_thr` = the --dsMT draw's threshold at f beside `thr`; `n_names` the names of the barcodes kept at f
    grid: bool = False
    bc_thr: int = None
    # (--dsAF) level "barcode": `af` the target allele fraction, `dropped_idents` the sorted FNV-1a idents of the barcodes that go
    # (every other barcode stays: ds_af_rules)
    af: float = None
    dropped_idents: object = None
    # (--dsAFDepth) a cell: `af` t and `frac` f; `dropped_idents` of t beside `bc_thr` = the --dsMT draw's threshold at f; `depth`: the
    # cells' AfCellTable in HBM (one for all cells of the run), `cell` this one's index in its masks (t x F + f)
    depth: object = None
    cell: int = None
    # (--spikeAF) level "barcode", nothing dropped: `af` the target allele fraction, `spike` the SpikeSet whose listed SNVs are written
    # into a copy of every run whose records span one (spike_run), at the threshold of `af`
    # (--spikeDepth) a cell: `spike` and `af` of its target beside `frac` f and `bc_thr` = the --dsMT draw's threshold at f: the spiked
    # copy of the target, then the philox selection at f with the same `seed`
    # (--spikeRpb) a cell: `spike` and `af` of its target beside level "read", `target` r, `prob_keep`, `groups` (the file-wide table of
    # the UNSPIKED file: spiking changes no name) and `thr`: the spiked copy of the target, then the philox read selection at r with the
    # same `seed`
    # (--spikeGrid) a cell: the same with `grid`, `frac` f and `bc_thr` - --dsGrid's composed philox rule at (f, r) over the spiked copy
    spike: object = None

    @property
    def spike_cell(self) -> bool:
        return self.spike is not None and self.bc_thr is not None

    @property
    def spike_rpb_cell(self) -> bool:
        return self.spike is not None and self.level == "read"

    @property
    def flag(self) -> str:
        if self.spike_rpb_cell:
            # (--spikePhaseRpb's cells are --spikeIndelRpb's under another flag: the SpikeSet carries its name)
            return getattr(self.spike, "rpb_flag", None) or ("--spikeIndelRpb" if getattr(self.spike, "indels", False) else "--spikeRpb")
        if self.spike is not None:
            return "--spikeDepth" if self.spike_cell else "--spikeAF"
        if self.depth is not None:
            return "--dsAFDepth"
        if self.af is not None:
            return "--dsAF"
        return "--dsGrid" if self.grid else "--dsRpb" if self.level == "read" else "--dsMT"

    @property
    def sampler(self) -> str:
        return "philox" if self.kept is None else "reference"

    @property
    def label(self) -> str:
        if self.spike_rpb_cell and self.grid:
            return "spiked allele fraction %g x fraction %g x target %g" % (self.af, self.frac, self.target)
        if self.spike_rpb_cell:
            return "spiked allele fraction %g x target %g" % (self.af, self.target)
        if self.spike_cell:
            return "spiked allele fraction %g x fraction %g" % (self.af, self.frac)
        if self.spike is not None:
            return "spiked allele fraction %g" % self.af
        if self.depth is not None:
            return "allele fraction %g x fraction %g" % (self.af, self.frac)
        if self.af is not None:
            return "allele fraction %g" % self.af
        if self.grid:
            return "fraction %g x target %g" % (self.frac, self.target)
        return "target %g" % self.target if self.level == "read" else "fraction %g" % self.frac


def reference_rules(path: str, fracs, params_list, seed: int):
    """DsRules of the reference's sampler: every placed barcode of the file in first-appearance order, py2 dict order, one
    random() each from Python 2's generator seeded with `seed`, kept when r <= f (ds.mt.py:23-72; tools.ds_mt.select_barcodes).
    Computed once per file."""
    from .py2compat import Py2Random, py2_dict_order
    order = bamio.placed_barcodes(path)
    py2 = py2_dict_order(order)
    idents = fnv64_array(order)
    unique = len(np.unique(idents)) == len(order)
    rules = []
    for f, P in zip(fracs, params_list):
        rng = Py2Random(int(seed))
        kept = {bc for bc in py2 if rng.random() <= f}
        ki = np.sort(fnv64_array(sorted(kept))) if unique else None
        rules.append(DsRule(float(f), P, kept=kept, seed=int(seed), kept_idents=ki))
    return rules


def group_placed_reads(path: str):
    """The file's placed read names grouped as ds.reads.withinMT.py:37-44 groups them -> (per_bc, order): the one pass over the file
    that --dsRpb and --dsGrid (reference sampler) share."""
    from .tools import ds_reads_within_mt as rw
    return rw.group_reads(bamio.placed_qnames(path))


def reference_read_rules(path: str, targets, params_list, seed: int, grouped=None):
    """DsRules of --dsRpb: for each target r the read names ds.reads.withinMT.py --rpb r --seed `seed` keeps (:22-90;
    tools.ds_reads_within_mt): per barcode its distinct names in first-appearance order, probKeep from the whole file's counts,
    barcodes in py2 dict order, the first name always kept, every further one when random() <= probKeep.  The names are read and
    grouped once per file (`grouped`: group_placed_reads(path) done already).  A file without a barcode of two or more names has no
    probKeep (the reference divides by zero): ValueError naming the file and the target."""
    from .py2compat import py2_dict_order
    from .tools import ds_reads_within_mt as rw
    per_bc, order = grouped if grouped is not None else group_placed_reads(path)
    py2 = py2_dict_order(order)
    names = [q for bc in order for q in per_bc[bc]]
    idents = fnv64_array(names)
    unique = len(np.unique(idents)) == len(names)
    rules = []
    for r, P in zip(targets, params_list):
        try:
            prob = rw.prob_keep(per_bc, r)
        except ZeroDivisionError:
            raise ValueError("--dsRpb %g: %s has no barcode with more than one read name, so ds.reads.withinMT.py's probKeep "
                             "(:58) is not defined (it divides by zero)" % (r, path))
        kept = rw.draw_reads(per_bc, py2, prob, seed)
        ki = np.sort(idents[np.fromiter((q in kept for q in names), bool, len(names))]) if unique else None
        rules.append(DsRule(1.0, P, kept=kept, seed=int(seed), kept_idents=ki, level="read", target=float(r), prob_keep=prob,
                            n_names=len(names)))
    return rules


def reference_grid_rules(path: str, cells, params_list, seed: int, kept_barcodes, grouped):
    """DsRules of --dsGrid with the reference's samplers: for every cell (f, r) the read names of ds.mt.py --pct f, then
    ds.reads.withinMT.py --rpb r on that BAM (both --seed `seed`).  The first BAM holds the kept barcodes whole, so the second script
    sees the file's grouping restricted to them: their names, first-appearance order, py2 dict order of that order, probKeep from their
    counts, one random() stream.  `kept_barcodes`: f -> the barcodes reference_rules keeps at f; `grouped`: group_placed_reads(path) -
    no further pass over the file.  A cell whose kept barcodes include none of two or more names: ValueError naming f and r."""
    from .py2compat import py2_dict_order
    from .tools import ds_reads_within_mt as rw
    per_bc, order = grouped
    names = [q for bc in order for q in per_bc[bc]]
    unique = len(np.unique(fnv64_array(names))) == len(names)
    sub, rules = {}, []
    for (f, r), P in zip(cells, params_list):
        if f not in sub:
            keep = kept_barcodes[f]
            order_f = [bc for bc in order if bc in keep]
            names_f = [q for bc in order_f for q in per_bc[bc]]
            sub[f] = ({bc: per_bc[bc] for bc in order_f}, py2_dict_order(order_f), names_f, fnv64_array(names_f))
        per_f, py2_f, names_f, idents_f = sub[f]
        try:
            prob = rw.prob_keep(per_f, r)
        except ZeroDivisionError:
            raise ValueError("--dsGrid fraction %g x target %g: no barcode kept at %g in %s has more than one read name, so "
                             "ds.reads.withinMT.py's probKeep (:58) is not defined (it divides by zero)" % (f, r, f, path))
        kept = rw.draw_reads(per_f, py2_f, prob, seed)
        ki = np.sort(idents_f[np.fromiter((q in kept for q in names_f), bool, len(names_f))]) if unique else None
        rules.append(DsRule(float(f), P, kept=kept, seed=int(seed), kept_idents=ki, level="read", target=float(r), prob_keep=prob,
                            n_names=len(names_f), grid=True))
    return rules


def frac_threshold(f: float) -> int:
    """The --dsMT philox draw's threshold at fraction f (smc_select_alignments): floor(f x 2^32), 2^32 at f >= 1."""
    return 1 << 32 if f >= 1.0 else int(np.floor(f * 4294967296.0))


def philox_grid_rules(path: str, cells, params_list, seed: int, groups):
    """DsRules of --dsGrid with both philox samplers, over the --dsRpbSampler philox targets' file-wide table `groups` (one table per
    file): a name is kept in cell (f, r) when its barcode passes the --dsMT philox draw at f and it is its barcode's first name or its
    read draw is below floor(probKeep_fr x 2^32); probKeep_fr as ds.reads.withinMT.py:58 computes it, in double, from the counters of
    the barcodes kept at f (ReadGroups.counts_frac) - a plain --dsRpb r --dsRpbSampler philox run on the BAM of the --dsSampler philox
    barcodes at f.  A cell whose kept barcodes include none of two or more names: ValueError naming f and r."""
    fr = list(dict.fromkeys(f for f, _ in cells))
    cf = dict(zip(fr, groups.counts_frac(seed, [frac_threshold(f) for f in fr])))
    rules = []
    for (f, r), P in zip(cells, params_list):
        c = cf[f]
        if c["multi_names"] == c["multi"]:
            raise ValueError("--dsGrid fraction %g x target %g: no barcode kept at %g in %s has more than one read name, so "
                             "ds.reads.withinMT.py's probKeep (:58) is not defined (it divides by zero)" % (f, r, f, path))
        prob = 1.0 * (float(r) - 1.0) * (c["one"] + c["multi"]) / (c["multi_names"] - c["multi"])
        rules.append(DsRule(float(f), P, kept=None, seed=int(seed), level="read", target=float(r), prob_keep=prob, n_names=c["names"],
                            groups=groups, thr=read_threshold(prob), grid=True, bc_thr=frac_threshold(f)))
    for rule, k in zip(rules, groups.kept_grid(seed, [r.bc_thr for r in rules], [r.thr for r in rules])):
        rule.n_kept = k
    return rules


RPB_DOMAIN = 0x64735250        # counter word 2 of the read-level philox draw (k_read_groups.inc: RG_DOMAIN, "dsRP")
RG_NAME_COLLISION, RG_BARCODE_COLLISION, RG_FULL, RG_MISS, RG_RESERVED = 1, 2, 4, 8, 16      # smc_read_groups_status bits
RG_MAX_TARGETS = 32
NAME_KEY_CHUNK = 1 << 20       # placed records per chunk of the file pass (24 MB of keys on the host)


class ReadGroups(object):
    """The file-wide read-name / barcode table of --dsRpbSampler philox in HBM (smc_read_groups_*, csrc/k_read_groups.inc): records
    added in chunks (bamio.NativeBam.name_keys), grouped by finish(), then masks per run and kept counts per target.  close() frees it
    (idempotent)."""

    COUNTS = ("records", "names", "barcodes", "one", "multi", "multi_names", "first_names")

    def __init__(self, eng):
        self.eng, self.L = eng, eng.L
        h = ctypes.c_void_p()
        _lib.check(self.L.smc_read_groups_create(eng.ctx, ctypes.byref(h)), "smc_read_groups_create")
        self._h = h

    def add(self, keys, first_ordinal: int):
        """uint64 [n, 3] keys of consecutive placed records (smc_bam_name_keys' layout = smc_read_key), the first one's ordinal."""
        keys = np.ascontiguousarray(keys, np.uint64)
        _lib.check(self.L.smc_read_groups_add(self._h, keys.ctypes.data, len(keys), int(first_ordinal)), "smc_read_groups_add")

    def finish(self) -> dict:
        c = np.zeros(8, np.int64)
        _lib.check(self.L.smc_read_groups_finish(self._h, c.ctypes.data), "smc_read_groups_finish")
        return dict(zip(self.COUNTS, (int(v) for v in c)))

    @staticmethod
    def _thr(thr, what="--dsRpb targets"):
        t = np.ascontiguousarray(thr, np.uint64)
        if len(t) > RG_MAX_TARGETS:
            raise ValueError("at most %d %s with the philox sampler" % (RG_MAX_TARGETS, what))
        return t

    def masks(self, d_idents, n_ids: int, seed: int, thr, d_masks):
        """Per read-name identity (device pointer, n_ids of them) a keep bit per target into d_masks: len(thr) masks of
        ceil(n_ids / 32) words, smc_select_alignments_keyed's read-level layout."""
        t = self._thr(thr)
        _lib.check(self.L.smc_read_groups_masks(self._h, d_idents, int(n_ids), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                                t.ctypes.data, len(t), d_masks, ctypes.c_void_p(0)), "smc_read_groups_masks")

    def kept(self, seed: int, thr) -> list:
        t = self._thr(thr)
        k = np.zeros(max(1, len(t)), np.int64)
        _lib.check(self.L.smc_read_groups_kept(self._h, ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), t.ctypes.data, len(t),
                                               k.ctypes.data), "smc_read_groups_kept")
        return [int(v) for v in k[:len(t)]]

    def counts_frac(self, seed: int, bc_thr) -> list:
        """(--dsGrid) Per fraction threshold (frac_threshold) the counters of the barcodes the --dsMT philox draw keeps: dicts of
        names / barcodes / one / multi / multi_names / first_names."""
        t = self._thr(bc_thr, "--dsMT fractions")
        c = np.zeros((max(1, len(t)), 8), np.int64)
        _lib.check(self.L.smc_read_groups_counts_frac(self._h, ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), t.ctypes.data, len(t),
                                                      c.ctypes.data), "smc_read_groups_counts_frac")
        return [dict(zip(self.COUNTS[1:], (int(v) for v in row[1:7]))) for row in c[:len(t)]]

    def counts_frac_seeds(self, seeds, bc_thr) -> np.ndarray:
        """(--spikeGrid) counts_frac for every seed in one launch -> uint64 [len(seeds), len(bc_thr), 4] = (barcodes, one, multi,
        multi_names) of the barcodes seeds[j] keeps at bc_thr[f]."""
        t = self._thr(bc_thr, "--dsMT fractions")
        s = np.ascontiguousarray([int(x) & 0xFFFFFFFFFFFFFFFF for x in seeds], np.uint64)
        c = np.zeros((len(s), len(t), 4), np.uint64)
        _lib.check(self.L.smc_read_groups_counts_frac_seeds(self._h, s.ctypes.data, len(s), t.ctypes.data, len(t), c.ctypes.data),
                   "smc_read_groups_counts_frac_seeds")
        return c

    def masks_grid(self, d_idents, n_ids: int, seed: int, bc_thr, rd_thr, d_masks):
        """(--dsGrid) masks() with a mask per cell: barcode threshold bc_thr[c] and read threshold rd_thr[c]."""
        b, r = self._thr(bc_thr, "--dsGrid cells"), self._thr(rd_thr, "--dsGrid cells")
        if len(b) != len(r):
            raise ValueError("masks_grid: %d barcode thresholds, %d read thresholds" % (len(b), len(r)))
        _lib.check(self.L.smc_read_groups_masks_grid(self._h, d_idents, int(n_ids), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                                     b.ctypes.data, r.ctypes.data, len(b), d_masks, ctypes.c_void_p(0)),
                   "smc_read_groups_masks_grid")

    def kept_grid(self, seed: int, bc_thr, rd_thr) -> list:
        b, r = self._thr(bc_thr, "--dsGrid cells"), self._thr(rd_thr, "--dsGrid cells")
        if len(b) != len(r):
            raise ValueError("kept_grid: %d barcode thresholds, %d read thresholds" % (len(b), len(r)))
        k = np.zeros(max(1, len(b)), np.int64)
        _lib.check(self.L.smc_read_groups_kept_grid(self._h, ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), b.ctypes.data, r.ctypes.data,
                                                    len(b), k.ctypes.data), "smc_read_groups_kept_grid")
        return [int(v) for v in k[:len(b)]]

    def status(self) -> int:
        st = ctypes.c_uint32(0)
        _lib.check(self.L.smc_read_groups_status(self._h, ctypes.byref(st)), "smc_read_groups_status")
        return int(st.value)

    def close(self):
        if self._h:
            self.L.smc_read_groups_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def read_threshold(prob: float) -> int:
    """floor(probKeep x 2^32) clamped to [0, 2^32]: probKeep >= 1 keeps every name, <= 0 only the barcodes' first names."""
    if not prob > 0.0:
        return 0
    return min(1 << 32, int(np.floor(prob * 4294967296.0)))


def philox_read_rules(path: str, targets, params_list, seed: int, eng, chunk: int = NAME_KEY_CHUNK, nthreads: int = 0, flag: str = None):
    """DsRules of --dsRpb --dsRpbSampler philox: the whole file's placed records streamed (bamio.NativeBam.name_keys, `chunk` records
    at a time) into one ReadGroups table in HBM, its counters back on the host, probKeep per target from them in double exactly as
    ds.reads.withinMT.py:58 computes it; a name is kept when it is its barcode's first or its philox draw falls below
    floor(probKeep x 2^32) - NOT the reference's sample.  The rules share the table (rule.groups); iter_resident_batches frees it when
    it ends.  ValueError: a hash collision (two texts behind one identity), or a file without a barcode of two or more names.
    `flag` (--spikeRpb): the flag the refusals name in place of --dsRpb / --dsRpbSampler philox - its cells have this sampler only, so
    the advice to use the reference sampler is left out."""
    groups = ReadGroups(eng)
    try:
        bam = bamio.NativeBam(path)
        try:
            for first, keys in bam.name_keys(chunk, nthreads):
                groups.add(keys, first)
        finally:
            bam.close()
        c = groups.finish()
        st = groups.status()
        if st:
            what = [w for b, w in ((RG_NAME_COLLISION, "two read names share a 64-bit name identity"),
                                   (RG_BARCODE_COLLISION, "two barcodes share a 64-bit identity"),
                                   (RG_FULL, "the table is full"), (RG_RESERVED, "a name or barcode hashes to the reserved identity 0"))
                    if st & b]
            raise ValueError("%s: %s: %s; the philox read sampler refuses the file%s"
                             % (flag or "--dsRpbSampler philox", path, ", ".join(what) or "status %#x" % st,
                                "" if flag else " (use --dsRpbSampler reference)"))
        one, multi, multi_names = c["one"], c["multi"], c["multi_names"]
        rules = []
        for r, P in zip(targets, params_list):
            if multi_names == multi:
                raise ValueError("%s %g: %s has no barcode with more than one read name, so ds.reads.withinMT.py's probKeep "
                                 "(:58) is not defined (it divides by zero)" % (flag or "--dsRpb", r, path))
            prob = 1.0 * (float(r) - 1.0) * (one + multi) / (multi_names - multi)
            rules.append(DsRule(1.0, P, kept=None, seed=int(seed), level="read", target=float(r), prob_keep=prob,
                                n_names=c["names"], groups=groups, thr=read_threshold(prob)))
        for rule, k in zip(rules, groups.kept(seed, [rule.thr for rule in rules])):
            rule.n_kept = k
        groups.counts = c
        return rules
    except BaseException:
        groups.close()
        raise


def close_rules(rules):
    """Free the device tables the rules hold (philox read rules); idempotent."""
    for rule in rules or ():
        if getattr(rule, "groups", None) is not None:
            rule.groups.close()
    # (--dsAFDepth: the cells of a run share ONE table - freed once)
    for table in {id(r.depth): r.depth for r in rules or () if getattr(r, "depth", None) is not None}.values():
        table.free()


def check32_array(texts) -> np.ndarray:
    """FNV-1a (32 bits) of every text: the check word smc_bam_name_keys writes beside each identity (smcounter_host.h)."""
    b = [t.encode() for t in texts]
    n = len(b)
    x = np.full(n, 2166136261, np.uint32)
    if not n:
        return x
    lens = np.fromiter(map(len, b), np.int64, n)
    m = np.array(b, dtype="S%d" % max(1, int(lens.max()))).view(np.uint8).reshape(n, -1)
    prime = np.uint32(16777619)
    with np.errstate(over="ignore"):
        for k in range(m.shape[1]):
            live = lens > k
            x[live] = (x[live] ^ m[live, k].astype(np.uint32)) * prime
    return x


def fnv64_array(texts) -> np.ndarray:
    """FNV-1a (64 bits) of every text, vectorised: what smc_bam_barcode_idents / smc_bam_pair_idents compute for a run's ids."""
    b = [t.encode() for t in texts]
    n = len(b)
    x = np.full(n, 1469598103934665603, np.uint64)
    if not n:
        return x
    lens = np.fromiter(map(len, b), np.int64, n)
    # (a fixed-width byte array, zero-padded - the texts hold no NUL byte - viewed as an n x width matrix)
    m = np.array(b, dtype="S%d" % max(1, int(lens.max()))).view(np.uint8).reshape(n, -1)
    prime = np.uint64(1099511628211)
    with np.errstate(over="ignore"):
        for k in range(m.shape[1]):
            live = lens > k
            x[live] = (x[live] ^ m[live, k].astype(np.uint64)) * prime
    return x


def philox_keep_host(L, idents, frac: float, seed: int) -> np.ndarray:
    """The philox rule restated on the host (smc_philox4x32_10_host): which of these barcode identities stay at fraction `frac`."""
    if frac >= 1.0:
        return np.ones(len(idents), bool)
    thr = int(np.floor(frac * 4294967296.0))
    key = (ctypes.c_uint32 * 2)(seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    out = (ctypes.c_uint32 * 4)()
    keep = np.zeros(len(idents), bool)
    for g, v in enumerate(np.asarray(idents, np.uint64).tolist()):
        ctr = (ctypes.c_uint32 * 4)(v & 0xFFFFFFFF, v >> 32, DS_DOMAIN, 0)
        L.smc_philox4x32_10_host(ctr, key, out)
        keep[g] = out[0] < thr
    return keep


def select_run(eng, up: RunOnDevice, A, lo: int, mask=None, idents=None, frac: float = 1.0, seed: int = 0, level: str = "barcode",
               d_mask=None):
    """smc_select_alignments: the run `up` (A: its counts) reduced to the kept barcodes' alignments -> (RunOnDevice of the kept ones,
    sharing the pools and the reference; counts dict for build_run; device buffer of orig_index).  `mask`: bool per run-wide barcode
    id (the host's set); else `idents` (uint64 per id) and the philox rule at `frac` / `seed`.  level "read"
    (smc_select_alignments_keyed, SMC_SEL_KEY_READ): the same per run-wide read-name id - whole read names kept or dropped - and the
    kept alignments' ids renumbered by first kept appearance (the decoder's numbering of the down-sampled BAM).  `d_mask`: the mask
    (bit per id) in HBM already (a device address: ReadGroups.masks wrote it)."""
    from .engine import DevBuf
    L = eng.L
    nl, n = A["nl"], up.n_aln
    by_read = level == "read"
    if level not in ("barcode", "read"):
        raise ValueError("select_run: level %r" % level)
    n_ids = int(A["n_pair"] if by_read else A["n_bc"])
    d_out = DevBuf(eng, 36 * max(1, n) + 256)
    d_orig = DevBuf(eng, 4 * max(1, n) + 256)
    d_loc = DevBuf(eng, 16 * max(1, nl) + 256)
    d_sum = DevBuf(eng, 256)
    d_rule = None
    if d_mask is not None:
        mptr, iptr = int(d_mask), None
    elif mask is not None:
        words = np.packbits(np.asarray(mask, bool)[:n_ids], bitorder="little")
        words = np.concatenate([words, np.zeros((-len(words)) % 4 + 4, np.uint8)]).view(np.uint32)
        d_rule = DevBuf(eng, words.nbytes + 256).upload(words)
        mptr, iptr = d_rule.data_ptr(), None
        n_ids = min(n_ids, len(mask))
    else:
        idents = np.ascontiguousarray(idents, np.uint64)[:n_ids]
        d_rule = DevBuf(eng, 8 * max(1, len(idents)) + 256).upload(idents if len(idents) else np.zeros(1, np.uint64))
        mptr, iptr = None, d_rule.data_ptr()
        n_ids = len(idents)
    tail = (ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), float(frac), d_out.data_ptr(), d_orig.data_ptr(), d_loc.data_ptr(),
            d_sum.data_ptr(), ctypes.c_void_p(0))
    if by_read:
        _lib.check(L.smc_select_alignments_keyed(eng.ctx, up.aln.data_ptr(), n, up.loc.data_ptr(), nl, int(lo), 1, int(A["n_bc"]),
                                                 int(A["n_pair"]), mptr, iptr, n_ids, *tail),
                   "smc_select_alignments_keyed")
    else:
        _lib.check(L.smc_select_alignments(eng.ctx, up.aln.data_ptr(), n, up.loc.data_ptr(), nl, int(lo), mptr, iptr, n_ids, *tail),
                   "smc_select_alignments")
    kept, deepest, slots = (int(v) for v in d_sum.download(np.uint32, 3))
    if d_rule is not None:
        d_rule.free()
    sel = RunOnDevice(d_out, up.cig, up.bq, d_loc, up.ref, kept, None)
    counts = dict(nl=nl, n_slots=slots, n_bc=A["n_bc"], n_pair=A["n_pair"], status=A["status"], deepest=deepest, aln=None)
    if A["status"] & 1:
        # (alignments flagged neither READ1 nor READ2: the same test as build_run's on the full run, on the kept ones)
        counts["aln"] = A["aln"][d_orig.download(np.uint32, kept)] if kept else A["aln"][:0]
    return sel, counts, d_orig


SEL_MAX_SELECTIONS = 2048      # SMC_SEL_MAX_SELECTIONS


class CopySelections(object):
    """What select_copies returns: of[f][c] = select_run's triple (RunOnDevice of the kept alignments, counts dict for build_run, the
    orig_index) for copy c at fracs[f] - views over the four buffers this owns until free(): the records, orig_index and descriptors
    of selection s = f x copies + c at s x n_aln / s x n_aln / s x nl entries, and the summaries (`summary`: uint32 [F, B, 3] = kept,
    deepest, slots, on the host).  The B selections of one fraction lie at the constant strides `strides` (records, orig_index,
    descriptors; bytes), so they can be handed on as one batch."""

    def __init__(self, bufs, of, summary, strides):
        self.bufs, self.of, self.summary, self.strides = bufs, of, summary, strides

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def _copies_at_one_stride(who, runs):
    """-> (n_aln, base address, byte stride) of copies whose records stand at a constant stride or are the same array."""
    n, base = runs[0].n_aln, runs[0].aln.data_ptr()
    stride = runs[1].aln.data_ptr() - base if len(runs) > 1 else 0
    if any(r.n_aln != n or r.aln.data_ptr() != base + c * stride for c, r in enumerate(runs)):
        raise ValueError("%s: the copies' records do not stand at one stride, or differ in length" % who)
    return n, base, int(stride)


def _copy_selections(eng, runs, A, n_outer, launch) -> CopySelections:
    """The outputs of a batched selection call of n_outer x len(runs) selections (s = outer x copies + copy): the four buffers, the
    call itself (`launch(records, orig_index, descriptors, summary)`), ONE download - the summaries - and select_run's triple per
    selection as views."""
    from .engine import DevBuf
    B, n, nl = len(runs), runs[0].n_aln, int(A["nl"])
    S = B * n_outer
    sa, so, sl = 36 * n, 4 * n, 16 * nl
    bufs = [DevBuf(eng, max(1, sa) * S + 256), DevBuf(eng, max(1, so) * S + 256), DevBuf(eng, max(1, sl) * S + 256), DevBuf(eng, 16 * S + 256)]
    try:
        launch(*(b.data_ptr() for b in bufs))
        summary = bufs[3].download(np.uint32, 4 * S).reshape(n_outer, B, 4)[:, :, :3].copy()     # (the default stream: behind the kernels)
        of = []
        for f in range(n_outer):
            of.append([])
            for c, up in enumerate(runs):
                s = f * B + c
                kept, deepest, slots = (int(v) for v in summary[f, c])
                d_orig = _BufView(bufs[1], s * so)
                sel = RunOnDevice(_BufView(bufs[0], s * sa), up.cig, up.bq, _BufView(bufs[2], s * sl), up.ref, kept, None,
                                  pairs_used=up.pairs_used)
                counts = dict(nl=nl, n_slots=slots, n_bc=A["n_bc"], n_pair=A["n_pair"], status=A["status"], deepest=deepest, aln=None)
                if A["status"] & 1:
                    # (select_run's gather: alignments flagged neither READ1 nor READ2)
                    counts["aln"] = A["aln"][d_orig.download(np.uint32, kept)] if kept else A["aln"][:0]
                of[f].append((sel, counts, d_orig))
    except BaseException:
        for b in bufs:
            b.free()
        raise
    return CopySelections(bufs, of, summary, (sa, so, sl))


def select_copies(eng, runs, A, lo: int, idents, seeds, fracs) -> CopySelections:
    """smc_select_alignments_copies: the philox selections of the B copies `runs` of one run (RunOnDevices of equal n_aln whose records
    stand at a constant stride - _SpikedCopies.runs - or are the same array; A: the run's counts) at every fraction of `fracs`, copy c
    drawn with seeds[c] -> CopySelections.  Every selection is what select_run(eng, runs[c], A, lo, idents=idents, frac=fracs[f],
    seed=seeds[c]) gives; one call and ONE download (the summaries) in place of B x F of each."""
    from .engine import DevBuf
    B, F = len(runs), len(fracs)
    if B < 1 or F < 1 or B * F > SEL_MAX_SELECTIONS or len(seeds) != B:
        raise ValueError("select_copies: %d copies (%d seeds) x %d fractions; 1 .. %d selections" % (B, len(seeds), F, SEL_MAX_SELECTIONS))
    n, base, stride = _copies_at_one_stride("select_copies", runs)
    nl = int(A["nl"])
    idents = np.ascontiguousarray(idents, np.uint64)[:int(A["n_bc"])]
    seeds = np.array([int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds], np.uint64)
    fr = np.ascontiguousarray(fracs, np.float64)
    d_id = DevBuf(eng, 8 * max(1, len(idents)) + 256).upload(idents if len(idents) else np.zeros(1, np.uint64))

    def launch(*outs):
        _lib.check(eng.L.smc_select_alignments_copies(eng.ctx, base, stride, B, n, None, nl, int(lo), d_id.data_ptr(), len(idents),
                                                      seeds.ctypes.data, fr.ctypes.data, F, *outs, ctypes.c_void_p(0)),
                   "smc_select_alignments_copies")
    try:
        return _copy_selections(eng, runs, A, F, launch)
    finally:
        d_id.free()


def select_copies_reads(eng, runs, A, lo: int, d_masks, n_words: int, copy_stride_words: int, n_masks: int) -> CopySelections:
    """smc_select_alignments_reads_copies: the READ-level selections of the B copies `runs` (as select_copies takes them) under n_masks
    keep masks each, already in HBM: mask (c, m) at d_masks + 4 x (c x copy_stride_words + m x n_words) bytes, a bit per run-wide
    read-name id (ReadGroups.masks' layout; a copy stride of 0: one set for all) -> CopySelections, of[m][c].  Every selection is what
    select_run(eng, runs[c], A, lo, level="read", d_mask=that mask) gives, ids renumbered; one call and ONE download."""
    B, M = len(runs), int(n_masks)
    if B < 1 or M < 1 or B * M > SEL_MAX_SELECTIONS:
        raise ValueError("select_copies_reads: %d copies x %d masks; 1 .. %d selections" % (B, M, SEL_MAX_SELECTIONS))
    n, base, stride = _copies_at_one_stride("select_copies_reads", runs)
    nl = int(A["nl"])

    def launch(*outs):
        _lib.check(eng.L.smc_select_alignments_reads_copies(eng.ctx, base, stride, B, n, None, nl, int(lo), int(A["n_bc"]), int(A["n_pair"]),
                                                            int(d_masks), int(n_words), int(copy_stride_words), M, int(A["n_pair"]), *outs,
                                                            ctypes.c_void_p(0)),
                   "smc_select_alignments_reads_copies")
    return _copy_selections(eng, runs, A, M, launch)


# ---- in-run dilution of listed variants (--dsAF): tools.ds_allele_fraction's drop of the barcodes that carry a listed allele
AF_DOMAIN = 0x64734146         # counter word 2 of the barcode draw ("dsAF": tools.ds_allele_fraction.philox_word0)
AF_MAX_INS = 255               # SMC_AF_MAX_INS: inserted letters of a listed insertion
AF_RUN_LOCI = 512              # listed variants of one chromosome within this many positions share a decoded run of the pre-pass
_AF_TIMES = {"decode": 0.0, "upload": 0.0, "kernel + download": 0.0, "barcodes of the file": 0.0}   # seconds per stage of the last ds_af_sets / ds_af_rules


def af_run_variants(variants, chrom: str, lo: int, fasta):
    """The listed variants (tools.ds_allele_fraction.Variant, all on `chrom`) of the run that starts at 0-based `lo` as
    smc_allele_carriers takes them -> (abi.AF_VARIANT_DTYPE array, the pool of inserted letters).  A deletion whose deleted letters
    are not the reference's is a key no read shows (the caller writes the reference's letters into the key, smCounter.py:394-396)."""
    from .tools import ds_allele_fraction as af
    var = np.zeros(len(variants), abi.AF_VARIANT_DTYPE)
    pool = bytearray()
    for k, v in enumerate(variants):
        var[k]["locus"] = v.pos - 1 - lo
        kind = v.kind
        if kind == af.SNV:
            letter, ln = v.alt, 0
        elif kind == af.INS:
            letter, ln = v.ref, len(v.alt) - 1
            var[k]["ins_off"] = len(pool)
            pool += v.alt[1:].encode()
        else:
            letter, ln = v.alt, len(v.ref) - 1
            if fasta.fetch(chrom, v.pos, v.pos + ln).upper() != v.ref[1:]:
                kind = af.NONE
        var[k]["kind"], var[k]["letter"], var[k]["len"] = kind, ord(letter), ln
    return var, np.frombuffer(bytes(pool) or b"\0", np.uint8).copy()


def _listed_spans(variants, order):
    """Listed variants cut into the spans that are decoded as one run each: from the first not yet taken (`order`: the indexes into
    `variants` by chromosome and position) those of its chromosome less than AF_RUN_LOCI positions on -> a generator of (chrom, lo, hi,
    the span's indexes).  The caller answers each with send(n), the variants its run holds - one cut short: the rest starts the next."""
    i = 0
    while i < len(order):
        v0, j = variants[order[i]], i
        while j + 1 < len(order) and variants[order[j + 1]].chrom == v0.chrom and variants[order[j + 1]].pos - v0.pos < AF_RUN_LOCI:
            j += 1
        i += yield v0.chrom, v0.pos - 1, variants[order[j]].pos, order[i:j + 1]
        yield                                          # (what send() returns; the loop's next step resumes here)


def _set_spans(variants, sets, order):
    """_listed_spans for phase sets (--spikeScanMnv): a set is never split over two decoded runs.  `order`: the indexes into `sets` by
    chromosome and leader position; from the first set not yet taken those of its chromosome whose LAST member stands less than
    AF_RUN_LOCI positions behind that set's leader -> a generator of (chrom, lo, hi, the span's set indexes), hi the last member's
    position.  The caller answers each with send(n), the sets its run holds whole (sets_inside) - one cut short: the rest, whole
    sets, starts the next."""
    first = lambda i: variants[sets[i].members[0]].pos
    last = lambda i: max(variants[k].pos for k in sets[i].members)
    i = 0
    while i < len(order):
        c0, p0, j = sets[order[i]].chrom, first(order[i]), i
        while j + 1 < len(order) and sets[order[j + 1]].chrom == c0 and last(order[j + 1]) - p0 < AF_RUN_LOCI:
            j += 1
        i += yield c0, p0 - 1, max(last(k) for k in order[i:j + 1]), order[i:j + 1]
        yield                                          # (what send() returns; the loop's next step resumes here)


def sets_inside(variants, sets, span, lo: int, nl: int):
    """The leading sets of `span` (_set_spans') that a run of `nl` loci from 0-based `lo` holds WHOLE: it ends in front of the first
    set with a member beyond the run - that set and everything behind it is deferred, so the sets are handed out in order."""
    out = []
    for i in span:
        if any(variants[k].pos - 1 - lo >= nl for k in sets[i].members):
            break
        out.append(i)
    return out


def allele_carriers_run(eng, up: RunOnDevice, A, lo: int, var: np.ndarray, ins: np.ndarray, counts: bool = False):
    """smc_allele_carriers over the run `up` (A: its counts) -> (covers, carries: bool [n_var, n_bc] by run-wide barcode id; the
    (reads, alt) counters uint32 [n_var, n_bc, 2] when `counts`, else None)."""
    from .engine import DevBuf
    n_var, n_bc = len(var), int(A["n_bc"])
    nw = 2 * ((n_bc + 63) // 64)
    if not n_var or not n_bc:
        z = np.zeros((n_var, n_bc), bool)
        return z, z.copy(), (np.zeros((n_var, n_bc, 2), np.uint32) if counts else None)
    var = np.ascontiguousarray(var, abi.AF_VARIANT_DTYPE)
    d_var = DevBuf(eng, var.nbytes + 256).upload(var.view(np.uint8).reshape(-1))
    d_ins = DevBuf(eng, len(ins) + 256).upload(np.ascontiguousarray(ins, np.uint8))
    d_bits = DevBuf(eng, 2 * 4 * nw * n_var + 256)
    d_cnt = DevBuf(eng, 8 * n_bc * n_var + 256) if counts else None
    try:
        _lib.check(eng.L.smc_allele_carriers(eng.ctx, up.aln.data_ptr(), up.n_aln, up.cig.data_ptr(), up.bq.data_ptr(), up.loc.data_ptr(),
                                             int(A["nl"]), int(lo), n_bc, d_var.data_ptr(), var.ctypes.data, n_var, d_ins.data_ptr(), len(ins),
                                             d_bits.data_ptr(), d_bits.data_ptr() + 4 * nw * n_var,
                                             d_cnt.data_ptr() if counts else None, ctypes.c_void_p(0)), "smc_allele_carriers")
        bits = d_bits.download(np.uint32, 2 * nw * n_var)            # (a copy on the default stream: behind the kernels)
        cnt = d_cnt.download(np.uint32, 2 * n_bc * n_var).reshape(n_var, n_bc, 2) if counts else None
    finally:
        for b in (d_var, d_ins, d_bits, d_cnt):
            if b is not None:
                b.free()
    b = np.unpackbits(bits.view(np.uint8), bitorder="little").reshape(2, n_var, 32 * nw)[:, :, :n_bc].astype(bool)
    return b[0], b[1], cnt


def ds_af_sets(path: str, fasta, variants, params, eng, nthreads: int = 0, max_reads: int = 128_000_000, keep: list = None,
               keep_bytes: int = None):
    """The pre-pass of --dsAF: only the runs around the listed loci are decoded (variants of one chromosome within AF_RUN_LOCI
    positions share one), uploaded and put through smc_allele_carriers; the runs' bits become file-wide identities (FNV-1a of the
    barcode text) -> (covers, carries): per variant, in the order given, the uint64 identities of the barcodes that cover / carry it.
    `keep` (--dsAFReps): a list that gets an AfRun per run - decoded and in HBM still, each with a decoder handle of its own (the
    handle holds the run's records: allele keys, barcode texts), while their host arrays stay within `keep_bytes`; a run beyond
    that is listed without its arrays and decoded again by the replicate stage."""
    import time
    nthreads = nthreads or bamio.host_threads()
    order = sorted(range(len(variants)), key=lambda k: (variants[k].chrom, variants[k].pos))
    covers, carries = [None] * len(variants), [None] * len(variants)
    for k in _AF_TIMES:
        _AF_TIMES[k] = 0.0
    bam = bamio.NativeBam(path)
    try:
        spans = _listed_spans(variants, order)
        for chrom, lo, hi, span in spans:
            t0 = time.perf_counter()
            own = bamio.NativeBam(path) if keep is not None else None
            A = (own or bam).alignments_run(chrom, lo, hi, max_reads, params, nthreads)
            t1 = time.perf_counter()
            nl = int(A["nl"])
            if nl < 1:
                raise bamio.BamError("--dsAF: the run %s:%d-%d of the pre-pass could not be decoded" % (chrom, lo + 1, hi))
            group = [k for k in span if variants[k].pos - 1 - lo < nl]
            var, ins = af_run_variants([variants[k] for k in group], chrom, lo, fasta)
            run_ref = fasta.fetch(chrom, lo, lo + nl).upper()
            up = upload_run(eng, A, run_ref)
            t2 = time.perf_counter()
            held = False
            try:
                cov, car, _ = allele_carriers_run(eng, up, A, lo, var, ins)
                idents = (own or bam).barcode_idents(A["n_bc"])
                if keep is not None:
                    size = sum(int(A[x].nbytes) for x in ("aln", "cig", "bq", "loc"))
                    held = size + sum(r.nbytes for r in keep) <= (AF_KEEP_BYTES if keep_bytes is None else keep_bytes)
                    keep.append(AfRun(chrom, lo, hi, list(group), nl, size if held else 0, own if held else None, A if held else None,
                                      up if held else None, run_ref if held else None, idents if held else None))
            finally:
                if not held:
                    up.free()
                    if own is not None:
                        own.close()
            for r, k in enumerate(group):
                covers[k], carries[k] = idents[cov[r][:len(idents)]], idents[car[r][:len(idents)]]
            t3 = time.perf_counter()
            _AF_TIMES["decode"] += t1 - t0; _AF_TIMES["upload"] += t2 - t1; _AF_TIMES["kernel + download"] += t3 - t2
            spans.send(len(group))
    finally:
        bam.close()
    return covers, carries


def ds_af_rules(path: str, fasta, variants, targets, params_list, seed: int, eng, nthreads: int = 0, keep: dict = None, depth: dict = None):
    """DsRules of --dsAF: one per target allele fraction, barcode level, a dropped-identity set (tools.ds_allele_fraction's steps 2-4
    over the pre-pass's sets) -> (rules, titrate()'s result: per target the dropped identities and per variant N, V, a, k, N', V').
    ValueError: two barcode texts of the file share an identity.  `keep` (--dsAFReps): a dict that gets what the replicate stage
    starts from - "runs" (ds_af_sets' kept runs), "covers" and "carries".  `depth` (--dsAFDepth): a dict with "fracs" and "params" (of
    the T x F cells, targets outer); it gets "rules" (a DsRule per cell over one AfCellTable in HBM: close_rules frees it) and
    "counts", uint32 [V, T, F, 2] = the achieved (N', V') of every cell (smc_af_depth_counts)."""
    import time
    from .tools import ds_allele_fraction as af
    t0 = time.perf_counter()
    af.unique_idents(bamio.placed_barcodes(path), path)
    t1 = time.perf_counter()
    runs = [] if keep is not None else None
    try:
        covers, carries = ds_af_sets(path, fasta, variants, params_list[0] if params_list else None, eng, nthreads, keep=runs)
    except BaseException:
        free_af_runs(runs)
        raise
    if keep is not None:
        keep.update(runs=runs, covers=covers, carries=carries)
    _AF_TIMES["barcodes of the file"] = t1 - t0
    res = af.titrate(covers, carries, targets, seed)
    rules = [DsRule(1.0, P, seed=int(seed), af=float(t), dropped_idents=r["dropped"]) for t, P, r in zip(targets, params_list, res)]
    if depth is not None:
        from . import dsaf
        fracs = list(depth["fracs"])
        idents, thr = dsaf.carrier_table(carries, [[row["thr"] for row in r["rows"]] for r in res])
        table = AfCellTable(eng, idents, thr, [int(seed) & 0xFFFFFFFFFFFFFFFF], [frac_threshold(f) for f in fracs])
        try:
            depth["counts"] = table.counts(covers, carries)[:, 0]
            depth["rules"] = [DsRule(float(f), depth["params"][t * len(fracs) + k], seed=int(seed), af=float(targets[t]),
                                     dropped_idents=res[t]["dropped"], bc_thr=frac_threshold(f), depth=table, cell=t * len(fracs) + k)
                              for t in range(len(targets)) for k, f in enumerate(fracs)]
        except BaseException:
            free_af_runs(runs)
            table.free()
            raise
    return rules, res


# ---- in-silico spike-ins (--spikeAF): tools.spike_variants' rewrite of whole barcodes' bases, on the run's arrays in HBM
SPIKE_DOMAIN = 0x73704146      # counter word 2 of the draw ("spAF": tools.spike_variants.draw, k_spike.inc: SPK_DOMAIN)
SPIKE_MAX_TARGETS = 32


class SpikeSet(object):
    """The listed SNVs of --spikeAF by chromosome, ascending by position, as smc_spike_alleles takes them (without thresholds).  With
    phase sets (tools.spike_variants.PhasedVariants: --spikePhase) every record's `lead` says how far back its set's leader stands;
    lead_pos[k]: the leader's 1-based position of variant k of the list given - counter word 3 of its draw, its own without sets."""

    def __init__(self, variants, indels: bool = False):
        from .tools import ds_allele_fraction as af
        from .tools import spike_variants as sv
        self.lead_pos = sv.leaders(variants)
        self.variants = list(variants)
        # (--spikeIndels) a list that holds an insertion or a deletion: the records are smc_spike_indels' (with --spikeIndelPhase their
        # `lead` too), ins[chrom] the pool of inserted letters
        # (--spikeIndelReps, --spikeIndelDepth: `indels` - smc_spike_indels' records whatever the list holds)
        self.indels = bool(indels) or any(v.kind != af.SNV for v in self.variants)
        self.by_chrom, self.ins = {}, {}
        for c in sorted({v.chrom for v in self.variants}):
            order = sorted((k for k, v in enumerate(self.variants) if v.chrom == c), key=lambda k: self.variants[k].pos)
            # (the leader has the set's smallest position: it stands in front, on the same chromosome; `lead` is a 16-bit field of
            # both records)
            at = {self.variants[k].pos: j for j, k in enumerate(order)}
            lead = [j - at[self.lead_pos[k]] for j, k in enumerate(order)]
            far = next((j for j, x in enumerate(lead) if x > 0xFFFF), None)
            if far is not None:
                raise ValueError("%s:%d: its phase set's leader stands %d records in front, beyond the field's 65535" %
                                 (c, self.variants[order[far]].pos, lead[far]))
            if self.indels:
                var, self.ins[c], _ = spike_indel_variants([self.variants[k] for k in order], 0)
            else:
                var = np.zeros(len(order), abi.SPIKE_VARIANT_DTYPE)
                for j, k in enumerate(order):
                    v = self.variants[k]
                    var[j]["pos0"], var[j]["ref"], var[j]["alt"] = v.pos - 1, ord(v.ref), ord(v.alt)
            var["lead"] = lead
            self.by_chrom[c] = (var, order)

    def chrom_variants(self, chrom: str, t: float):
        """-> (the chromosome's records at the threshold of target t, the index of each in the list given)."""
        from .tools import spike_variants as sv
        var, order = self.by_chrom.get(chrom, (np.zeros(0, abi.SPIKE_INDEL_VARIANT_DTYPE if self.indels else abi.SPIKE_VARIANT_DTYPE), []))
        var = var.copy()
        var["thr"] = sv.threshold(t)
        return var, order

    def run_variants(self, chrom: str, A, t: float):
        """The chromosome's records when an alignment of run `A` may span one of them (a position between the run's smallest start and
        its largest end), else none: that run is built as it is."""
        var, _ = self.chrom_variants(chrom, t)
        if not len(var) or not len(A["aln"]):
            return var[:0]
        lo, hi = int(A["aln"]["pos"].min()), int(A["aln"]["end"].max())
        return var if bool(((var["pos0"] >= lo) & (var["pos0"] < hi)).any()) else var[:0]


def _spike_inputs(eng, who: str, up: RunOnDevice, A, var, dtype, idents, nm, n_indel, copies=None):
    """What the four rewrite wrappers start with: the records as `dtype` and the identities of the run's barcodes, both contiguous, and
    these two, NM and the indel lengths per alignment in HBM -> (var, idents, the four DevBufs: free them).  ValueError naming `who`:
    NM or the indel lengths of fewer alignments than the run's or, with copies = (seeds, thresholds), not one threshold per seed."""
    n = up.n_aln
    if len(nm) < n or len(n_indel) < n or (copies is not None and len(copies[1]) != len(copies[0])):
        raise ValueError("%s: %d alignments, NM of %d" % (who, n, len(nm)) +
                         ("; %d seeds, %d thresholds" % (len(copies[0]), len(copies[1])) if copies is not None else ""))
    var = np.ascontiguousarray(var, dtype)
    idents = np.ascontiguousarray(idents, np.uint64)[:int(A["n_bc"])]
    return var, idents, [_up8(eng, a) for a in (var, idents, np.ascontiguousarray(nm, np.int32), np.ascontiguousarray(n_indel, np.int32))]


def spike_run(eng, up: RunOnDevice, A, var: np.ndarray, idents, seed: int, mismatch_thr: float, nm, n_indel):
    """smc_spike_alleles over the run `up` (A: its host arrays) -> (RunOnDevice whose aln and bq are the spiked copies - cig, loc and
    ref are the run's own: free the two copies only -, uint32 [n_var, 2]: records rewritten / NM increments per variant)."""
    from .engine import DevBuf
    n, n_pairs, n_var = up.n_aln, len(A["bq"]) // 2, len(var)
    var, idents, tmp = _spike_inputs(eng, "spike_run", up, A, var, abi.SPIKE_VARIANT_DTYPE, idents, nm, n_indel)
    tmp.append(DevBuf(eng, 8 * max(1, n_var) + 256))
    d_aln, d_bq = DevBuf(eng, 36 * max(1, n) + 256), DevBuf(eng, 2 * max(1, n_pairs) + 256)
    try:
        _lib.check(eng.L.smc_spike_alleles(eng.ctx, up.aln.data_ptr(), n, up.cig.data_ptr(), up.bq.data_ptr(), n_pairs, tmp[0].data_ptr(),
                                           var.ctypes.data, n_var, tmp[1].data_ptr(), len(idents), ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF),
                                           float(mismatch_thr), tmp[2].data_ptr(), tmp[3].data_ptr(), d_aln.data_ptr(), d_bq.data_ptr(),
                                           tmp[4].data_ptr(), ctypes.c_void_p(0)), "smc_spike_alleles")
        stats = tmp[4].download(np.uint32, 2 * n_var).reshape(n_var, 2) if n_var else np.zeros((0, 2), np.uint32)   # (behind the kernel)
    except BaseException:
        d_aln.free(); d_bq.free()
        raise
    finally:
        for b in tmp:
            b.free()
    return RunOnDevice(d_aln, up.cig, d_bq, up.loc, up.ref, n, up.loc_host), stats


def spike_indel_variants(variants, thr):
    """Listed variants of one chromosome (tools.ds_allele_fraction.Variant: SNVs, insertions, deletions) as smc_spike_indels takes
    them, ascending by position -> (abi.SPIKE_INDEL_VARIANT_DTYPE array, the pool of inserted letters, the index of each record in the
    list given).  `thr`: one threshold for all, or one per variant of the list given."""
    from .tools import ds_allele_fraction as af
    order = sorted(range(len(variants)), key=lambda k: variants[k].pos)
    var = np.zeros(len(order), abi.SPIKE_INDEL_VARIANT_DTYPE)
    pool = bytearray()
    for j, k in enumerate(order):
        v = variants[k]
        var[j]["pos0"], var[j]["kind"], var[j]["thr"] = v.pos - 1, v.kind, thr if isinstance(thr, int) else thr[k]
        if v.kind == af.SNV:
            var[j]["ref"], var[j]["alt"] = ord(v.ref), ord(v.alt)
        else:
            var[j]["ref"] = var[j]["alt"] = ord(v.ref[0])
            var[j]["len"] = len(v.alt) - 1 if v.kind == af.INS else len(v.ref) - 1
            if v.kind == af.INS:
                var[j]["ins_off"] = len(pool)
                pool += v.alt[1:].encode()
    return var, np.frombuffer(bytes(pool) or b"\0", np.uint8).copy(), order


def spike_indel_caps(A, var):
    """Upper bounds of the pools of a copy smc_spike_indels writes, from the run's host arrays: for every alignment that spans a listed
    insertion / deletion its l_seq + the inserted letters it spans, and its n_cig + 2 per such variant -> (cap_pairs, cap_cig)."""
    aln = A["aln"]
    indel = var[var["kind"] != 0]
    n_pairs, n_cig = len(A["bq"]) // 2, len(A["cig"])
    if not len(indel) or not len(aln):
        return n_pairs, n_cig
    first, last = np.searchsorted(indel["pos0"], aln["pos"], "left"), np.searchsorted(indel["pos0"], aln["end"], "left")
    s = np.concatenate([[0], np.cumsum(np.where(indel["kind"] == 1, indel["len"], 0).astype(np.int64))])
    hit = last > first
    return (n_pairs + int((aln["l_seq"].astype(np.int64) + s[last] - s[first])[hit].sum()),
            n_cig + int((aln["n_cig"].astype(np.int64) + 2 * (last - first))[hit].sum()))


def spike_indel_limits(A, var):
    """The first alignment of run `A` (host arrays) at which the 16-bit limits of smc_spike_indels' walk COULD bind - it spans k listed
    insertions / deletions with s inserted letters in all and n_cig + 2 k > 65535 or l_seq + s > 65535 -, or None.  Without such a
    record whether a record takes a listed variant depends on no other variant's draw (--spikeIndelReps counts on that)."""
    aln = A["aln"]
    indel = var[var["kind"] != 0]
    if not len(indel) or not len(aln):
        return None
    first, last = np.searchsorted(indel["pos0"], aln["pos"], "left"), np.searchsorted(indel["pos0"], aln["end"], "left")
    s = np.concatenate([[0], np.cumsum(np.where(indel["kind"] == 1, indel["len"], 0).astype(np.int64))])
    bad = np.flatnonzero((aln["n_cig"].astype(np.int64) + 2 * (last - first) > 65535) | (aln["l_seq"].astype(np.int64) + s[last] - s[first] > 65535))
    return int(bad[0]) if len(bad) else None


def _refuse_indel_limits(A, var, flag: str, chrom: str) -> None:
    """ValueError naming `flag`, before anything is spiked: run `A` of `chrom` has a record at which spike_indel_limits' limits could bind."""
    bad = spike_indel_limits(A, var)
    if bad is not None:
        a = A["aln"][bad]
        raise ValueError("%s: the record at %s:%d (l_seq %d, %d CIGAR operations) spans listed indels that could take l_seq or the CIGAR "
                         "beyond 65535: whether it takes one would depend on the draws of the others" %
                         (flag, chrom, int(a["pos"]) + 1, int(a["l_seq"]), int(a["n_cig"])))


def spike_indel_touch(eng, up: RunOnDevice, A, var: np.ndarray) -> np.ndarray:
    """smc_spike_indel_touch over the run `up` (A: its host arrays) -> uint32 [n_var, n_bc]: per record of `var` and run-wide barcode
    id the records that take the insertion / deletion when the barcode is spiked (0 throughout for an SNV)."""
    from .engine import DevBuf
    n_var, n_bc = len(var), int(A["n_bc"])
    if not n_var or not n_bc:
        return np.zeros((n_var, n_bc), np.uint32)
    var = np.ascontiguousarray(var, abi.SPIKE_INDEL_VARIANT_DTYPE)
    d_var, d_out = DevBuf(eng, var.nbytes + 256).upload(var.view(np.uint8).reshape(-1)), DevBuf(eng, 4 * n_var * n_bc + 256)
    try:
        _lib.check(eng.L.smc_spike_indel_touch(eng.ctx, up.aln.data_ptr(), up.n_aln, up.cig.data_ptr(), len(A["cig"]), len(A["bq"]) // 2,
                                               d_var.data_ptr(), var.ctypes.data, n_var, n_bc, d_out.data_ptr(), ctypes.c_void_p(0)),
                   "smc_spike_indel_touch")
        return d_out.download(np.uint32, n_var * n_bc).reshape(n_var, n_bc)      # (the default stream: behind the kernel)
    finally:
        d_var.free(); d_out.free()


def spike_indel_run(eng, up: RunOnDevice, A, var: np.ndarray, ins: np.ndarray, idents, seed: int, mismatch_thr: float, nm, n_indel,
                    caps=None, mism: bool = True):
    """smc_spike_indels over the run `up` (A: its host arrays) -> (RunOnDevice whose aln, cig and bq are the spiked copies - loc and
    ref are the run's own: free the three copies only -, uint32 [n_var, 2] statistics, uint64 [3] totals, NM' and n_indel' per
    alignment).  `caps`: (cap_pairs, cap_cig), spike_indel_caps' bounds without it.  SmcError when the copy did not fit them."""
    from .engine import DevBuf
    n, n_pairs, n_cw, n_var = up.n_aln, len(A["bq"]) // 2, len(A["cig"]), len(var)
    var, idents, tmp = _spike_inputs(eng, "spike_indel_run", up, A, var, abi.SPIKE_INDEL_VARIANT_DTYPE, idents, nm, n_indel)
    cap_pairs, cap_cig = caps if caps is not None else spike_indel_caps(A, var)
    ins = np.ascontiguousarray(ins, np.uint8)
    tmp += [_up8(eng, ins), DevBuf(eng, 8 * max(1, n_var) + 256), DevBuf(eng, 24 + 256), DevBuf(eng, 4 * max(1, n) + 256),
            DevBuf(eng, 4 * max(1, n) + 256)]
    d_aln, d_bq, d_cig = DevBuf(eng, 36 * max(1, n) + 256), DevBuf(eng, 2 * max(1, cap_pairs) + 256), DevBuf(eng, 4 * max(1, cap_cig) + 256)
    try:
        _lib.check(eng.L.smc_spike_indels(eng.ctx, up.aln.data_ptr(), n, up.cig.data_ptr(), n_cw, up.bq.data_ptr(), n_pairs, tmp[0].data_ptr(),
                                          var.ctypes.data, n_var, tmp[4].data_ptr(), len(ins), tmp[1].data_ptr(), len(idents),
                                          ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), float(mismatch_thr), tmp[2].data_ptr(),
                                          tmp[3].data_ptr(), cap_pairs, cap_cig, d_aln.data_ptr(), d_bq.data_ptr(), d_cig.data_ptr(),
                                          tmp[7].data_ptr(), tmp[8].data_ptr(), tmp[5].data_ptr(), tmp[6].data_ptr(), ctypes.c_void_p(0)),
                   "smc_spike_indels")
        stats = tmp[5].download(np.uint32, 2 * n_var).reshape(n_var, 2) if n_var else np.zeros((0, 2), np.uint32)   # (behind the kernels)
        totals = tmp[6].download(np.uint64, 3)
        nm_out, n_indel_out = (tmp[7].download(np.int32, n), tmp[8].download(np.int32, n)) if mism else (None, None)
        if caps is None and int(totals[2]):
            raise _lib.SmcError("smc_spike_indels: the copy needs %d pairs / %d CIGAR words, more than the bounds %d / %d" %
                                (int(totals[0]), int(totals[1]), cap_pairs, cap_cig))
    except BaseException:
        d_aln.free(); d_bq.free(); d_cig.free()
        raise
    finally:
        for b in tmp:
            b.free()
    return RunOnDevice(d_aln, d_cig, d_bq, up.loc, up.ref, n, up.loc_host, pairs_used=int(totals[0])), stats, totals, nm_out, n_indel_out


def spike_indel_reads(A, v, hit) -> int:
    """The records of run `A` (host arrays) that the listed insertion / deletion `v` rewrites when the barcodes `hit` (bool by run-wide
    barcode id) are spiked: the whole footprint inside one M / = / X operation and inside l_seq, n_cig + 2 and l_seq (+ s) within 16
    bits.  (The limits are taken per variant, not over the variants a record took before: the difference needs a CIGAR of more than
    32,000 operations.)"""
    from .tools import ds_allele_fraction as af
    aln, cig = A["aln"], A["cig"]
    p = v.pos - 1
    n = len(v.alt) - 1 if v.kind == af.INS else len(v.ref) - 1
    fp = 1 if v.kind == af.INS else n + 1
    gid = aln["bc_gid"]
    ok = (aln["pos"] <= p) & (p < aln["end"]) & (gid < len(hit))
    ok[ok] = hit[gid[ok]]
    ok &= (aln["n_cig"].astype(np.int64) + 2 <= 65535) & ((v.kind != af.INS) | (aln["l_seq"].astype(np.int64) + n <= 65535))
    # (a CIGAR of one aligned operation - nearly every record: no walk)
    w0 = cig[np.minimum(aln["cig_off"], max(0, len(cig) - 1))] if len(cig) else np.zeros(len(aln), np.uint32)
    plain = ok & (aln["n_cig"] == 1) & np.isin(w0 & 15, (0, 7, 8))
    d0 = p - aln["pos"].astype(np.int64)
    count = int((plain & (d0 + fp < (w0 >> 4).astype(np.int64)) & (d0 + fp < aln["l_seq"].astype(np.int64))).sum())
    for i in np.flatnonzero(ok & ~plain).tolist():
        a = aln[i]
        x, y = int(a["pos"]), 0
        for w in cig[int(a["cig_off"]):int(a["cig_off"]) + int(a["n_cig"])].tolist():
            op, l = w & 15, w >> 4
            if op in (0, 7, 8):
                if x <= p < x + l:
                    count += p - x + fp < l and y + p - x + fp < int(a["l_seq"])
                    break
                x += l
                y += l
            elif op in (2, 3):
                if x <= p < x + l:
                    break
                x += l
            elif op in (1, 4):
                y += l
    return count


def spike_copy(eng, up: RunOnDevice, A, spikes: SpikeSet, chrom: str, var: np.ndarray, idents, seed: int, mismatch_thr: float, nm, n_indel):
    """The spiked copy of run `up` for the records `var` of `spikes` on `chrom`: spike_run, or spike_indel_run when the set holds an
    insertion or a deletion -> (RunOnDevice, statistics); free the copy with free_spiked."""
    if spikes.indels:
        return spike_indel_run(eng, up, A, var, spikes.ins[chrom], idents, seed, mismatch_thr, nm, n_indel, mism=False)[:2]
    return spike_run(eng, up, A, var, idents, seed, mismatch_thr, nm, n_indel)


def free_spiked(spiked: RunOnDevice, up: RunOnDevice) -> None:
    """The arrays of a spiked copy of `up` that are its own: aln and bq, and the CIGAR pool of a copy smc_spike_indels wrote."""
    spiked.aln.free(); spiked.bq.free()
    if spiked.cig is not up.cig:
        spiked.cig.free()


def _spike_single_counters(eng, up: RunOnDevice, A, lo: int, spikes: SpikeSet, chrom: str, members, var, ins, idents, seed: int, P, nm, n_indel,
                           cov, cnt0, four: bool):
    """The counters the counts calls of the spike family start from, for the variants `members` (indexes into the list `spikes` was
    made of; `var`, `ins`: af_run_variants' records of them; `cov`, `cnt0`: smc_allele_carriers' cover bits and counters of them on
    the run `up`).  `single`: one copy with every barcode spiked at every position of the chromosome's list - thr 2^32 - then the
    `alt` counters on it.  -> (the chromosome's records at that threshold, the index of each in the list, per member the identities
    of the barcodes that cover it, per member uint32 [covering barcodes, 3] = (reads, alt0, single)).  `four`: a fourth column, what
    the rewrite changes: an SNV's single-letter reads - all of which then show ALT -, an indel's eligible records
    (smc_spike_indel_touch)."""
    from .tools import ds_allele_fraction as af
    svar, sorder = spikes.chrom_variants(chrom, 0.5)
    svar["thr"] = 1 << 32
    spiked, _ = spike_copy(eng, up, A, spikes, chrom, svar, idents, seed, P.mismatchThr, nm, n_indel)
    try:
        _, _, cnt_all = allele_carriers_run(eng, spiked, A, lo, var, ins, counts=True)
    finally:
        free_spiked(spiked, up)
    touch = spike_indel_touch(eng, up, A, svar) if four else None
    at_of = {m: n for n, m in enumerate(sorder)}
    covers, counters = [], []
    for r, m in enumerate(members):
        c = cov[r][:len(idents)]
        covers.append(idents[c])
        cols = [cnt0[r, :len(idents), 0][c], cnt0[r, :len(idents), 1][c], cnt_all[r, :len(idents), 1][c]]
        if four:
            cols.append(cols[2] if spikes.variants[m].kind == af.SNV else touch[at_of[m], :len(idents)][c])
        counters.append(np.stack(cols, axis=1).astype(np.uint32))
    return svar, sorder, covers, counters


def copy_allele_key(spiked: RunOnDevice, A, decoder_key):
    """`allele_key` for a copy smc_spike_indels wrote of run `A`: a relocated record's texts come from the copy - smc_bam_allele_key's
    rules (csrc/smc_bam.cpp) over its records and the pairs behind the run's own, downloaded once, when the first such key is asked
    for -, every other record keeps the decoder's answer (its site is a base the rewrite leaves alone or turns into a fixed key)."""
    n_pairs = len(A["bq"]) // 2
    got = {}

    def key(ai, qpos, indel):
        if "aln" not in got:
            got["aln"] = spiked.aln.download(abi.DEV_ALN_DTYPE, spiked.n_aln)
        a = got["aln"][int(ai)]
        so, ls, qpos, indel = int(a["seq_off"]), int(a["l_seq"]), int(qpos), int(indel)
        if so < n_pairs:
            return decoder_key(ai, qpos, indel)
        if "bq" not in got:
            got["bq"] = spiked.bq.download(np.uint8, 2 * (spiked.pairs_used - n_pairs), 2 * n_pairs)
        letters = got["bq"][2 * (so - n_pairs):2 * (so - n_pairs + ls):2]
        if not (0 <= qpos < ls):
            raise bamio.BamError("allele key of alignment %d at query position %d of %d" % (ai, qpos, ls))
        site = chr(letters[qpos])
        if indel > 0:
            return "INS|%s|%s%s" % (site, site, letters[qpos + 1:qpos + 1 + indel].tobytes().decode())
        if indel < 0:
            return "D%d|%s" % (-indel, site)
        return site
    return key


def spike_rules(path: str, fasta, variants, targets, params_list, seed: int, eng, nthreads: int = 0, max_reads: int = 128_000_000,
                keep: dict = None, keep_bytes: int = None, depth: dict = None, phase: dict = None, indel_counters: bool = False,
                rpb: dict = None):
    """DsRules of --spikeAF, one per target, and the pre-pass: only the runs around the listed loci are decoded (as ds_af_sets groups
    them); smc_allele_carriers gives N and V0 of every variant, then per target smc_spike_alleles writes the spiked copy and
    smc_allele_carriers on it gives V1.  The kernel's statistics are checked against the host's restatement of the draws: the records
    rewritten at v are the reads with v's key of the spiked covering barcodes in the spiked copy, and no other barcode's counters move.
    -> (rules, per target dict(target, rows: per variant dict(N, V0, S, READS, V1))).  ValueError: two barcode texts of the file share
    an identity.
    `keep` (--spikeReps): a dict that gets what the replicate stage starts from - "runs": an AfRun per run of the pre-pass, decoded
    and in HBM still (each with a decoder handle of its own and its alignments' (NM, indel length) in `mism`) while their host arrays
    stay within `keep_bytes` (AF_KEEP_BYTES), a run beyond that without its arrays; "covers": per variant the identities of the
    barcodes that cover it; "counters": per variant uint32 [covering barcodes, 3] = (reads, alt0, single) - smc_allele_carriers'
    counters on the run, and its `alt` counter on one copy spiked at threshold 2^32 (every read the rewrite can touch shows ALT
    there, and no other does); "spikes": the SpikeSet.
    `depth` (--spikeDepth: dict with "fracs" and the "params" of the T x F cells, targets outer): it gets "rules", the cells' DsRules,
    and "counts", per variant and cell dict(N, V0, S, READS, V1) - one smc_spike_depth_counts call with this seed over the covers
    and counters above.  Every cell's (N, V0, V1) is also counted a second way - select_run at f over the spiked copy of t (over the
    run itself for V0), then smc_allele_carriers on the selection - and a difference raises RuntimeError.
    `phase` (--spikePhase: dict with "sets", the tools.spike_variants.PhaseSets of two members or more): every member of a set is
    drawn with its leader's position (SpikeSet.lead_pos) in the rewrite, in the host's restatement of the draws and in the counts
    calls.  The dict gets "joint" (per set the identities of the barcodes that cover every member and their counters, spike_joint),
    "counts", per set and target dict(N_ALL, V0_ALL, S_ALL, V1_ALL) from one smc_spike_phase_counts call with this seed, and with
    `depth` "depth_counts", the same per cell from a second call.  (N_ALL, V0_ALL, V1_ALL) of every target is also counted a second
    way - the AND over the members of smc_allele_carriers' cover and carrier bits, on the run and on the spiked copy of that target
    - and a difference raises RuntimeError.
    `indel_counters` (--spikeIndelReps, --spikeIndelDepth): the spike-ins are smc_spike_indels' whatever the list holds, and the
    counters are FOUR per covering barcode, uint32 [covering barcodes, 4] = (reads, alt0, alt1, touch): alt1 the `alt` counter on the
    copy spiked at threshold 2^32 - for an insertion / a deletion alt0 plus the eligible records whose anchor letter is REF's -, touch
    the records the rewrite changes when the barcode is hit - alt1 for an SNV, smc_spike_indel_touch's for an insertion / a deletion.
    The cells' counts then come from smc_spike_indel_counts, and with `phase` (--spikeIndelPhase: the members of a set may be
    insertions and deletions, every record of SpikeSet carries its `lead`) the joint rows hold four counters per member and the joint
    numbers come from smc_spike_indel_phase_counts; the second count is the same AND of smc_allele_carriers' bits, INS / DEL keys
    included.  ValueError, before anything is spiked: a run with a record at which the
    16-bit limits of the rewrite could bind (spike_indel_limits) - the counters would depend on the other variants' draws.
    `rpb` (--spikeRpb: dict with "targets", the reads-per-barcode targets, and the "params" of the T x Rr cells, targets outer; SNV
    lists only): philox_read_rules builds the file-wide table of the UNSPIKED file once; per run of the pre-pass smc_spike_read_bits
    gives a flag byte per record and listed SNV, the first names come from the table at threshold 0 and the covering records of every
    variant become a CSR (spike_rpb_records) - kept in keep["records"] for the replicate stage; one smc_spike_rpb_counts call with
    this seed gives "counts", per variant and cell dict(N, V0, S, READS, V1) over the reads the cell keeps, and "rules" gets the
    cells' DsRules (level "read" over the shared table).  Every cell's (N, V0, V1) is also counted a second way - select_run by
    read mask over the spiked copy of t (over the run itself for V0), then smc_allele_carriers on the selection - and a difference
    raises RuntimeError.  ValueError / BamError: what --dsRpbSampler philox refuses.
    `rpb` with `indel_counters` (--spikeIndelRpb): the list may hold insertions and deletions.  The flag byte per record comes from
    smc_spike_indel_read_bits - bits 1 / 2 / 3 = alt0 / alt1 / touch -, its per-barcode sums must equal the four counters above, and the
    counts come from smc_spike_indel_rpb_counts.  The second count is the same: an indel copy has pools of its own, but its records
    stand in the run's order and number, so the read mask selects the same records and select_run hands on the copy's pools.
    `rpb` with "flag" "--spikePhaseRpb", `indel_counters` and `phase` (--spikePhaseRpb): phase sets on the reads-per-barcode axis.  The
    per-variant counts are drawn with the leaders' positions; the covering records of every (joint barcode, member) become one CSR
    (spike_joint_records, kept in phase["joint_records"]) and one smc_spike_phase_rpb_counts call with this seed gives
    phase["rpb_counts"], per set and cell dict(N_ALL, V0_ALL, S_ALL, V1_ALL) over the reads the cell keeps.  They are counted a second
    way as well: the read selections hand back smc_allele_carriers' cover and carrier bits as identities, and per set and cell the AND
    over the members - on the selection of the spiked copy of t for N_ALL' and V1_ALL', on that of the run itself for V0_ALL' - must
    give the same numbers, else RuntimeError naming set and cell.  The refusals and DsRule.flag name --spikePhaseRpb.
    `rpb` with "fracs" and "flag" "--spikeGrid" (--spikeGrid: SNV lists only; "reps": R or None; "params" of the T x F x Rr cells,
    targets outer, then fractions, then r): a read rule per PAIR (f, r) over the same table (_spike_grid_rules: every replicate's
    thresholds up front in rpb["rep_thr"] [R, F, Rr], the run's own rules from philox_grid_rules); the masks are masks_grid's, the
    counts come from one smc_spike_grid_counts call, "counts" and "rules" run over the T x F x Rr cells; the second count is the same."""
    from .tools import ds_allele_fraction as af
    from .tools import spike_variants as sv
    af.unique_idents(bamio.placed_barcodes(path), path)
    nthreads = nthreads or bamio.host_threads()
    if rpb is not None:
        # (--spikeIndelRpb - `indel_counters` - lifts the indel part; an indel in the list without it is --spikeRpb's to refuse)
        # (--spikePhaseRpb - rpb["flag"], with `indel_counters` - lifts the phase part as well)
        phase_rpb = indel_counters and rpb.get("flag") == "--spikePhaseRpb"
        grid = rpb.get("fracs") is not None
        if grid and (depth is not None or phase is not None or indel_counters or any(v.kind != af.SNV for v in variants)):
            raise ValueError("--spikeGrid: phase sets or indel spike-ins on the grid are not built")
        if depth is not None or (phase is not None and not phase_rpb) or (not indel_counters and any(v.kind != af.SNV for v in variants)):
            raise ValueError("--spikeRpb: cells of barcode depths, phase sets or indel spike-ins are not built")
        # (the file-wide table of the UNSPIKED file serves every cell and replicate: spiking changes no name, barcode or record count -
        # an indel rewrite changes a record's length and CIGAR only)
        read_rules = philox_read_rules(path, list(rpb["targets"]), [params_list[0]] * len(rpb["targets"]), seed, eng, nthreads=nthreads,
                                       flag=rpb.get("flag") or ("--spikeIndelRpb" if indel_counters else "--spikeRpb"))
        try:
            if grid:
                read_rules = _spike_grid_rules(path, rpb, params_list[0], seed, read_rules)
            return _spike_rules(path=path, fasta=fasta, variants=variants, targets=targets, params_list=params_list, seed=seed, eng=eng,
                                nthreads=nthreads, max_reads=max_reads, keep=keep, keep_bytes=keep_bytes, depth=depth, phase=phase,
                                indel_counters=indel_counters, rpb=rpb, read_rules=read_rules)
        except BaseException:
            close_rules(read_rules)
            raise
    return _spike_rules(path=path, fasta=fasta, variants=variants, targets=targets, params_list=params_list, seed=seed, eng=eng,
                        nthreads=nthreads, max_reads=max_reads, keep=keep, keep_bytes=keep_bytes, depth=depth, phase=phase,
                        indel_counters=indel_counters, rpb=None, read_rules=None)


def _spike_grid_rules(path, rpb, P, seed, read_rules):
    """(--spikeGrid) The F x Rr read rules of the grid (fractions outer), over the table of philox_read_rules' `read_rules`.  First the
    thresholds of EVERY replicate (rpb["reps"], None: the run alone) from one counts_frac_seeds launch - a (replicate, fraction) that
    keeps no barcode of two or more names ends the run here, before any file is written -, kept in rpb["rep_thr"] / rpb["rep_prob"]
    for the replicate stage; then philox_grid_rules' rules of the run's own seed, whose thresholds must be replicate 0's.
    rpb["file_names"]: the file's distinct read names (the budget page's denominator)."""
    from . import dsaf
    groups = read_rules[0].groups
    rpb["rep_thr"], rpb["rep_prob"] = grid_read_thresholds(groups, dsaf.rep_seeds(seed, rpb.get("reps") or 1), rpb["fracs"], rpb["targets"])
    cells = [(f, r) for f in rpb["fracs"] for r in rpb["targets"]]
    rules = philox_grid_rules(path, cells, [P] * len(cells), seed, groups)
    if [int(r.thr) for r in rules] != [int(x) for x in rpb["rep_thr"][0].reshape(-1)]:
        raise RuntimeError("--spikeGrid: the thresholds of replicate 0 are not the run's own cells'")
    rpb["file_names"] = int(groups.counts["names"])
    return rules


def _spike_rules(*, path, fasta, variants, targets, params_list, seed, eng, nthreads, max_reads, keep, keep_bytes, depth, phase,
                 indel_counters, rpb, read_rules):
    """spike_rules' body; `read_rules` (--spikeRpb): philox_read_rules' rules of the reads-per-barcode targets, whose table the caller
    closes when this raises."""
    from .tools import ds_allele_fraction as af
    from .tools import spike_variants as sv
    spikes = SpikeSet(variants, indels=indel_counters)
    spikes.rpb_flag = (rpb or {}).get("flag")          # (--spikePhaseRpb: the flag DsRule.flag names for the cells)
    rpb_flag = (rpb or {}).get("flag") or ("--spikeIndelRpb" if indel_counters else "--spikeRpb")
    grid = rpb is not None and rpb.get("fracs") is not None      # (--spikeGrid: a read rule per pair (f, r), fractions outer)
    cell_text = (lambda r: "fraction %g x target %g" % (read_rules[r].frac, read_rules[r].target)) if grid else \
        (lambda r: "target %g" % rpb["targets"][r])
    P = params_list[0]
    rows = [[None] * len(variants) for _ in targets]
    psets = list(phase["sets"]) if phase is not None else []
    want_counters = keep is not None or depth is not None or bool(psets) or rpb is not None
    records = [None] * len(variants)                   # (--spikeRpb) per variant spike_rpb_records' CSR of its covering records
    second_rpb = {}                                    # (--spikeRpb) (variant, target index, r index) -> [N', V0', V1'] counted on selections
    bits = {}                        # (--spikePhase) variant -> (identities that cover it, that carry it before, per target after)
    rbits = {}                       # (--spikePhaseRpb) (variant, r index) -> [identities that carry it before on the selection at r, per target
    #                                  (identities that cover it, that carry it) on the selection of the spiked copy]
    covers, counters = [None] * len(variants), [None] * len(variants)
    if keep is not None:
        keep.update(runs=[], covers=covers, counters=counters, spikes=spikes)
    fracs = list(depth["fracs"]) if depth is not None else []
    second = {}                      # (--spikeDepth) (variant, target index, fraction index) -> [N', V0', V1'] counted on selections
    order = sorted(range(len(variants)), key=lambda k: (variants[k].chrom, variants[k].pos))
    bam = bamio.NativeBam(path)
    try:
        spans = _listed_spans(variants, order)
        for chrom, lo, hi, span in spans:
            own = bamio.NativeBam(path) if keep is not None else None
            dec = own or bam
            held = False
            up = read_masks = None                     # (--spikeRpb: read_masks, _run_read_masks' of this run while the second count needs them)
            try:
                A = dec.alignments_run(chrom, lo, hi, max_reads, P, nthreads)
                nl = int(A["nl"])
                if nl < 1:
                    raise bamio.BamError("--spikeAF: the run %s:%d-%d of the pre-pass could not be decoded" % (chrom, lo + 1, hi))
                group = [k for k in span if variants[k].pos - 1 - lo < nl]
                var, ins = af_run_variants([variants[k] for k in group], chrom, lo, fasta)
                if indel_counters:
                    _refuse_indel_limits(A, spikes.chrom_variants(chrom, 0.5)[0],
                                         rpb_flag if rpb is not None else "--spikeIndelReps / --spikeIndelDepth", chrom)
                idents = dec.barcode_idents(A["n_bc"])
                nm, n_indel = dec.run_mismatches(len(A["aln"]))
                run_ref = fasta.fetch(chrom, lo, lo + nl).upper()
                up = upload_run(eng, A, run_ref)
                cov, car, cnt0 = allele_carriers_run(eng, up, A, lo, var, ins, counts=want_counters)
                for f, frac in enumerate(fracs):
                    # (V0' of the cells at f: the carriers before spiking among the barcodes the selection keeps)
                    sel, sel_counts, d_orig = select_run(eng, up, A, lo, idents=idents, frac=frac, seed=seed)
                    try:
                        _, car_f, _ = allele_carriers_run(eng, sel, sel_counts, lo, var, ins)
                    finally:
                        sel.free(shared=False); d_orig.free()
                    for r, k in enumerate(group):
                        for t in range(len(targets)):
                            second[(k, t, f)] = [None, int(car_f[r].sum()), None]
                if rpb is not None:
                    p_idents = pair_idents_or_refuse(dec, A, rpb_flag, chrom, lo, nl)
                    read_masks = _run_read_masks(eng, read_rules[0].groups, read_rules, p_idents, chrom, lo, nl)

                def read_selected(run, r):
                    # (the cells' second count: the read selection at r over `run`, then smc_allele_carriers on it -> (N', carriers) per variant)
                    kept = _KeptRun(*select_run(eng, run, A, lo, d_mask=read_masks[0].data_ptr() + 4 * read_masks[1] * r, level="read"), A=A,
                                    key=dec.allele_key, name=dec.barcode_name, idents=lambda n: idents, by_read=True)
                    try:
                        cov_r, car_r, _ = allele_carriers_run(eng, kept.run, kept.counts, lo, var, ins)
                        who = None
                        if psets and rpb is not None:
                            # (--spikePhaseRpb: the bits as identities - a read selection renumbers the kept records' barcode ids by
                            # first kept appearance, so each new id is traced back through the kept records' places in the run)
                            ids = kept.idents()
                            who = [(ids[cov_r[x][:len(ids)]], ids[car_r[x][:len(ids)]]) for x in range(len(group))]
                    finally:
                        kept.free()
                    return cov_r.sum(axis=1), car_r.sum(axis=1), who
                for r in range(len(read_rules or ())):
                    n_r, car_r, who = read_selected(up, r)
                    for x, k in enumerate(group):
                        for t in range(len(targets)):
                            second_rpb[(k, t, r)] = [int(n_r[x]), int(car_r[x]), None]
                        if who is not None:
                            rbits[(k, r)] = [who[x][1], [None] * len(targets)]
                for t, target in enumerate(targets):
                    svar, sorder = spikes.chrom_variants(chrom, target)
                    spiked, stats = spike_copy(eng, up, A, spikes, chrom, svar, idents, seed, P.mismatchThr, nm, n_indel)
                    try:
                        cov1, car1, cnt1 = allele_carriers_run(eng, spiked, A, lo, var, ins, counts=True)
                        for r in range(len(read_rules or ())):
                            n_r, car_r, who = read_selected(spiked, r)
                            for x, k in enumerate(group):
                                if who is not None:
                                    rbits[(k, r)][1][t] = who[x]
                                if second_rpb[(k, t, r)][0] != int(n_r[x]):
                                    raise RuntimeError("%s: %s:%d at %g x %s: the read selection keeps %d covering barcodes of "
                                                       "the run and %d of its spiked copy" % (rpb_flag, variants[k].chrom, variants[k].pos, target,
                                                                                             cell_text(r), second_rpb[(k, t, r)][0], int(n_r[x])))
                                second_rpb[(k, t, r)][2] = int(car_r[x])
                        for f, frac in enumerate(fracs):
                            sel, sel_counts, d_orig = select_run(eng, spiked, A, lo, idents=idents, frac=frac, seed=seed)
                            try:
                                cov_f, car_f, _ = allele_carriers_run(eng, sel, sel_counts, lo, var, ins)
                            finally:
                                sel.free(shared=False); d_orig.free()
                            for r, k in enumerate(group):
                                second[(k, t, f)][0], second[(k, t, f)][2] = int(cov_f[r].sum()), int(car_f[r].sum())
                    finally:
                        free_spiked(spiked, up)
                    for r, k in enumerate(group):
                        v = variants[k]
                        hit = sv.draw(idents, seed, spikes.lead_pos[k]) < np.uint64(sv.threshold(target))
                        if psets:
                            b = bits.setdefault(k, (idents[cov[r][:len(idents)]], idents[car[r][:len(idents)]], [None] * len(targets)))
                            b[2][t] = idents[car1[r][:len(idents)]]
                        reads = int(stats[sorder.index(k), 0])
                        if v.kind == af.SNV:
                            shown = int(cnt1[r, hit[:cnt1.shape[1]], 1].sum())
                        else:
                            # (an insertion / a deletion: the eligible records of the spiked barcodes, restated from the host's arrays -
                            # a read that shows it already, or whose anchor holds another letter, moves the `alt` counters otherwise)
                            shown = spike_indel_reads(A, v, hit)
                        if not np.array_equal(cov1[r], cov[r]) or reads != shown or \
                                bool((car1[r] != car[r])[~hit[:car.shape[1]]].any()):
                            raise RuntimeError("--spikeAF %g: the kernel's statistics at %s:%d (%d records rewritten) do not agree with the "
                                               "host's restatement of the draws" % (target, v.chrom, v.pos, reads))
                        rows[t][k] = dict(N=int(cov[r].sum()), V0=int(car[r].sum()), S=int((hit[:cov.shape[1]] & cov[r]).sum()), READS=reads,
                                          V1=int(car1[r].sum()))
                if want_counters:
                    svar, sorder, covers_g, counters_g = _spike_single_counters(eng, up, A, lo, spikes, chrom, group, var, ins, idents, seed, P,
                                                                                nm, n_indel, cov, cnt0, indel_counters)
                    for r, k in enumerate(group):
                        covers[k], counters[k] = covers_g[r], counters_g[r]
                if rpb is not None:
                    # (a flag byte per record and listed SNV, the first names from the table at threshold 0 - the first mask of a launch
                    # with that one threshold -, then the CSR of every variant's covering records)
                    read_masks[0].free()
                    read_masks = None
                    if indel_counters:
                        # (--spikeIndelRpb: the group's records of the chromosome's list - ascending, as the group is; the inserted
                        # letters stay where the chromosome's pool has them)
                        read_bits = spike_indel_read_bits(eng, up, A, lo, svar[[sorder.index(k) for k in group]], spikes.ins[chrom])
                    else:
                        read_bits = spike_read_bits(eng, up, A, lo, var)
                    first = run_first_names(eng, read_rules[0].groups, p_idents, chrom, lo, nl)
                    shifts = (1, 2, 3) if indel_counters else (1, 2)
                    for r, k in enumerate(group):
                        gids = np.flatnonzero(cov[r][:len(idents)])
                        records[k] = spike_rpb_records(A, read_bits[r], gids, p_idents, first)
                        sums = np.stack([np.add.reduceat(((records[k][2] >> s) & 1).astype(np.int64), records[k][0][:-1].astype(np.int64))
                                         if len(gids) else np.zeros(0, np.int64) for s in shifts], axis=1)
                        if not np.array_equal(np.diff(records[k][0].astype(np.int64)), counters[k][:, 0]) or \
                                not np.array_equal(sums, counters[k][:, 1:1 + len(shifts)]):
                            raise RuntimeError("%s: %s:%d: the records' bits do not sum to the pre-pass's counters" %
                                               (rpb_flag, variants[k].chrom, variants[k].pos))
                if keep is not None:
                    size = sum(int(A[x].nbytes) for x in ("aln", "cig", "bq", "loc"))
                    held = size + sum(r.nbytes for r in keep["runs"]) <= (AF_KEEP_BYTES if keep_bytes is None else keep_bytes)
                    keep["runs"].append(AfRun(chrom, lo, hi, list(group), nl, size if held else 0, own if held else None,
                                              A if held else None, up if held else None, run_ref if held else None,
                                              idents if held else None, (nm, n_indel) if held else None))
            except BaseException:
                if keep is not None:
                    free_af_runs(keep["runs"])
                raise
            finally:
                if read_masks is not None:
                    read_masks[0].free()
                if not held:
                    if up is not None:
                        up.free()
                    if own is not None:
                        own.close()
            spans.send(len(group))
    finally:
        bam.close()
    rules = [DsRule(1.0, Pt, seed=int(seed), af=float(t), spike=spikes) for t, Pt in zip(targets, params_list)]
    if rpb is not None:
        try:
            rthr = [r.thr for r in read_rules]
            if grid:
                # (one call over the pairs (f, r): [V, 1, T, F, Rr, 5] -> [V, T, F x Rr, 5], the order of the read rules)
                got = spike_grid_counts(eng, spikes.lead_pos, covers, records, [int(seed) & 0xFFFFFFFFFFFFFFFF], [sv.threshold(t) for t in targets],
                                        [frac_threshold(f) for f in rpb["fracs"]], rpb["rep_thr"][:1])[:, 0]
                got = got.reshape(got.shape[0], got.shape[1], -1, 5)
            else:
                got = spike_rpb_counts(eng, spikes.lead_pos, covers, records, [int(seed) & 0xFFFFFFFFFFFFFFFF], [sv.threshold(t) for t in targets],
                                       rthr, four=indel_counters)[:, 0]
            for (k, t, r), mine in second_rpb.items():
                if [int(got[k, t, r, c]) for c in (0, 1, 4)] != mine:
                    v = variants[k]
                    raise RuntimeError("%s: %s:%d at %g x %s: the counts call says (N, V0, V1) = %r, the selection of the "
                                       "spiked copy %r" % (rpb_flag, v.chrom, v.pos, targets[t], cell_text(r),
                                                           [int(got[k, t, r, c]) for c in (0, 1, 4)], mine))
        except BaseException:
            if keep is not None:
                free_af_runs(keep["runs"])
            raise
        names = ("N", "V0", "S", "READS", "V1")
        rpb["counts"] = [[dict(zip(names, (int(x) for x in got[k, t, r]))) for t in range(len(targets)) for r in range(len(read_rules))]
                         for k in range(len(variants))]
        rpb["rules"] = [dataclasses.replace(read_rules[r], params=Pc, af=float(t), spike=spikes)
                        for (t, r), Pc in zip(((t, r) for t in targets for r in range(len(read_rules))), rpb["params"])]
        if keep is not None:
            keep["records"] = records
    if depth is not None:
        try:
            got = (spike_indel_counts if indel_counters else spike_depth_counts)(
                eng, spikes.lead_pos, covers, counters, [int(seed) & 0xFFFFFFFFFFFFFFFF], [sv.threshold(t) for t in targets],
                [frac_threshold(f) for f in fracs])[:, 0]
            for (k, t, f), mine in second.items():
                if [int(got[k, t, f, c]) for c in (0, 1, 4)] != mine:
                    v = variants[k]
                    raise RuntimeError("--spikeDepth: %s:%d at %g x fraction %g: the counts call says (N, V0, V1) = %r, the selection of the "
                                       "spiked copy %r" % (v.chrom, v.pos, targets[t], fracs[f], [int(got[k, t, f, c]) for c in (0, 1, 4)], mine))
        except BaseException:
            if keep is not None:
                free_af_runs(keep["runs"])
            raise
        names = ("N", "V0", "S", "READS", "V1")
        depth["counts"] = [[dict(zip(names, (int(x) for x in got[k, t, f]))) for t in range(len(targets)) for f in range(len(fracs))]
                           for k in range(len(variants))]
        depth["rules"] = [DsRule(float(f), Pc, seed=int(seed), af=float(t), spike=spikes, bc_thr=frac_threshold(f))
                          for (t, f), Pc in zip(((t, f) for t in targets for f in fracs), depth["params"])]
    if psets:
        try:
            joint = spike_joint(psets, covers, counters)
            lead = [spikes.lead_pos[s.members[0]] for s in psets]
            s0, thr = [int(seed) & 0xFFFFFFFFFFFFFFFF], [sv.threshold(t) for t in targets]
            # (--spikeIndelPhase: four counters per member - smc_spike_indel_phase_counts)
            phase_counts = spike_indel_phase_counts if indel_counters else spike_phase_counts
            got = phase_counts(eng, lead, joint, s0, thr, [1 << 32])[:, 0, :, 0]
            both = lambda sets: len(functools.reduce(np.intersect1d, sets))
            for g, ps in enumerate(psets):
                for t in range(len(targets)):
                    mine = [both([bits[k][0] for k in ps.members]), both([bits[k][1] for k in ps.members]),
                            both([bits[k][2][t] for k in ps.members])]
                    if [int(got[g, t, c]) for c in (0, 1, 3)] != mine:
                        raise RuntimeError("--spikePhase: set %s at %g: the counts call says (N_ALL, V0_ALL, V1_ALL) = %r, the carrier bits of "
                                           "the spiked copy %r" % (ps.name, targets[t], [int(got[g, t, c]) for c in (0, 1, 3)], mine))
            names = ("N_ALL", "V0_ALL", "S_ALL", "V1_ALL")
            phase["joint"] = joint
            phase["counts"] = [[dict(zip(names, (int(x) for x in got[g, t]))) for t in range(len(targets))] for g in range(len(psets))]
            if depth is not None:
                cells = phase_counts(eng, lead, joint, s0, thr, [frac_threshold(f) for f in fracs])[:, 0]
                phase["depth_counts"] = [[dict(zip(names, (int(x) for x in cells[g, t, f]))) for t in range(len(targets))
                                          for f in range(len(fracs))] for g in range(len(psets))]
            if rpb is not None:
                # (--spikePhaseRpb: the joint numbers over the reads each cell keeps, counted per record - and a second time as the
                # AND over the members of the selections' bits: on the spiked copy of t for N_ALL' and V1_ALL', on the run for V0_ALL')
                joint_records = spike_joint_records(psets, covers, records)
                cells = spike_phase_rpb_counts(eng, lead, [len(ps.members) for ps in psets], joint_records, s0, thr,
                                               [r.thr for r in read_rules])[:, 0]
                for g, ps in enumerate(psets):
                    for t in range(len(targets)):
                        for r in range(len(read_rules)):
                            n_all = functools.reduce(np.intersect1d, [rbits[(k, r)][1][t][0] for k in ps.members])
                            mine = [len(n_all), len(functools.reduce(np.intersect1d, [n_all] + [rbits[(k, r)][0] for k in ps.members])),
                                    both([rbits[(k, r)][1][t][1] for k in ps.members])]
                            if [int(cells[g, t, r, c]) for c in (0, 1, 3)] != mine:
                                raise RuntimeError("%s: set %s at %g x target %g: the counts call says (N_ALL, V0_ALL, V1_ALL) = %r, the "
                                                   "selection of the spiked copy %r" % (rpb_flag, ps.name, targets[t], rpb["targets"][r],
                                                                                        [int(cells[g, t, r, c]) for c in (0, 1, 3)], mine))
                phase["joint_records"] = joint_records
                phase["rpb_counts"] = [[dict(zip(names, (int(x) for x in cells[g, t, r]))) for t in range(len(targets))
                                        for r in range(len(read_rules))] for g in range(len(psets))]
        except BaseException:
            if keep is not None:
                free_af_runs(keep["runs"])
            raise
    return rules, [dict(target=t, rows=r) for t, r in zip(targets, rows)]


# ---- replicate dilutions (--dsAFReps): R seeds, the masks and the achieved counts on the device, only the listed runs called
AF_KEEP_BYTES = 1 << 30        # host bytes of the pre-pass's runs that stay decoded for the replicate stage (as many again in HBM)
AF_REP_BATCH_SLOTS = 16 << 20  # read slots of one replicate batch: as many replicates of a run as fit are called with one plan
AF_REP_MAX_TARGETS = 32        # SMC_AF_REP_MAX_TARGETS


@dataclasses.dataclass
class AfRun:
    """A run of the --dsAF pre-pass kept for the replicate stage: the listed variants it holds (`group`: their indexes) and, while
    `A` is not None, its alignments on the host, its arrays in HBM (`up`), the decoder handle that holds its records (`bam`) and the
    identities of its barcodes by run-wide id."""
    chrom: str
    lo: int
    hi: int
    group: list
    nl: int
    nbytes: int = 0
    bam: object = None
    A: object = None
    up: object = None
    run_ref: str = None
    idents: object = None
    mism: object = None         # (--spikeReps) the alignments' (NM, inserted plus deleted length), as the decoder gives them

    def load(self, path: str, fasta, eng, params, max_reads: int, nthreads: int, mism: bool = False) -> int:
        """Decode the run with a handle of its own, upload it and fill the fields above (`mism`: that one too) -> the loci the decoder
        gave.  Fewer than one, or not the `nl` this run already has (the pre-pass's): nothing but the decode is done and the caller
        refuses; a run without `nl` gets the decoder's.  free() takes back whatever a load that failed has made."""
        self.bam = bamio.NativeBam(path)
        self.A = self.bam.alignments_run(self.chrom, self.lo, self.hi, max_reads, params, nthreads or bamio.host_threads())
        nl = int(self.A["nl"])
        if nl < 1 or self.nl not in (0, nl):
            return nl
        self.nl = nl
        self.run_ref = fasta.fetch(self.chrom, self.lo, self.lo + nl).upper()
        self.up = upload_run(eng, self.A, self.run_ref)
        self.idents = self.bam.barcode_idents(self.A["n_bc"])
        self.mism = self.bam.run_mismatches(len(self.A["aln"])) if mism else None
        return nl

    def free(self):
        if self.up is not None:
            self.up.free()
        if self.bam is not None:
            self.bam.close()
        self.up = self.bam = self.A = self.idents = self.mism = None


def free_af_runs(runs):
    for r in runs or ():
        r.free()


class AfCellTable(object):
    """The carrier table and the seeds of --dsAFReps / --dsAFDepth in HBM (dsaf.carrier_table; csrc/k_af_depth.inc) with their host
    copies, and the two calls over them.  `depth_thr` (--dsAFDepth): the thresholds of the barcode fractions (frac_threshold(f), host
    memory: they travel by value) - the results then have one dimension more, the fractions', behind the targets'."""

    def __init__(self, eng, idents, thr, seeds, depth_thr=None):
        self.eng = eng
        self.idents = np.ascontiguousarray(idents, np.uint64)
        self.thr = np.ascontiguousarray(thr, np.uint64)              # [carriers, targets]
        self.seeds = np.ascontiguousarray(seeds, np.uint64)
        if self.thr.ndim != 2 or self.thr.shape[0] != len(self.idents):
            raise ValueError("AfCellTable: %d carriers, thresholds of shape %r" % (len(self.idents), self.thr.shape))
        self.n_targets = int(self.thr.shape[1])
        self.depth_thr = None if depth_thr is None else np.ascontiguousarray(depth_thr, np.uint64)
        self.n_fracs = None if depth_thr is None else len(self.depth_thr)
        self.d_idents, self.d_thr, self.d_seeds = _up8(eng, self.idents), _up8(eng, self.thr), _up8(eng, self.seeds)

    def _call(self, kind: str, head: tuple, tail: tuple, depth):
        """smc_af_rep_<kind> or, with `depth` thresholds, smc_af_depth_<kind>: `head`, the table (the thresholds behind the targets),
        the seeds, `tail`, the default stream."""
        name = "smc_af_%s_%s" % ("rep" if depth is None else "depth", kind)
        args = [self.eng.ctx, *head, self.d_idents.data_ptr(), self.d_thr.data_ptr(), self.idents.ctypes.data, self.thr.ctypes.data,
                len(self.idents), self.n_targets]
        if depth is not None:
            args += [depth.ctypes.data, len(depth)]
        args += [self.d_seeds.data_ptr(), len(self.seeds), *tail, ctypes.c_void_p(0)]
        _lib.check(getattr(self.eng.L, name)(*args), name)

    def masks(self, d_run_idents, n_ids: int, d_masks, n_words: int, d_draws=None, plain: bool = False):
        """smc_af_rep_masks / smc_af_depth_masks: len(seeds) x n_targets [x n_fracs] keep masks of `n_words` words each over a run's
        barcode identities (device addresses) - mask (j x T + t) [x F + f] is what select_run(d_mask=...) takes.  d_draws: uint32
        [len(seeds), n_ids], the AF draw of every carrier (0 for the others) or, with fractions, the depth draw of every id.
        `plain`: the targets' masks of a table with fractions, as if it had none."""
        self._call("masks", (d_run_idents, int(n_ids)), (d_masks, int(n_words), d_draws), None if plain else self.depth_thr)

    def counts(self, covers, carries, plain: bool = False) -> np.ndarray:
        """smc_af_rep_counts / smc_af_depth_counts: uint32 [V, R, T, 2] or [V, R, T, F, 2] = (N', V') of every variant, replicate and
        target [and fraction], from the identities that cover / carry each variant (made unique here, as titrate() does)."""
        from .engine import DevBuf
        depth = None if plain else self.depth_thr
        shape = (len(covers), len(self.seeds), self.n_targets) + (() if depth is None else (len(depth),)) + (2,)
        covers = [np.unique(np.asarray(c, np.uint64)) for c in covers]
        off = np.zeros(len(covers) + 1, np.uint32)
        off[1:] = np.cumsum([len(c) for c in covers])
        ident = np.concatenate(covers) if covers else np.zeros(0, np.uint64)
        carry = np.concatenate([np.isin(c, np.asarray(k, np.uint64)) for c, k in zip(covers, carries)]).astype(np.uint8) if covers \
            else np.zeros(0, np.uint8)
        n_out = int(np.prod(shape))
        bufs = [_up8(self.eng, a) for a in (ident, carry, off)] + [DevBuf(self.eng, 4 * max(1, n_out) + 256)]
        try:
            self._call("counts", (bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), off.ctypes.data, len(covers)),
                       (bufs[3].data_ptr(),), depth)
            out = bufs[3].download(np.uint32, n_out) if n_out else np.zeros(0, np.uint32)      # (the default stream: behind the kernel)
        finally:
            for b in bufs:
                b.free()
        return out.reshape(shape)

    def free(self):
        for b in (self.d_idents, self.d_thr, self.d_seeds):
            b.free()


AfRepTable = AfDepthTable = AfCellTable       # (one class: what the callers wrote before there was one)


def mask_words(n_ids: int) -> int:
    """Words per keep mask as select_run pads a host mask: the bits' bytes rounded up to whole words, and one word more."""
    return (int(n_ids) + 31) // 32 + 1


def _narrow_retry(eng, P, call):
    """call(bits): with 16-bit read words while the engine builds them and the params' minBQ fits, and when that answers NARROW (a build
    has no room in them) once more with 32 - as every batch of the file from there on."""
    out = call(16 if (eng.word_bits == 16 and 0 <= P.minBQ <= 63) else 32)
    if out == NARROW:
        eng.word_bits = 32
        out = call(32)
    return out


def _build_copies(eng, run: AfRun, n_copies: int, kept_runs, P, bits, flag, fasta, max_depth, sampler, sampler_seed, extras=None):
    """The builds of a replicate stage's batch: `kept_runs` - an iterable of `n_copies` _KeptRun over the kept run `run`, its selections
    or its spiked copies, each made when the loop asks for it and freed behind its build - built one behind the other into one
    _DsBatch with the cell's params `P`, as _ds_build_run appends successive runs to a rule's -> the batch (the caller frees it), or
    NARROW (a build has no room in 16-bit read words).  BamError naming `flag`: a build the device builder does not take.
    `extras`: per copy the BuildExtras its build leaves its extras list in - the batch then has no tables."""
    lo, nl = run.lo, run.nl
    ns_full = int(run.A["n_slots"])
    cap = n_copies * (ns_full + nl) + ns_full + nl + 64
    d = _DsBatch(eng, cap, bits, False)
    cp = abi.c_params(P)
    try:
        n_loc = 0
        for c, kept in enumerate(kept_runs):
            try:
                done = build_run(kept.counts, eng.L, eng, cp, P, run.chrom, lo, fasta, run.run_ref, [d.words] + d.planes, d.uaux, d.slots,
                                 d.slots + n_loc, cap, max_depth, kept.allele_key, kept.barcode_name, sampler=sampler, sampler_seed=sampler_seed,
                                 barcode_idents=kept.barcode_idents, uploaded=kept.run, extras=extras[c] if extras is not None else None)
            finally:
                kept.free()
            if done is None:
                raise bamio.BamError(_ds_refused(run.chrom, lo, lo + nl, "a replicate: the device builder does not take it", flag))
            if done == NARROW:
                d.free()
                return NARROW
            d.add(done)
            n_loc += nl
        return d
    except BaseException:
        d.free()
        raise


BUILD_ST_UNFLAGGED = 64         # SMC_LISTED_UNFLAGGED: smc_build_listed declined a copy (an alignment flagged neither READ1 nor READ2)
LISTED_MAX_LOCI, LISTED_MAX_COPIES = 64, 1024      # SMC_LISTED_MAX_LOCI, SMC_LISTED_MAX_COPIES
LISTED_SHARED_ORDER, LISTED_DENSE_LOCUS = 1, 2     # smc_build_listed's flags
LISTED_XMAX = 58                                   # BL_XMAX: the alleles beyond the six fixed ones a listed locus holds
LISTED_COPY_DTYPE = np.dtype([("aln", "<u8"), ("cig", "<u8"), ("bq", "<u8"), ("loc", "<u8"), ("n_aln", "<i4"), ("n_bc", "<i4"),
                              ("n_pair", "<i4"), ("reserved", "<i4")])     # smc_listed_copy
assert LISTED_COPY_DTYPE.itemsize == 48


def listed_takes(run, n_listed: int) -> bool:
    """Can the listed builder take `n_listed` loci of the kept run `run` at all?  Not a run with an alignment flagged neither READ1 nor
    READ2 (every copy of it would be declined), and no more loci than one call lists."""
    return 1 <= n_listed <= LISTED_MAX_LOCI and not (int(run.A["status"]) & 1)


def listed_layout(loc_host, offsets, n_copies: int) -> dict:
    """Where smc_build_listed puts the dense batch of n_copies x len(offsets) loci: the slot capacity of listed locus g is align4 of
    loc_host[offsets[g]].n - the depth in the unselected, unspiked run: spiking changes no span, a selection only drops records.
    -> dict(caps: uint32 [G], stride: the slots of a copy, n_slots, n_ustart: the batch's, slot(c, g) / ustart(c, g): first slot /
    first umi_start entry of locus g of copy c behind the batch's bases, index(c, g): its place among the batch's loci and rows)."""
    offsets = [int(a) for a in offsets]
    if any(b <= a for a, b in zip(offsets, offsets[1:])) or (offsets and (offsets[0] < 0 or offsets[-1] >= len(loc_host))):
        raise ValueError("listed_layout: the offsets %r do not ascend within the run's %d loci" % (offsets, len(loc_host)))
    caps = np.array([(int(loc_host["n"][a]) + 3) & ~3 for a in offsets], np.uint32)
    capoff = [0] + [int(x) for x in np.cumsum(caps.astype(np.int64))]
    S, G = capoff[-1], len(offsets)
    return dict(caps=caps, stride=S, n_slots=n_copies * S, n_ustart=n_copies * (S + G) + 1,
                slot=lambda c, g: c * S + capoff[g], ustart=lambda c, g: c * (S + G) + capoff[g] + g, index=lambda c, g: c * G + g)


def _build_listed(eng, run: "AfRun", kept_list, at, P, bits, sampler, sampler_seed, shared: bool, dense: bool = False):
    """smc_build_listed: the loci at run offsets `at` (ascending) of every _KeptRun of `kept_list` - spiked copies of the kept run `run`
    (`shared`: one barcode-major order serves them all) or selections of them - as ONE dense _DsBatch of copies x listed loci, locus g
    of copy c at c x len(at) + g, with the cell's params `P`: one call, ONE download of the copies' counters, one of the descriptors
    and - where a copy has extras entries - one of all the copies' extras stretches.  The copies stay the caller's (nothing is freed
    here).  `dense` (--spikeScanIndel): the device entries' locus field holds g (SMC_LISTED_DENSE_LOCUS), and the extras stretches and
    their counts stay in HBM for smc_scan_detect_keys - the answer's third member, which the caller frees.
    -> (the batch - the caller frees it -, per copy its extras entries [n, 5] with the RUN offset in the locus field, None or
    dict(x, cnt: the DevBufs, xcap)), NARROW (no room in 16-bit read words), or None: the listed builder declines (an alignment flagged
    neither READ1 nor READ2, a depth beyond the unselected run's, more alleles than it holds) - the caller builds the whole way."""
    from .engine import DevBuf
    lo, nl, B, G = run.lo, run.nl, len(kept_list), len(at)
    if not listed_takes(run, G) or not 1 <= B <= LISTED_MAX_COPIES or any(k.counts["status"] != 0 for k in kept_list):
        return None
    lay = listed_layout(run.up.loc_host, at, B)
    cap = lay["n_ustart"] + 64
    xcap = LISTED_XMAX * G                     # (every allele beyond the six fixed ones of every listed locus: the list cannot overflow)
    desc = np.zeros(B, LISTED_COPY_DTYPE)
    for c, k in enumerate(kept_list):
        r = k.run
        desc[c] = (r.aln.data_ptr(), r.cig.data_ptr(), r.bq.data_ptr(), r.loc.data_ptr(), r.n_aln, int(k.counts["n_bc"]), int(k.counts["n_pair"]), 0)
    offs = np.array(list(at) + [0], np.uint32)
    cp = abi.c_params(P)
    d = _DsBatch(eng, cap, bits, False)
    bufs = [DevBuf(eng, desc.nbytes + 256).upload(desc), DevBuf(eng, LOCUS_DTYPE.itemsize * B * G + 256), DevBuf(eng, 20 * xcap * B + 256),
            DevBuf(eng, 8 * B + 256)]
    d_desc, d_loci, d_x, d_cnt = bufs
    keep = None
    try:
        _lib.check(eng.L.smc_build_listed(eng.ctx, ctypes.byref(cp), d_desc.data_ptr(), B, (LISTED_SHARED_ORDER if shared else 0) | (LISTED_DENSE_LOCUS if dense else 0),
                                          lo, nl, run.up.ref.data_ptr(), offs.ctypes.data, lay["caps"].ctypes.data, G, bits, 0, 0, d.words.data_ptr(),
                                          d.uaux[0].data_ptr(), d.uaux[1].data_ptr(), d.uaux[2].data_ptr(), d_loci.data_ptr(), d_x.data_ptr(), xcap,
                                          d_cnt.data_ptr(), ctypes.c_void_p(0)), "smc_build_listed")
        cnt = d_cnt.download(np.uint32, 2 * B).reshape(B, 2)
        verdict = True
        for c in range(B):
            st = _build_status(cnt[c], xcap, bits == 16, run.chrom, lo, nl)
            if st is None:
                verdict = None
                break
            if st == NARROW:
                verdict = NARROW
        if verdict is not True:
            d.free()
            return verdict
        lc = d_loci.download(LOCUS_DTYPE, B * G)
        pos = np.array([lo + 1 + a for a in at], np.int64)
        if any(k.by_read for k in kept_list):       # (renumbered barcodes: a copy's identities are its own)
            for c, k in enumerate(kept_list):
                lc[c * G:(c + 1) * G] = _philox_marks_over_cap(eng, eng.L, cp, P, _BufView(d_loci, LOCUS_DTYPE.itemsize * G * c), lc[c * G:(c + 1) * G], pos,
                                                               d.words, bits == 16, d.uaux, sampler, sampler_seed, k.counts["n_bc"], k.barcode_idents,
                                                               k.barcode_name)
        else:                                       # (the run's ids in every copy: one call over the B x G loci)
            k = kept_list[0]
            lc = _philox_marks_over_cap(eng, eng.L, cp, P, d_loci, lc, np.tile(pos, B), d.words, bits == 16, d.uaux, sampler, sampler_seed,
                                        run.A["n_bc"], k.barcode_idents, k.barcode_name)
        for c, k in enumerate(kept_list):
            _py2_sample_over_cap(P, lc[c * G:(c + 1) * G], lambda g: str(lo + int(at[g]) + 1), d.uaux, k.barcode_name)
        xl = [np.zeros((0, 5), np.uint32)] * B
        if cnt[:, 0].any():
            # (all B stretches in one copy, 1160 x G bytes each: the scan's batches hold at most SPIKE_MAX_COPIES = 64 copies, so 74 KB x G
            # - 148 KB at the two loci a default pass lists, 4.75 MB at the 64 a call takes; the entry's own limit of 1024 copies would
            # make it 76 MB, and a caller with such batches should bring the stretches down by the largest count instead)
            allx = d_x.download(np.uint32, 5 * xcap * B).reshape(B, xcap, 5)
            xl = [allx[c, :int(cnt[c, 0])].copy() for c in range(B)]
            if dense:
                for x in xl:
                    x[:, 0] = np.asarray(at, np.uint32)[x[:, 0]]
        d.LC, d.slots, d.tables = [lc], lay["n_slots"], None
        if dense:
            keep = dict(x=d_x, cnt=d_cnt, xcap=xcap)
        return d, xl, keep
    except BaseException:
        d.free()
        raise
    finally:
        for b in bufs:
            if keep is None or (b is not d_x and b is not d_cnt):
                b.free()


def _check_listed_rows(eng, run: "AfRun", held, c0: int, d_rows, listed, P, bits, flag, fasta, max_depth, sampler, sampler_seed, variants, what):
    """(--spikeScanBuild listed) The self-check of a listed batch whose called rows are `d_rows`: copy c0 - replicate 0 - is also built
    the whole way (_build_copies on that one _KeptRun, which frees it: its place in `held` is taken by a stand-in that keeps its
    allele_key; 32-bit read words and no table, whatever the batch has) and called with a plan of its own; the smc_row bytes of every
    listed locus must be the listed build's.  RuntimeError naming the locus otherwise."""
    from .engine import DevBuf
    G, nl, size = len(listed), run.nl, abi.ROW_DTYPE.itemsize
    k0 = held[c0]
    if k0.d_orig is not None:
        k0.orig_index()                         # (its allele_key outlives the selection's arrays)
    held[c0] = _FreedKept(k0.allele_key)
    # (32-bit read words whatever the batch's: an unlisted locus of the run may have no room in 16-bit ones, and a row does not depend on
    # the width - nothing to retry, and the run's word width stays the main pass's business)
    # (no table is made of this build - rows are compared, not printed: its extras list stays in a region of its own)
    xcap = build_xcap(nl)
    xb = [DevBuf(eng, 20 * xcap + 256), DevBuf(eng, 256)]
    plan = rows = w = None
    try:
        w = _build_copies(eng, run, 1, iter([k0]), P, 32, flag, fasta, max_depth, sampler, sampler_seed, extras=[BuildExtras(xb[0], xb[1])])
        plan = eng.make_plan(w.loci())
        rows = plan.run_into_devbuf([w.words, w.uaux[0]], P)
        for g in range(G):
            a = int(listed["offset"][g])
            mine = d_rows.download(abi.ROW_DTYPE, 1, (c0 * G + g) * size)
            theirs = rows.download(abi.ROW_DTYPE, 1, a * size)
            if mine.tobytes() != theirs.tobytes():
                raise RuntimeError("--spikeScanBuild listed: replicate 0 at %s:%d%s: the row of the listed build is not the whole build's "
                                   "(fields %s)" % (run.chrom, run.lo + 1 + a, what,
                                                    ", ".join(f for f in abi.ROW_DTYPE.names if mine[f].tobytes() != theirs[f].tobytes())))
    finally:
        if plan is not None:
            plan.close()
        for b in [rows, w] + xb:
            if b is not None:
                b.free()


class _FreedKept(object):
    """What stands in `held` for a _KeptRun the self-check's whole build has freed: its allele_key, and nothing left to free."""

    def __init__(self, allele_key):
        self.allele_key = allele_key

    def free(self):
        pass


def _listed_rows(d: _DsBatch, out_rows, run: AfRun, at, n_copies: int, P, fasta):
    """The raw row strings of the loci at offsets `at` of the run in every one of the `n_copies` builds of batch `d`, whose called rows
    `out_rows` are -> per copy the listed loci's text, in the order of `at`."""
    from . import vc
    lo, nl = run.lo, run.nl
    idx = np.array([b * nl + a for b in range(n_copies) for a in at], np.int64)
    view = vc.LocusView([run.chrom] * len(idx), [lo + 1 + a for _ in range(n_copies) for a in at],
                        [run.run_ref[a] if a < len(run.run_ref) else "" for _ in range(n_copies) for a in at], [d.tables[i] for i in idx.tolist()])
    text = vc._strings(out_rows[idx].copy(), view, P, fasta)
    g = len(at)
    return [list(text[b * g:(b + 1) * g]) for b in range(n_copies)]


def _copy_rows(eng, run: AfRun, variants, n_copies: int, kept_runs, P, bits, flag, fasta, max_depth, sampler, sampler_seed):
    """_build_copies, the batch called with one plan, and of its rows those of the variants of run.group (indexes into `variants`) ->
    per copy the listed loci's raw rows, in the order of run.group, or NARROW."""
    d = _build_copies(eng, run, n_copies, kept_runs, P, bits, flag, fasta, max_depth, sampler, sampler_seed)
    if d == NARROW:
        return NARROW
    try:
        plan = eng.make_plan(d.loci())
        try:
            out_rows = plan.run_devbuf([d.words, d.uaux[0]], P)
        finally:
            plan.close()
        return _listed_rows(d, out_rows, run, [variants[k].pos - 1 - run.lo for k in run.group], n_copies, P, fasta)
    finally:
        d.free()


def _af_rep_call(eng, run: AfRun, table: AfCellTable, d_masks, n_words, todo, P, fasta, variants, max_depth, sampler, sampler_seed, bits):
    """The builds of `todo` - indexes of masks in `d_masks`, all of one cell (a target, or with --dsAFDepth a target x fraction: the
    params `P` are that cell's) - of a kept run appended to one device batch (_build_copies) and the batch called with one plan ->
    (per mask index the listed loci's raw rows, in the order of run.group), or NARROW (a build has no room in 16-bit read words)."""
    kept_runs = (_KeptRun(*select_run(eng, run.up, run.A, run.lo, d_mask=d_masks.data_ptr() + 4 * n_words * m), run.A, run.bam.allele_key,
                          run.bam.barcode_name, lambda n: run.idents) for m in todo)
    text = _copy_rows(eng, run, variants, len(todo), kept_runs, P, bits, "--dsAFReps", fasta, max_depth, sampler, sampler_seed)
    return NARROW if text == NARROW else dict(zip(todo, text))


def ds_af_replicates(path: str, fasta, variants, targets, params_list, seed: int, n_reps: int, eng, keep: dict, res, sampler: str = "reference",
                     sampler_seed: int = 0, nthreads: int = 0, max_reads: int = 128_000_000, depth: dict = None):
    """The replicate stage of --dsAFReps.  Replicate j is --dsAF with seed (seed + j) mod 2^64: from the pre-pass's sets the carrier
    table goes up once and smc_af_rep_counts gives every (N', V'); then per kept run smc_af_rep_masks makes all R x T keep masks in
    one launch, and every (j, t) is select_run(d_mask) -> build_run -> the locus kernels, the replicates of a target appended to one
    device batch and called with one plan per batch-full.  Replicates of a run whose masks are equal bit for bit are built once.
    -> dict(seeds, counts: uint32 [V, R, T, 2], rows: {(variant index, target index, replicate): the raw row string at the variant's
    locus}, times: seconds per part).
    `depth` (--dsAFDepth: dict with "fracs" and the "params" of the T x F cells, targets outer): the stage runs over CELLS - the T
    plain targets first, then the T x F cells, each with its own params; the cells' masks and counts come from smc_af_depth_masks /
    _counts with the same seeds (replicate j draws both streams with s_j), behind the targets' in one device buffer.  `rows` is then
    keyed by the cell's index (0 .. T - 1 the targets, T + t x F + f the cells) and "depth_counts" is uint32 [V, R, T, F, 2]."""
    import time
    from . import dsaf
    from .engine import DevBuf
    t_start = time.perf_counter()
    T = len(targets)
    if T > AF_REP_MAX_TARGETS:
        raise ValueError("--dsAFReps: %d --dsAF targets, at most %d" % (T, AF_REP_MAX_TARGETS))
    seeds = dsaf.rep_seeds(seed, n_reps)
    idents, thr = dsaf.carrier_table(keep["carries"], [[row["thr"] for row in r["rows"]] for r in res])
    table = AfCellTable(eng, idents, thr, seeds, [frac_threshold(f) for f in depth["fracs"]] if depth is not None else None)
    F = len(depth["fracs"]) if depth is not None else 0
    cell_params = list(params_list) + (list(depth["params"]) if depth is not None else [])
    depth_counts = None
    times = {"counts": 0.0, "masks": 0.0, "decode again": 0.0, "builds": 0, "batches": 0}
    rows = {}
    max_depth = eng.L.smc_build_max_depth()
    try:
        t0 = time.perf_counter()
        counts = table.counts(keep["covers"], keep["carries"], plain=True)
        if depth is not None:
            depth_counts = table.counts(keep["covers"], keep["carries"])
        times["counts"] = time.perf_counter() - t0
        for run in keep["runs"]:
            if run.A is None:
                # (over the byte cap of the pre-pass: decoded and uploaded again)
                t0 = time.perf_counter()
                nl = run.load(path, fasta, eng, params_list[0], max_reads, nthreads)
                if nl != run.nl:
                    raise bamio.BamError("--dsAFReps: the run %s:%d-%d was decoded as %d loci, the pre-pass had %d" %
                                         (run.chrom, run.lo + 1, run.hi, nl, run.nl))
                times["decode again"] += time.perf_counter() - t0
            n_bc = int(run.A["n_bc"])
            n_words = mask_words(n_bc)
            d_id = DevBuf(eng, 8 * max(1, n_bc) + 256).upload(np.ascontiguousarray(run.idents, np.uint64) if n_bc else np.zeros(1, np.uint64))
            n_plain = n_reps * T                                       # (the targets' masks stand first in the buffer, then the cells')
            d_masks = DevBuf(eng, 4 * (n_plain + n_reps * T * F) * n_words + 256)
            try:
                t0 = time.perf_counter()
                table.masks(d_id.data_ptr(), n_bc, d_masks.data_ptr(), n_words, plain=True)
                if depth is not None:
                    table.masks(d_id.data_ptr(), n_bc, d_masks.data_ptr() + 4 * n_plain * n_words, n_words)
                host = d_masks.download(np.uint32, (n_plain + n_reps * T * F) * n_words).reshape(-1, n_words)      # (behind the kernels)
                # (per cell: the replicates' masks and their indexes in the buffer)
                index_of = [[j * T + t for j in range(n_reps)] for t in range(T)] + \
                           [[n_plain + j * T * F + c for j in range(n_reps)] for c in range(T * F)]
                of_cell = [(host[index], index) for index in index_of]
                times["masks"] += time.perf_counter() - t0
                per_build = int(run.A["n_slots"]) + run.nl
                room = max(1, AF_REP_BATCH_SLOTS // max(1, per_build))
                for t, (cell_masks, index) in enumerate(of_cell):
                    # (equal masks, equal rows: a variant that is left alone at t, or draws that drop the same carriers of this run)
                    first = {}
                    for j in range(n_reps):
                        first.setdefault(cell_masks[j].tobytes(), j)
                    todo = [index[j] for j in sorted(first.values())]
                    got = {}
                    for b in range(0, len(todo), room):
                        part = todo[b:b + room]
                        got.update(_narrow_retry(eng, cell_params[t], lambda bits: _af_rep_call(
                            eng, run, table, d_masks, n_words, part, cell_params[t], fasta, variants, max_depth, sampler, sampler_seed, bits)))
                        times["builds"] += len(part)
                        times["batches"] += 1
                    for j in range(n_reps):
                        text = got[index[first[cell_masks[j].tobytes()]]]
                        for k, line in zip(run.group, text):
                            rows[(k, t, j)] = line
            finally:
                d_id.free()
                d_masks.free()
            run.free()
    finally:
        table.free()
        free_af_runs(keep["runs"])
    times["stage"] = time.perf_counter() - t_start
    return dict(seeds=seeds, counts=counts, rows=rows, times=times, depth_counts=depth_counts)


# ---- replicate spike-ins (--spikeReps): R seeds, the achieved counts and B spiked copies per call on the device
SPIKE_MAX_COPIES = 64          # SMC_SPIKE_MAX_COPIES
SPIKE_REP_BATCH_BYTES = 1 << 30   # bytes of spiked copies (records + pair pools) one smc_spike_alleles_reps call of the stage writes


def _spike_counts_call(eng, name: str, arrays, shape, call) -> np.ndarray:
    """The device side of the three counts wrappers below: `arrays` go up, call(their device addresses, the output's) runs the entry
    `name` on the default stream, the uint32 counters of `shape` come down, and everything is freed."""
    from .engine import DevBuf
    n_out = int(np.prod(shape))
    bufs = [_up8(eng, a) for a in arrays] + [DevBuf(eng, 4 * max(1, n_out) + 256)]
    try:
        _lib.check(call([b.data_ptr() for b in bufs[:-1]], bufs[-1].data_ptr()), name)
        out = bufs[-1].download(np.uint32, n_out) if n_out else np.zeros(0, np.uint32)         # (the default stream: behind the kernel)
    finally:
        for b in bufs:
            b.free()
    return out.reshape(shape)


def _spike_flat_covers(who: str, positions, covers, counters, width: int = 3):
    """The variants' covers as the counts entries take them -> (identities, counters [n, width], offsets [V + 1], positions)."""
    n_var = len(covers)
    off = np.zeros(n_var + 1, np.uint32)
    off[1:] = np.cumsum([len(c) for c in covers])
    ident = np.concatenate([np.asarray(c, np.uint64) for c in covers]) if n_var else np.zeros(0, np.uint64)
    if any(np.asarray(c).size != width * len(x) for c, x in zip(counters, covers)):
        raise ValueError("%s: %d counters per covering barcode expected" % (who, width))
    cnt = np.concatenate([np.asarray(c, np.uint32).reshape(-1, width) for c in counters]) if n_var else np.zeros((0, width), np.uint32)
    if len(cnt) != len(ident):
        raise ValueError("%s: %d covering barcodes, counters of %d" % (who, len(ident), len(cnt)))
    return ident, cnt, off, np.array([int(p) & 0xFFFFFFFF for p in positions], np.uint32)


def spike_rep_counts(eng, positions, covers, counters, seeds, thresholds) -> np.ndarray:
    """smc_spike_rep_counts -> uint32 [V, R, T, 3] = (S, READS, V1) of every variant, replicate and target.  positions[v]: 1-based;
    covers[v]: the uint64 identities of the barcodes that cover v; counters[v]: uint32 [len(covers[v]), 3] = (reads, alt0, single);
    thresholds: floor(t * 2^32) per target."""
    ident, cnt, off, pos = _spike_flat_covers("spike_rep_counts", positions, covers, counters)
    seeds, thr = np.ascontiguousarray(seeds, np.uint64), np.ascontiguousarray(thresholds, np.uint64)
    return _spike_counts_call(
        eng, "smc_spike_rep_counts", [ident, cnt, off, pos, seeds], (len(covers), len(seeds), len(thr), 3),
        lambda d, d_out: eng.L.smc_spike_rep_counts(eng.ctx, d[0], d[1], d[2], off.ctypes.data, d[3], len(covers), d[4], len(seeds),
                                                    thr.ctypes.data, len(thr), d_out, ctypes.c_void_p(0)))


def spike_depth_counts(eng, positions, covers, counters, seeds, thresholds, depth_thresholds) -> np.ndarray:
    """smc_spike_depth_counts -> uint32 [V, R, T, F, 5] = (N', V0', S', READS', V1') of every variant, replicate and cell.  The
    arguments are spike_rep_counts'; depth_thresholds: frac_threshold(f) per barcode fraction."""
    ident, cnt, off, pos = _spike_flat_covers("spike_depth_counts", positions, covers, counters)
    seeds = np.ascontiguousarray(seeds, np.uint64)
    thr, dthr = np.ascontiguousarray(thresholds, np.uint64), np.ascontiguousarray(depth_thresholds, np.uint64)
    return _spike_counts_call(
        eng, "smc_spike_depth_counts", [ident, cnt, off, pos, seeds], (len(covers), len(seeds), len(thr), len(dthr), 5),
        lambda d, d_out: eng.L.smc_spike_depth_counts(eng.ctx, d[0], d[1], d[2], off.ctypes.data, d[3], len(covers), d[4], len(seeds),
                                                      thr.ctypes.data, len(thr), dthr.ctypes.data, len(dthr), d_out, ctypes.c_void_p(0)))


def spike_indel_counts(eng, positions, covers, counters, seeds, thresholds, depth_thresholds=None) -> np.ndarray:
    """smc_spike_indel_counts -> spike_rep_counts' uint32 [V, R, T, 3] (`depth_thresholds` None) or spike_depth_counts' [V, R, T, F, 5]
    from counters[v]: uint32 [len(covers[v]), 4] = (reads, alt0, alt1, touch).  The other arguments are theirs."""
    ident, cnt, off, pos = _spike_flat_covers("spike_indel_counts", positions, covers, counters, 4)
    seeds, thr = np.ascontiguousarray(seeds, np.uint64), np.ascontiguousarray(thresholds, np.uint64)
    dthr = None if depth_thresholds is None else np.ascontiguousarray(depth_thresholds, np.uint64)
    shape = (len(covers), len(seeds), len(thr)) + ((3,) if dthr is None else (len(dthr), 5))
    return _spike_counts_call(
        eng, "smc_spike_indel_counts", [ident, cnt, off, pos, seeds], shape,
        lambda d, d_out: eng.L.smc_spike_indel_counts(eng.ctx, d[0], d[1], d[2], off.ctypes.data, d[3], len(covers), d[4], len(seeds),
                                                      thr.ctypes.data, len(thr), None if dthr is None else dthr.ctypes.data,
                                                      0 if dthr is None else len(dthr), d_out, ctypes.c_void_p(0)))


SPB_COVERS, SPB_ALT, SPB_SINGLE, SPB_FIRST = 1, 2, 4, 1      # k_spike_rpb.inc: smc_spike_read_bits' bits; bit 0 of a record's flag byte
SPB_ALT1, SPB_TOUCH = 4, 8                                   # smc_spike_indel_read_bits' bits 2 and 3 (an SNV list's bytes have no bit 3)


def spike_read_bits(eng, up: RunOnDevice, A, lo: int, var: np.ndarray) -> np.ndarray:
    """smc_spike_read_bits over the run `up` (A: its host arrays) -> uint8 [n_var, n_aln]: per listed SNV (af_run_variants' records) and
    alignment bit 0 = the record covers the position, bit 1 = it shows ALT as it is, bit 2 = its allele key there is a single letter."""
    n_var, n = len(var), up.n_aln
    if not n_var or not n:
        return np.zeros((n_var, n), np.uint8)
    d_out = spike_read_bits_dev(eng, up, A, lo, var)
    try:
        return d_out.download(np.uint8, n_var * n).reshape(n_var, n)                      # (the default stream: behind the kernel)
    finally:
        d_out.free()


def spike_read_bits_dev(eng, up: RunOnDevice, A, lo: int, var: np.ndarray):
    """spike_read_bits that leaves the bytes in HBM -> the DevBuf of n_var x n_aln bytes (the caller frees it); enqueued on the default
    stream, nothing waits.  What smc_scan_phase_rpb_counts takes as d_bits."""
    from .engine import DevBuf
    n_var, n = len(var), up.n_aln
    var = np.ascontiguousarray(var, abi.AF_VARIANT_DTYPE)
    d_var = DevBuf(eng, var.nbytes + 256).upload(var.view(np.uint8).reshape(-1) if n_var else np.zeros(4, np.uint8))
    d_out = DevBuf(eng, n_var * n + 256)
    try:
        _lib.check(eng.L.smc_spike_read_bits(eng.ctx, up.aln.data_ptr(), n, up.cig.data_ptr(), len(A["cig"]), up.bq.data_ptr(), len(A["bq"]) // 2,
                                             up.loc.data_ptr(), int(A["nl"]), int(lo), d_var.data_ptr(), var.ctypes.data, n_var,
                                             d_out.data_ptr(), ctypes.c_void_p(0)), "smc_spike_read_bits")
        return d_out                            # (d_var goes back to the spare list: whatever takes it next is behind the kernel on this stream)
    except BaseException:
        d_out.free()
        raise
    finally:
        d_var.free()


def spike_indel_read_bits(eng, up: RunOnDevice, A, lo: int, var: np.ndarray, ins: np.ndarray) -> np.ndarray:
    """smc_spike_indel_read_bits over the run `up` (A: its host arrays) -> uint8 [n_var, n_aln]: per listed variant (`var`: smc_spike_indels'
    records of the run's listed loci, ascending; `ins`: the pool their insertions point into) and alignment bit 0 = the record covers
    the position, bit 1 = it shows the key as it is, bit 2 = it shows it when its barcode is spiked, bit 3 = the rewrite changes it then."""
    from .engine import DevBuf
    n_var, n = len(var), up.n_aln
    if not n_var or not n:
        return np.zeros((n_var, n), np.uint8)
    var = np.ascontiguousarray(var, abi.SPIKE_INDEL_VARIANT_DTYPE)
    ins = np.ascontiguousarray(ins, np.uint8)
    d_var = DevBuf(eng, var.nbytes + 256).upload(var.view(np.uint8).reshape(-1))
    d_ins = DevBuf(eng, ins.nbytes + 256).upload(ins if ins.nbytes else np.zeros(4, np.uint8))
    d_out = DevBuf(eng, n_var * n + 256)
    try:
        _lib.check(eng.L.smc_spike_indel_read_bits(eng.ctx, up.aln.data_ptr(), n, up.cig.data_ptr(), len(A["cig"]), up.bq.data_ptr(),
                                                   len(A["bq"]) // 2, up.loc.data_ptr(), int(A["nl"]), int(lo), d_var.data_ptr(), var.ctypes.data,
                                                   n_var, d_ins.data_ptr(), len(ins), d_out.data_ptr(), ctypes.c_void_p(0)),
                   "smc_spike_indel_read_bits")
        return d_out.download(np.uint8, n_var * n).reshape(n_var, n)                      # (the default stream: behind the kernel)
    finally:
        d_var.free(); d_ins.free(); d_out.free()


def spike_rpb_records(A, bits: np.ndarray, gids: np.ndarray, p_idents: np.ndarray, first: np.ndarray):
    """The CSR smc_spike_rpb_counts takes for ONE listed variant of run `A`: `bits` its row of spike_read_bits, `gids` the run-wide ids
    of its covering barcodes (ascending), `p_idents` the identity of every read-name id of the run, `first` (bool per read-name id)
    whether the name is its barcode's first, file-wide -> (uint32 [len(gids) + 1] offsets, uint64 name identities, uint8 flags), a
    barcode's records in file order.  A flag carries bits 1 .. 3 of the record's byte (spike_indel_read_bits': alt0, alt1, touch; bit 3
    of spike_read_bits' bytes is 0)."""
    aln = A["aln"]
    idx = np.flatnonzero(bits & SPB_COVERS)
    bc = aln["bc_gid"][idx].astype(np.int64)
    idx = idx[np.argsort(bc, kind="stable")]
    per = np.bincount(bc, minlength=int(A["n_bc"]))
    gids = np.asarray(gids, np.int64)
    if int(per[gids].sum()) != len(idx):
        raise ValueError("spike_rpb_records: %d covering records, %d of them in the %d covering barcodes" % (len(idx), int(per[gids].sum()), len(gids)))
    off = np.zeros(len(gids) + 1, np.uint32)
    off[1:] = np.cumsum(per[gids])
    pair = aln["pair_gid"][idx]
    flag = (bits[idx] & (SPB_ALT | SPB_SINGLE | SPB_TOUCH)) | np.where(np.asarray(first, bool)[pair], SPB_FIRST, 0).astype(np.uint8)
    return off, np.ascontiguousarray(np.asarray(p_idents, np.uint64)[pair]), flag.astype(np.uint8)


def run_first_names(eng, groups: ReadGroups, p_idents, chrom: str = "?", lo: int = 0, nl: int = 0) -> np.ndarray:
    """bool per read-name id of a run (`p_idents`: their identities): the name is its barcode's first in the file - the names
    ReadGroups.masks keeps at threshold 0, where no draw passes (the seed does not matter)."""
    rule = DsRule(1.0, None, seed=0, level="read", groups=groups, thr=0)
    buf, n_words, _ = _run_read_masks(eng, groups, [rule], p_idents, chrom, lo, nl)
    try:
        words = buf.download(np.uint32, max(1, n_words))
    finally:
        buf.free()
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:len(p_idents)].astype(bool)


def _spike_rpb_flat(csrs, n_segs, head):
    """The record CSRs of the rows of one counts call, one after the other: csrs[g] = (offsets over n_segs[g] segments, name identities,
    flag bytes) -> (uint32 offsets over every segment, uint64 names, uint8 flags).  head(g): how a ValueError names row g."""
    rec_off, base = [np.zeros(1, np.int64)], 0
    for g, ((o, names, flags), n) in enumerate(zip(csrs, n_segs)):
        o = np.asarray(o, np.int64)
        if len(o) != n + 1 or len(names) != len(flags) or int(o[0]) != 0 or int(o[-1]) != len(names):
            raise ValueError("%s, %d offsets over %d names and %d flags" % (head(g), len(o), len(names), len(flags)))
        rec_off.append(o[1:] + base)
        base += len(names)
    cat = lambda k, dtype: np.concatenate([np.asarray(c[k], dtype) for c in csrs]) if len(csrs) else np.zeros(0, dtype)
    return np.concatenate(rec_off).astype(np.uint32), cat(1, np.uint64), cat(2, np.uint8)


def spike_rpb_counts(eng, positions, covers, records, seeds, thresholds, read_thresholds, four: bool = False) -> np.ndarray:
    """smc_spike_rpb_counts -> uint32 [V, R, T, Rr, 5] = (N', V0', S', READS', V1') of every variant, replicate and cell.  positions,
    covers, seeds, thresholds: spike_rep_counts'; records[v]: spike_rpb_records' (offsets [len(covers[v]) + 1], name identities, flag
    bytes) of variant v; read_thresholds: read_threshold(probKeep) per reads-per-barcode target.  `four` (--spikeIndelRpb):
    smc_spike_indel_rpb_counts - the flags' bits 2 and 3 are alt1 and touch."""
    n_var = len(covers)
    off = np.zeros(n_var + 1, np.uint32)
    off[1:] = np.cumsum([len(c) for c in covers])
    ident = np.concatenate([np.asarray(c, np.uint64) for c in covers]) if n_var else np.zeros(0, np.uint64)
    rec_off, name, flag = _spike_rpb_flat(records, [len(c) for c in covers],
                                          lambda v: "spike_rpb_counts: variant %d: %d covering barcodes" % (v, len(covers[v])))
    pos = np.array([int(p) & 0xFFFFFFFF for p in positions], np.uint32)
    seeds = np.ascontiguousarray(seeds, np.uint64)
    thr, rthr = np.ascontiguousarray(thresholds, np.uint64), np.ascontiguousarray(read_thresholds, np.uint64)
    entry = "smc_spike_indel_rpb_counts" if four else "smc_spike_rpb_counts"
    return _spike_counts_call(
        eng, entry, [ident, off, rec_off, name, flag, pos, seeds], (n_var, len(seeds), len(thr), len(rthr), 5),
        lambda d, d_out: getattr(eng.L, entry)(eng.ctx, d[0], d[1], off.ctypes.data, d[2], rec_off.ctypes.data, d[3], d[4], len(name),
                                                    d[5], n_var, d[6], len(seeds), thr.ctypes.data, len(thr), rthr.ctypes.data, len(rthr),
                                                    d_out, ctypes.c_void_p(0)))


def spike_grid_counts(eng, positions, covers, records, seeds, thresholds, frac_thresholds, read_thresholds) -> np.ndarray:
    """smc_spike_grid_counts -> uint32 [V, R, T, F, Rr, 5] = (N', V0', S', READS', V1') of every variant, replicate and cell (spike
    target x barcode fraction x reads-per-barcode target).  positions, covers, records, seeds, thresholds: spike_rpb_counts';
    frac_thresholds: frac_threshold(f) per fraction; read_thresholds: uint64 [R, F, Rr], read_threshold(probKeep) of every replicate's
    own (fraction, target) - grid_read_thresholds makes them."""
    n_var = len(covers)
    off = np.zeros(n_var + 1, np.uint32)
    off[1:] = np.cumsum([len(c) for c in covers])
    ident = np.concatenate([np.asarray(c, np.uint64) for c in covers]) if n_var else np.zeros(0, np.uint64)
    rec_off, name, flag = _spike_rpb_flat(records, [len(c) for c in covers],
                                          lambda v: "spike_grid_counts: variant %d: %d covering barcodes" % (v, len(covers[v])))
    pos = np.array([int(p) & 0xFFFFFFFF for p in positions], np.uint32)
    seeds = np.ascontiguousarray(seeds, np.uint64)
    thr, bthr = np.ascontiguousarray(thresholds, np.uint64), np.ascontiguousarray(frac_thresholds, np.uint64)
    rthr = np.ascontiguousarray(read_thresholds, np.uint64)
    if rthr.ndim != 3 or rthr.shape[:2] != (len(seeds), len(bthr)):
        raise ValueError("spike_grid_counts: read thresholds of shape %r for %d replicates x %d fractions" % (rthr.shape, len(seeds), len(bthr)))
    n_rr = int(rthr.shape[2])
    return _spike_counts_call(
        eng, "smc_spike_grid_counts", [ident, off, rec_off, name, flag, pos, seeds, rthr.reshape(-1)],
        (n_var, len(seeds), len(thr), len(bthr), n_rr, 5),
        lambda d, d_out: eng.L.smc_spike_grid_counts(eng.ctx, d[0], d[1], off.ctypes.data, d[2], rec_off.ctypes.data, d[3], d[4], len(name),
                                                     d[5], n_var, d[6], len(seeds), thr.ctypes.data, len(thr), bthr.ctypes.data, len(bthr),
                                                     d[7], rthr.ctypes.data, n_rr, d_out, ctypes.c_void_p(0)))


def grid_prob_keep(c, r: float):
    """ds.reads.withinMT.py:58's probKeep at target r from the counters of the barcodes a fraction keeps (dict or sequence of one,
    multi, multi_names), as philox_grid_rules computes it; None where no kept barcode has two or more names (it divides by zero)."""
    one, multi, multi_names = (c["one"], c["multi"], c["multi_names"]) if isinstance(c, dict) else c
    if multi_names == multi:
        return None
    return 1.0 * (float(r) - 1.0) * (one + multi) / (multi_names - multi)


def grid_read_thresholds(groups: ReadGroups, seeds, fractions, rpb_targets, flag: str = "--spikeGrid"):
    """(--spikeGrid) The read thresholds of every (replicate, fraction, target): ONE counts_frac_seeds launch gives the counters of the
    barcodes each seed keeps at each fraction, probKeep and read_threshold follow on the host exactly as philox_grid_rules makes them
    for one seed -> (uint64 [R, F, Rr] thresholds, float64 [R, F, Rr] probKeep).  ValueError: a (replicate, fraction) at which no kept
    barcode has two or more read names - it names the replicate, its seed and the fraction."""
    seeds = [int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds]
    c = groups.counts_frac_seeds(seeds, [frac_threshold(f) for f in fractions])
    thr = np.zeros((len(seeds), len(fractions), len(rpb_targets)), np.uint64)
    prob = np.zeros(thr.shape, np.float64)
    for j, s in enumerate(seeds):
        for k, f in enumerate(fractions):
            for q, r in enumerate(rpb_targets):
                p = grid_prob_keep(tuple(int(x) for x in c[j, k, 1:4]), r)
                if p is None:
                    raise ValueError("%s: replicate %d (seed %d), fraction %g: no barcode kept there has more than one read name, so "
                                     "ds.reads.withinMT.py's probKeep (:58) is not defined (it divides by zero)" % (flag, j, s, f))
                prob[j, k, q], thr[j, k, q] = p, read_threshold(p)
    return thr, prob


def _spike_joint_index(s, covers):
    """Phase set `s` -> (uint64 [n]: the identities of the barcodes that cover EVERY member, ascending; per member, in the set's order,
    int64 [n]: where each of them stands in covers[member])."""
    ids = [np.asarray(covers[k], np.uint64) for k in s.members]
    both = np.unique(functools.reduce(np.intersect1d, ids))
    orders = [np.argsort(x, kind="stable") for x in ids]
    return both, [o[np.searchsorted(x[o], both)] if len(both) else np.zeros(0, np.int64) for x, o in zip(ids, orders)]


def spike_joint(sets, covers, counters):
    """Per phase set (tools.spike_variants.PhaseSet) -> (uint64 [n]: the identities of the barcodes that cover EVERY member, ascending;
    uint32 [n, M, 3]: their (reads, alt0, single) at each member, in the set's order).  covers[v] / counters[v]: per listed variant
    its covering identities and their counters, as spike_rep_counts takes them - or, with four counters per covering barcode
    (spike_indel_counts': reads, alt0, alt1, touch), uint32 [n, M, 4]."""
    out = []
    for s in sets:
        both, at = _spike_joint_index(s, covers)
        first = np.asarray(counters[s.members[0]])
        width = int(first.shape[1]) if first.ndim == 2 else 3
        cnt = np.zeros((len(both), len(s.members), width), np.uint32)
        for m, k in enumerate(s.members):
            cnt[:, m] = np.asarray(counters[k], np.uint32).reshape(-1, width)[at[m]]
        out.append((both, cnt))
    return out


def _spike_joint_counts(eng, who: str, entry, width: int, lead_positions, joint, seeds, thresholds, depth_thresholds) -> np.ndarray:
    """The two wrappers below: the joint rows of `width` counters per member flattened as both entries take them, then `entry`."""
    G, seeds = len(joint), np.ascontiguousarray(seeds, np.uint64)
    thr, dthr = np.ascontiguousarray(thresholds, np.uint64), np.ascontiguousarray(depth_thresholds, np.uint64)
    cnts = [np.ascontiguousarray(c, np.uint32) for _, c in joint]
    for (ids, _), c in zip(joint, cnts):
        if c.ndim != 3 or c.shape[0] != len(ids) or c.shape[2] != width:
            raise ValueError("%s: %d joint barcodes, counters of shape %r (%d per member expected)" % (who, len(ids), c.shape, width))
    off = np.zeros(G + 1, np.uint32)
    off[1:] = np.cumsum([len(ids) for ids, _ in joint])
    set_m = np.array([c.shape[1] for c in cnts], np.uint32)
    cnt_off = np.zeros(G, np.uint32)
    if G > 1:
        cnt_off[1:] = np.cumsum([c.size for c in cnts])[:-1]
    ident = np.concatenate([np.asarray(ids, np.uint64) for ids, _ in joint]) if G else np.zeros(0, np.uint64)
    cnt = np.concatenate([c.reshape(-1) for c in cnts]) if G else np.zeros(0, np.uint32)
    pos = np.array([int(p) & 0xFFFFFFFF for p in lead_positions], np.uint32)
    return _spike_counts_call(
        eng, "smc_" + who, [ident, cnt, off, set_m, cnt_off, pos, seeds], (G, len(seeds), len(thr), len(dthr), 4),
        lambda d, d_out: entry(eng.ctx, d[0], d[1], d[2], off.ctypes.data, d[3], set_m.ctypes.data, d[4], d[5], G, d[6], len(seeds),
                               thr.ctypes.data, len(thr), dthr.ctypes.data, len(dthr), d_out, ctypes.c_void_p(0)))


def spike_phase_counts(eng, lead_positions, joint, seeds, thresholds, depth_thresholds) -> np.ndarray:
    """smc_spike_phase_counts -> uint32 [G, R, T, F, 4] = (N_ALL', V0_ALL', S_ALL', V1_ALL') of every phase set, replicate and cell.
    lead_positions[g]: the 1-based position of the set's leader; joint[g]: (uint64 [n_g] identities of the barcodes that cover every
    member, uint32 [n_g, M_g, 3] their (reads, alt0, single) per member) - spike_joint's; the rest as spike_depth_counts takes it."""
    return _spike_joint_counts(eng, "spike_phase_counts", eng.L.smc_spike_phase_counts, 3, lead_positions, joint, seeds, thresholds,
                               depth_thresholds)


def spike_indel_phase_counts(eng, lead_positions, joint, seeds, thresholds, depth_thresholds) -> np.ndarray:
    """smc_spike_indel_phase_counts -> spike_phase_counts' uint32 [G, R, T, F, 4] from joint[g]'s uint32 [n_g, M_g, 4] = (reads, alt0,
    alt1, touch) per member - spike_joint's over spike_indel_counts' counters."""
    return _spike_joint_counts(eng, "spike_indel_phase_counts", eng.L.smc_spike_indel_phase_counts, 4, lead_positions, joint, seeds,
                               thresholds, depth_thresholds)


def spike_joint_records(sets, covers, records):
    """Per phase set -> (uint64 [n]: the identities of the barcodes that cover EVERY member, ascending - spike_joint's first array;
    uint32 [n * M + 1]: the offsets of the (joint barcode, member) segments, barcode-major and the members in the set's order; uint64
    name identities; uint8 flag bytes) - what spike_phase_rpb_counts takes.  covers[v]: per listed variant its covering identities;
    records[v]: its spike_rpb_records CSR over them.  The members of one set may lie in different runs of the pre-pass: they are joined
    by identity.  A record that spans several members stands in the segment of each."""
    out = []
    for s in sets:
        both, at = _spike_joint_index(s, covers)
        n, M = len(both), len(s.members)
        start, length = np.zeros((n, M), np.int64), np.zeros((n, M), np.int64)
        base, pools = 0, []
        for m, k in enumerate(s.members):
            o, names, flags = records[k]
            o = np.asarray(o, np.int64)
            if len(o) != len(covers[k]) + 1 or len(names) != len(flags):
                raise ValueError("spike_joint_records: set %s, member %d: %d covering barcodes, %d offsets over %d names and %d flags" %
                                 (s.name, m, len(covers[k]), len(o), len(names), len(flags)))
            start[:, m], length[:, m] = o[at[m]] + base, o[at[m] + 1] - o[at[m]]
            base += len(names)
            pools.append((np.asarray(names, np.uint64), np.asarray(flags, np.uint8)))
        off = np.zeros(n * M + 1, np.int64)
        off[1:] = np.cumsum(length.reshape(-1))
        # (every segment's records, segment after segment: the index of record i of segment s is start[s] + i)
        take = np.repeat(start.reshape(-1) - off[:-1], length.reshape(-1)) + np.arange(int(off[-1]), dtype=np.int64)
        name = np.concatenate([p[0] for p in pools])[take] if int(off[-1]) else np.zeros(0, np.uint64)
        flag = np.concatenate([p[1] for p in pools])[take] if int(off[-1]) else np.zeros(0, np.uint8)
        out.append((both, off.astype(np.uint32), np.ascontiguousarray(name), np.ascontiguousarray(flag)))
    return out


def spike_phase_rpb_counts(eng, lead_positions, set_members, joint_records, seeds, thresholds, read_thresholds) -> np.ndarray:
    """smc_spike_phase_rpb_counts -> uint32 [G, R, T, Rr, 4] = (N_ALL', V0_ALL', S_ALL', V1_ALL') of every phase set, replicate and cell
    (spike target x reads-per-barcode target), counted over the reads each cell keeps.  lead_positions[g]: the 1-based position of the
    set's leader; set_members[g]: M_g; joint_records[g]: spike_joint_records' (joint identities [n_g], segment offsets [n_g * M_g + 1],
    name identities, flag bytes); seeds, thresholds, read_thresholds: spike_rpb_counts'."""
    G = len(joint_records)
    set_m = np.array([int(m) for m in set_members], np.uint32)
    off = np.zeros(G + 1, np.uint32)
    off[1:] = np.cumsum([len(j[0]) for j in joint_records])
    n_segs = [len(j[0]) * int(m) for j, m in zip(joint_records, set_m)]
    seg_base = np.cumsum([0] + n_segs)[:-1].astype(np.uint32)
    rec_off, name, flag = _spike_rpb_flat(
        [j[1:] for j in joint_records], n_segs,
        lambda g: "spike_phase_rpb_counts: set %d: %d joint barcodes of %d members" % (g, len(joint_records[g][0]), int(set_m[g])))
    ident = np.concatenate([np.asarray(j[0], np.uint64) for j in joint_records]) if G else np.zeros(0, np.uint64)
    pos = np.array([int(p) & 0xFFFFFFFF for p in lead_positions], np.uint32)
    seeds = np.ascontiguousarray(seeds, np.uint64)
    thr, rthr = np.ascontiguousarray(thresholds, np.uint64), np.ascontiguousarray(read_thresholds, np.uint64)
    return _spike_counts_call(
        eng, "smc_spike_phase_rpb_counts", [ident, off, set_m, seg_base, rec_off, name, flag, pos, seeds],
        (G, len(seeds), len(thr), len(rthr), 4),
        lambda d, d_out: eng.L.smc_spike_phase_rpb_counts(eng.ctx, d[0], d[1], off.ctypes.data, d[2], set_m.ctypes.data, d[3],
                                                          seg_base.ctypes.data, d[4], rec_off.ctypes.data, d[5], d[6], len(name), d[7], G,
                                                          d[8], len(seeds), thr.ctypes.data, len(thr), rthr.ctypes.data, len(rthr), d_out,
                                                          ctypes.c_void_p(0)))


SCAN_RPB_MAX_CELLS = 32           # SMC_AF_DEPTH_MAX_CELLS: spike targets x read thresholds of one counts call
SCAN_BITS_BUDGET = 256 << 20      # bytes of read bits (bit rows x alignments) one smc_scan_phase_rpb_counts call of the stage keeps in HBM


def run_barcode_major(A, p_idents, first) -> dict:
    """The run `A` in barcode-major order, as smc_scan_phase_rpb_counts takes it: ONE stable argsort of bc_gid, so a barcode's records
    stay in file order.  p_idents: the identity of every read-name id of the run; first: bool per read-name id, the name is its
    barcode's first, file-wide -> dict(bm_aln uint32 [n_aln]: the alignment's index in the run, bm_name uint64: the identity of its
    read name, bm_first uint8: 1 where that name is a first one, bc_start uint32 [n_bc + 1]: where each barcode's records begin)."""
    aln, n_bc = A["aln"], int(A["n_bc"])
    bc = aln["bc_gid"].astype(np.int64)
    if len(bc) and int(bc.max()) >= n_bc:
        raise ValueError("run_barcode_major: a record of barcode %d in a run of %d barcodes" % (int(bc.max()), n_bc))
    order = np.argsort(bc, kind="stable")
    pair = aln["pair_gid"][order]
    bc_start = np.zeros(n_bc + 1, np.uint32)
    bc_start[1:] = np.cumsum(np.bincount(bc, minlength=n_bc))
    return dict(bm_aln=order.astype(np.uint32), bm_name=np.ascontiguousarray(np.asarray(p_idents, np.uint64)[pair]),
                bm_first=np.asarray(first, bool)[pair].astype(np.uint8), bc_start=bc_start)


class RunOrder(object):
    """run_barcode_major's arrays and the barcodes' identities on the device, for every smc_scan_phase_rpb_counts call over one
    decoded run; `host`: the arrays as they went up (bc_start is the entry's host copy).  free() when the run goes."""

    def __init__(self, eng, order: dict, idents):
        self.host = dict(order, idents=np.ascontiguousarray(idents, np.uint64))
        self.n_aln, self.n_bc = len(order["bm_aln"]), len(order["bc_start"]) - 1
        if len(self.host["idents"]) < self.n_bc:
            raise ValueError("RunOrder: %d identities for %d barcodes" % (len(self.host["idents"]), self.n_bc))
        self.bufs = []
        try:
            for k in ("bm_aln", "bm_name", "bm_first", "bc_start", "idents"):
                self.bufs.append(_up8(eng, np.ascontiguousarray(self.host[k])))
        except BaseException:
            self.free()
            raise

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def scan_set_chunks(n_sets: int, members: int, n_aln: int, budget: int = None):
    """[(first set, end)]: a pass's sets cut so that the read bits of a chunk - `members` bit rows per set, n_aln bytes each - stay under
    `budget` bytes (SCAN_BITS_BUDGET unless given; one set at the least)."""
    per = max(1, int(SCAN_BITS_BUDGET if budget is None else budget) // max(1, int(members) * max(1, int(n_aln))))
    return [(a, min(n_sets, a + per)) for a in range(0, n_sets, per)]


def scan_phase_rpb_counts(eng, run_order: RunOrder, d_bits, n_var: int, rows, joint_gids, lead_positions, seeds, thresholds,
                          read_thresholds) -> np.ndarray:
    """smc_scan_phase_rpb_counts -> uint32 [rows, R, T, Rr, 4] = (N_ALL', V0_ALL', S_ALL', V1_ALL') of every row, replicate and cell,
    spike_phase_rpb_counts' words without a record CSR.  run_order: the decoded run's RunOrder; d_bits: spike_read_bits_dev's buffer of
    n_var x n_aln bytes, left in HBM; rows[g]: the indices of the bit rows of row g's members, in order (one index: a listed variant);
    joint_gids[g]: the run-wide ids of the barcodes that cover every member of row g, in any order; lead_positions[g]: the 1-based
    position row g is drawn with; seeds, thresholds, read_thresholds: spike_rpb_counts'."""
    G = len(rows)
    if len(joint_gids) != G or len(lead_positions) != G:
        raise ValueError("scan_phase_rpb_counts: %d rows, %d joint lists, %d positions" % (G, len(joint_gids), len(lead_positions)))
    row_off, joint_off = np.zeros(G + 1, np.uint32), np.zeros(G + 1, np.uint32)
    row_off[1:] = np.cumsum([len(r) for r in rows])
    joint_off[1:] = np.cumsum([len(j) for j in joint_gids])
    cat = lambda xs: np.concatenate([np.asarray(x, np.uint32).reshape(-1) for x in xs]) if G else np.zeros(0, np.uint32)
    row_var, joint_gid = np.ascontiguousarray(cat(rows)), np.ascontiguousarray(cat(joint_gids))
    pos = np.array([int(p) & 0xFFFFFFFF for p in lead_positions], np.uint32)
    seeds = np.ascontiguousarray(seeds, np.uint64)
    thr, rthr = np.ascontiguousarray(thresholds, np.uint64), np.ascontiguousarray(read_thresholds, np.uint64)
    o, bc_start = run_order.bufs, run_order.host["bc_start"]
    return _spike_counts_call(
        eng, "smc_scan_phase_rpb_counts", [row_off, row_var, joint_off, joint_gid, pos, seeds], (G, len(seeds), len(thr), len(rthr), 4),
        lambda d, d_out: eng.L.smc_scan_phase_rpb_counts(eng.ctx, o[0].data_ptr(), o[1].data_ptr(), o[2].data_ptr(), run_order.n_aln,
                                                         o[3].data_ptr(), bc_start.ctypes.data, o[4].data_ptr(), run_order.n_bc,
                                                         d_bits.data_ptr(), int(n_var), d[0], row_off.ctypes.data, d[1], row_var.ctypes.data,
                                                         d[2], joint_off.ctypes.data, d[3], d[4], G, d[5], len(seeds), thr.ctypes.data,
                                                         len(thr), rthr.ctypes.data, len(rthr), d_out, ctypes.c_void_p(0)))


def scan_phase_rpb_counts_rule(run_order, bits, rows, joint_gids, lead_positions, seeds, thresholds, read_thresholds, detail=None):
    """abi.scan_phase_rpb_counts_rule on scan_phase_rpb_counts' arguments (run_order: a RunOrder or its host dict; bits: uint8 [n_var,
    n_aln] on the host)."""
    h = run_order.host if isinstance(run_order, RunOrder) else run_order
    row_off, joint_off = np.cumsum([0] + [len(r) for r in rows]), np.cumsum([0] + [len(j) for j in joint_gids])
    cat = lambda xs: np.concatenate([np.asarray(x, np.int64).reshape(-1) for x in xs]) if len(xs) else np.zeros(0, np.int64)
    return abi.scan_phase_rpb_counts_rule(h["bm_aln"], h["bm_name"], h["bm_first"], h["bc_start"], h["idents"], bits, row_off, cat(rows),
                                          joint_off, cat(joint_gids), lead_positions, seeds, thresholds, read_thresholds, detail)


def spike_copy_strides(n_aln: int, n_pairs: int):
    """The byte strides between the copies of one smc_spike_alleles_reps call: a copy's records / pair pool rounded up to 256 bytes."""
    return (36 * max(1, n_aln) + 255) & ~255, (2 * max(1, n_pairs) + 255) & ~255


def spike_run_copies(eng, up: RunOnDevice, A, var: np.ndarray, idents, seeds, thresholds, mismatch_thr: float, nm, n_indel,
                     strides=None, fill=None):
    """smc_spike_alleles_reps over the run `up`: copy c with seeds[c] and every variant at thresholds[c] -> (the copies' records, their
    pair pools - two DevBufs, copy c at c x stride: free both -, (record stride, pool stride) in bytes, uint32 [copies, n_var, 2]
    statistics).  `strides`: other than spike_copy_strides'; `fill`: a byte both outputs are filled with first (tests)."""
    from .engine import DevBuf
    n, n_pairs, n_var, B = up.n_aln, len(A["bq"]) // 2, len(var), len(seeds)
    sa, sb = strides or spike_copy_strides(n, n_pairs)
    seeds, thr = np.ascontiguousarray(seeds, np.uint64), np.ascontiguousarray(thresholds, np.uint64)
    var, idents, tmp = _spike_inputs(eng, "spike_run_copies", up, A, var, abi.SPIKE_VARIANT_DTYPE, idents, nm, n_indel, (seeds, thr))
    tmp.append(DevBuf(eng, 8 * max(1, n_var * B) + 256))
    d_aln, d_bq = DevBuf(eng, sa * max(1, B) + 256), DevBuf(eng, sb * max(1, B) + 256)
    try:
        if fill is not None:
            d_aln.upload(np.full(sa * max(1, B), fill, np.uint8)); d_bq.upload(np.full(sb * max(1, B), fill, np.uint8))
        _lib.check(eng.L.smc_spike_alleles_reps(eng.ctx, up.aln.data_ptr(), n, up.cig.data_ptr(), up.bq.data_ptr(), n_pairs, tmp[0].data_ptr(),
                                                var.ctypes.data, n_var, tmp[1].data_ptr(), len(idents), seeds.ctypes.data, thr.ctypes.data, B,
                                                float(mismatch_thr), tmp[2].data_ptr(), tmp[3].data_ptr(), d_aln.data_ptr(), sa,
                                                d_bq.data_ptr(), sb, tmp[4].data_ptr(), ctypes.c_void_p(0)), "smc_spike_alleles_reps")
        stats = tmp[4].download(np.uint32, 2 * n_var * B).reshape(B, n_var, 2) if n_var * B else np.zeros((B, 0, 2), np.uint32)
    except BaseException:
        d_aln.free(); d_bq.free()
        raise
    finally:
        for b in tmp:
            b.free()
    return d_aln, d_bq, (sa, sb), stats


class _BufView(object):
    """A stretch of a DevBuf that reads like a buffer of its own (data_ptr, download); the owner frees the allocation."""

    def __init__(self, buf, offset_bytes: int):
        self.buf, self.off, self.word_bits = buf, int(offset_bytes), 32

    def data_ptr(self) -> int:
        return self.buf.data_ptr() + self.off

    def download(self, dtype, count: int, offset_bytes: int = 0):
        return self.buf.download(dtype, count, self.off + offset_bytes)

    def free(self):
        pass


def spike_indel_copy_strides(n_aln: int, cap_pairs: int, cap_cig: int):
    """The byte strides between the copies of one smc_spike_indels_reps call: a copy's records, its pair pool (128 bytes more, as
    smc_build_planes wants behind any pair pool) and its CIGAR pool at their capacities, each rounded up to 256 bytes."""
    return (36 * max(1, n_aln) + 255) & ~255, (2 * max(1, cap_pairs) + 128 + 255) & ~255, (4 * max(1, cap_cig) + 255) & ~255


def spike_indel_run_copies(eng, up: RunOnDevice, A, var: np.ndarray, ins: np.ndarray, idents, seeds, thresholds, mismatch_thr: float, nm, n_indel,
                           caps=None, strides=None, fill=None, mism: bool = False):
    """smc_spike_indels_reps over the run `up`: copy c with seeds[c] and every variant at thresholds[c] -> dict(aln, bq, cig: three
    DevBufs, copy c at c x its stride - free all three -, strides: (records, pair pool, CIGAR pool) in bytes, caps, stats: uint32
    [copies, n_var, 2], totals: uint64 [copies, 3], nm / n_indel: int32 [copies, n_aln] with `mism`).  `caps`: (cap_pairs, cap_cig),
    spike_indel_caps' bounds without it; `strides`: other than spike_indel_copy_strides'; `fill`: a byte the three outputs are
    filled with first (tests).  One download of all totals; SmcError when a copy did not fit spike_indel_caps' bounds."""
    from .engine import DevBuf
    n, n_pairs, n_cw, n_var, B = up.n_aln, len(A["bq"]) // 2, len(A["cig"]), len(var), len(seeds)
    seeds, thr = np.ascontiguousarray(seeds, np.uint64), np.ascontiguousarray(thresholds, np.uint64)
    var, idents, tmp = _spike_inputs(eng, "spike_indel_run_copies", up, A, var, abi.SPIKE_INDEL_VARIANT_DTYPE, idents, nm, n_indel, (seeds, thr))
    cap_pairs, cap_cig = caps if caps is not None else spike_indel_caps(A, var)
    sa, sb, sc = strides or spike_indel_copy_strides(n, cap_pairs, cap_cig)
    ins = np.ascontiguousarray(ins, np.uint8)
    nB = max(1, B)
    tmp += [_up8(eng, ins), DevBuf(eng, 8 * max(1, n_var) * nB + 256), DevBuf(eng, 24 * nB + 256), DevBuf(eng, 4 * max(1, n) * nB + 256),
            DevBuf(eng, 4 * max(1, n) * nB + 256)]
    out = [DevBuf(eng, sa * nB + 256), DevBuf(eng, sb * nB + 256), DevBuf(eng, sc * nB + 256)]
    try:
        if fill is not None:
            for b, st in zip(out, (sa, sb, sc)):
                b.upload(np.full(st * nB, fill, np.uint8))
        _lib.check(eng.L.smc_spike_indels_reps(eng.ctx, up.aln.data_ptr(), n, up.cig.data_ptr(), n_cw, up.bq.data_ptr(), n_pairs, tmp[0].data_ptr(),
                                               var.ctypes.data, n_var, tmp[4].data_ptr(), len(ins), tmp[1].data_ptr(), len(idents),
                                               seeds.ctypes.data, thr.ctypes.data, B, float(mismatch_thr), tmp[2].data_ptr(), tmp[3].data_ptr(),
                                               cap_pairs, cap_cig, out[0].data_ptr(), sa, out[1].data_ptr(), sb, out[2].data_ptr(), sc,
                                               tmp[7].data_ptr(), tmp[8].data_ptr(), tmp[5].data_ptr(), tmp[6].data_ptr(), ctypes.c_void_p(0)),
                   "smc_spike_indels_reps")
        totals = tmp[6].download(np.uint64, 3 * B).reshape(B, 3)                     # (the default stream: behind the kernels)
        stats = tmp[5].download(np.uint32, 2 * n_var * B).reshape(B, n_var, 2) if n_var * B else np.zeros((B, 0, 2), np.uint32)
        nm_out, n_indel_out = (tmp[7].download(np.int32, n * B).reshape(B, n), tmp[8].download(np.int32, n * B).reshape(B, n)) if mism and n \
            else (None, None)
        if caps is None and totals[:, 2].any():
            c = int(np.flatnonzero(totals[:, 2])[0])
            raise _lib.SmcError("smc_spike_indels_reps: copy %d needs %d pairs / %d CIGAR words, more than the bounds %d / %d" %
                                (c, int(totals[c, 0]), int(totals[c, 1]), cap_pairs, cap_cig))
    except BaseException:
        for b in out:
            b.free()
        raise
    finally:
        for b in tmp:
            b.free()
    return dict(aln=out[0], bq=out[1], cig=out[2], strides=(sa, sb, sc), caps=(cap_pairs, cap_cig), stats=stats, totals=totals, nm=nm_out,
                n_indel=n_indel_out)


class _SpikedCopies(object):
    """The spiked copies of the kept run `run` at one threshold, copy c with seeds[c], from one spike_run_copies call or, with `ins` (the
    chromosome's pool of inserted letters; `caps`: spike_indel_run_copies'), one spike_indel_run_copies call, whose buffers this owns
    until free().  runs[c]: copy c as a RunOnDevice - records and pair pool at c x their strides, the run's CIGAR pool or an indel copy's
    own at c x its stride with pairs_used from totals[c, 0], the run's loc and ref.  stats, strides, caps, totals: the call's."""

    def __init__(self, eng, run: AfRun, svar, seeds, thr: int, P, ins=None, caps=None):
        up, B = run.up, len(seeds)
        self.eng, self.run, self.seeds = eng, run, seeds
        args = (run.idents, seeds, [thr] * B, P.mismatchThr, run.mism[0], run.mism[1])
        if ins is None:
            aln, bq, self.strides, self.stats = spike_run_copies(eng, up, run.A, svar, *args)
            self.owned, self.caps, self.totals = [aln, bq], None, None
            cig, pairs = [up.cig] * B, [None] * B
        else:
            made = spike_indel_run_copies(eng, up, run.A, svar, ins, *args, caps=caps)
            aln, bq, self.strides, self.stats, self.caps, self.totals = (made[x] for x in ("aln", "bq", "strides", "stats", "caps", "totals"))
            self.owned = [aln, bq, made["cig"]]
            cig, pairs = [_BufView(made["cig"], c * self.strides[2]) for c in range(B)], [int(x) for x in self.totals[:, 0]]
        self.runs = [RunOnDevice(_BufView(aln, c * self.strides[0]), cig[c], _BufView(bq, c * self.strides[1]), up.loc, up.ref, up.n_aln,
                                 up.loc_host, pairs_used=pairs[c]) for c in range(B)]

    def addresses(self) -> dict:
        """scan_detect_keys' `copies` (indel copies)."""
        aln, bq, cig = (b.data_ptr() for b in self.owned)
        return dict(aln=aln, cig=cig, bq=bq, strides=self.strides, n_aln=self.run.up.n_aln, cap_pairs=self.caps[0])

    def check_reads(self, var_at, want_reads, variants, flag: str) -> None:
        """The rewrite's READS of every copy and variant of run.group (var_at[g]: where run.group[g] stands in the records) against the
        counts call's want_reads[c][g].  A difference raises RuntimeError naming `flag`."""
        for c, seed in enumerate(self.seeds):
            for g, k in enumerate(self.run.group):
                if int(self.stats[c, var_at[g], 0]) != int(want_reads[c][g]):
                    v = variants[k]
                    raise RuntimeError("%s: seed %d at %s:%d: the rewrite touched %d records, the counts call says %d" %
                                       (flag, int(seed), v.chrom, v.pos, int(self.stats[c, var_at[g], 0]), int(want_reads[c][g])))

    def check_carriers(self, c: int, on: RunOnDevice, counts, want, var, ins, variants, flag: str, what: str = ""):
        """(N, V1) of every variant of run.group (var, ins: af_run_variants' of them) by smc_allele_carriers on copy c or a selection of it
        (`on`, `counts`) against the counts call's want[g] -> (covers, carries).  A difference: RuntimeError naming `flag` and the cell `what`."""
        cov, car, _ = allele_carriers_run(self.eng, on, counts, self.run.lo, var, ins)
        for g, k in enumerate(self.run.group):
            mine, theirs = (int(cov[g].sum()), int(car[g].sum())), tuple(int(x) for x in want[g])
            if mine != theirs:
                v = variants[k]
                raise RuntimeError("%s: seed %d at %s:%d%s: the copy holds (N, V1) = %r, the counts call says %r" %
                                   (flag, int(self.seeds[c]), v.chrom, v.pos, what, mine, theirs))
        return cov, car

    def free(self):
        for b in self.owned:
            b.free()


def _copy_room(run: AfRun, svar, four: bool, n_selections: int = 0, by_read: bool = False, listed_slots: int = 0):
    """How many spiked copies of the kept run one rewrite call makes: as many as fit SPIKE_REP_BATCH_BYTES - a copy is its records and
    pair pool or, with `four` counters, records, both pools at their capacities and the call's scratch of 8 bytes per alignment -,
    AF_REP_BATCH_SLOTS read slots and SMC_SPIKE_MAX_COPIES, and at least one -> (copies, spike_indel_caps of `svar` on the run or None).
    `n_selections` (--spikeScanDepth: the fractions): a copy also has that many selections alive beside it (select_copies: records,
    orig_index and descriptors at their capacities), and copies x selections stays within SEL_MAX_SELECTIONS.  `by_read`
    (--spikeScanRpb: the selections are select_copies_reads', one per reads-per-barcode target): each also has the renumbering's
    scratch, 8 bytes per barcode id and read-name id.  `listed_slots` (--spikeScanBuild listed: the slots and umi_start entries of a
    copy's listed loci, listed_layout's stride + G): a copy takes those read slots of the batch, not the whole run's."""
    n, caps = run.up.n_aln, spike_indel_caps(run.A, svar) if four else None
    per_copy = sum(spike_indel_copy_strides(n, *caps)) + 8 * n if four else sum(spike_copy_strides(n, len(run.A["bq"]) // 2))
    per_copy += n_selections * (40 * max(1, n) + 16 * max(1, run.nl) + 16 +
                                (8 * (int(run.A["n_bc"]) + int(run.A["n_pair"])) if by_read else 0))
    return max(1, min(SPIKE_MAX_COPIES, SPIKE_REP_BATCH_BYTES // per_copy, AF_REP_BATCH_SLOTS // max(1, listed_slots or int(run.A["n_slots"]) + run.nl),
                      SEL_MAX_SELECTIONS // max(1, n_selections))), caps


def _spike_rep_call(eng, run: AfRun, svar, var_at, part_seeds, thr: int, want_reads, P, fasta, variants, max_depth, sampler, sampler_seed, bits,
                    cells=(), indel: dict = None, read_cells: dict = None):
    """The _SpikedCopies of a kept run at one target, one per seed of `part_seeds`, each built behind the other into one device batch
    (as _af_rep_call appends its selections) and the batch called with one plan -> (per copy the listed loci's raw rows, in the order
    of run.group), or NARROW.  var_at, want_reads: check_reads'.
    `cells` (--spikeDepth: (fraction, params) of the target's cells): every copy is also selected at each fraction with its own seed
    (select_run's philox rule) and built; a cell's selections share one device batch and one plan of their own, called with that
    cell's params -> (the copies' rows, per cell the same), or NARROW.
    `indel` (--spikeIndelReps: dict(ins: _SpikedCopies', want: per copy and variant of run.group the counts call's (N, V1), want_cells:
    per cell the same (N', V1'))): a relocated record's allele texts come from the copy (copy_allele_key); and beside READS every
    copy's N and V1 - on the copy, on its selection for a cell - must equal the counts call's.
    `read_cells` (--spikeRpb: dict(params: the VcParams of the target's cells, one per reads-per-barcode target, masks: per copy the
    address of its first keep mask - ReadGroups.masks with the copy's seed, one mask per target -, n_words: words per mask)): every
    copy is also selected per r by read name (select_run, level "read") and built; a cell's selections share one batch and one plan
    -> (the copies' rows, per cell the same), or NARROW.  With `indel` (--spikeIndelRpb) want_cells holds the cells' (N', V1') per
    reads-per-barcode target, and `read_cells` their "labels" for the message.  With "want_cells" and no `indel` (--spikeGrid: a
    cell per pair (f, r), the masks masks_grid's) every selection's (N', V1') is held against it the same way."""
    A, lo, B = run.A, run.lo, len(part_seeds)
    grid_want = read_cells.get("want_cells") if read_cells and indel is None else None
    if indel is not None or grid_want is not None:
        af_var, af_ins = af_run_variants([variants[k] for k in run.group], run.chrom, lo, fasta)
    flag = (read_cells.get("flag") or ("--spikeIndelRpb" if indel is not None else "--spikeRpb")) if read_cells else \
        "--spikeDepth" if cells else "--spikeReps"
    copies = _SpikedCopies(eng, run, svar, part_seeds, thr, P, indel["ins"] if indel is not None else None)

    def kept_copies(frac, read):
        """The B copies (`frac` None) or their selections at `frac` - `read` r: by read name at the r-th reads-per-barcode target -, with
        `indel` each checked against the counts call's (N, V1) before it is handed on.  With indel["bits"] (--spikePhaseRpb) the cover
        and carrier bits of the sets' members on the selection at `read` are kept as identities - kept.idents(): the identity of every
        barcode id of the selection -, key (variant, copy, read)."""
        for c, copy in enumerate(copies.runs):
            if read is not None:
                # (--spikeGrid: the batch's selections were made by one call; else one select_run per copy and target)
                picked = sels.of[read][c] if sels is not None else \
                    select_run(eng, copy, A, lo, d_mask=read_cells["masks"][c] + 4 * read_cells["n_words"] * read, level="read")
                cell, what = read, " x " + read_cells["labels"][read]
            elif frac is None:
                picked, cell, what = (copy, A, None), None, ""
            else:
                picked = select_run(eng, copy, A, lo, idents=run.idents, frac=frac, seed=int(part_seeds[c]))
                cell, what = cell_at[frac], " x fraction %g" % frac
            kept = _KeptRun(*picked, A, run.bam.allele_key, run.bam.barcode_name, lambda n: run.idents,
                            copy=copy if indel is not None else None, by_read=read is not None)
            if indel is not None:
                try:
                    cov, car = copies.check_carriers(c, kept.run, kept.counts, indel["want"][c] if cell is None else indel["want_cells"][cell][c],
                                                     af_var, af_ins, variants, "--spikeIndelReps", what)
                    if read is not None and indel.get("bits") is not None:
                        ids = kept.idents()
                        for g, k in enumerate(run.group):
                            if k in indel["members"]:
                                indel["bits"][(k, c, read)] = (ids[cov[g][:len(ids)]], ids[car[g][:len(ids)]])
                except BaseException:
                    kept.free()
                    raise
            elif grid_want is not None and read is not None:
                try:
                    copies.check_carriers(c, kept.run, kept.counts, grid_want[read][c], af_var, af_ins, variants, flag, what)
                except BaseException:
                    kept.free()
                    raise
            yield kept

    def batch_rows(Pb, frac, read=None):
        """kept_copies built into one batch and called with one plan at params `Pb`."""
        return _copy_rows(eng, run, variants, B, kept_copies(frac, read), Pb, bits, flag, fasta, max_depth, sampler, sampler_seed)
    cell_at = {frac: f for f, (frac, _) in enumerate(cells)}
    sels = None
    try:
        copies.check_reads(var_at, want_reads, variants, "--spikeReps")      # (the message names --spikeReps whichever flag is in force)
        full = batch_rows(P, None)
        if full == NARROW or not (cells or read_cells):
            return full
        of_cell = []
        for frac, Pc in cells:
            of_cell.append(batch_rows(Pc, frac))
            if of_cell[-1] == NARROW:
                return NARROW
        if read_cells and read_cells.get("copy_stride") is not None:
            # (--spikeGrid: the B copies at all F x Rr pairs by ONE smc_select_alignments_reads_copies call and one download)
            sels = select_copies_reads(eng, copies.runs, A, lo, read_cells["masks"][0], read_cells["n_words"], read_cells["copy_stride"],
                                       len(read_cells["params"]))
        for r, Pc in enumerate(read_cells["params"] if read_cells else ()):
            of_cell.append(batch_rows(Pc, None, r))
            if of_cell[-1] == NARROW:
                return NARROW
        return full, of_cell
    finally:
        if sels is not None:
            sels.free()
        copies.free()


def _grid_seed_masks(eng, read_rules, seeds, rep_thr, p_idents, chrom, lo, nl):
    """(--spikeGrid) The keep masks of every seed and pair (f, r) over a run's read-name identities in ONE device buffer - seed j's
    len(read_rules) masks at j x len(read_rules) x n_words words, the layout smc_select_alignments_reads_copies takes for a batch of
    consecutive seeds; one ReadGroups.masks_grid launch per seed, with that seed's own read thresholds rep_thr[j] ([F, Rr]).
    -> (the buffer, words per mask); the caller frees the buffer."""
    from .engine import DevBuf
    groups, Q = read_rules[0].groups, len(read_rules)
    n = len(p_idents)
    n_words = (n + 31) // 32
    d_id = DevBuf(eng, 8 * max(1, n) + 256).upload(np.ascontiguousarray(p_idents, np.uint64) if n else np.zeros(1, np.uint64))
    buf = DevBuf(eng, 4 * max(1, n_words * Q * len(seeds)) + 256)
    try:
        for j, s in enumerate(seeds):
            groups.masks_grid(d_id.data_ptr(), n, int(s), [r.bc_thr for r in read_rules], [int(t) for t in np.asarray(rep_thr[j]).reshape(-1)],
                              buf.data_ptr() + 4 * n_words * Q * j)
        st = groups.status()
    except BaseException:
        buf.free()
        raise
    finally:
        d_id.free()
    if st & RG_MISS:
        buf.free()
        raise bamio.BamError("--spikeGrid: the run %s:%d-%d has a read name the file-wide table does not hold (status %#x)"
                             % (chrom, lo + 1, lo + nl, st))
    return buf, n_words


def spike_replicates(path: str, fasta, variants, targets, params_list, seed: int, n_reps: int, eng, keep: dict, sampler: str = "reference",
                     sampler_seed: int = 0, nthreads: int = 0, max_reads: int = 128_000_000, depth: dict = None, phase: dict = None,
                     rpb: dict = None):
    """The replicate stage of --spikeReps.  Replicate j is --spikeAF with seed (seed + j) mod 2^64.  One smc_spike_rep_counts call
    gives (S, READS, V1) of every variant, replicate and target from what the pre-pass kept (spike_rules' `keep`) - no spiked copy is
    needed for them; then per kept run and target as many replicates as _copy_room allows are spiked by one smc_spike_alleles_reps
    call, built one behind the other and called with one plan.  Every copy's statistics are checked against the counts call's READS.
    -> dict(seeds, counts: uint32 [V, R, T, 3], rows: {(variant index, target index, replicate): the raw row string at the variant's
    locus}, times: seconds per part and the numbers of rewrite calls, builds and batches).
    `depth` (--spikeDepth: dict with "fracs" and the "params" of the T x F cells, targets outer): one smc_spike_depth_counts call gives
    "depth_counts", uint32 [V, R, T, F, 5], and every copy is also selected and built once per fraction (_spike_rep_call's `cells`):
    `rows` then also holds (variant index, T + t x F + f, replicate).  The copies' READS are checked against the f = 1 numbers, as
    without it.
    `phase` (--spikePhase: spike_rules' dict): the draws are the sets' (SpikeSet.lead_pos), and the result gets "phase_counts", uint32
    [G, R, T, 4] = (N_ALL, V0_ALL, S_ALL, V1_ALL) of every set, replicate and target from one smc_spike_phase_counts call, with
    `depth` also "phase_depth_counts", uint32 [G, R, T, F, 4], from a second (--spikeIndelPhase: smc_spike_indel_phase_counts, the
    joint rows then hold four counters per member).
    `rpb` (--spikeRpb: spike_rules' dict with "targets", the "params" of the T x Rr cells and their "rules"): one smc_spike_rpb_counts
    call with all R seeds over the records the pre-pass kept (keep["records"]) gives "rpb_counts", uint32 [V, R, T, Rr, 5]; every copy
    is also selected per r with the keep masks of ITS seed - one ReadGroups.masks call per seed and run - and built
    (_spike_rep_call's `read_cells`): `rows` then also holds (variant index, T + t x Rr + r, replicate).  With four counters
    (--spikeIndelRpb) the counts come from smc_spike_indel_rpb_counts and the copies from smc_spike_indels_reps; beside READS every copy's
    (N, V1), and every cell's (N', V1') on its selection, must equal the counts calls'.
    `rpb` with `phase` (--spikePhaseRpb: phase["joint_records"] from the pre-pass): one smc_spike_phase_rpb_counts call with all R
    seeds gives "phase_rpb_counts", uint32 [G, R, T, Rr, 4]; per copy and cell the AND over a set's members of the selection's cover and
    carrier bits must give its (N_ALL', V1_ALL') (_check_joint_bits).
    `rpb` with "fracs" (--spikeGrid): one smc_spike_grid_counts call with all R seeds and THEIR thresholds (rpb["rep_thr"]) gives
    "rpb_counts", uint32 [V, R, T, F x Rr, 5]; the masks of replicate j are masks_grid's with its seed and its thresholds; every copy
    is selected and built per pair (f, r), and each selection's (N', V1') must equal the counts call's."""
    import time
    from . import dsaf
    from .tools import spike_variants as sv
    t_start = time.perf_counter()
    T = len(targets)
    if T > SPIKE_MAX_TARGETS:
        raise ValueError("--spikeReps: %d --spikeAF targets, at most %d" % (T, SPIKE_MAX_TARGETS))
    seeds = dsaf.rep_seeds(seed, n_reps)
    thr = [sv.threshold(t) for t in targets]
    spikes = keep["spikes"]
    times = {"counts": 0.0, "calls": 0.0, "decode again": 0.0, "rewrites": 0, "builds": 0, "batches": 0}
    rows = {}
    max_depth = eng.L.smc_build_max_depth()
    try:
        t0 = time.perf_counter()
        # (--spikeIndelReps: four counters per covering barcode - the stride-4 entry)
        four = bool(keep["counters"]) and np.asarray(keep["counters"][0]).ndim == 2 and np.asarray(keep["counters"][0]).shape[1] == 4
        counts = (spike_indel_counts if four else spike_rep_counts)(eng, spikes.lead_pos, keep["covers"], keep["counters"], seeds, thr)
        depth_counts = None
        F = len(depth["fracs"]) if depth is not None else 0
        if depth is not None:
            depth_counts = (spike_indel_counts if four else spike_depth_counts)(eng, spikes.lead_pos, keep["covers"], keep["counters"], seeds, thr,
                                                                                [frac_threshold(f) for f in depth["fracs"]])
        phase_counts = phase_depth_counts = phase_rpb_counts = joint_bits = None
        if phase is not None and phase.get("joint"):
            lead = [spikes.lead_pos[s.members[0]] for s in phase["sets"]]
            joint_counts = spike_indel_phase_counts if four else spike_phase_counts
            phase_counts = joint_counts(eng, lead, phase["joint"], seeds, thr, [1 << 32])[:, :, :, 0]
            if depth is not None:
                phase_depth_counts = joint_counts(eng, lead, phase["joint"], seeds, thr, [frac_threshold(f) for f in depth["fracs"]])
        rpb_counts, read_rules = None, []
        if rpb is not None:
            grid = rpb.get("fracs") is not None
            F = len(rpb["rules"]) // T                             # (the cells of one target: Rr, or with --spikeGrid F x Rr)
            read_rules = rpb["rules"][:F]
            if grid:
                # (--spikeGrid: every replicate's own thresholds, made by the pre-pass; [V, R, T, F, Rr, 5] -> [V, R, T, F x Rr, 5])
                rpb_counts = spike_grid_counts(eng, spikes.lead_pos, keep["covers"], keep["records"], seeds, thr,
                                               [frac_threshold(f) for f in rpb["fracs"]], rpb["rep_thr"])
                rpb_counts = rpb_counts.reshape(rpb_counts.shape[:3] + (-1, 5))
            else:
                rpb_counts = spike_rpb_counts(eng, spikes.lead_pos, keep["covers"], keep["records"], seeds, thr, [r.thr for r in read_rules], four=four)
            if phase is not None and phase.get("joint_records"):
                # (--spikePhaseRpb: one call with all R seeds over the (joint barcode, member) records of the pre-pass)
                phase_rpb_counts = spike_phase_rpb_counts(eng, [spikes.lead_pos[s.members[0]] for s in phase["sets"]],
                                                          [len(s.members) for s in phase["sets"]], phase["joint_records"], seeds, thr,
                                                          [r.thr for r in read_rules])
                joint_bits, seen = {}, set()
        times["counts"] = time.perf_counter() - t0
        for run in keep["runs"]:
            if run.A is None:
                # (over the byte cap of the pre-pass: decoded and uploaded again)
                t0 = time.perf_counter()
                nl = run.load(path, fasta, eng, params_list[0], max_reads, nthreads, mism=True)
                if nl != run.nl:
                    raise bamio.BamError("--spikeReps: the run %s:%d-%d was decoded as %d loci, the pre-pass had %d" %
                                         (run.chrom, run.lo + 1, run.hi, nl, run.nl))
                times["decode again"] += time.perf_counter() - t0
            svar, sorder = spikes.chrom_variants(run.chrom, targets[0])
            var_at = [sorder.index(k) for k in run.group]
            # (--spikeGrid: a batch's copies are selected at all F x Rr pairs by one call - their selections live beside them)
            room, _ = _copy_room(run, svar, four, F, True) if rpb is not None and grid else _copy_room(run, svar, four)
            t0 = time.perf_counter()
            seed_masks, grid_masks = {}, None
            try:
                if rpb is not None and grid:
                    p_idents = pair_idents_or_refuse(run.bam, run.A, read_rules[0].flag, run.chrom, run.lo, run.nl)
                    grid_masks, n_words = _grid_seed_masks(eng, read_rules, seeds, rpb["rep_thr"], p_idents, run.chrom, run.lo, run.nl)
                    seed_masks = {j: (_BufView(grid_masks, 4 * n_words * F * j), n_words, None) for j in range(n_reps)}
                elif rpb is not None:
                    # (the keep masks of every reads-per-barcode target, per seed: one launch each over the run's read-name identities)
                    p_idents = pair_idents_or_refuse(run.bam, run.A, read_rules[0].flag, run.chrom, run.lo, run.nl)
                    for j in range(n_reps):
                        seed_masks[j] = _run_read_masks(eng, read_rules[0].groups, [dataclasses.replace(r, seed=seeds[j]) for r in read_rules],
                                                        p_idents, run.chrom, run.lo, run.nl)
                _spike_rep_targets(eng=eng, run=run, svar=svar, var_at=var_at, seeds=seeds, thr=thr, counts=counts, depth_counts=depth_counts,
                                   rpb_counts=rpb_counts,
                                   params_list=params_list, fasta=fasta, variants=variants, max_depth=max_depth, sampler=sampler,
                                   sampler_seed=sampler_seed, depth=depth, rpb=rpb, seed_masks=seed_masks, keep=keep, spikes=spikes,
                                   four=four, room=room, n_reps=n_reps, rows=rows, times=times, joint_bits=joint_bits,
                                   members={k for s in phase["sets"] for k in s.members} if joint_bits is not None else ())
                if joint_bits is not None:
                    seen.update(run.group)
                    _check_joint_bits(phase["sets"], seen, joint_bits, phase_rpb_counts, seeds, targets, rpb["targets"], read_rules[0].flag)
            finally:
                for buf, _, _ in seed_masks.values():
                    buf.free()
                if grid_masks is not None:
                    grid_masks.free()
            times["calls"] += time.perf_counter() - t0
            run.free()
    finally:
        free_af_runs(keep["runs"])
    times["stage"] = time.perf_counter() - t_start
    return dict(seeds=seeds, counts=counts, rows=rows, times=times, depth_counts=depth_counts, phase_counts=phase_counts,
                phase_depth_counts=phase_depth_counts, rpb_counts=rpb_counts, phase_rpb_counts=phase_rpb_counts)


def _check_joint_bits(sets, seen, joint_bits, counts, seeds, targets, rpb_targets, flag):
    """(--spikePhaseRpb) Every set whose members' runs are all done (`seen`: the variants so far): per copy and cell the AND over the
    members of the selection's cover / carrier identities (joint_bits[(variant, target, r, replicate)], dropped here) against (N_ALL',
    V1_ALL') of the counts call, uint32 [G, R, T, Rr, 4].  A difference raises RuntimeError."""
    for g, ps in enumerate(sets):
        if not all(k in seen for k in ps.members) or (ps.members[0], 0, 0, 0) not in joint_bits:
            continue
        for t in range(len(targets)):
            for r in range(len(rpb_targets)):
                for j in range(len(seeds)):
                    got = [joint_bits.pop((k, t, r, j)) for k in ps.members]
                    mine = [len(functools.reduce(np.intersect1d, [x[c] for x in got])) for c in (0, 1)]
                    if mine != [int(counts[g, j, t, r, c]) for c in (0, 3)]:
                        raise RuntimeError("%s: set %s, seed %d at %g x target %g: the copy's selection holds (N_ALL, V1_ALL) = %r, the counts "
                                           "call says %r" % (flag, ps.name, int(seeds[j]), targets[t], rpb_targets[r], mine,
                                                             [int(counts[g, j, t, r, c]) for c in (0, 3)]))


def _spike_rep_targets(*, eng, run, svar, var_at, seeds, thr, counts, depth_counts, rpb_counts, params_list, fasta, variants, max_depth, sampler,
                       sampler_seed, depth, rpb, seed_masks, keep, spikes, four, room, n_reps, rows, times, joint_bits=None, members=()):
    """spike_replicates' calls for one kept run: per target as many replicates per _spike_rep_call as `room` allows; `rows` and `times`
    are filled.  seed_masks[j] (--spikeRpb): _run_read_masks' of replicate j."""
    T = len(params_list)
    F = len(depth["fracs"]) if depth is not None else len(rpb["rules"]) // T if rpb is not None else 0
    cell_counts = depth_counts if depth is not None else rpb_counts      # (the cells' [V, R, T, F or Rr, 5]; --spikeGrid: [V, R, T, F x Rr, 5])
    for t in range(T):
        P = params_list[t]
        cells = [(depth["fracs"][f], depth["params"][t * F + f]) for f in range(F)] if depth is not None else []
        for b in range(0, n_reps, room):
            js = list(range(b, min(n_reps, b + room)))
            want = [[int(counts[k, j, t, 1]) for k in run.group] for j in js]
            args = (eng, run, svar, var_at, [seeds[j] for j in js], thr[t], want, P, fasta, variants, max_depth, sampler, sampler_seed)
            indel = None
            if four:
                n_cov = [len(keep["covers"][k]) for k in run.group]
                indel = dict(ins=spikes.ins[run.chrom], want=[[(n, int(counts[k, j, t, 2])) for k, n in zip(run.group, n_cov)] for j in js],
                             want_cells=[[[(int(cell_counts[k, j, t, f, 0]), int(cell_counts[k, j, t, f, 4])) for k in run.group]
                                          for j in js] for f in range(F)],
                             bits={} if joint_bits is not None else None, members=members)
            read_cells = None
            if rpb is not None:
                read_cells = dict(params=rpb["params"][t * F:(t + 1) * F], masks=[seed_masks[j][0].data_ptr() for j in js],
                                  n_words=seed_masks[js[0]][1], flag=rpb.get("flag"),
                                  labels=[("fraction %g x " % r.frac if r.grid else "") + "target %g" % r.target for r in rpb["rules"][:F]])
                if rpb.get("fracs") is not None:
                    # (--spikeGrid: every copy's cell is held against the counts call's (N', V1'), as the indel cells are)
                    read_cells["want_cells"] = [[[(int(cell_counts[k, j, t, f, 0]), int(cell_counts[k, j, t, f, 4])) for k in run.group]
                                                 for j in js] for f in range(F)]
                    # (the masks of the batch's consecutive seeds stand at one stride: one selection call for all copies and pairs)
                    read_cells["copy_stride"] = F * seed_masks[js[0]][1]
            def call(bits):
                times["rewrites"] += 1                                 # (a call that answers NARROW has spiked its copies too)
                return _spike_rep_call(*args, bits, cells, indel, read_cells)
            out = _narrow_retry(eng, P, call)
            full, of_cell = out if (cells or read_cells) else (out, [])
            if joint_bits is not None:
                for (k, c, r), val in indel["bits"].items():
                    joint_bits[(k, t, r, js[c])] = val
            for c, part in [(t, full)] + [(T + t * F + f, part) for f, part in enumerate(of_cell)]:
                for j, text in zip(js, part):
                    for k, line in zip(run.group, text):
                        rows[(k, c, j)] = line
            times["builds"] += len(js) * (1 + F)
            times["batches"] += 1 + F


# ---- --spikeScan: a measured detection rate at every locus of the target; the called batches' rows stay in HBM
SCAN_ALT_ID = {"A": 0, "T": 1, "G": 2, "C": 3}      # (pileup.BASE_ALLELES: the fixed allele ids smc_scan_detect compares cand[0] with)


def scan_detect(eng, d_rows, n_copies: int, n_loci: int, listed, threshold):
    """smc_scan_detect over the rows of a called batch in HBM (`d_rows`: n_copies x n_loci rows, e.g. Plan.run_into_devbuf's) ->
    (abi.SCAN_VERDICT_DTYPE [n_copies, G], the indices copy x G + listed locus of the records the host has to decide, ascending - the
    kernel appends them in no fixed order).  listed: abi.SCAN_LOCUS_DTYPE [G]; threshold: the truncated-PI cut of the .cut files."""
    from .engine import DevBuf
    listed = np.ascontiguousarray(listed, abi.SCAN_LOCUS_DTYPE)
    B, G = int(n_copies), len(listed)
    n = B * G
    bufs = [DevBuf(eng, listed.nbytes + 256).upload(listed.view(np.uint8).reshape(-1) if G else np.zeros(4, np.uint8)),
            DevBuf(eng, 16 * max(1, n) + 256), DevBuf(eng, 4 * max(1, n) + 256), DevBuf(eng, 256)]
    try:
        _lib.check(eng.L.smc_scan_detect(eng.ctx, d_rows.data_ptr() if d_rows is not None else None, B, int(n_loci), bufs[0].data_ptr(),
                                         listed.ctypes.data, G, float(threshold), bufs[1].data_ptr(), bufs[2].data_ptr(), bufs[3].data_ptr(),
                                         ctypes.c_void_p(0)), "smc_scan_detect")
        n_host = int(bufs[3].download(np.uint32, 1)[0])              # (the default stream: behind the kernel)
        rec = bufs[1].download(abi.SCAN_VERDICT_DTYPE, n) if n else np.zeros(0, abi.SCAN_VERDICT_DTYPE)
        if n_host > n:
            raise _lib.SmcError("smc_scan_detect: %d records for the host out of %d" % (n_host, n))
        todo = np.sort(bufs[2].download(np.uint32, n_host)) if n_host else np.zeros(0, np.uint32)
    finally:
        for b in bufs:
            b.free()
    return rec.reshape(B, G), todo


def scan_detect_sets(eng, d_rows, n_copies: int, n_loci: int, listed, set_off, threshold, records_of=None):
    """smc_scan_detect_sets over the rows of a called batch in HBM -> (uint32 [n_copies, n_sets]: the joint words (abi.scan_joint_rule),
    the indices copy x G + listed record of the HOST members of the sets whose joint verdict is HOST, ascending, and the member records
    abi.SCAN_VERDICT_DTYPE [len(records_of), G] of the copies `records_of` - all of them with None).  listed: abi.SCAN_LOCUS_DTYPE [G];
    set_off: uint32 [n_sets + 1], the sets' tiling of the listed records.  What comes down: 4 bytes per (copy, set), the list, and 16
    bytes per listed record of the copies asked for."""
    from .engine import DevBuf
    listed = np.ascontiguousarray(listed, abi.SCAN_LOCUS_DTYPE)
    set_off = np.ascontiguousarray(set_off, np.uint32)
    B, G, S = int(n_copies), len(listed), len(set_off) - 1
    n = B * G
    want = list(range(B)) if records_of is None else [int(c) for c in records_of]
    bufs = [DevBuf(eng, listed.nbytes + 256).upload(listed.view(np.uint8).reshape(-1) if G else np.zeros(4, np.uint8)),
            _up8(eng, set_off), DevBuf(eng, 16 * max(1, n) + 256), DevBuf(eng, 4 * max(1, B * S) + 256), DevBuf(eng, 4 * max(1, n) + 256),
            DevBuf(eng, 256)]
    try:
        _lib.check(eng.L.smc_scan_detect_sets(eng.ctx, d_rows.data_ptr() if d_rows is not None else None, B, int(n_loci), bufs[0].data_ptr(),
                                              listed.ctypes.data, G, bufs[1].data_ptr(), set_off.ctypes.data, S, float(threshold),
                                              bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr(), bufs[5].data_ptr(),
                                              ctypes.c_void_p(0)), "smc_scan_detect_sets")
        n_host = int(bufs[5].download(np.uint32, 1)[0])              # (the default stream: behind the kernel)
        if n_host > n:
            raise _lib.SmcError("smc_scan_detect_sets: %d records for the host out of %d" % (n_host, n))
        joint = bufs[3].download(np.uint32, B * S) if B * S and G else np.zeros(B * S, np.uint32)
        rec = np.zeros((len(want), G), abi.SCAN_VERDICT_DTYPE)
        for i, c in enumerate(want if G else ()):
            if not 0 <= c < B:
                raise ValueError("scan_detect_sets: the records of copy %d of %d" % (c, B))
            bufs[2].download(abi.SCAN_VERDICT_DTYPE, G, 16 * c * G, out=rec[i])
        todo = np.sort(bufs[4].download(np.uint32, n_host)) if n_host else np.zeros(0, np.uint32)
    finally:
        for b in bufs:
            b.free()
    return joint.reshape(B, S), todo, rec


def scan_joint_members(words, set_off) -> np.ndarray:
    """The member verdicts that smc_scan_detect_sets' joint words hold -> int64 [B, G]: member m of set s is CALLED / HOST / NOT by bit
    m of byte 0 / 1 / 2 of words[c, s]."""
    words = np.asarray(words, np.uint32)
    off = np.asarray(set_off, np.int64)
    out = np.zeros((words.shape[0], int(off[-1]) if len(off) else 0), np.int64)
    for s in range(len(off) - 1):
        for m in range(int(off[s + 1] - off[s])):
            w = words[:, s].astype(np.int64) >> m
            out[:, off[s] + m] = np.where(w & 1, abi.SCAN_CALLED, np.where((w >> abi.SCAN_JOINT_HOST_SHIFT) & 1, abi.SCAN_HOST, abi.SCAN_NOT))
    return out


def scan_detect_keys(eng, d_rows, n_copies: int, n_loci: int, var, ins, copies: dict, extras: dict, threshold):
    """smc_scan_detect_keys over the rows of a called batch in HBM -> scan_detect's pair and the resolved ids, uint32 [n_copies, G]
    (abi.SCAN_ID_NONE: no extras entry of the copy shows the key; abi.SCAN_ID_HOST: the host has to look).  var, ins:
    af_run_variants' records of the listed variants, `locus` ascending, and their pool of inserted letters.  copies: dict(aln, cig,
    bq: device addresses of copy 0's arrays, strides: the three byte strides - 0: shared -, n_aln, cap_pairs: the pairs of a copy's
    pool).  extras: dict(x, cnt: device addresses of copy 0's extras list and of its count, x_stride, cnt_stride: in words, xcap)."""
    from .engine import DevBuf
    var = np.ascontiguousarray(var, abi.AF_VARIANT_DTYPE)
    ins = np.ascontiguousarray(ins, np.uint8)
    B, G = int(n_copies), len(var)
    n = B * G
    bufs = [_up8(eng, var), _up8(eng, ins), DevBuf(eng, 4 * max(1, n) + 256), DevBuf(eng, 16 * max(1, n) + 256), DevBuf(eng, 4 * max(1, n) + 256),
            DevBuf(eng, 256)]
    sa, sb, sc = copies["strides"]
    try:
        _lib.check(eng.L.smc_scan_detect_keys(eng.ctx, d_rows.data_ptr() if d_rows is not None else None, B, int(n_loci), bufs[0].data_ptr(),
                                              var.ctypes.data, G, bufs[1].data_ptr(), len(ins), copies["aln"], int(sa), copies["cig"],
                                              int(sc), copies["bq"], int(sb), int(copies["n_aln"]), int(copies["cap_pairs"]), extras["x"],
                                              int(extras["x_stride"]), extras["cnt"], int(extras["cnt_stride"]), int(extras["xcap"]),
                                              float(threshold), bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr(),
                                              bufs[5].data_ptr(), ctypes.c_void_p(0)), "smc_scan_detect_keys")
        n_host = int(bufs[5].download(np.uint32, 1)[0])              # (the default stream: behind the kernels)
        rec = bufs[3].download(abi.SCAN_VERDICT_DTYPE, n) if n else np.zeros(0, abi.SCAN_VERDICT_DTYPE)
        ids = bufs[2].download(np.uint32, n) if n else np.zeros(0, np.uint32)
        if n_host > n:
            raise _lib.SmcError("smc_scan_detect_keys: %d records for the host out of %d" % (n_host, n))
        todo = np.sort(bufs[4].download(np.uint32, n_host)) if n_host else np.zeros(0, np.uint32)
    finally:
        for b in bufs:
            b.free()
    return rec.reshape(B, G), todo, ids.reshape(B, G)


def scan_filter(eng, d_rows, n_copies: int, n_loci: int, offsets, gate_bits, always_bits):
    """smc_scan_filter over the rows of a called batch in HBM -> uint32 [n_copies, G]: per copy and listed locus the FILTER column of
    the row as bits (abi.SCAN_FILTER_NAMES), abi.SCAN_FLT_HOST where the host has to print the row - it says something where the detect
    call's verdict is CALLED.  offsets: the listed loci within a copy; gate_bits, always_bits: spike.scan_filter_words' of the listed
    variants.  One upload of 12 bytes per listed locus, one launch, 4 bytes per record down."""
    from .engine import DevBuf
    B, G = int(n_copies), len(offsets)
    host = np.ascontiguousarray(np.stack([np.asarray(a, np.uint32).reshape(G) for a in (offsets, gate_bits, always_bits)]))
    n = B * G
    if not B and d_rows is None:                # (no copy, no rows: nothing to ask)
        return np.zeros((0, G), np.uint32)
    bufs = [DevBuf(eng, host.nbytes + 256).upload(host.view(np.uint8).reshape(-1) if G else np.zeros(4, np.uint8)), DevBuf(eng, 4 * max(1, n) + 256)]
    try:
        at = bufs[0].data_ptr()
        _lib.check(eng.L.smc_scan_filter(eng.ctx, d_rows.data_ptr() if d_rows is not None else None, B, int(n_loci), at, host[0].ctypes.data,
                                         at + 4 * G, host[1].ctypes.data, at + 8 * G, host[2].ctypes.data, G, bufs[1].data_ptr(),
                                         ctypes.c_void_p(0)), "smc_scan_filter")
        out = bufs[1].download(np.uint32, n) if n else np.zeros(0, np.uint32)      # (the default stream: behind the kernel)
    finally:
        for b in bufs:
            b.free()
    return out.reshape(B, G)


class ScanFilterSets:
    """What scan_filter_sets uploads, kept on the device for several calls: the listed loci's offsets, gate and always words and the
    sets' offsets - constants of a pass's variants in a run.  free() when done."""

    def __init__(self, eng, offsets, gate_bits, always_bits, set_off):
        from .engine import DevBuf
        G = len(offsets)
        self.host = np.ascontiguousarray(np.stack([np.asarray(a, np.uint32).reshape(G) for a in (offsets, gate_bits, always_bits)]))
        self.set_off = np.ascontiguousarray(set_off, np.uint32)
        self.bufs = [DevBuf(eng, self.host.nbytes + 256).upload(self.host.view(np.uint8).reshape(-1) if G else np.zeros(4, np.uint8)),
                     _up8(eng, self.set_off)]

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []


def scan_filter_sets(eng, d_rows, n_copies: int, n_loci: int, offsets, gate_bits, always_bits, set_off, members_of=None, consts=None):
    """smc_scan_filter_sets over the rows of a called batch in HBM -> (uint32 [n_copies, n_sets]: the joint FILTER words
    (abi.scan_filter_joint_rule), uint32 [len(members_of), G]: scan_filter's member words of the copies `members_of` - all of them with
    None).  offsets, gate_bits, always_bits: scan_filter's; set_off: uint32 [n_sets + 1], the sets' tiling of the listed loci.  One
    launch; 4 bytes per (copy, set) come down, and 4 per member of the copies asked for - the other member words stay in HBM.
    `consts` (a ScanFilterSets of the same four arrays): they are on the device already - nothing is uploaded."""
    from .engine import DevBuf
    B, G = int(n_copies), len(offsets)
    mine = consts if consts is not None else ScanFilterSets(eng, offsets, gate_bits, always_bits, set_off)
    host, set_off = mine.host, mine.set_off
    if host.shape[1] != G:
        raise ValueError("scan_filter_sets: the constants hold %d listed loci, the call names %d" % (host.shape[1], G))
    S, n = len(set_off) - 1, B * G
    want = list(range(B)) if members_of is None else [int(c) for c in members_of]
    bufs = list(mine.bufs) + [DevBuf(eng, 4 * max(1, n) + 256), DevBuf(eng, 4 * max(1, B * S) + 256)]
    try:
        at = bufs[0].data_ptr()
        _lib.check(eng.L.smc_scan_filter_sets(eng.ctx, d_rows.data_ptr() if d_rows is not None else None, B, int(n_loci), at,
                                              host[0].ctypes.data, at + 4 * G, host[1].ctypes.data, at + 8 * G, host[2].ctypes.data, G,
                                              bufs[1].data_ptr(), set_off.ctypes.data, S, bufs[2].data_ptr(), bufs[3].data_ptr(),
                                              ctypes.c_void_p(0)), "smc_scan_filter_sets")
        joint = bufs[3].download(np.uint32, B * S) if B * S and G else np.zeros(B * S, np.uint32)    # (the default stream: behind the kernel)
        mem = np.zeros((len(want), G), np.uint32)
        for i, c in enumerate(want if G else ()):
            if not 0 <= c < B:
                raise ValueError("scan_filter_sets: the member words of copy %d of %d" % (c, B))
            bufs[2].download(np.uint32, G, 4 * c * G, out=mem[i])
    finally:
        for b in bufs[2:]:
            b.free()
        if consts is None:
            mine.free()
    return joint.reshape(B, S), mem


def _filter_names(word: int) -> str:
    return ";".join(name for bit, name in abi.SCAN_FILTER_NAMES if word & bit) or "PASS"


def scan_called_host(text, v, threshold: int, repeats) -> bool:
    """Was `v` called in the raw row `text`, the way the replicate pages decide it: the row through the repeat filters and the .cut
    rule (dsaf.replicate_entry), then REF and ALT compared (spike._called)."""
    from . import dsaf, spike as _spike
    row, cut = dsaf.replicate_entry(text, threshold, *repeats)
    return bool(_spike._called(v, [(None, row, cut)]))


def _scan_call(eng, run: AfRun, svar, var_at, listed, part_seeds, thr: int, want_reads, P, fasta, variants, max_depth, sampler, sampler_seed,
               bits, threshold, repeats, check0, indel: dict = None, depth: dict = None, rpb: dict = None, flt: dict = None, build: dict = None,
               mnv: dict = None):
    """The _SpikedCopies of the run at one target, one per seed of `part_seeds`, each built behind the other into one device batch and
    the batch called with one plan - _spike_rep_call's way - but the rows stay in HBM: smc_scan_detect gives a verdict per (copy,
    listed locus), and only the rows it leaves to the host come down, one by one, to be printed and cut the existing way.  run.group:
    the pass's variants of this run; listed: their abi.SCAN_LOCUS_DTYPE records; check0: the copy that is replicate 0 (or None) - its
    listed rows come down as well, and a device verdict of CALLED or NOT that the host's decision does not share ends the run.
    -> (bool [copies, listed]: called, the number of verdicts the host decided), or NARROW.
    `indel` (--spikeScanIndel: dict(ins, caps: _SpikedCopies' - SmcError when a copy did not fit the caps -, var, var_ins:
    af_run_variants' records of run.group - they stand where `listed` does -, want: per copy and variant the counts call's (N, V1))):
    every build leaves its extras list in HBM and makes no table (BuildExtras); smc_scan_detect_keys resolves the key's allele id per
    copy from them; replicate 0's (N, V1) on the copy must be the counts call's; and the table of a row that comes down is made from
    its copy's extras, the texts through copy_allele_key on the copy, which is alive until this call returns.
    `depth` (--spikeScanDepth: dict(fracs, params, thresholds: per fraction the cell's VcParams and truncated-PI cut, var, var_ins:
    af_run_variants' records of run.group, want: per fraction, copy and variant the counts call's (N', V1'))): behind the full-depth
    batch ONE select_copies call makes the copies' selections at every fraction, each copy with its own seed; per fraction the B
    selections are built behind each other into one batch and called with one plan at the cell's params, the verdicts at the cell's
    cut - with `indel` the selections' records at the batched stride, the CIGAR words and pairs at the copies' -; replicate 0's (N',
    V1') by smc_allele_carriers on its selection must be the counts call's.
    -> (called, per fraction the same, the verdicts the host decided over all of them, 1 + the fractions built), or NARROW.
    `rpb` (--spikeScanRpb: dict(targets, params, thresholds: per reads-per-barcode target the cell's VcParams and cut, var, var_ins,
    want: as `depth`'s per target r, masks: the device address of the first copy's first keep mask, n_words: words per mask,
    copy_stride: words from a copy's masks to the next one's)): the same with ONE select_copies_reads call in place of select_copies
    - whole read names kept by the copy's seed's masks, the kept ids renumbered -, the builds told so (_KeptRun's by_read).
    `flt` (--spikeScanFilter: dict(gate, always: spike.scan_filter_words' of run.group)): behind every detect call smc_scan_filter
    gives the FILTER word per (copy, listed locus) from the same rows.  A CALLED record whose word has abi.SCAN_FLT_HOST joins the rows
    that come down, and so gets its FILTER from the printed row, as a HOST verdict the host calls does; replicate 0's CALLED rows come
    down anyway, and the names of the printed row must be the device word's.  flt["out"] is filled: per batch decided - full depth,
    then the cells in order - (uint32 [copies, listed]: the 14 name bits, meaningful where called, the records whose FILTER the host
    decided).
    `build` (--spikeScanBuild listed: a dict whose "listed", "whole" and "checks" are counted up): every batch is ONE _build_listed call
    - a dense batch of copies x listed loci, row c x G + g, every table from the copy's extras entries - in place of a whole build per
    copy (with `indel` the entry writes g into its extras entries' locus field, the stretches stay in HBM and smc_scan_detect_keys gets
    n_loci = G and variant records whose locus is g); a batch the listed builder declines is built the whole way and counted under
    "whole"; the listed
    rows of replicate 0 are also made by a whole build of that one copy, and a row that differs in a byte ends the run.
    `mnv` (--spikeScanMnv: dict(set_off: the tiling of run.group by phase sets, var, var_ins: af_run_variants' records of run.group,
    want: per copy and member the counts call's (N, V1), want_joint: per copy and set smc_spike_phase_counts' (N_ALL, V1_ALL)); not
    with `indel`, `rpb` or `flt`): the verdicts come from smc_scan_detect_sets - the joint words, the list and replicate 0's
    member records come down, the member verdicts of the other copies are read from the words' bits.  Only the HOST members of sets
    whose joint verdict is HOST are decided by the host; replicate 0's member rows come down anyway, are decided the host way and
    held against the device's member verdicts, and the joint verdict against their AND; replicate 0's (N, V1) per member and (N_ALL,
    V1_ALL) per set are counted a second time, by smc_allele_carriers' cover and carrier bits on the spiked copy and their AND over
    the members.  mnv["out"] is filled: (bool [copies, sets]: the MNV was called, the joint verdicts the host decided).
    `mnv` with "gate" and "always" (--spikeScanMnvFilter: spike.scan_filter_words' of run.group): behind every smc_scan_detect_sets call
    smc_scan_filter_sets gives the joint FILTER word per (copy, set) from the same rows; the member words stay in HBM but replicate
    0's.  The host reads a joint word only where the set ends CALLED.  Every member row of a set whose joint verdict is HOST, and of a
    set the device calls whose joint FILTER word has abi.SCAN_FLT_HOST, comes down and is printed the existing way; where such a set
    ends CALLED its joint word is made from the printed rows' FILTER columns (spike.scan_filter_of_text, abi.scan_filter_joint_rule).
    Replicate 0: the names of each printed row of a called member must be the device's member word, and the joint words
    abi.scan_filter_joint_rule of the member words.  mnv["flt_out"] is filled: (uint32 [copies, sets]: the joint words without bit 31,
    meaningful where the set is called, the called sets whose FILTER the host decided).
    `mnv` beside `depth` (--spikeScanMnvDepth; mnv["want_joint_cells"]: per fraction, copy and set the counts call's (N_ALL', V1_ALL')):
    `depth`'s cells with the joint verdicts per cell - the ONE select_copies call, every fraction's selections one batch, decided at the
    cell's params and cut by smc_scan_detect_sets (and smc_scan_filter_sets); replicate 0's (N_ALL', V1_ALL') of every cell is counted
    a second time, the AND over the members of smc_allele_carriers' bits on its selection.  mnv["out"] and mnv["flt_out"] are LISTS:
    full depth first, then the cells in order.
    `mnv` beside `rpb` (--spikeScanMnvRpb; mnv["want_joint_cells"]: per r, copy and set smc_scan_phase_rpb_counts' (N_ALL', V1_ALL')):
    `rpb`'s cells with the joint verdicts per cell in the same way - the ONE select_copies_reads call, every r's selections one batch."""
    from . import dsaf, spike as _spike, vc
    from .engine import DevBuf
    A, lo, nl, chrom = run.A, run.lo, run.nl, run.chrom
    B, G = len(part_seeds), len(run.group)
    flag, entry = ("--spikeScan", "smc_scan_detect") if indel is None else ("--spikeScanIndel", "smc_scan_detect_keys")
    if mnv is not None:
        flag, entry = "--spikeScanMnv", "smc_scan_detect_sets"
    copies = _SpikedCopies(eng, run, svar, part_seeds, thr, P, *((indel["ins"], indel.get("caps")) if indel is not None else ()))
    runs, extras, xbufs, sels = copies.runs, None, [], None
    fconsts = {}                                # (--spikeScanMnvFilter: scan_filter_sets' constants on the device, by layout)

    def decide(kept_runs, Pb, cut, where, key_of, what, shared=False):
        """`kept_runs` built into one batch and called with one plan at params `Pb`; the verdicts at the cut `cut` -> (called, the
        verdicts the host decided), or NARROW.  where: scan_detect_keys' `copies` of these builds; key_of(c): allele_key of build c;
        shared: the builds are spiked copies of one run (one barcode-major order serves a listed build of them)."""
        d = d_rows = plan = None
        held, xl, n_rows, spots = [], None, nl, listed          # held: the _KeptRuns a listed build leaves to this call to free
        xkeep = None                                            # (a listed build of `indel`: its extras stretches and counts, in HBM)
        try:
            if build is not None:
                held = list(kept_runs)
                got = _build_listed(eng, run, held, [int(a) for a in listed["offset"]], Pb, bits, sampler, sampler_seed, shared, dense=indel is not None)
                if got == NARROW:
                    return NARROW
                if got is None:
                    kept_runs, held = iter(held), []            # (declined: the whole way, which frees each behind its build)
                else:
                    d, xl, xkeep = got
                    build["listed"] += B
                    n_rows, spots = G, listed.copy()
                    spots["offset"] = np.arange(G)
            if d is None:
                built = _build_copies(eng, run, B, kept_runs, Pb, bits, flag, fasta, max_depth, sampler, sampler_seed, extras)
                if built == NARROW:
                    return NARROW
                d = built
                if build is not None:
                    build["whole"] += B
            plan = eng.make_plan(d.loci())
            d_rows = plan.run_into_devbuf([d.words, d.uaux[0]], Pb)
            row_at = (lambda i, a: i) if xl is not None else (lambda i, a: (i // G) * nl + a)
            if xl is not None:
                keys_of = {}
                if check0 is not None:
                    if indel is not None:
                        keys_of[check0] = key_of(check0)         # (a selection's key asks for its orig_index: before the check frees it)
                    _check_listed_rows(eng, run, held, check0, d_rows, listed, Pb, bits, flag, fasta, max_depth, sampler, sampler_seed, variants, what)
                    build["checks"] += G

                def table_of(c, a):
                    if c not in keys_of:                        # (with `indel` a relocated record's texts come from the copy: key_of)
                        keys_of[c] = held[c].allele_key if indel is None else key_of(c)
                    return extras_table(xl[c], a, keys_of[c], chrom, lo, fasta)
                if mnv is not None:
                    words_j, todo, rec0 = scan_detect_sets(eng, d_rows, B, G, spots, mnv["set_off"], cut, [] if check0 is None else [check0])
                elif indel is None:
                    rec, todo = scan_detect(eng, d_rows, B, G, spots, cut)
                else:
                    # (a copy has G rows: the variant records name the dense locus, as the entries of the listed build do)
                    var = np.array(indel["var"], abi.AF_VARIANT_DTYPE)
                    var["locus"] = np.arange(G)
                    rec, todo, _ = scan_detect_keys(
                        eng, d_rows, B, G, var, indel["var_ins"], where,
                        dict(x=xkeep["x"].data_ptr(), cnt=xkeep["cnt"].data_ptr(), x_stride=5 * xkeep["xcap"], cnt_stride=2, xcap=xkeep["xcap"]), cut)
            elif mnv is not None:
                words_j, todo, rec0 = scan_detect_sets(eng, d_rows, B, nl, listed, mnv["set_off"], cut, [] if check0 is None else [check0])
                table_of = lambda c, a: d.tables[c * nl + a]
            elif indel is None:
                rec, todo = scan_detect(eng, d_rows, B, nl, listed, cut)         # (its downloads wait for the plan's kernels)
                table_of = lambda c, a: d.tables[c * nl + a]
            else:
                rec, todo, _ = scan_detect_keys(
                    eng, d_rows, B, nl, indel["var"], indel["var_ins"], where,
                    dict(x=xbufs[0].data_ptr(), cnt=xbufs[1].data_ptr(), x_stride=5 * xcap, cnt_stride=2, xcap=xcap), cut)
                lists, keys = {}, {}

                def table_of(c, a):
                    if c not in lists:
                        n_x = min(int(extras[c].n), xcap)
                        lists[c] = extras[c].x.download(np.uint32, 5 * n_x).reshape(n_x, 5) if n_x else np.zeros((0, 5), np.uint32)
                        keys[c] = key_of(c)
                    return extras_table(lists[c], a, keys[c], chrom, lo, fasta)
            if mnv is not None:
                # (the member verdicts of every copy from the joint words' bits; the records of replicate 0 alone came down)
                verdict = scan_joint_members(words_j, mnv["set_off"])
                rec = np.zeros((B, G), abi.SCAN_VERDICT_DTYPE)
                rec["mt_verdict"] = verdict.astype(np.uint32) << 30
                if check0 is not None:
                    if not np.array_equal(rec0[0]["mt_verdict"] >> 30, verdict[check0]):
                        raise RuntimeError("%s: %s:%d-%d%s: the joint words' member bits are not the member records' verdicts" %
                                           (flag, chrom, lo + 1, lo + nl, what))
                    rec[check0] = rec0[0]
                want_list = abi.scan_joint_rule(verdict, mnv["set_off"])
                if not np.array_equal(want_list[0], words_j):
                    raise RuntimeError("%s: %s:%d-%d%s: a joint word is not the joint rule of its member bits" % (flag, chrom, lo + 1, lo + nl, what))
            else:
                verdict = (rec["mt_verdict"] >> 30).astype(np.int64)
            called = verdict == abi.SCAN_CALLED
            words, fhost, n_fhost = None, set(), 0
            if flt is not None:
                words = scan_filter(eng, d_rows, B, n_rows, spots["offset"], flt["gate"], flt["always"])
                fhost = set(int(x) for x in np.flatnonzero((called & ((words & abi.SCAN_FLT_HOST) != 0)).reshape(-1)))
            jflt = mnv is not None and mnv.get("gate") is not None       # (--spikeScanMnvFilter)
            fsets, seen_of = [], {}
            if jflt:
                off = np.asarray(mnv["set_off"], np.int64)
                # (the offsets, the two words per member and the sets' offsets go up once per layout - the run's offsets, or 0 .. G-1
                # of a listed build - and serve full depth and every cell)
                if (xl is not None) not in fconsts:
                    fconsts[xl is not None] = ScanFilterSets(eng, spots["offset"], mnv["gate"], mnv["always"], mnv["set_off"])
                words_f, mem0 = scan_filter_sets(eng, d_rows, B, n_rows, spots["offset"], mnv["gate"], mnv["always"], mnv["set_off"],
                                                 [] if check0 is None else [check0], consts=fconsts[xl is not None])
                if check0 is not None and not np.array_equal(abi.scan_filter_joint_rule(mem0, mnv["set_off"])[0], words_f[check0]):
                    raise RuntimeError("--spikeScanMnvFilter: replicate 0 at %s:%d-%d%s: a joint FILTER word is not the joint rule of its "
                                       "member words" % (chrom, lo + 1, lo + nl, what))
                # (the sets whose FILTER the host may have to decide: every member row comes down - a set the host has to call, and a
                # set the device calls whose joint FILTER word has bit 31)
                jv_f = (words_j >> 30).astype(np.int64)
                fsets = [(int(c), int(s_)) for c, s_ in zip(*np.nonzero((jv_f == abi.SCAN_HOST) |
                                                                       ((jv_f == abi.SCAN_CALLED) & ((words_f & abi.SCAN_FLT_HOST) != 0))))]
                fhost = set(c * G + g for c, s_ in fsets for g in range(int(off[s_]), int(off[s_ + 1])))
            theirs = set(int(x) for x in todo)
            if theirs != (set(int(x) for x in want_list[1]) if mnv is not None else
                          set(int(x) for x in np.flatnonzero(verdict.reshape(-1) == abi.SCAN_HOST))):
                raise RuntimeError("%s: %s:%d-%d%s: the list of the records for the host is not that of the HOST verdicts" %
                                   (flag, chrom, lo + 1, lo + nl, what))
            mine = sorted(theirs | fhost | (set(check0 * G + g for g in range(G)) if check0 is not None else set()))
            if mine:
                at = [int(listed["offset"][i % G]) for i in mine]
                got = np.empty(len(mine), abi.ROW_DTYPE)
                for n, (i, a) in enumerate(zip(mine, at)):
                    d_rows.download(abi.ROW_DTYPE, 1, row_at(i, a) * abi.ROW_DTYPE.itemsize, out=got[n:n + 1])
                view = vc.LocusView([chrom] * len(mine), [lo + 1 + a for a in at], [run.run_ref[a] if a < len(run.run_ref) else "" for a in at],
                                    [table_of(i // G, a) for i, a in zip(mine, at)])
                text = vc._strings(got, view, Pb, fasta)
                for i, line in zip(mine, text):
                    v = variants[run.group[i % G]]
                    if line.startswith(vc.EXC_PREFIX):
                        raise RuntimeError("%s: %s:%d%s: the row of seed %d could not be printed:\n%s" %
                                           (flag, v.chrom, v.pos, what, int(part_seeds[i // G]), line))
                    host = scan_called_host(line, v, cut, repeats)
                    if i in theirs or (mnv is not None and verdict[i // G, i % G] == abi.SCAN_HOST):
                        called[i // G, i % G] = host        # (mnv: replicate 0's HOST member beside a NOT one - not listed, decided anyway)
                    elif host != bool(called[i // G, i % G]):
                        # (only replicate 0's rows come down here beside the host's own - unless the keys of `indel` or the joint
                        # FILTER words bring rows of other copies down: then the message names the copy's seed)
                        who = "replicate 0 of" if indel is None and not jflt else "seed %d at" % int(part_seeds[i // G])
                        raise RuntimeError("%s: %s %s:%d %s>%s%s: %s says %s (PI %.17g, threshold %d), the row as "
                                           "the run would print and cut it says %s:\n%s" %
                                           (flag, who, v.chrom, v.pos, v.ref, v.alt, what, entry,
                                            "CALLED" if called[i // G, i % G] else "NOT", float(rec[i // G, i % G]["pi"]),
                                            cut, "called" if host else "not called", line))
                    if jflt and host:
                        seen_of[i] = _spike.scan_filter_of_text(dsaf.replicate_entry(line, cut, *repeats)[0][-1])
                        # (replicate 0: the names of a called member's printed row are the device's member word, unless that has bit 31)
                        if check0 is not None and i // G == check0 and not int(mem0[0, i % G]) & abi.SCAN_FLT_HOST and \
                                seen_of[i] != int(mem0[0, i % G]) & abi.SCAN_FLT_NAMES_MASK:
                            raise RuntimeError("--spikeScanMnvFilter: seed %d at %s:%d %s>%s%s: smc_scan_filter_sets says %#x (%s), the row "
                                               "as the run would print it says %#x (%s):\n%s" %
                                               (int(part_seeds[i // G]), v.chrom, v.pos, v.ref, v.alt, what, int(mem0[0, i % G]),
                                                _filter_names(int(mem0[0, i % G])), seen_of[i], _filter_names(seen_of[i]), line))
                    if flt is not None and host:
                        seen = _spike.scan_filter_of_text(dsaf.replicate_entry(line, cut, *repeats)[0][-1])
                        if i in theirs or i in fhost:
                            words[i // G, i % G] = seen
                            n_fhost += 1
                        elif seen != int(words[i // G, i % G]) & abi.SCAN_FLT_NAMES_MASK:
                            raise RuntimeError("--spikeScanFilter: seed %d at %s:%d %s>%s%s: smc_scan_filter says %#x (%s), the row as the "
                                               "run would print it says %#x (%s):\n%s" %
                                               (int(part_seeds[i // G]), v.chrom, v.pos, v.ref, v.alt, what, int(words[i // G, i % G]),
                                                _filter_names(int(words[i // G, i % G])), seen, _filter_names(seen), line))
            if flt is not None:
                flt["out"].append((words & np.uint32(abi.SCAN_FLT_NAMES_MASK), n_fhost))
            if mnv is not None:
                # (every member of replicate 0 was decided the host way above: `called` holds the host's answers there, so the AND over
                # a set's members is the host's joint verdict - the device's NOT must agree with it)
                off = np.asarray(mnv["set_off"], np.int64)
                jv = (words_j >> 30).astype(np.int64)
                all_called = np.logical_and.reduceat(called, off[:-1], axis=1) if G else np.zeros((B, 0), bool)
                if check0 is not None and bool((all_called[check0] & (jv[check0] == abi.SCAN_NOT)).any()):
                    raise RuntimeError("%s: replicate 0 at %s:%d-%d%s: a set whose members the host all calls has the joint verdict NOT" %
                                       (flag, chrom, lo + 1, lo + nl, what))
                mnv["out"].append((all_called & (jv != abi.SCAN_NOT), int((jv == abi.SCAN_HOST).sum())))
                if jflt:
                    # (a called set whose FILTER the host decides: its joint word from the printed rows' FILTER columns)
                    n_jhost = 0
                    for c, s_ in fsets:
                        if mnv["out"][-1][0][c, s_]:
                            mine_w = [[seen_of[c * G + g] for g in range(int(off[s_]), int(off[s_ + 1]))]]
                            words_f[c, s_] = abi.scan_filter_joint_rule(mine_w, [0, len(mine_w[0])])[0, 0]
                            n_jhost += 1
                    mnv["flt_out"].append((words_f & np.uint32(~abi.SCAN_FLT_HOST & 0xFFFFFFFF), n_jhost))
            return called, len(theirs)
        finally:
            if plan is not None:
                plan.close()
            for b in (d_rows, d) + ((xkeep["x"], xkeep["cnt"]) if xkeep is not None else ()):
                if b is not None:
                    b.free()
            for k in held:
                k.free()
    if flt is not None:
        flt["out"] = []                         # (a narrower retry starts over)
    if mnv is not None:
        mnv["out"], mnv["flt_out"] = [], []     # (per batch decided: full depth first, then the cells in order)
    try:
        if indel is not None and copies.totals[:, 2].any():
            raise _lib.SmcError("smc_spike_indels_reps: a copy of %s:%d-%d did not fit spike_indel_caps' bounds" % (chrom, lo + 1, lo + nl))
        copies.check_reads(var_at, want_reads, variants, flag)
        if mnv is not None and check0 is not None:
            cov1, car1 = copies.check_carriers(check0, runs[check0], A, mnv["want"][check0], mnv["var"], mnv["var_ins"], variants, flag)
            for s_, (a, b) in enumerate(zip(mnv["set_off"][:-1], mnv["set_off"][1:])):
                mine = (int(cov1[a:b].all(axis=0).sum()), int(car1[a:b].all(axis=0).sum()))
                if mine != tuple(int(x) for x in mnv["want_joint"][check0][s_]):
                    v = variants[run.group[int(a)]]
                    raise RuntimeError("%s: seed %d, the set at %s:%d: the AND of the copy's cover and carrier bits holds (N_ALL, V1_ALL) = "
                                       "%r, the counts call says %r" % (flag, int(part_seeds[check0]), v.chrom, v.pos, mine,
                                                                        tuple(int(x) for x in mnv["want_joint"][check0][s_])))
        if indel is not None:
            if check0 is not None:
                copies.check_carriers(check0, runs[check0], A, indel["want"][check0], indel["var"], indel["var_ins"], variants, flag)
            xcap = build_xcap(nl)
            xbufs += [DevBuf(eng, 20 * xcap * B + 256), DevBuf(eng, 8 * B + 256)]
            extras = [BuildExtras(_BufView(xbufs[0], 20 * xcap * c), _BufView(xbufs[1], 8 * c)) for c in range(B)]
        # (every alignment is there: the decoder's allele keys hold, as in the main pass's spike branch; a record the indel rewrite
        # relocated has its texts in the copy - no table is made of those builds here)
        kept = (_KeptRun(runs[c], A, None, A, run.bam.allele_key, run.bam.barcode_name, lambda n: run.idents) for c in range(B))
        full = decide(kept, P, threshold, copies.addresses() if indel is not None else None,
                      lambda c: copy_allele_key(runs[c], A, run.bam.allele_key), "", shared=True)
        cells = depth or rpb
        if full == NARROW or cells is None:
            return full
        if rpb is not None:
            sels = select_copies_reads(eng, runs, A, lo, rpb["masks"], rpb["n_words"], rpb["copy_stride"], len(rpb["targets"]))
            cell_flag = "--spikeScanRpb" if mnv is None else "--spikeScanMnvRpb"
            axis = [" x %s %g" % (cell_flag, r) for r in rpb["targets"]]
        else:
            sels = select_copies(eng, runs, A, lo, run.idents, part_seeds, depth["fracs"])
            axis, cell_flag = [" x fraction %g" % f for f in depth["fracs"]], "--spikeScanDepth" if mnv is None else "--spikeScanMnvDepth"
        of_cell, n_host = [], full[1]
        for f, what in enumerate(axis):
            if check0 is not None:
                sel, counts, _ = sels.of[f][check0]
                cov1, car1 = copies.check_carriers(check0, sel, counts, cells["want"][f][check0], cells["var"], cells["var_ins"], variants,
                                                   cell_flag, what)
                for s_, (a, b) in enumerate(zip(mnv["set_off"][:-1], mnv["set_off"][1:]) if mnv is not None else ()):
                    mine = (int(cov1[a:b].all(axis=0).sum()), int(car1[a:b].all(axis=0).sum()))
                    if mine != tuple(int(x) for x in mnv["want_joint_cells"][f][check0][s_]):
                        v = variants[run.group[int(a)]]
                        raise RuntimeError("%s: seed %d, the set at %s:%d%s: the AND of the selection's cover and carrier bits holds (N_ALL', "
                                           "V1_ALL') = %r, the counts call says %r" %
                                           (cell_flag, int(part_seeds[check0]), v.chrom, v.pos, what, mine,
                                            tuple(int(x) for x in mnv["want_joint_cells"][f][check0][s_])))
            kept = [_KeptRun(*sels.of[f][c], A, run.bam.allele_key, run.bam.barcode_name, lambda n: run.idents,
                             copy=runs[c] if indel is not None else None, by_read=rpb is not None) for c in range(B)]
            where = None
            if indel is not None:
                # (the records of this cell's selections at the batched stride; n_aln bounds the index an extras entry holds: no
                # build walks more than its kept records, and the largest kept count stays inside every selection's own stretch)
                where = dict(copies.addresses(), aln=sels.bufs[0].data_ptr() + f * B * sels.strides[0],
                             strides=(sels.strides[0],) + tuple(copies.strides[1:]), n_aln=max(k.run.n_aln for k in kept))
            cell = decide(iter(kept), cells["params"][f], cells["thresholds"][f], where, lambda c: kept[c].allele_key, what)
            if cell == NARROW:
                return NARROW
            of_cell.append(cell[0])
            n_host += cell[1]
        return full[0], of_cell, n_host, 1 + len(of_cell)
    finally:
        for b in xbufs + list(fconsts.values()):
            b.free()
        if sels is not None:
            sels.free()
        copies.free()


def spike_scan(path: str, fasta, variants, passes, targets, params, seed: int, n_reps: int, eng, threshold: int, repeats,
               sampler: str = "reference", sampler_seed: int = 0, nthreads: int = 0, max_reads: int = 128_000_000, indel: bool = False,
               depth: dict = None, rpb: dict = None, flt: bool = False, build: str = "whole", mnv: int = 0, mnv_axes: dict = None):
    """The stage of --spikeScan.  variants: the scan's SNV at every scanned locus (tools.spike_scan_lists.scan_variants); passes: [(k,
    the indices of pass k)] (scan_passes).  A pass is the run --spikeAF <targets> --spikeVariants <its list> --spikeReps n_reps --dsSeed
    seed: replicate j has seed (seed + j) mod 2^64, and the draws, the rewrite, NM and the thresholds are that run's.
    The scanned loci are cut into runs as the pre-pass cuts listed variants (AF_RUN_LOCI); every run is decoded and uploaded ONCE and
    kept as an AfRun while its passes are made.  Per pass with a locus in the run: the pre-pass's counters of its variants
    (smc_allele_carriers with counts on the run, and on one copy spiked at threshold 2^32 with the pass's list), one
    smc_spike_rep_counts call for (S, READS, V1) of every variant, replicate and target, then per target as many copies per
    smc_spike_alleles_reps call as _copy_room allows, each built behind the last and the batch called with one plan
    (_scan_call).  The rewrite takes the pass's whole list of the chromosome: a variant is rewritten in whichever run decodes a read
    that spans it.  No batch of rows is downloaded.
    `indel` (--spikeScanIndel: `variants` are the scan's insertion or deletion at every locus, tools.spike_scan_lists.scan_indels): a
    pass is the run --spikeAF <targets> --spikeVariants <its list> --spikeIndelReps n_reps.  The counters are the four of
    _spike_single_counters, the counts come from one smc_spike_indel_counts call, the copies from smc_spike_indels_reps under the same
    room rule, and the verdicts from smc_scan_detect_keys (_scan_call's `indel`).  ValueError before anything is spiked: a run with a
    record at which the rewrite's 16-bit limits could bind (_refuse_indel_limits).
    `depth` (--spikeScanDepth: dict(fracs, params, thresholds: per fraction f the VcParams of its cells - mtDepth max(1,
    py2_round(f x mtDepth)) - and their truncated-PI cut)): a pass is then the run with --spikeDepth <fracs> (--spikeIndelDepth) beside
    it.  One smc_spike_depth_counts (smc_spike_indel_counts) call per pass and run gives the cells' (N', V0', S', READS', V1'); behind
    every full-depth batch ONE select_copies call makes its copies' selections at all fractions, and every fraction's are built and
    called as one batch at the cell's params (_scan_call's `depth`).  The result gets depth_counts: uint32 [V, R, T, F, 5],
    depth_called: bool [V, T, F, R], and the passes' dicts "selects": the select_copies calls.
    `rpb` (--spikeScanRpb: dict(targets, params, thresholds: per reads-per-barcode target r the VcParams of its cells - the scan's with
    rpb = r - and their cut); not with `depth`): a pass is then the run with --spikeRpb <targets> (--spikeIndelRpb) beside it.  Once
    per file philox_read_rules builds the table of read names and gives probKeep and the threshold per r; once per decoded run come
    the read-name identities (pair_idents_or_refuse), the barcodes' first names (run_first_names) and the keep masks of all R seeds x
    Rr targets in ONE buffer - R ReadGroups.masks launches, seed j's masks at j x Rr; per pass and run one spike_rpb_counts call gives
    the cells' (N', V0', S', READS', V1'); behind every full-depth batch ONE select_copies_reads call makes its copies' selections at
    all r, and every r's are built and called as one batch (_scan_call's `rpb`).  The result gets rpb_counts: uint32 [V, R, T, Rr, 5],
    rpb_called: bool [V, T, Rr, R], rpb_rules: per r dict(seed, prob_keep, thr, n_kept, n_names), and the passes' dicts "selects".
    ValueError / BamError naming --spikeScanRpb: what --dsRpbSampler philox refuses.
    `flt` (--spikeScanFilter): the two words of every variant are made once (spike.scan_filter_words: params.hpLen, `fasta`, `repeats`),
    and behind every detect call smc_scan_filter decides the FILTER column per (copy, listed locus) on the same rows (_scan_call's
    `flt`).  The result gets filter: uint32 [V, T, R] - the 14 name bits of abi.SCAN_FILTER_NAMES where `called` -, with an axis
    depth_filter / rpb_filter: uint32 [V, T, F, R], and filter_host: the called records whose FILTER the host decided.
    `build` "listed" (--spikeScanBuild): every batch of copies is one smc_build_listed call over the pass's loci of the run
    (_scan_call's `build`), a batch holds as many copies as their listed slots allow (_copy_room), and the passes' dicts get "listed"
    and "whole" - the builds made either way - and "checks": the replicate-0 rows compared with a whole build's.
    `mnv` L (--spikeScanMnv): `variants` are tools.spike_scan_lists.scan_mnvs' member SNVs with their phase sets of L, `passes` hold
    indices of SETS (mnv_passes); a pass is the run --spikeAF <targets> --spikeVariants <its list of MNV lines> --spikeReps n_reps
    --spikePhase: its SpikeSet is built from the pass's PhasedVariants, so every member is drawn with its leader's position.  The runs
    are cut so that no set is split over two of them (_set_spans, sets_inside).  The result gets joint_counts: uint32 [sets, R, T, 4] =
    (N_ALL, V0_ALL, S_ALL, V1_ALL), joint_called: bool [sets, T, R] and joint_host: the joint verdicts the host decided; base and
    counts are per member, `called` holds the member verdicts only as far as a joint verdict needed them.  ValueError: beside `indel`,
    `depth`, `rpb` or `flt` (not built).
    `mnv_axes` (--spikeScanMnvFilter: dict(flt=True); only with `mnv`): the two words of every member SNV are made once
    (spike.scan_filter_words), and behind every smc_scan_detect_sets call smc_scan_filter_sets decides the joint FILTER word per (copy,
    set) on the same rows (_scan_call's `mnv` with "gate").  The result gets joint_filter: uint32 [sets, T, R] - the OR of the members'
    14 name bits, bit abi.SCAN_FLT_MEMBER_SHIFT + m where member m is not PASS, where joint_called - and joint_filter_host: the called
    sets whose FILTER the host decided.  `mnv_axes["depth"]` (--spikeScanMnvDepth: the dict `depth=` takes): a pass is then the run
    with --spikeDepth <fracs> beside --spikeReps --spikePhase; the stage runs `depth`'s cells with the joint verdicts per cell, the joint
    counts of every (set, replicate, target, fraction) from the ONE smc_spike_phase_counts call per pass and run.  The result gets
    joint_depth_counts: uint32 [sets, R, T, F, 4], joint_depth_called: bool [sets, T, F, R], with flt joint_depth_filter: uint32 [sets,
    T, F, R], and depth's own depth_counts / depth_called per member.  `mnv_axes["reads"]` (--spikeScanMnvRpb: the dict `rpb=` takes;
    not beside "depth" - the grid is not built): a pass is then the run --spikeIndelReps n_reps --spikePhaseRpb <r...> on its MNV lines;
    the stage runs `rpb`'s cells with the joint verdicts per cell - philox_read_rules once per file, _scan_read_masks once per decoded
    run (with the run's barcode-major order on the device), per pass, run and chunk of sets ONE smc_scan_phase_rpb_counts call for the
    joint and the members' counts of every r (_scan_joint_rpb, which also holds the first pass of every run against the host's record
    lists), ONE select_copies_reads call per full-depth batch.  The result gets joint_rpb_counts: uint32 [sets, R, T, Rr, 4],
    joint_rpb_called: bool [sets, T, Rr, R], rpb_rules, and with flt joint_rpb_filter: uint32 [sets, T, Rr, R].  ValueError: without
    `mnv`; any other key ("rpb" among them, as before).
    -> dict(seeds, base: per variant (N, V0), counts: uint32 [V, R, T, 3] = (S, READS, V1), called: bool [V, T, R], passes: per pass
    of `passes` dict(variants, copies, builds, host, seconds), times: dict(stage, runs, decode))."""
    import time
    from . import dsaf
    from .tools import spike_variants as sv
    t_start = time.perf_counter()
    T, R, V = len(targets), int(n_reps), len(variants)
    if T > SPIKE_MAX_TARGETS:
        raise ValueError("--spikeScan: %d targets, at most %d" % (T, SPIKE_MAX_TARGETS))
    if mnv and (indel or depth is not None or rpb is not None or flt):
        raise ValueError("--spikeScanMnv: indel members and the depth, reads-per-barcode and filter axes of an MNV scan are not built")
    mnv_axes = dict(mnv_axes or {})
    if mnv_axes and not mnv:
        raise ValueError("--spikeScanMnvFilter: the axes of an MNV scan need --spikeScanMnv")
    if set(mnv_axes) - {"flt", "depth", "reads"}:
        raise ValueError("--spikeScanMnv: the reads-per-barcode axis of an MNV scan is not built")
    if mnv_axes.get("depth") is not None and mnv_axes.get("reads") is not None:
        raise ValueError("--spikeScanMnvRpb: the grid of barcode fractions x reads-per-barcode targets is not built")
    if mnv_axes.get("depth") is not None:
        depth = mnv_axes["depth"]               # (the cells are --spikeScanDepth's: one select_copies call, a batch per fraction)
    if mnv_axes.get("reads") is not None:
        rpb = mnv_axes["reads"]                 # (the cells are --spikeScanRpb's: one select_copies_reads call, a batch per r)
    rpb_flag = "--spikeScanMnvRpb" if mnv else "--spikeScanRpb"
    seeds = dsaf.rep_seeds(seed, R)
    thr = [sv.threshold(t) for t in targets]
    P = params
    nthreads = nthreads or bamio.host_threads()
    max_depth = eng.L.smc_build_max_depth()
    pass_at = np.full(V, -1, np.int64)          # variant -> its pass's index in `passes`
    local = np.zeros(V, np.int64)               # ... and its place in that pass's list
    if mnv:
        from .tools import spike_scan_lists as lists
        sets = variants.sets
        set_of = np.zeros(V, np.int64)          # member -> its set
        for i, ps in enumerate(sets):
            set_of[list(ps.members)] = i
        for p, (_, members) in enumerate(passes):
            for r, i in enumerate(members):     # (mnv_pass_variants lays a pass's list out set by set)
                pass_at[list(sets[i].members)] = p
                local[list(sets[i].members)] = r * mnv + np.arange(mnv)
        spikes = [SpikeSet(lists.mnv_pass_variants(variants, members)) for _, members in passes]
        mnv = dict(L=int(mnv), set_of=set_of, counts=np.zeros((len(sets), R, T, 4), np.uint32), called=np.zeros((len(sets), T, R), bool), host=0)
        if mnv_axes.get("flt"):
            from . import spike as _spike
            gate, always = _spike.scan_filter_words(variants, params.hpLen, fasta, *repeats)
            mnv["flt"] = dict(gate=gate, always=always, words=np.zeros((len(sets), T, R), np.uint32), host=0)
        if (depth or rpb) is not None:
            Fm = len(depth["fracs"]) if depth is not None else len(rpb["targets"])
            mnv.update(cell_counts=np.zeros((len(sets), R, T, Fm, 4), np.uint32), cell_called=np.zeros((len(sets), T, Fm, R), bool))
            if mnv.get("flt"):
                mnv["flt"]["cell_words"] = np.zeros((len(sets), T, Fm, R), np.uint32)
    else:
        mnv = None
        for p, (_, members) in enumerate(passes):
            pass_at[members] = p
            local[members] = np.arange(len(members))
        spikes = [SpikeSet([variants[i] for i in members], indels=indel) for _, members in passes]
    base, counts, called = [None] * V, np.zeros((V, R, T, 3), np.uint32), np.zeros((V, T, R), bool)
    stats = [dict(variants=0, copies=0, builds=0, host=0, seconds=0.0) for _ in passes]
    if build not in ("whole", "listed"):
        raise ValueError("--spikeScanBuild: whole or listed expected, got %r" % (build,))
    listed_build = build == "listed"
    for st in stats if listed_build else ():
        st.update(listed=0, whole=0, checks=0)
    if depth is not None and rpb is not None:
        raise ValueError("--spikeScanRpb: the grid of barcode fractions x reads-per-barcode targets is not built")
    if depth is not None:
        F = len(depth["fracs"])
        depth = dict(depth, counts=np.zeros((V, R, T, F, 5), np.uint32), called=np.zeros((V, T, F, R), bool))
    read_rules = None
    if rpb is not None:
        F = len(rpb["targets"])
        # (the file-wide table of the UNSPIKED file serves every pass, cell and replicate: spiking changes no name, barcode or record count)
        read_rules = philox_read_rules(path, list(rpb["targets"]), [P] * F, seed, eng, nthreads=nthreads, flag=rpb_flag)
        # (under `mnv` a member's cells have no READS': the four columns of a row of one member)
        rpb = dict(rpb, counts=np.zeros((V, R, T, F, 5 if mnv is None else 4), np.uint32), called=np.zeros((V, T, F, R), bool),
                   read_thr=[r.thr for r in read_rules])
    for st in stats if (depth or rpb) is not None else ():
        st["selects"] = 0
    if flt:
        from . import spike as _spike
        gate, always = _spike.scan_filter_words(variants, P.hpLen, fasta, *repeats)
        flt = dict(gate=gate, always=always, words=np.zeros((V, T, R), np.uint32), host=0,
                   cell_words=np.zeros((V, T, F, R), np.uint32) if (depth or rpb) is not None else np.zeros((V, T, 0, R), np.uint32))
    else:
        flt = None
    times = {"decode": 0.0, "runs": 0}
    if mnv is not None:
        spans = _set_spans(variants, sets, sorted(range(len(sets)), key=lambda i: (sets[i].chrom, variants[sets[i].members[0]].pos)))
    else:
        order = sorted(range(V), key=lambda k: (variants[k].chrom, variants[k].pos))
        spans = _listed_spans(variants, order)
    try:
        for chrom, lo, hi, span in spans:
            t0 = time.perf_counter()
            run = AfRun(chrom, lo, hi, [], 0)
            try:
                nl = run.load(path, fasta, eng, P, max_reads, nthreads, mism=True)
                if nl < 1:
                    raise bamio.BamError("--spikeScan: the run %s:%d-%d could not be decoded" % (chrom, lo + 1, hi))
                if mnv is not None:
                    taken = sets_inside(variants, sets, span, lo, nl)          # (whole sets only; `span` holds sets here)
                    if not taken:
                        raise bamio.BamError("--spikeScanMnv: the run %s:%d-%d came back with %d loci, fewer than the MNV's %d" %
                                             (chrom, lo + 1, hi, nl, mnv["L"]))
                    inside = [k for i in taken for k in sets[i].members]
                else:
                    inside = [k for k in span if variants[k].pos - 1 - lo < nl]
                times["decode"] += time.perf_counter() - t0
                times["runs"] += 1
                in_run = sorted({int(pass_at[k]) for k in inside})
                for p in in_run if indel else ():
                    _refuse_indel_limits(run.A, spikes[p].chrom_variants(chrom, 0.5)[0], "--spikeScanIndel", chrom)
                if rpb is not None:
                    rpb.update(_scan_read_masks(eng, run, read_rules, seeds, rpb_flag, order=mnv is not None))
                    rpb["check_host"] = True    # (--spikeScanMnvRpb: the first pass of the run also counts the existing way)
                for p in in_run:
                    t0 = time.perf_counter()
                    run.group = [k for k in inside if pass_at[k] == p]
                    slots = 0
                    if listed_build and listed_takes(run, len(run.group)):     # (else every batch is whole builds: whole-run slots)
                        slots = listed_layout(run.up.loc_host, [variants[k].pos - 1 - lo for k in run.group], 1)["n_ustart"]
                    room, caps = _copy_room(run, spikes[p].chrom_variants(chrom, 0.5)[0] if indel else None, indel,
                                            len((depth or rpb)["params"]) if (depth or rpb) is not None else 0, rpb is not None, slots)
                    _scan_pass(eng, run, spikes[p], [int(local[k]) for k in run.group], variants, seeds, thr, P, fasta, max_depth, sampler,
                               sampler_seed, threshold, repeats, room, base, counts, called, stats[p], caps, depth, rpb, flt, listed_build,
                               **(dict(mnv=mnv) if mnv is not None else {}))
                    stats[p]["variants"] += len(run.group)
                    stats[p]["seconds"] += time.perf_counter() - t0
            finally:
                if rpb is not None and rpb.get("masks") is not None:
                    rpb.pop("masks").free()
                if rpb is not None and rpb.get("order") is not None:
                    rpb.pop("order").free()
                run.free()
            spans.send(len(inside) if mnv is None else len(taken))
    finally:
        close_rules(read_rules)
    times["stage"] = time.perf_counter() - t_start
    out = dict(seeds=seeds, base=base, counts=counts, called=called, passes=stats, times=times)
    if depth is not None:
        out.update(depth_counts=depth["counts"], depth_called=depth["called"])
    if rpb is not None:
        if mnv is None:
            out.update(rpb_counts=rpb["counts"], rpb_called=rpb["called"])
        out.update(rpb_rules=[dict(seed=r.seed, prob_keep=r.prob_keep, thr=r.thr, n_kept=r.n_kept, n_names=r.n_names) for r in read_rules])
    if mnv is not None:
        out.update(joint_counts=mnv["counts"], joint_called=mnv["called"], joint_host=mnv["host"])
        if mnv.get("flt"):
            out.update(joint_filter=mnv["flt"]["words"], joint_filter_host=mnv["flt"]["host"])
        if depth is not None:
            out.update(joint_depth_counts=mnv["cell_counts"], joint_depth_called=mnv["cell_called"])
            if mnv.get("flt"):
                out["joint_depth_filter"] = mnv["flt"]["cell_words"]
        if rpb is not None:
            out.update(joint_rpb_counts=mnv["cell_counts"], joint_rpb_called=mnv["cell_called"])
            if mnv.get("flt"):
                out["joint_rpb_filter"] = mnv["flt"]["cell_words"]
    if flt is not None:
        out.update(filter=flt["words"], filter_host=flt["host"])
        if (depth or rpb) is not None:
            out["depth_filter" if depth is not None else "rpb_filter"] = flt["cell_words"]
    return out


def _scan_read_masks(eng, run: AfRun, read_rules, seeds, flag: str = "--spikeScanRpb", order: bool = False) -> dict:
    """(--spikeScanRpb) What the passes of one decoded run share on the read axis: the identity of every read-name id (BamError naming
    the flag: an id that stands for two names), whether a name is its barcode's first, and the keep masks of every seed and
    reads-per-barcode target in ONE device buffer - seed j's len(read_rules) masks at j x len(read_rules) x n_words words, the layout
    smc_select_alignments_reads_copies takes for a batch of consecutive seeds; one ReadGroups.masks launch per seed.
    -> dict(p_idents, first, masks, n_words); the caller frees `masks`.  `order` (--spikeScanMnvRpb): the dict also gets "order", the
    run's RunOrder - the run in barcode-major order from A["aln"], p_idents and first, ONE stable argsort, on the device for every
    smc_scan_phase_rpb_counts call over the run; the caller frees it with the masks."""
    from .engine import DevBuf
    groups, Rr = read_rules[0].groups, len(read_rules)
    p_idents = pair_idents_or_refuse(run.bam, run.A, flag, run.chrom, run.lo, run.nl)
    first = run_first_names(eng, groups, p_idents, run.chrom, run.lo, run.nl)
    n = len(p_idents)
    n_words = (n + 31) // 32
    d_id = DevBuf(eng, 8 * max(1, n) + 256).upload(np.ascontiguousarray(p_idents, np.uint64) if n else np.zeros(1, np.uint64))
    buf = DevBuf(eng, 4 * max(1, n_words * Rr * len(seeds)) + 256)
    try:
        for j, s in enumerate(seeds):
            groups.masks(d_id.data_ptr(), n, int(s), [r.thr for r in read_rules], buf.data_ptr() + 4 * n_words * Rr * j)
        st = groups.status()
    except BaseException:
        buf.free()
        raise
    finally:
        d_id.free()
    if st & RG_MISS:
        buf.free()
        raise bamio.BamError("%s: the run %s:%d-%d has a read name the file-wide table does not hold (status %#x)"
                             % (flag, run.chrom, run.lo + 1, run.lo + run.nl, st))
    out = dict(p_idents=p_idents, first=first, masks=buf, n_words=n_words)
    if order:
        try:
            out["order"] = RunOrder(eng, run_barcode_major(run.A, p_idents, first), run.idents)
        except BaseException:
            buf.free()
            raise
    return out


def _scan_joint_rpb(eng, run: AfRun, rpb: dict, var, cov, covers, lead, first, L: int, seeds, thr, joint_counts, variants):
    """(--spikeScanMnvRpb) _scan_pass' cells of the read axis for a pass of MNV sets in one run: per chunk of sets (scan_set_chunks: the
    bit rows stay under SCAN_BITS_BUDGET) smc_spike_read_bits leaves the members' bytes in HBM and ONE smc_scan_phase_rpb_counts call
    over the run's barcode-major order (rpb["order"]) counts every r - the chunk's sets as rows, then every member as a row of one.
    var, cov, covers, lead: the pass's members in the run, their records, cover rows, covering identities and draw positions; first:
    where each set begins in them -> (uint32 [sets, R, T, Rr, 4] joint, uint32 [members, R, T, Rr, 4] per member).
    Where the cells' limit leaves room the threshold 2^32 rides along as one more r, and its joint words must be `joint_counts`, the
    full-depth numbers of smc_spike_phase_counts.  rpb["check_host"] (the first pass of a decoded run; taken out here): the joint words
    are also made the existing way - the bytes downloaded, spike_rpb_records, spike_joint_records, smc_spike_phase_rpb_counts - and a
    word that differs ends the run."""
    from .tools import spike_variants as sv
    A, up, lo, chrom, n_ids = run.A, run.up, run.lo, run.chrom, len(run.idents)
    order, rthr = rpb["order"], list(rpb["read_thr"])
    Rr, n_sets = len(rthr), len(first)
    ride = len(thr) * (Rr + 1) <= SCAN_RPB_MAX_CELLS              # (full depth as one more read threshold)
    call_thr = rthr + ([1 << 32] if ride else [])
    joint = np.zeros((n_sets, len(seeds), len(thr), len(call_thr), 4), np.uint32)
    cells = np.zeros((len(var), len(seeds), len(thr), len(call_thr), 4), np.uint32)
    cover = np.asarray(cov)[:, :n_ids] != 0
    for a, b in scan_set_chunks(n_sets, L, up.n_aln):
        rows_v = list(range(first[a], first[b - 1] + L))        # the chunk's members: bit row k of the chunk is member rows_v[k]
        d_bits = spike_read_bits_dev(eng, up, A, lo, var[rows_v])
        try:
            rows = [list(range((s_ - a) * L, (s_ - a + 1) * L)) for s_ in range(a, b)] + [[k] for k in range(len(rows_v))]
            gids = [np.flatnonzero(cover[first[s_]:first[s_] + L].all(axis=0)).astype(np.uint32) for s_ in range(a, b)] + \
                   [np.flatnonzero(cover[g]).astype(np.uint32) for g in rows_v]
            pos = [lead[first[s_]] for s_ in range(a, b)] + [lead[g] for g in rows_v]
            got = scan_phase_rpb_counts(eng, order, d_bits, len(rows_v), rows, gids, pos, seeds, thr, call_thr)
            if rpb.pop("check_host", False):
                bits = d_bits.download(np.uint8, len(rows_v) * up.n_aln).reshape(len(rows_v), up.n_aln)
                records = [spike_rpb_records(A, bits[k], np.flatnonzero(cover[g]), rpb["p_idents"], rpb["first"]) for k, g in enumerate(rows_v)]
                sets = [sv.PhaseSet("", chrom, tuple(r)) for r in rows[:b - a]]
                theirs = spike_phase_rpb_counts(eng, pos[:b - a], [L] * (b - a), spike_joint_records(sets, [covers[g] for g in rows_v], records),
                                                seeds, thr, call_thr)
                if not np.array_equal(theirs, got[:b - a]):
                    s_ = a + int(np.argwhere(theirs != got[:b - a])[0][0])
                    v = variants[run.group[first[s_]]]
                    raise RuntimeError("--spikeScanMnvRpb: the set at %s:%d: smc_scan_phase_rpb_counts and smc_spike_phase_rpb_counts on the "
                                       "host's records disagree: %r against %r" % (v.chrom, v.pos, got[s_ - a].tolist(), theirs[s_ - a].tolist()))
        finally:
            d_bits.free()
        joint[a:b] = got[:b - a]
        cells[rows_v] = got[b - a:]
    if ride and not np.array_equal(joint[:, :, :, Rr], joint_counts):
        s_ = int(np.argwhere(joint[:, :, :, Rr] != joint_counts)[0][0])
        v = variants[run.group[first[s_]]]
        raise RuntimeError("--spikeScanMnvRpb: the set at %s:%d: at the read threshold 2^32 smc_scan_phase_rpb_counts gives %r, "
                           "smc_spike_phase_counts %r" % (v.chrom, v.pos, joint[s_, :, :, Rr].tolist(), np.asarray(joint_counts)[s_].tolist()))
    return joint[:, :, :, :Rr], cells[:, :, :, :Rr]


def _scan_pass(eng, run: AfRun, spikes: SpikeSet, members, variants, seeds, thr, P, fasta, max_depth, sampler, sampler_seed, threshold,
               repeats, room, base, counts, called, stat, caps=None, depth: dict = None, rpb: dict = None, flt: dict = None, listed_build: bool = False,
               mnv: dict = None):
    """spike_scan's work for one pass in one run: run.group are the pass's variants there (indices into `variants`), members[g] the
    place of run.group[g] in the pass's list (`spikes`).  base, counts, called and stat are filled.  `caps` (--spikeScanIndel:
    spike_indel_caps of the pass's list on the run): the indel branch.  `depth` (--spikeScanDepth: spike_scan's dict with "counts" and
    "called"): the cells' counters of the pass from ONE smc_spike_depth_counts (indel: smc_spike_indel_counts) call, and per batch of
    copies the cells' verdicts (_scan_call's `depth`); both are filled.  `rpb` (--spikeScanRpb: spike_scan's dict with "counts",
    "called" and the run's "p_idents", "first", "masks", "n_words"): the same on the read axis - smc_spike_read_bits
    (smc_spike_indel_read_bits) on the pass's variants, spike_rpb_records per variant and ONE spike_rpb_counts call for the cells'
    counters; a batch's mask base is that of its first seed.  `flt` (--spikeScanFilter: spike_scan's dict with "gate", "always",
    "words", "cell_words" and "host"): per batch the FILTER words of the copies (_scan_call's `flt`); the last three are filled.
    `listed_build` (--spikeScanBuild listed): _scan_call's `build` is `stat`, whose "listed", "whole" and "checks" count up.
    `mnv` (--spikeScanMnv: spike_scan's dict with "L", "set_of", "counts", "called" and "host"): run.group holds the members of whole
    phase sets of L, set by set; the joint barcodes of every set come from spike_joint and (N_ALL, V0_ALL, S_ALL, V1_ALL) of every set,
    replicate and target from ONE smc_spike_phase_counts call; per batch the joint verdicts (_scan_call's `mnv`).  `called` holds the
    member verdicts as far as a joint verdict needed them.  With mnv["flt"] (--spikeScanMnvFilter: dict(gate, always, words, host)) per
    batch the joint FILTER words of the copies (_scan_call's `mnv` with "gate"); "words", "cell_words" and "host" are filled.  With
    `depth` beside it (--spikeScanMnvDepth) the ONE smc_spike_phase_counts call also takes the fractions' thresholds and gives (N_ALL',
    V0_ALL', S_ALL', V1_ALL') of every cell: mnv["cell_counts"] and mnv["cell_called"] are filled."""
    A, up, lo, chrom = run.A, run.up, run.lo, run.chrom
    idents, (nm, n_indel) = run.idents, run.mism
    group = run.group
    var, ins = af_run_variants([variants[k] for k in group], chrom, lo, fasta)
    cov, car, cnt0 = allele_carriers_run(eng, up, A, lo, var, ins, counts=True)
    svar, sorder, covers, counters = _spike_single_counters(eng, up, A, lo, spikes, chrom, members, var, ins, idents, seeds[0], P, nm, n_indel,
                                                            cov, cnt0, caps is not None)
    for g, k in enumerate(group):
        base[k] = (int(cov[g].sum()), int(car[g].sum()))
    lead = [spikes.lead_pos[m] for m in members]
    mine = (spike_rep_counts if caps is None else spike_indel_counts)(eng, lead, covers, counters, seeds, thr)       # [G, R, T, 3]
    cells = None
    if depth is not None:
        cells = (spike_depth_counts if caps is None else spike_indel_counts)(eng, lead, covers, counters, seeds, thr,
                                                                             [frac_threshold(f) for f in depth["fracs"]])   # [G, R, T, F, 5]
    at_of = {m: n for n, m in enumerate(sorder)}
    var_at = [at_of[m] for m in members]
    axis = depth or rpb                         # (the cells' dict: one axis at most)
    if rpb is not None and mnv is None:
        read_bits = spike_read_bits(eng, up, A, lo, var) if caps is None else \
            spike_indel_read_bits(eng, up, A, lo, svar[var_at], spikes.ins[chrom])
        records = [spike_rpb_records(A, read_bits[g], np.flatnonzero(cov[g][:len(idents)]), rpb["p_idents"], rpb["first"])
                   for g in range(len(group))]
        cells = spike_rpb_counts(eng, lead, covers, records, seeds, thr, rpb["read_thr"], four=caps is not None)   # [G, R, T, Rr, 5]
    listed = np.zeros(len(group), abi.SCAN_LOCUS_DTYPE)
    for g, k in enumerate(group):
        counts[k] = mine[g]
        if cells is not None:
            axis["counts"][k] = cells[g]
        # (--spikeScanIndel: a key has no fixed id - smc_scan_detect_keys takes `var`, and of `listed` only the offsets are read)
        listed[g] = (variants[k].pos - 1 - lo, SCAN_ALT_ID[variants[k].alt] if caps is None else 0)
    R, F = len(seeds), len(depth["fracs"]) if depth is not None else len(rpb["targets"]) if rpb is not None else 0
    if mnv is not None:
        from .tools import spike_variants as sv
        set_off = np.arange(0, len(group) + 1, mnv["L"], dtype=np.uint32)
        first = [int(a) for a in set_off[:-1]]
        joint = spike_joint([sv.PhaseSet("", chrom, tuple(range(a, a + mnv["L"]))) for a in first], covers, counters)
        # (ONE call: full depth - the threshold 2^32 keeps every barcode - and behind it the cells of --spikeScanMnvDepth)
        joint_all = spike_phase_counts(eng, [lead[a] for a in first], joint, seeds, thr,
                                       [1 << 32] + ([frac_threshold(f) for f in depth["fracs"]] if depth is not None else []))
        joint_counts, joint_cells = joint_all[:, :, :, 0], joint_all[:, :, :, 1:]      # [sets, R, T, 4], [sets, R, T, F, 4]
        if rpb is not None:
            # (--spikeScanMnvRpb: the cells of the read axis, the sets' joint numbers and the members' own, counted per record on the device)
            joint_cells, cells = _scan_joint_rpb(eng, run, rpb, var, cov, covers, lead, first, mnv["L"], seeds, thr, joint_counts, variants)
            for g, k in enumerate(group):
                rpb["counts"][k] = cells[g]
        set_ids = [int(mnv["set_of"][group[a]]) for a in first]
        for s_, i in enumerate(set_ids):
            mnv["counts"][i] = joint_counts[s_]
            if axis is not None:
                mnv["cell_counts"][i] = joint_cells[s_]
    for t in range(len(thr)):
        for b in range(0, R, room):
            js = list(range(b, min(R, b + room)))
            want = [[int(mine[g, j, t, 1]) for g in range(len(group))] for j in js]
            args = (eng, run, svar, var_at, listed, [seeds[j] for j in js], thr[t], want, P, fasta, variants, max_depth, sampler, sampler_seed)
            tail = (threshold, repeats, js.index(0) if 0 in js else None)
            tail += (dict(ins=spikes.ins[chrom], caps=caps, var=var, var_ins=ins,
                          want=[[(len(covers[g]), int(mine[g, j, t, 2])) for g in range(len(group))] for j in js]) if caps is not None else None,)
            if axis is not None:
                # (N' and V1': the first and the last column, of the five of a listed variant or the four of a member under --spikeScanMnvRpb)
                want = [[[(int(cells[g, j, t, f, 0]), int(cells[g, j, t, f, -1])) for g in range(len(group))] for j in js] for f in range(F)]
                if depth is not None:
                    tail += (dict(fracs=depth["fracs"], params=depth["params"], thresholds=depth["thresholds"], var=var, var_ins=ins, want=want),)
                else:
                    # (the masks of seed j stand at j x Rr masks: the batch's seeds are consecutive)
                    tail += (None, dict(targets=rpb["targets"], params=rpb["params"], thresholds=rpb["thresholds"], var=var, var_ins=ins,
                                        want=want, masks=rpb["masks"].data_ptr() + 4 * rpb["n_words"] * F * js[0], n_words=rpb["n_words"],
                                        copy_stride=rpb["n_words"] * F),)
            fl = dict(gate=flt["gate"][group], always=flt["always"][group]) if flt is not None else None
            more = {}
            if mnv is not None:
                more["mnv"] = dict(**(dict(gate=mnv["flt"]["gate"][group], always=mnv["flt"]["always"][group]) if mnv.get("flt") else {}),
                                   set_off=set_off, var=var, var_ins=ins,
                                   want=[[(len(covers[g]), int(mine[g, j, t, 2])) for g in range(len(group))] for j in js],
                                   want_joint=[[(int(joint_counts[s_, j, t, 0]), int(joint_counts[s_, j, t, 3])) for s_ in range(len(first))]
                                               for j in js],
                                   want_joint_cells=[[[(int(joint_cells[s_, j, t, f, 0]), int(joint_cells[s_, j, t, f, 3]))
                                                       for s_ in range(len(first))] for j in js] for f in range(F)])
            if listed_build:
                before = {k: stat[k] for k in ("listed", "whole", "checks")}

                def call(bits):
                    stat.update(before)         # (a narrower retry starts over)
                    return _scan_call(*args, bits, *tail, flt=fl, build=stat, **more)
            else:
                call = lambda bits: _scan_call(*args, bits, *tail, flt=fl, **more)
            got = _narrow_retry(eng, P, call)
            if mnv is not None:
                outs, fouts = more["mnv"]["out"], more["mnv"]["flt_out"]
                for c, j in enumerate(js):
                    for s_, i in enumerate(set_ids):
                        mnv["called"][i, t, j] = outs[0][0][c, s_]
                        for f in range(F):
                            mnv["cell_called"][i, t, f, j] = outs[1 + f][0][c, s_]
                        if mnv.get("flt"):
                            mnv["flt"]["words"][i, t, j] = fouts[0][0][c, s_]
                            for f in range(F):
                                mnv["flt"]["cell_words"][i, t, f, j] = fouts[1 + f][0][c, s_]
                mnv["host"] += sum(n for _, n in outs)
                if mnv.get("flt"):
                    mnv["flt"]["host"] += sum(n for _, n in fouts)
            yes, n_host, builds = (got[0], got[2], got[3]) if axis is not None else (got[0], got[1], 1)
            for c, j in enumerate(js):
                for g, k in enumerate(group):
                    called[k, t, j] = yes[c, g]
                    for f in range(F):
                        axis["called"][k, t, f, j] = got[1][f][c, g]
                    if flt is not None:
                        flt["words"][k, t, j] = fl["out"][0][0][c, g]
                        for f in range(F):
                            flt["cell_words"][k, t, f, j] = fl["out"][1 + f][0][c, g]
            if flt is not None:
                flt["host"] += sum(n for _, n in fl["out"])
            stat["copies"] += len(js)
            stat["builds"] += len(js) * builds
            stat["host"] += n_host
            if axis is not None:
                stat["selects"] = stat.get("selects", 0) + 1


def _fnv64(text: str) -> int:
    """FNV-1a, 64 bits, of a barcode's text (as smc_bam_barcode_idents computes it natively)."""
    x = 1469598103934665603
    for c in text.encode():
        x = ((x ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return x


def synth_allele_key(A):
    """`allele_key` for a run of synth.generate_alignments (what smc_bam_allele_key answers for a decoded run)."""
    def key(ai, qpos, indel):
        a = A["aln"][int(ai)]
        so, ls = int(a["seq_off"]), int(a["l_seq"])
        site = chr(A["seq"][so + int(qpos)])
        indel = int(indel)
        if indel > 0:
            return "INS|%s|%s%s" % (site, site, A["seq"][so + int(qpos) + 1:so + min(ls, int(qpos) + 1 + indel)].tobytes().decode())
        if indel < 0:
            return "D%d|%s" % (-indel, site)
        return site
    return key


def resident_from_alignments(A, eng, params, all_planes: bool = True, chrom: str = None, sampler: str = "reference",
                             sampler_seed: int = 0) -> ResidentBatch:
    """One run of synthetic alignments (synth.generate_alignments) -> a ResidentBatch built by smc_build_planes; raises when
    the device path does not take the run."""
    from . import synth
    from .engine import DevBuf
    L = eng.L
    chrom = chrom or synth.ALN_CHROM
    nl, ns, lo = A["nl"], A["n_slots"], int(A["start0"])
    cap = ns + 64
    planes = [DevBuf(eng, 4 * cap) if all_planes else None for k in range(4)]
    uaux = [DevBuf(eng, 4 * (cap + nl + 8192)) for _ in range(3)]
    run_ref = synth.aln_ref_fetch(lo, lo + nl)
    ref = synth.CyclicRef()
    for bits in ((16, 32) if (not all_planes and eng.word_bits == 16 and 0 <= params.minBQ <= 63) else (32,)):
        words = DevBuf(eng, (bits // 8) * cap, walk_output=True)
        words.word_bits = bits
        done = build_run(A, L, eng, abi.c_params(params), params, chrom, lo, ref, run_ref, [words] + planes, uaux, 0, 0, cap + nl,
                         L.smc_build_max_depth(), synth_allele_key(A), lambda gid: "B%d" % gid, sampler=sampler, sampler_seed=sampler_seed)
        if done != NARROW:
            break
        words.free()
    if done is None:
        raise RuntimeError("smc_build_planes did not take the run (status / size)")
    nl, ns, lc, tb = done
    uaux[1].free(); uaux[2].free()
    return ResidentBatch(planes=planes + [uaux[0]], words=words, n_slots=ns, n_ustart=ns + nl + 1, loci=lc, chrom=[chrom] * nl,
                         pos=np.arange(lo + 1, lo + 1 + nl, dtype=np.int64), ref=list(run_ref), alleles=tb, n_device_runs=1)


def DevLoci(eng, loci: np.ndarray):
    """The descriptors of a batch uploaded as a device array (for engine.make_plan_dev)."""
    from .engine import DevBuf
    loci = np.ascontiguousarray(loci)
    return DevBuf(eng, max(32, loci.nbytes)).upload(loci.view(np.uint8).reshape(-1))
