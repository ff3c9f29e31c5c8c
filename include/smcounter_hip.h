/*
 * smcounter_hip.h - C ABI of the MI355X (gfx950) implementation of smCounter's per-locus
 * variant-calling hot path.
 *
 * What this replaces in the reference (/root/reference/smCounter.py):
 *   - vc()            smCounter.py:274-600   one call per locus inside a multiprocessing worker
 *   - calProb()       smCounter.py:26-98     per-barcode posterior
 *   - filterVariants  smCounter.py:182-269   FILTER flags (all but the two that read the FASTA)
 *   - the Pool dispatch of main()  smCounter.py:683-685  (one apply_async per locus) becomes one
 *     smc_plan_run() over a structure-of-arrays batch of loci.
 * The reference has no FFI of its own (it is pure Python); the binding a maintainer would add is
 * the ctypes stub shown in INTEGRATION.md.
 *
 * Conventions: plain C, caller owns every buffer, no exceptions cross the boundary; every entry
 * point returns 0 on success or a negative SMC_E_* code, and smc_last_error() returns the
 * message of the last failure on the calling thread.  One host thread per GPU.
 */
#ifndef SMCOUNTER_HIP_H
#define SMCOUNTER_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMC_ABI_VERSION 11
#define SMC_MAX_ALLELES 64 /* allele ids per locus; ids 0-5 are A,T,G,C,N,'DEL' */

/* error codes */
#define SMC_OK 0
#define SMC_E_ARG (-1)     /* bad argument */
#define SMC_E_HIP (-2)     /* HIP runtime failure (message has the hipError string) */
#define SMC_E_NOGPU (-3)   /* no usable gfx950 device */
#define SMC_E_INPUT (-4)   /* batch violates the layout contract */

/* row.status */
#define SMC_ST_OK 0
#define SMC_ST_ZERO_COVERAGE 1      /* usedMT == 0: the 45-field Zero_Coverage row, smCounter.py:492-494 */
#define SMC_ST_DOWNSAMPLED 0x100    /* more barcodes than ds: reference would random.sample (:496-498) */
#define SMC_ST_BAD_INPUT 0x200      /* an id in the batch was out of the range its descriptor declares */
#define SMC_ST_UNDERFLOW 0x400      /* a barcode of the locus has so many fragments that calProb's products (smCounter.py:62-77:
                                     * 0.9^n for unpaired fragments) left the normal double range (n > ~ 6,700): the reference's own
                                     * posterior there is made of denormal rounding and depends on the order it multiplies in (py2
                                     * dict order of read ids).  The row is computed; its PI / UMT columns are not pinned. */

/* FILTER bits in smc_cand.flt, in the order filterVariants appends them (smCounter.py:187-266) */
#define SMC_F_LM 0x001
#define SMC_F_LSM 0x002
#define SMC_F_HP 0x004   /* set by the host: needs the reference sequence (smCounter.py:195-199) */
#define SMC_F_LOWC 0x008 /* set by the host (smCounter.py:202-203) */
#define SMC_F_DP 0x010
#define SMC_F_SB 0x020
#define SMC_F_LOWQ 0x040
#define SMC_F_R1CP 0x080
#define SMC_F_R2CP 0x100
#define SMC_F_PRIMERCP 0x200

/* per-read flag bits inside meta (bits 16-23); see smcounter_amd/features.py */
#define SMC_FL_R2 1
#define SMC_FL_REV 2
#define SMC_FL_MMOK 4
#define SMC_KIND_SHIFT 3
#define SMC_KIND_BASE 0
#define SMC_KIND_GAP 1      /* 'DEL': inside a deletion, quality forced to minBQ (smCounter.py:416-418) */
#define SMC_KIND_INS 2
#define SMC_KIND_DELSTART 3

/* Read class: bits 27-31 of every `frag` plane word (bits 0-26 hold the fragment slot). What a read adds to its
 * allele's tallies and whether it enters bcDict depends only on a handful of predicates that the feature extraction
 * knows (it has the run's parameters): the class names the combination, the default kernel looks the tally
 * increments up by class and never touches base quality / MAPQ / distance arithmetic for the tallies, nor the
 * `dist` plane at all. incCond = (bq >= minBQ or in-deletion) and mapq >= minMQ and mismatch-ok (smCounter.py:378).
 *   in-deletion ('DEL', kind 1):                  0 + incCond
 *   insertion / deletion start (kind 2, 3):       2 + 2 * reverse + incCond
 *   regular base (kind 0):                        6 + 8 * reverse + sub, with sub =
 *       0 not included, bq >= minBQ   1 not included, bq < minBQ (lowQReads, :428)
 *       2 included read 1, distToBcEnd > 20   3 included read 1, distToBcEnd <= 20            (:432-440)
 *       4 + (distToBcEnd <= 20) + 2 * (distToPrimerEnd <= primerDist)   included read 2       (:441-452)
 * The raw fields stay in the planes (the CPU restatement under oracle/ computes everything from them, so the parity
 * tests check the classes too).  The class bakes in minBQ / minMQ / mismatchThr / primerDist: planes are only valid for the
 * parameter set they were built with, which is why every locus descriptor carries smc_param_fingerprint() of it and
 * smc_plan_run refuses any other (SMC_E_INPUT). */
#define SMC_FRAG_SLOT_MASK 0x07FFFFFFu
#define SMC_FRAG_CLASS_SHIFT 27
#define SMC_N_READ_CLASS 22
/* The read word: what the locus kernels read, ONE uint32 per read (4 of the raw-field planes' 16 bytes cross HBM).
 *   bits 0-7 allele id, 8-15 base quality (<= 126; minBQ for a read inside a deletion) - the low half of the meta word;
 *   bit 16 the read is the first of its fragment at this locus (the fragment slots are dense and ascending, so the slot
 *          number itself carries nothing else); bit 17 the read is included (incCond, smCounter.py:378) and bit 18 its class is
 *          one of the SMC_N_READ_CLASS known ones - both functions of the class (smc_class_bits below), spelled out so that the
 *          scan takes them with the fragment bit in one byte instead of looking the class up; bits 19-26 zero; bits 27-31 the
 *          read class (as in the frag word).
 * smc_build_planes writes it directly; smc_pack_words folds a batch's meta and frag planes into it (and checks the slot
 * contract, which the words can no longer break); smc_plan_run_words runs on it. */
#define SMC_RW_NF 0x00010000u
#define SMC_RW_INC 0x00020000u
#define SMC_RW_OK 0x00040000u
#define SMC_RW_CLASS_SHIFT 27
#if defined(__HIPCC__)
#define SMC_HOST_DEVICE __host__ __device__   /* (the device plane builder evaluates it too) */
#else
#define SMC_HOST_DEVICE
#endif
SMC_HOST_DEVICE static inline uint32_t smc_read_class(int kind, int rev, int r2, int inc, int bq_ok, int le20, int prle) {
    if (kind == 1) return (uint32_t)(0 + (inc ? 1 : 0));
    if (kind != 0) return (uint32_t)(2 + (rev ? 2 : 0) + (inc ? 1 : 0));
    uint32_t sub;
    if (!inc) sub = bq_ok ? 0u : 1u;
    else if (!r2) sub = 2u + (le20 ? 1u : 0u);
    else sub = 4u + (le20 ? 1u : 0u) + (prle ? 2u : 0u);
    return 6u + (rev ? 8u : 0u) + sub;
}

/* bits 17-18 of the read word for a class: included = the incCond half of smc_read_class's encoding, known = class < 22 */
SMC_HOST_DEVICE static inline uint32_t smc_class_bits(uint32_t cls) {
    if (cls >= SMC_N_READ_CLASS) return 0u;
    const int inc = cls < 6u ? (int)(cls & 1u) : (((cls - 6u) & 7u) >= 2u);
    return SMC_RW_OK | (inc ? SMC_RW_INC : 0u);
}

/* The read word in 16 bits (ABI 7): what smc_build_planes_w16 writes and smc_plan_run_words16 reads - the intermediate between the
 * walk over the alignments and the locus kernels at half the bytes (the walk is bound by what it writes).  The same
 * information as the 32-bit word, for runs whose allele ids stay below 16 and whose base qualities below 64 (a run that
 * breaks either is reported - status bit 32 of smc_build_planes_w16 - and built with 32-bit words instead):
 *   bits 0-3 allele id; bit 4 first read of its fragment at this locus; bit 5 included (incCond); bits 6-7 and 14-15 the low and
 *   the high half of a 4-bit class index; bits 8-13 base quality.
 * (included << 4 | class index) is the read class renumbered so that inclusion is a bit of its own (smc_class16 below:
 *   not included: 0 inside a deletion, 1 + reverse at an insertion / deletion start, 3 + 2 * reverse + (bq < minBQ) on a base;
 *   included:     0, 1 + reverse as above, 3 + 6 * reverse + (smc_read_class's sub - 2) on a base);
 * "the class is a known one" (bit 18 of the 32-bit word) has no bit: the builder writes no other. */
SMC_HOST_DEVICE static inline uint32_t smc_class16(uint32_t cls) {          /* smc_read_class's number -> included << 4 | index; 31: no class */
    if (cls < 2u) return (cls & 1u) << 4;
    if (cls < 6u) return ((cls & 1u) << 4) | (1u + ((cls - 2u) >> 1));
    if (cls >= SMC_N_READ_CLASS) return 31u;
    { const uint32_t rev = (cls - 6u) >> 3, sub = (cls - 6u) & 7u;
      return sub < 2u ? 3u + 2u * rev + sub : 16u | (3u + 6u * rev + (sub - 2u)); }
}
SMC_HOST_DEVICE static inline uint32_t smc_class16_inv(uint32_t c16) {      /* and back; 31 for a code smc_class16 never returns */
    const uint32_t inc = (c16 >> 4) & 1u, idx = c16 & 15u;
    if (idx == 0u) return inc;
    if (idx < 3u) return 2u + 2u * (idx - 1u) + inc;
    if (!inc) return idx < 7u ? 6u + 8u * ((idx - 3u) >> 1) + ((idx - 3u) & 1u) : 31u;
    return idx < 15u ? 6u + 8u * ((idx - 3u) / 6u) + 2u + (idx - 3u) % 6u : 31u;
}
/* a 32-bit read word (allele < 16, quality < 64, a known class) as a 16-bit one, and back */
SMC_HOST_DEVICE static inline uint32_t smc_read_word16(uint32_t w) {
    const uint32_t c = smc_class16(w >> SMC_RW_CLASS_SHIFT);
    return (w & 15u) | ((w & SMC_RW_NF) ? 16u : 0u) | ((c >> 4) & 1u) << 5 | (c & 3u) << 6 | ((w >> 8) & 63u) << 8 | ((c >> 2) & 3u) << 14;
}
SMC_HOST_DEVICE static inline uint32_t smc_read_word32(uint32_t h) {
    const uint32_t c16 = ((h >> 5) & 1u) << 4 | ((h >> 6) & 3u) | ((h >> 14) & 3u) << 2, cls = smc_class16_inv(c16);
    return (h & 15u) | ((h >> 8) & 63u) << 8 | ((h & 16u) ? SMC_RW_NF : 0u) | smc_class_bits(cls) | cls << SMC_RW_CLASS_SHIFT;
}

/* The numeric arguments vc() receives (smCounter.py:274) that the device path needs, plus the two
 * values vc() derives before the pileup loop. mismatchThr and hpLen are consumed on the host
 * (feature extraction / reference-sequence test). */
typedef struct smc_params {
    int32_t min_bq;      /* minBQ */
    int32_t min_mq;      /* minMQ */
    int32_t mt_drop;     /* mtDrop */
    int32_t primer_dist; /* primerDist */
    int32_t ds;          /* maxMT if > 0 else int(round(2.0 * mtDepth))   smCounter.py:486 */
    int32_t reserved;
    double smt;          /* strong-MT threshold 2.0 / 3.0 / 4.0 by rpb    smCounter.py:302-308 */
    double mismatch_thr; /* mismatchThr: consumed by the feature extraction (flag bit / read class); here so that a run can
                          * be checked against the parameters its planes were built with */
} smc_params;

/* 15-bit fingerprint (never 0) of the four parameters the feature extraction folds into the planes (read class, the
 * mismatch-ok flag, the in-deletion quality).  Stored in smc_locus.flags bits 1-15 by whoever builds a batch; smc_plan_create
 * requires one common non-zero value over the batch, smc_plan_run compares it with the fingerprint of the run's smc_params
 * and returns SMC_E_INPUT when they differ (planes built for one parameter set give silently wrong rows under another). */
static inline uint16_t smc_param_fingerprint(int32_t min_bq, int32_t min_mq, double mismatch_thr, int32_t primer_dist) {
    union { double d; uint64_t u; } cv;
    cv.d = mismatch_thr;
    uint64_t h = 0x9E3779B97F4A7C15ull;
    const uint64_t w[4] = {(uint64_t)(uint32_t)min_bq, (uint64_t)(uint32_t)min_mq, cv.u, (uint64_t)(uint32_t)primer_dist};
    for (int i = 0; i < 4; ++i) {
        h ^= w[i];
        h *= 0xBF58476D1CE4E5B9ull;
        h ^= h >> 29;
    }
    const uint16_t fp = (uint16_t)((h >> 17) & 0x7FFFu);
    return fp ? fp : (uint16_t)1;
}
#define SMC_LF_FP_SHIFT 1 /* smc_locus.flags bits 1-15: smc_param_fingerprint of the parameters the planes were built with */

/* One per locus, 32 bytes. Reads of locus l occupy plane slots [4*read_off4, 4*read_off4 + n_reads)
 * (every locus starts on a 4-read boundary). Within the locus the reads are SORTED barcode-major:
 * by barcode id, then by fragment slot, then by pileup order (stable), so a barcode's reads are one
 * contiguous run, a fragment's reads are adjacent, and the first-seen mate still comes first
 * (smCounter.py:468-479 depends on that order only within a fragment).
 * umi ids are < n_umi (dense, order of first appearance in the pileup). frag ids are locus-level
 * fragment slots < n_frag, grouped by barcode: the fragments of barcode u occupy one contiguous slot
 * range, ranges ordered by u, each fragment's slot fixed by its first appearance within the barcode;
 * n_frag = number of distinct fragments (= allFrag, smCounter.py:483).
 * umi_start[umi_off + u], u = 0..n_umi, is the index (relative to the locus) of barcode u's first read;
 * the last entry equals n_reads. Every barcode has at least one read. Given barcode-major reads, umi_start
 * determines the umi plane; the kernels use umi_start and the fragment-start bit of the read words and load neither the umi
 * plane nor - with the read class (smc_read_class above) - the dist plane: `umi` and `dist` may be NULL in smc_plan_run /
 * smc_call_batch_host (they are the raw fields the CPU restatement checks the classes and the order against). Checked per
 * locus, violations flag the row SMC_ST_BAD_INPUT: fragment slots dense and ascending, 0 .. n_frag - 1 (smc_pack_words),
 * allele < n_alleles, a known read class, umi_start ascending and covering [0, n_reads), every barcode starting a fragment.
 * Base qualities are Phred values <= 126 (BAM holds 0..93); larger bytes are clamped to 126. */
/* smc_locus.flags */
#define SMC_LF_SAMPLED 1u /* the host has applied the reference's down-sampling (smCounter.py:496-498): barcodes whose
                           * umi_start entry has bit 31 set are keys of bcDict the sample dropped; the number kept must be
                           * min(#keys, ds), else the row is SMC_ST_BAD_INPUT. Without this flag a locus over the cap gets
                           * the non-parity stand-in (ds lowest barcode ids). */
#define SMC_USTART_DROPPED 0x80000000u
typedef struct smc_locus {
    uint32_t read_off4; /* first plane slot / 4 */
    uint32_t umi_off;   /* first entry of this locus in the umi_start array */
    int32_t n_reads;
    int32_t n_umi;
    int32_t n_frag;
    uint8_t ref_allele; /* allele id of the reference base, 255 if it is not a key */
    uint8_t n_alleles;  /* size of the locus's allele table, <= SMC_MAX_ALLELES */
    uint16_t flags;
    uint64_t snp_mask;  /* bit a set: allele a is a single letter (TYPE 'SNP', smCounter.py:107) */
} smc_locus;

/* per-allele tallies of the pileup scan; index names follow the reference's dicts */
enum {
    SMC_T_CNT = 0,   /* alleleCnt        smCounter.py:379,401,459 */
    SMC_T_FWD,       /* forwardCnt       :389,411,457 */
    SMC_T_REV,       /* reverseCnt       :387,409,455 */
    SMC_T_LOWQ,      /* lowQReads        :428-429 */
    SMC_T_R1N,       /* len(r1BcEndPos)  :438-439 */
    SMC_T_R1LE,      /* #r1BcEndPos <= 20          :234 */
    SMC_T_R2N,       /* len(r2BcEndPos)  :449-451 */
    SMC_T_R2BCLE,    /* #r2BcEndPos <= 20          :244 */
    SMC_T_R2PRLE,    /* #r2PrimerEndPos <= primerDist  :256 */
    SMC_T_CONCORD,   /* concordPairCnt   :475-476 */
    SMC_T_DISCORD,   /* discordPairCnt   :479 */
    SMC_T_PAD,
    SMC_NT = 12
};

typedef struct smc_cand {
    int32_t allele;      /* allele id, -1 when the candidate does not exist */
    int32_t flt_applied; /* 1 if filterVariants ran (PI >= 5 and TYPE in SNP/INDEL, :549/:563) */
    uint32_t flt;        /* SMC_F_* bits decided on the device */
    int32_t vmf_lt_099;  /* 1.0*MTCnt/usedMT < 0.99, the gate of HP and LowC (:198,:202) */
    int32_t vdp;         /* alleleCnt[allele] */
    int32_t vmt;         /* MTCnt[allele] */
    int32_t vsm;         /* strongMTCnt[allele] */
    int32_t pad;
    int32_t tal[SMC_NT]; /* tallies of this allele: alleleCnt and the pair counts (SMC_T_CNT, _CONCORD, _DISCORD) always; the eight
                          * that only filterVariants reads (SMC_T_FWD .. SMC_T_R2PRLE) where flt_applied - the device does not
                          * count them for a locus no candidate of which reaches the filters */
    double pi;           /* finalDict[allele], unrounded */
    double p_sb, p_r1, p_r2, p_pr; /* Fisher two-sided p-values of the four tests, NaN if not run */
} smc_cand;

/* One per locus: everything the 45-column row (smCounter.py:575-600) is printed from. 432 bytes. */
typedef struct smc_row {
    int32_t status;
    int32_t n_touched;   /* number of keys in finalDict */
    int32_t cvg, all_frag, all_mt, used_frag, used_mt; /* DP FR MT UFR UMT */
    int32_t mt3, mt5, mt7, mt10;
    int32_t max_allele, second_allele; /* maxBase / secondMaxBase (:535-537) */
    int32_t biallelic;   /* condition of :555 */
    int32_t dp[4], umt[4], vsm[4]; /* A,T,G,C: alleleCnt, MTCnt, strongMTCnt */
    double pi[4];        /* A,T,G,C: finalDict, unrounded */
    uint64_t touched_mask;
    int32_t ref_tal[SMC_NT]; /* tallies of the reference allele: alleleCnt always, the filter-only eight where a candidate has
                              * flt_applied; its pair counts are not kept (nothing reads them: the DP filter looks at the candidate's) */
    smc_cand cand[2];    /* [0] origAlt (:541), [1] secondMaxBase when biallelic */
} smc_row;

/* What travels between GPUs: the part of smc_row that the 45-column row is PRINTED from (smCounter.py:575-600; rows.py),
 * 168 bytes instead of 432.  The tallies and Fisher p-values stay behind: filterVariants has already run on the device
 * and left its verdict in the FILTER bits.  Replaces the pickled result strings of the reference's pool
 * (`[p.get() for p in results]`, smCounter.py:685). */
#define SMC_WIRE_BIALLELIC 0x10000u   /* smc_wire_row.status bit 16: smc_row.biallelic; bits 0-15: smc_row.status */
#define SMC_WIRE_FLT_MASK 0x3FFu      /* smc_wire_cand.flags bits 0-9: SMC_F_* */
#define SMC_WIRE_FLT_APPLIED 0x400u   /* bit 10: smc_cand.flt_applied */
#define SMC_WIRE_VMF_LT_099 0x800u    /* bit 11: smc_cand.vmf_lt_099 */
typedef struct smc_wire_cand {
    int16_t allele;  /* -1: no such candidate */
    uint16_t flags;
    int32_t vdp, vmt, vsm;
    double pi;
} smc_wire_cand;
typedef struct smc_wire_row {
    uint32_t status;
    int32_t cvg, all_frag, all_mt, used_frag, used_mt;
    int32_t mt3, mt5, mt7, mt10;
    int32_t dp[4], umt[4], vsm[4];
    double pi[4];
    smc_wire_cand cand[2];
} smc_wire_row;

/* ---- input of the device plane builder (smc_build_planes): a run's alignments as a structure of arrays, one entry per
 * ALIGNMENT, produced by the decoder (libsmc_bam.so: smc_bam_alignments, smcounter_host.h) */
#define SMC_DA_R1 1u
#define SMC_DA_R2 2u
#define SMC_DA_REV 4u
#define SMC_DA_MMOK 16u /* mismatchPer100b <= mismatchThr (smCounter.py:352-356, third term of incCond :378) */
typedef struct smc_dev_aln {
    int32_t pos, end;          /* 0-based reference span [pos, end) */
    uint32_t cig_off, seq_off; /* first CIGAR word / first base (and quality) in the pools */
    uint16_t n_cig;
    uint8_t oflag, mapq;
    uint16_t left_sp, qalen;   /* leading soft clip, query_alignment_length (:336-349, :434-448) */
    uint16_t l_seq, pad;
    uint32_t bc_gid, pair_gid; /* run-wide ids of the barcode and of (barcode, read id), dense, in file order */
} smc_dev_aln;
typedef struct smc_dev_locus {
    uint32_t w0, w1;           /* alignments [w0, w1) are the candidates that can cover the locus */
    uint32_t slot_off, n;      /* first (4-aligned) read slot of the locus in the run's planes, pileup depth */
} smc_dev_locus;

typedef struct smc_ctx smc_ctx;
typedef struct smc_plan smc_plan;

int smc_abi_version(void);
const char* smc_last_error(void);
int smc_row_size(void);   /* sizeof(smc_row), for binding self-checks */
int smc_locus_size(void); /* sizeof(smc_locus) */

/* Number of gfx950 devices visible; does not initialise any of them. */
int smc_device_count(void);

/* (diagnostic, no GPU needed) the read-class table the kernel uses: out[2c], out[2c+1] for class c < 32 - nine 5-bit
 * tally increments in SMC_T_* order (six in the first word, three in the second); second word bit 31 = incCond. */
void smc_class_table(uint32_t* out);

/* Bind a context to one device (one per process / host thread). */
int smc_create(int device, smc_ctx** out);
void smc_destroy(smc_ctx* ctx);

/* Build a launch plan for a batch: bins loci by on-chip table size, uploads the descriptors and the
 * bin index lists. `loci` is host memory; it is copied. Replaces the construction of the
 * apply_async task list, smCounter.py:684. */
int smc_plan_create(smc_ctx* ctx, const smc_locus* loci, int64_t n_loci, smc_plan** out);
void smc_plan_destroy(smc_plan* plan);
/* The same plan for a batch whose descriptors are already on the DEVICE (smc_build_planes has just written them): the binning
 * runs there, only a small record (and the few loci deep enough to be cut into parts) comes back.  Enqueued on `stream`
 * behind whatever wrote `d_loci`; synchronises on it.  `d_loci` stays the caller's and must outlive the plan.  Plans of one
 * context may be made on different streams one after the other (the record they sum into is the context's: a plan's kernels wait
 * for the plan before it to be through with it); a plan is run by one stream at a time. */
int smc_plan_create_dev(smc_ctx* ctx, const smc_locus* d_loci, int64_t n_loci, void* stream, smc_plan** out);
/* (ABI 8) The same plan WITHOUT the host in the loop: nothing here waits for the device.  The launches are sized from the record of
 * the context's last plan (scaled to this batch's loci, with room) instead of this batch's own, which the device sums while the
 * host goes on; whether the batch FITS those sizes is decided on the device: one that does not launches nothing.  So, after the
 * caller has synchronised the stream for the rows, smc_plan_spec_ok(plan, &ok) says whether they are this batch's (ok = 1) or the
 * plan has to be made again - by this function, which then goes the exact way (as it does for a context's first plan: there is
 * nothing to size it from), or by smc_plan_create_dev - and run again (ok = 0).  For callers that make plan after plan of batches of
 * one kind - the runs of a BAM (smCounter.py:683-685 submits them one after the other), the steps of the bench: the host thread no
 * longer waits for the build of the planes, the device no longer idles around the read-back.  `prm`: the parameters the planes were
 * built with (every descriptor has to carry their fingerprint).  smc_plan_run (raw-field planes) is not for such a plan. */
int smc_plan_create_dev_spec(smc_ctx* ctx, const smc_params* prm, const smc_locus* d_loci, int64_t n_loci, void* stream, smc_plan** out);
int smc_plan_spec_ok(smc_plan* plan, int* ok);
/* Plans made by smc_plan_create_dev_spec in this context, how many of them went the exact way, how many the device found not to
 * fit (reads a counter on the device: synchronises it) - for a caller that destroys its plans unchecked (a benchmark loop). */
int smc_plan_spec_counts(smc_ctx* ctx, int64_t* made, int64_t* exact, int64_t* not_fitting);
/* Forget what the context's next such plan would be sized from (it then goes the exact way): for a caller that knows its next batch
 * is of another kind than the last one. */
int smc_plan_hint_reset(smc_ctx* ctx);

/* (ABI 8) The NON-parity down-sampling of loci over the barcode cap, on the device.  smCounter.py:496-498 seeds Python 2's
 * Mersenne twister with the position STRING and samples bcDict's keys in Python 2's dict order; the parity path reproduces that on
 * the host from the barcode texts and marks the dropped keys in umi_start (SMC_LF_SAMPLED / SMC_USTART_DROPPED above).  This call
 * leaves the same kind of marks without the host's sampler: every key of bcDict of a locus with n_umi > ds (and no marks yet) gets
 * the 64-bit value made of words 0 and 1 of Philox4x32-10(counter = (identity lo, identity hi, 0, 0), key = the two halves of
 * (position ^ seed)); the ds smallest stay (ties: the lower index).  `d_ident`: one 64-bit identity per umi_start entry (read
 * only at loci over the cap) - e.g. a hash of the barcode's text: the sample then depends on (seed, position, barcode) alone, not on
 * how the caller numbered the barcodes or cut the file into batches; NULL: the barcode's index in its locus.  With
 * `d_ident_index` (one uint32 per umi_start entry: what smc_build_planes leaves in u_gid at such loci - the run-wide barcode id)
 * `d_ident` is a table by that index instead.  Counter-based - no
 * state, no order - so the marks do not depend on the launch; oracle/smc_oracle.c restates it (smc_oracle_philox_marks).  NOT what
 * the reference samples: rows of such loci carry SMC_ST_DOWNSAMPLED and differ from smCounter's.  d_pos[l]: the 1-based position
 * of locus l; d_status: a word the call ORs bits into - 1: a locus with more than 2^18 barcodes was left to the stand-in (the ds
 * lowest indices).  Enqueued on `stream` after whatever wrote the words, before the batch's plan runs. */
int smc_philox_marks(smc_ctx* ctx, const smc_params* prm, smc_locus* d_loci, int64_t n_loci, const int64_t* d_pos, const void* d_words,
                     int word_bits, uint32_t* d_umi_start, const uint64_t* d_ident, const uint32_t* d_ident_index, uint64_t seed,
                     uint32_t* d_status, void* stream);
void smc_philox4x32_10_host(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);
/* (ABI 9) In-run molecule down-sampling (ds.mt.py:23-72 without the BAM in between): the alignments of one run (smc_dev_aln[n_aln],
 * smc_dev_locus[n_loci], as smc_build_planes takes them; the CIGAR and base pools are not touched) reduced to those of the KEPT
 * barcodes, and the descriptors recomputed as smc_bam_alignments computes them for the down-sampled BAM:
 *   d_aln_out[k], d_orig_index[k]   the kept alignments in file order, and each one's index in d_aln (capacity: n_aln each)
 *   d_loc_out[n_loci]               w0 = first kept alignment with end > p; w1 = max(w0, first kept alignment with pos > p);
 *                                   n = kept alignments with pos <= p < end; slot_off = exclusive scan of n rounded up to 4
 *                                   (p = start0 + locus index)
 *   d_summary[4]                    kept alignments, deepest n, total slots, 0
 * bc_gid / pair_gid stay as they were (with gaps, in order: the builder only compares them), as do the run's n_bc / n_pair, and every
 * kept alignment keeps its cig_off / seq_off.  Which barcodes are kept, by run-wide id g < n_ids:
 *   d_keep_mask != NULL  bit g of d_keep_mask (uint32 words) - a set the host chose (the reference's semantics);
 *   else                 Philox4x32-10(counter = (d_ident[g] lo, hi, 0x64734D54, 0), key = (seed lo, hi)) word 0 < floor(frac * 2^32);
 *                        frac >= 1 keeps every barcode.  The same draw for every fraction: the kept sets are nested.
 * The input windows d_loc are not read (may be NULL).  Asynchronous on `stream`; one scratch per context (calls of one context are
 * to be ordered on one stream). */
int smc_select_alignments(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0,
                          const uint32_t* d_keep_mask, const uint64_t* d_ident, int64_t n_ids, uint64_t seed, double frac,
                          smc_dev_aln* d_aln_out, uint32_t* d_orig_index, smc_dev_locus* d_loc_out, uint32_t* d_summary, void* stream);
/* (ABI 10) The same with the level of the keep rule's key.  SMC_SEL_KEY_BARCODE: the id g is bc_gid (smc_select_alignments exactly;
 * n_bc / n_pair are not read).  SMC_SEL_KEY_READ: g is pair_gid - the read-level rule of ds.reads.withinMT.py:37-82, which keeps whole
 * read names (every alignment of a kept name, none of the others); d_keep_mask is then a bit per run-wide read-name id, d_ident (the
 * philox rule) an identity per read-name id, and n_ids counts read-name ids.  The caller makes sure a read-name id stands for one
 * full query name of the file (smc_bam_pair_idents reports the ids that do not: pair_gid drops the name's last field).  A read name
 * is all in or all out, so the kept alignments keep the file order and the windows / depths / slots are those above.  The ids are
 * not: dropping a barcode's first reads can move its first appearance, and the plane builder's rows depend on the ids' order.  So at
 * the read level the kept alignments' bc_gid and pair_gid are renumbered densely by first kept appearance (ids < n_bc / n_pair, the
 * run's counts; the caller may keep passing those counts on to the builder) - the decoder's numbering of the down-sampled BAM.
 * The key is read from the record the kernels load anyway; the renumbering is five launches more over the kept records and
 * 8 bytes of scratch per id. */
#define SMC_SEL_KEY_BARCODE 0
#define SMC_SEL_KEY_READ 1
int smc_select_alignments_keyed(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0,
                                int32_t key, int64_t n_bc, int64_t n_pair, const uint32_t* d_keep_mask, const uint64_t* d_ident, int64_t n_ids,
                                uint64_t seed, double frac, smc_dev_aln* d_aln_out, uint32_t* d_orig_index, smc_dev_locus* d_loc_out,
                                uint32_t* d_summary, void* stream);
/* (ABI 11, additive: one entry more, the version number unchanged) The philox selections of n_copies copies of a run at n_fracs
 * fractions in one call - what n_copies x n_fracs smc_select_alignments calls give, without their launches, allocations and downloads.
 * Copy c's records stand at d_aln + c x aln_stride_bytes (0: the copies share the records; else a positive multiple of 4) and are drawn
 * with seeds[c]; a barcode's draw serves every fraction, so the kept sets of a copy are nested in the fraction.  `seeds` (n_copies) and
 * `fracs` (n_fracs doubles, each in (0, 1]) are HOST arrays, read before the call returns.  Selection s = f x n_copies + c, fractions
 * outer - the selections of one fraction lie at a constant stride:
 *   d_aln_out + s x n_aln, d_orig_index + s x n_aln   the kept records in file order and their indices in the copy
 *   d_loc_out + s x n_loci                            the n_loci descriptors
 *   d_summary + 4 x s                                 kept alignments, deepest n, total slots (the fourth word is not written)
 * For every (c, f) the first `kept` records, their indices, all descriptors and the three summary words are byte for byte what
 * smc_select_alignments writes for copy c's records with d_keep_mask = NULL, the same d_ident, seeds[c] and fracs[f] (the same
 * threshold floor(f x 2^32), 2^32 at f = 1: everything); nothing is written behind the kept records.  d_ident must hold n_ids
 * identities (it is read at f = 1 too).  SMC_E_INPUT, nothing launched: n_copies or n_fracs below 1, more than SMC_SEL_MAX_SELECTIONS
 * selections, a fraction outside (0, 1], a negative stride or one that is no multiple of 4, a NULL output.  Asynchronous on `stream`;
 * the scratch is the context's, once per selection (4 bytes per locus and 8 per 1024 alignments each), shared with smc_select_alignments:
 * calls of one context are to be ordered on one stream. */
#define SMC_SEL_MAX_SELECTIONS 2048
int smc_select_alignments_copies(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t aln_stride_bytes, int32_t n_copies, int64_t n_aln,
                                 const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0, const uint64_t* d_ident, int64_t n_ids,
                                 const uint64_t* seeds, const double* fracs, int32_t n_fracs, smc_dev_aln* d_aln_out, uint32_t* d_orig_index,
                                 smc_dev_locus* d_loc_out, uint32_t* d_summary, void* stream);
/* (ABI 11, additive: one entry more, the version number unchanged) The READ-level selections of n_copies copies of a run under n_masks
 * keep masks each in one call - what n_copies x n_masks smc_select_alignments_keyed calls at SMC_SEL_KEY_READ give, without their
 * launches, allocations and downloads.  Copy c's records stand at d_aln + c x aln_stride_bytes (0: the copies share the records; else
 * a positive multiple of 4).  The keep mask of (copy c, mask m) stands at d_masks + c x mask_copy_stride_words + m x mask_words
 * (uint32 words; a stride of 0: every copy uses the same masks) and holds a bit per run-wide read-name id, n_ids of them - the layout
 * smc_read_groups_masks writes for one seed, the seeds of a run behind each other.  The masks of a copy need not be nested.
 * Selection s = m x n_copies + c, masks outer - smc_select_alignments_copies' layout:
 *   d_aln_out + s x n_aln, d_orig_index + s x n_aln   the kept records in file order and their indices in the copy
 *   d_loc_out + s x n_loci                            the n_loci descriptors
 *   d_summary + 4 x s                                 kept alignments, deepest n, total slots (the fourth word is not written)
 * For every (c, m) the first `kept` records - with bc_gid and pair_gid renumbered by first kept appearance -, their indices, all
 * descriptors and the three summary words are byte for byte what smc_select_alignments_keyed(key = SMC_SEL_KEY_READ, n_bc, n_pair,
 * d_keep_mask = that mask, d_ident = NULL, n_ids) writes for copy c's records; nothing is written behind the kept records.
 * SMC_E_INPUT, nothing launched: n_copies or n_masks below 1, more than SMC_SEL_MAX_SELECTIONS selections, a negative record stride or
 * one that is no multiple of 4, a negative mask stride, mask_words below ceil(n_ids / 32), negative n_bc / n_pair / n_ids, NULL
 * d_masks, a NULL output.  Asynchronous on `stream`; the scratch is the context's, once per selection (4 bytes per locus, 16 per 1024
 * alignments and 8 per barcode id and read-name id each), shared with smc_select_alignments: calls of one context are to be ordered
 * on one stream. */
int smc_select_alignments_reads_copies(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t aln_stride_bytes, int32_t n_copies, int64_t n_aln,
                                       const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0, int64_t n_bc, int64_t n_pair,
                                       const uint32_t* d_masks, int64_t mask_words, int64_t mask_copy_stride_words, int32_t n_masks,
                                       int64_t n_ids, smc_dev_aln* d_aln_out, uint32_t* d_orig_index, smc_dev_locus* d_loc_out,
                                       uint32_t* d_summary, void* stream);
/* (ABI 11) The read-level philox sampler of --dsRpb (--dsRpbSampler philox): a file-wide table of read names and barcodes that stays
 * in HBM for the whole run (csrc/k_read_groups.inc).  Grouping as ds.reads.withinMT.py:37-58: the unit is the full read name, its
 * barcode field -2 of the stripped name; per barcode the names counted; one / multi = barcodes with one / two or more names,
 * multi_names = names in the latter.  A name is kept at a target when it is its barcode's first (its first record has the smallest
 * ordinal of the barcode's records) or when word 0 of Philox4x32-10(counter = (identity lo, identity hi, 0x64735250 "dsRP", 0),
 * key = (seed lo, seed hi)) < thr, thr = floor(probKeep * 2^32) in [0, 2^32] (the host computes probKeep from the counters).
 *   _create   an empty table.
 *   _add      n keys of consecutive placed records (host memory; smc_bam_name_keys writes them), the first one's ordinal in the file;
 *             copied to the device, inserted by _finish.  Ordinals below 2^32 - 1, every record once.
 *   _finish   sizes the two tables from the records added (power of two, load factor <= 0.5), inserts them, checks every record's
 *             check words against its slots', groups; counts[SMC_RG_N_COUNTS] (below) back on the host.
 *   _masks    per run: for n_ids read-name identities in HBM (smc_bam_pair_idents of the run, uploaded), n_thr <= SMC_RG_MAX_TARGETS
 *             thresholds (host) -> d_masks[t * ceil(n_ids / 32) + (g >> 5)] bit (g & 31): id g kept at target t - the mask
 *             smc_select_alignments_keyed takes at SMC_SEL_KEY_READ.  An identity the table does not hold sets SMC_RG_MISS.
 *   _kept     the file-wide kept names per target (host kept[n_thr]).
 *   _status   the SMC_RG_* bits so far (0: every key had one text).  After _finish / _masks / _kept (synchronises the device).
 * Everything runs on the null stream except _masks (`stream`). */
typedef struct smc_read_groups smc_read_groups;
typedef struct smc_read_key {          /* one placed record: 24 bytes, smc_bam_name_keys' 3 words */
    uint64_t name_id;                  /* FNV-1a 64 of the full read name */
    uint64_t bc_id;                    /* FNV-1a 64 of its barcode */
    uint32_t name_chk, bc_chk;         /* FNV-1a 32 of the same texts: the check words */
} smc_read_key;
#define SMC_RG_MAX_TARGETS 32
#define SMC_RG_N_COUNTS 8              /* records, names, barcodes, one, multi, multi_names, first names, 0 */
#define SMC_RG_NAME_COLLISION 1u       /* two records with one name identity and different check words (or barcodes) */
#define SMC_RG_BARCODE_COLLISION 2u    /* two records with one barcode identity and different check words */
#define SMC_RG_FULL 4u                 /* a probe went round a whole table */
#define SMC_RG_MISS 8u                 /* _masks: an identity the table does not hold */
#define SMC_RG_RESERVED 16u            /* an identity equal to 0 (the empty slot's mark) */
int smc_read_groups_create(smc_ctx* ctx, smc_read_groups** out);
int smc_read_groups_add(smc_read_groups* g, const smc_read_key* keys, int64_t n, int64_t first_ordinal);
int smc_read_groups_finish(smc_read_groups* g, int64_t* counts);
int smc_read_groups_masks(smc_read_groups* g, const uint64_t* d_idents, int64_t n_ids, uint64_t seed, const uint64_t* thr, int32_t n_thr,
                          uint32_t* d_masks, void* stream);
int smc_read_groups_kept(smc_read_groups* g, uint64_t seed, const uint64_t* thr, int32_t n_thr, int64_t* kept);
int smc_read_groups_status(smc_read_groups* g, uint32_t* status);
void smc_read_groups_destroy(smc_read_groups* g);
/* (ABI 11, additive: three entries more, the version number unchanged) --dsGrid: the barcode rule of smc_select_alignments' philox
 * rule and the read rule above composed, over the same finished table.  A name is kept in cell c when word 0 of
 * Philox4x32-10(counter = (its barcode's identity lo, hi, 0x64734D54 "dsMT", 0), key = seed) < bc_thr[c] - floor(f * 2^32), 2^32 at
 * f >= 1: the same draw and threshold as smc_select_alignments at frac f - and it is its barcode's first name or its own draw (above)
 * < rd_thr[c].  Thresholds <= 2^32, at most SMC_RG_MAX_TARGETS of them.
 *   _counts_frac  per fraction f < n_frac the counters of the barcodes kept at bc_thr[f] (host counts[f * SMC_RG_N_COUNTS + k], the
 *                 layout above: records 0 (not counted per barcode), names, barcodes, one, multi, multi_names, first names (one per
 *                 barcode), 0) - probKeep of a cell is the host's, from these.
 *   _masks_grid   per run: _masks with a mask per cell, d_masks[c * ceil(n_ids / 32) + (g >> 5)] (`stream`; SMC_RG_MISS as _masks).
 *   _kept_grid    the file-wide kept names per cell (host kept[n_cells]).
 * Everything runs on the null stream except _masks_grid. */
int smc_read_groups_counts_frac(smc_read_groups* g, uint64_t seed, const uint64_t* bc_thr, int32_t n_frac, int64_t* counts);
int smc_read_groups_masks_grid(smc_read_groups* g, const uint64_t* d_idents, int64_t n_ids, uint64_t seed, const uint64_t* bc_thr,
                               const uint64_t* rd_thr, int32_t n_cells, uint32_t* d_masks, void* stream);
int smc_read_groups_kept_grid(smc_read_groups* g, uint64_t seed, const uint64_t* bc_thr, const uint64_t* rd_thr, int32_t n_cells,
                              int64_t* kept);
/* (ABI 11, additive: one entry more, the version number unchanged) --lod: the limit of detection by barcode depth, as the reference's
 * mt_depths_lod.R computes it - roots[d], d = 0 .. max_depth, is the root on [0, 1] of pbinom(needed - 1, d, p) - 0.05 that R's
 * uniroot returns (R_zeroin2, tol = DBL_EPSILON^0.25, maxit 1000), NOT yet rounded to 4 decimals (the caller rounds); 1.0 where
 * d < 5, where the end values have the same sign (every d < needed) and where the search does not converge.  iters[d] (may be NULL):
 * passes of the search's loop (0: none made; 1001: no convergence).  roots / iters: HOST arrays of max_depth + 1 elements; device
 * scratch is the context's, the kernel runs on the null stream and the call returns with the values.  needed < 1, max_depth < 0 or
 * max_depth > SMC_LOD_MAX_DEPTH: SMC_E_INPUT, nothing is launched. */
#define SMC_LOD_MAX_DEPTH (1 << 24)
int smc_lod_table(smc_ctx* ctx, int needed, int max_depth, double* roots, int32_t* iters);
/* (ABI 11, additive: two entries more, the version number unchanged) FOR CHECKING, like smc_philox4x32_10_host: the arithmetic of
 * the four Fisher tests of k_filter_loci on arguments of the caller's choice (the filter kernel only sees the tallies the locus
 * kernel wrote).  Host pointers in and out, device scratch of the context, the null stream; both return with the values.
 *   smc_fisher_tables  tables[n][4] = a b c d, rows first (scipy.stats.fisher_exact([[a, b], [c, d]])): one wavefront per table
 *                      runs the filter kernel's own device function with the context's log-factorial table -> oddsratio[n],
 *                      pvalue[n] (two-sided; a zero margin: NaN, 1; b * c == 0: inf).  A negative count, or a table whose counts add
 *                      up to more than INT32_MAX (the tallies are int): SMC_E_INPUT, nothing is launched.  n == 0: nothing happens.
 *   smc_lfact_values   out[i] = the log(v!) a Fisher test uses for v = n_values[i] >= 0: the context's table below 65536, Stirling's
 *                      series from there on.  n_values[i] < 0: the series (the constants below 8) at ~n_values[i] whatever its size
 *                      - what the table was filled from, so that the two can be compared at one argument.
 * At most 2^24 tables / values per call. */
int smc_fisher_tables(smc_ctx* ctx, const int64_t* tables, int64_t n, double* oddsratio, double* pvalue);
int smc_lfact_values(smc_ctx* ctx, const int64_t* n_values, int64_t n, double* out);
/* (ABI 11, additive: one entry more, the version number unchanged) --dsAF: which barcodes of a run cover / carry a listed allele.
 * The run as smc_build_planes takes it (d_aln[n_aln], the CIGAR pool, the (letter, quality) pair pool, d_loc[n_loci], start0, n_bc:
 * nothing of it is written); d_var[n_var]: the listed variants of the run, each a locus index and an allele key by the keys the
 * caller uses (smCounter.py:371-460):
 *   SMC_AF_SNV  the letter `letter` with no insertion or deletion starting behind it
 *   SMC_AF_INS  INS|X|XS: `letter` = X, the `len` letters S at d_ins[ins_off ..] (len <= SMC_AF_MAX_INS), compared with the read's
 *               inserted letters as the host's slice clamps them at the read's end
 *   SMC_AF_DEL  DEL|XD|X: `letter` = X, `len` = the deleted positions (the letters D are the reference's: a deletion listed with other
 *               letters is one no read shows - SMC_AF_NONE)
 *   SMC_AF_NONE a key no read shows
 * Per variant v and run-wide barcode id g < n_bc, over the pileup of v's locus (the alignments with pos <= p < end: the loc[].n reads
 * of the plane builder, no quality or mapping filter): reads = the barcode's reads there, alt = those that show v's key.
 *   d_covers / d_carries  [n_var][2 * ceil(n_bc / 64)] uint32 words each: bit g of v's mask - reads > 0 / 2 * alt > reads; the bits
 *                         at and beyond n_bc are 0.  8-byte aligned.
 *   d_counts              [n_var][n_bc][2] uint32 (reads, alt), 8-byte aligned; NULL: the counters stay in the context's scratch
 * Enqueued on `stream`; nothing waits.  n_var > SMC_AF_MAX_VARIANTS, a locus index beyond n_loci, a kind beyond SMC_AF_NONE, a len
 * beyond SMC_AF_MAX_INS, inserted letters beyond the n_ins bytes of d_ins: SMC_E_INPUT, nothing is launched (d_var / d_ins are DEVICE arrays: `var_host`, the same n_var records in host
 * memory, is what is checked and what sizes the launch). */
#define SMC_AF_SNV 0u
#define SMC_AF_INS 1u
#define SMC_AF_DEL 2u
#define SMC_AF_NONE 3u
#define SMC_AF_MAX_INS 255
#define SMC_AF_MAX_VARIANTS 4096
typedef struct smc_af_variant {
    uint32_t locus;            /* index into d_loc: p = start0 + locus */
    uint32_t kind, letter;     /* SMC_AF_*; the site's letter (the ALT of an SNV, the anchor of an insertion / deletion) */
    uint32_t len, ins_off;     /* inserted letters (and where they start in d_ins) / deleted positions */
    uint32_t pad[3];
} smc_af_variant;
int smc_allele_carriers(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, const uint8_t* d_bq,
                        const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0, int64_t n_bc, const smc_af_variant* d_var,
                        const smc_af_variant* var_host, int32_t n_var, const uint8_t* d_ins, int64_t n_ins, uint32_t* d_covers, uint32_t* d_carries,
                        uint32_t* d_counts, void* stream);
/* (ABI 11, additive: two entries more, the version number unchanged) --dsAFReps: R replicates of the --dsAF dilution, replicate j
 * with the seed seeds[j]; everything but the barcode draw u_j(b) = word 0 of Philox4x32-10(counter = (identity lo, identity hi,
 * 0x64734146 "dsAF", 0), key = (seeds[j] lo, hi)) is the same in every replicate.  The CARRIER TABLE is the host's: d_car[n_car],
 * the identities of the barcodes that carry a listed variant, ascending and unique, and d_car_thr[n_car][n_targets], per carrier
 * and target the smallest floor(k * 2^32) among the variants it carries (in [0, 2^32]: 64-bit words).  A barcode is DROPPED in
 * replicate j at target t when the table holds it at c and u_j >= d_car_thr[c][t]; every other barcode is kept.  `car_host` /
 * `car_thr_host`: the same table in host memory - what is checked.
 *   _masks   for the n_ids run-wide barcode identities of one decoded run (d_idents: smc_bam_barcode_idents, uploaded):
 *            d_masks[(j * n_targets + t) * n_words + (g >> 5)] bit (g & 31) = id g is kept - n_reps * n_targets masks of n_words
 *            uint32 words each, n_words >= ceil(n_ids / 32); the bits at and beyond n_ids and the words behind them are written
 *            as 0.  Each is a mask smc_select_alignments takes as d_keep_mask.  d_draws (may be NULL): [n_reps][n_ids] the "dsAF"
 *            draw u_j of every carrier, 0 for the others (tests).
 *   _counts  the achieved numbers, file-wide: d_cov_ident / d_cov_carry hold the covering barcodes of all n_var listed variants one
 *            behind the other (variant v's at [cov_off[v], cov_off[v + 1]); carry != 0: the barcode carries v) ->
 *            d_out[v][j][t][2] uint32 = (N', V'): the kept covering barcodes and the kept carriers of v.  d_cov_off: the n_var + 1
 *            offsets in device memory, `cov_off_host` the same on the host.  d_out is zeroed by the call.
 * Both ARE the smc_af_depth_* entries below at one fraction whose threshold is 2^32 (every barcode passes the depth rule; its draw
 * is not made): the same kernels, the same checks, the entry's own name in the messages.
 * Enqueued on `stream`; nothing waits.  SMC_E_INPUT, nothing launched: a table that is not strictly ascending, a threshold above
 * 2^32, n_targets above SMC_AF_REP_MAX_TARGETS, n_reps above SMC_AF_REP_MAX_REPS, n_words below ceil(n_ids / 32),
 * n_reps * n_targets * n_words (or n_var * n_reps * n_targets * 2) of 2^32 - 256 words or more, offsets that decrease. */
#define SMC_AF_REP_MAX_TARGETS 32      /* (= SMC_RG_MAX_TARGETS: the masks one run's launch makes for the selection) */
#define SMC_AF_REP_MAX_REPS 1000
int smc_af_rep_masks(smc_ctx* ctx, const uint64_t* d_idents, int64_t n_ids, const uint64_t* d_car, const uint64_t* d_car_thr,
                     const uint64_t* car_host, const uint64_t* car_thr_host, int64_t n_car, int32_t n_targets, const uint64_t* d_seeds,
                     int32_t n_reps, uint32_t* d_masks, int64_t n_words, uint32_t* d_draws, void* stream);
int smc_af_rep_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint8_t* d_cov_carry, const uint32_t* d_cov_off,
                      const uint32_t* cov_off_host, int32_t n_var, const uint64_t* d_car, const uint64_t* d_car_thr,
                      const uint64_t* car_host, const uint64_t* car_thr_host, int64_t n_car, int32_t n_targets, const uint64_t* d_seeds,
                      int32_t n_reps, uint32_t* d_out, void* stream);
/* (ABI 11, additive: two entries more, the version number unchanged) --dsAFDepth: the cells (target t, barcode fraction f) of the
 * --dsAF dilution.  A barcode is KEPT in cell (t, f) of replicate j when smc_af_rep_masks keeps it at t (the carrier table and the
 * "dsAF" draw above, key seeds[j]) AND its depth draw d_j(b) = word 0 of Philox4x32-10(counter = (identity lo, identity hi,
 * 0x64734D54 "dsMT", 0), key = (seeds[j] lo, hi)) - smc_select_alignments' philox rule - is below depth_thr[f].  `depth_thr`: HOST
 * memory, n_fracs words, floor(f * 2^32) each and 2^32 at f = 1 (every barcode stays: the masks and the counts are smc_af_rep_*'s,
 * which are these entries at that one fraction).  The depth draw is made for every barcode - unless no threshold is below 2^32 and
 * d_draws is NULL, when it decides nothing - the "dsAF" draw for carriers only.
 *   _masks   d_masks[((j * n_targets + t) * n_fracs + f) * n_words + (g >> 5)] bit (g & 31) = id g is kept: n_reps * n_targets *
 *            n_fracs masks in smc_af_rep_masks' layout.  d_draws (may be NULL): [n_reps][n_ids] the "dsMT" depth draw d_j of every
 *            id - not the "dsAF" draw smc_af_rep_masks reports (tests).
 *   _counts  d_out[v][j][t][f][2] uint32 = (N', V') of the cell, from the covering barcodes as smc_af_rep_counts takes them.
 * Enqueued on `stream`; nothing waits.  SMC_E_INPUT, nothing launched: what smc_af_rep_masks / _counts refuse, a depth threshold
 * above 2^32, n_targets * n_fracs above SMC_AF_DEPTH_MAX_CELLS, an output of 2^32 - 256 words or more. */
#define SMC_AF_DEPTH_MAX_CELLS 32      /* (= SMC_RG_MAX_TARGETS) */
int smc_af_depth_masks(smc_ctx* ctx, const uint64_t* d_idents, int64_t n_ids, const uint64_t* d_car, const uint64_t* d_car_thr,
                       const uint64_t* car_host, const uint64_t* car_thr_host, int64_t n_car, int32_t n_targets,
                       const uint64_t* depth_thr, int32_t n_fracs, const uint64_t* d_seeds, int32_t n_reps, uint32_t* d_masks,
                       int64_t n_words, uint32_t* d_draws, void* stream);
int smc_af_depth_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint8_t* d_cov_carry, const uint32_t* d_cov_off,
                        const uint32_t* cov_off_host, int32_t n_var, const uint64_t* d_car, const uint64_t* d_car_thr,
                        const uint64_t* car_host, const uint64_t* car_thr_host, int64_t n_car, int32_t n_targets,
                        const uint64_t* depth_thr, int32_t n_fracs, const uint64_t* d_seeds, int32_t n_reps, uint32_t* d_out, void* stream);
/* (ABI 11, additive: one entry more, the version number unchanged) --spikeAF: listed SNVs planted in a run's bases, whole barcodes
 * at a time.  The run as smc_build_planes takes it (d_aln[n_aln], the CIGAR pool, the (letter, quality) pair pool of n_pairs pairs:
 * nothing of it is written).  d_var[n_var]: the listed variants of the run's chromosome, strictly ascending by 0-based position - ANY
 * reference position, not only a locus of the run: an alignment that spans it is rewritten in whichever run it was decoded.
 * d_idents[n_bc]: the identity of every run-wide barcode id (smc_bam_barcode_idents, uploaded).  d_nm / d_n_indel[n_aln]: per
 * alignment its NM (0 when absent) and its CIGAR's inserted plus deleted length (smc_bam_run_mismatches, uploaded).
 * Barcode b is SPIKED at variant v when word 0 of Philox4x32-10(counter = (identity lo, identity hi, 0x73704146 "spAF",
 * (pos0 + 1) mod 2^32), key = (seed lo, seed hi)) < thr - one draw per barcode and variant.  Every alignment of a spiked barcode with
 * pos <= pos0 < end whose allele key there is a single letter (a base, not inside a deletion, with no insertion or deletion starting
 * behind it: the plane builder's rules) gets `alt` as that base's letter; its NM grows by 1 when the old letter was `ref`.
 *   d_aln_out[n_aln]    the records, each with SMC_DA_MMOK recomputed as smc_bam_alignments computes it, from the new NM:
 *                       100.0 * max(0, NM' - n_indel) / l_seq <= mismatch_thr in double, 0.0 for l_seq == 0
 *   d_bq_out            the pair pool (2 * n_pairs bytes, copied here from d_bq) with the letters rewritten; qualities stay
 *   d_stats[n_var][2]   uint32: records rewritten at v (one that showed `alt` already counts), records whose NM grew; zeroed here
 * Enqueued on `stream`; nothing waits.  SMC_E_INPUT, nothing launched and nothing copied: positions not strictly ascending, a letter
 * outside ACGT, ref equal to alt, a threshold above 2^32, more than SMC_AF_MAX_VARIANTS variants (d_var is a DEVICE array:
 * `var_host`, the same n_var records in host memory, is what is checked).
 * PHASE SETS (--spikePhase).  `lead` names, per record, the leader of its set: the member with the smallest position, var[k - lead].
 * Record k is drawn with counter word 3 = (var[k - lead].pos0 + 1) mod 2^32 in place of its own position, so a barcode is spiked at
 * every member of a set or at none; with lead = 0 everywhere the call is bit for bit what it was.  Also SMC_E_INPUT, nothing launched
 * and nothing copied: var_host[k].lead > k, or a leader whose own `lead` is not 0 (smc_spike_alleles_reps refuses the same). */
typedef struct smc_spike_variant {
    int32_t pos0;              /* 0-based reference position */
    uint8_t ref, alt;          /* ASCII, out of A C G T */
    uint16_t lead;             /* records back, in this array, to the leader of the variant's phase set; 0: its own leader */
    uint64_t thr;              /* floor(t * 2^32), in [0, 2^32] */
} smc_spike_variant;
int smc_spike_alleles(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, const uint8_t* d_bq, int64_t n_pairs,
                      const smc_spike_variant* d_var, const smc_spike_variant* var_host, int32_t n_var, const uint64_t* d_idents,
                      int64_t n_bc, uint64_t seed, double mismatch_thr, const int32_t* d_nm, const int32_t* d_n_indel,
                      smc_dev_aln* d_aln_out, uint8_t* d_bq_out, uint32_t* d_stats, void* stream);
/* (ABI 11, additive: one entry more, the version number unchanged) --spikeIndels: listed insertions and deletions, and SNVs beside
 * them, planted in a copy of a run.  The run, d_idents, d_nm / d_n_indel, the seed and the draw (counter word 3 = (pos0 + 1) mod 2^32)
 * are smc_spike_alleles'; n_cig_words: the words of the CIGAR pool.  d_var[n_var]: strictly ascending by pos0, footprints disjoint.
 *   SMC_AF_SNV  ref / alt as smc_spike_variant has them, len 0: smc_spike_alleles' rule
 *   SMC_AF_INS  pos0 the anchor, ref = alt = the anchor's letter, the `len` inserted letters at d_ins[ins_off ..]; footprint [pos0, pos0 + 1]
 *   SMC_AF_DEL  pos0 the anchor, ref = alt = the anchor's letter, `len` deleted positions; footprint [pos0, pos0 + len + 1]
 * A record of a spiked barcode takes an insertion / a deletion when the whole footprint lies inside ONE M / = / X operation of its
 * ORIGINAL CIGAR and inside its l_seq bases, and l_seq (+ len, an insertion) and n_cig + 2 stay <= 65535 - counted over the variants
 * taken before it, in ascending position.  M(n) becomes M(a) I(len) M(n - a) / M(a) D(len) M(n - a - len), the operation's type kept;
 * inserted letters take the anchor's quality; l_seq and qalen move by len, NM and n_indel grow by len; pos, end, left_sp, flags, mapq
 * and the ids stay.  Such a record is RELOCATED: its pairs and CIGAR words are written behind the run's own, the relocated records in
 * alignment order, densely; its SNVs (resolved on the original CIGAR) are written on the way.  Every other record takes the SNV rule
 * in place.  Outputs, all DEVICE memory:
 *   d_aln_out[n_aln]                 the records (seq_off, cig_off, n_cig, l_seq, qalen of a relocated one new; SMC_DA_MMOK of every
 *                                    record from NM', n_indel' and the new l_seq, as smc_bam_alignments computes it)
 *   d_bq_out (2 * cap_pairs bytes)   the run's 2 * n_pairs bytes, then the relocated records' pairs.  For smc_build_planes allocate
 *                                    128 bytes more, as for any pair pool
 *   d_cig_out (cap_cig words)        the run's n_cig_words, then the relocated records' operations
 *   d_nm_out / d_n_indel_out[n_aln]  NM' and n_indel'
 *   d_stats[n_var][2]                uint32: records rewritten at v, records whose NM grew at v (every one, for an insertion / a deletion)
 *   d_totals[3]                      uint64: pairs and CIGAR words the copy needs, the run's own included; [2] bit 1 = more than
 *                                    cap_pairs / cap_cig (both below 2^32).  Nothing beyond the capacities is written: a record that
 *                                    does not fit is stored as the run has it, and the copy is not to be used
 * An upper bound of the capacities from the host's arrays: n_pairs + over the alignments that span a listed insertion / deletion
 * l_seq + the `len` of the insertions they span, n_cig_words + over the same alignments n_cig + 2 per such variant.
 * Three launches behind the copies, enqueued on `stream`; nothing waits for the host, no workgroup waits for another; the offsets are
 * a sum in a fixed order: two calls give the same bytes.  SMC_E_INPUT, nothing launched and nothing copied: what smc_spike_alleles
 * refuses, a kind beyond SMC_AF_DEL, a len outside 1 .. SMC_AF_MAX_INS (0 for an SNV), ref != alt for an insertion / a deletion,
 * inserted letters beyond the n_ins bytes of d_ins, overlapping footprints, capacities below the run's own or of 2^32 or more.
 * PHASE SETS (--spikeIndelPhase).  `lead` is smc_spike_variant's: records back, in this position-sorted array, to the leader of the
 * record's set - the member with the smallest position, an SNV's or an anchor's.  Record k, of whatever kind, is drawn with counter
 * word 3 = (var[k - lead].pos0 + 1) mod 2^32 in place of its own position: a barcode is spiked at every member or at none, and every
 * member is then applied under its own rule above.  A record between two members that is no member (lead 0) draws on its own.  With
 * lead = 0 everywhere the call is bit for bit what it was (the field is the upper half of what was a 32-bit `len` <= 255).  Also
 * SMC_E_INPUT, nothing launched and nothing copied: var_host[k].lead > k, or a leader whose own `lead` is not 0
 * (smc_spike_indels_reps refuses the same; smc_spike_indel_touch makes no draw and does not read the field). */
typedef struct smc_spike_indel_variant {
    int32_t pos0;              /* 0-based reference position: of the SNV, of the anchor */
    uint8_t kind;              /* SMC_AF_SNV, SMC_AF_INS, SMC_AF_DEL */
    uint8_t ref, alt;          /* ASCII, out of A C G T; an insertion / a deletion: the anchor's letter in both */
    uint8_t pad;
    uint16_t len;              /* inserted letters / deleted positions (1 .. SMC_AF_MAX_INS); 0 for an SNV */
    uint16_t lead;             /* records back, in this array, to the leader of the variant's phase set; 0: its own leader */
    uint32_t ins_off;          /* where the inserted letters start in d_ins */
    uint64_t thr;              /* floor(t * 2^32), in [0, 2^32] */
} smc_spike_indel_variant;
int smc_spike_indels(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, int64_t n_cig_words, const uint8_t* d_bq,
                     int64_t n_pairs, const smc_spike_indel_variant* d_var, const smc_spike_indel_variant* var_host, int32_t n_var,
                     const uint8_t* d_ins, int64_t n_ins, const uint64_t* d_idents, int64_t n_bc, uint64_t seed, double mismatch_thr,
                     const int32_t* d_nm, const int32_t* d_n_indel, int64_t cap_pairs, int64_t cap_cig, smc_dev_aln* d_aln_out,
                     uint8_t* d_bq_out, uint32_t* d_cig_out, int32_t* d_nm_out, int32_t* d_n_indel_out, uint32_t* d_stats,
                     uint64_t* d_totals, void* stream);
/* (ABI 11, additive: two entries more, the version number unchanged) --spikeReps: R replicates of the --spikeAF spike-in, replicate
 * j with the seed s_j; the run, the variants and the rewrite rule are smc_spike_alleles'.
 *   smc_spike_alleles_reps   n_copies spiked copies of one run from one call.  `seeds` / `thr`: HOST memory, n_copies words each - copy
 *            c is drawn with seeds[c] and EVERY variant at the threshold thr[c] (in [0, 2^32]; the variants' own `thr` field is not
 *            read).  Copy c lies at d_aln_out + c * aln_stride (n_aln records), d_bq_out + c * bq_stride (2 * n_pairs bytes) and
 *            d_stats[c][n_var][2], and is byte for byte what smc_spike_alleles writes with seeds[c] and every thr = thr[c]; the
 *            bytes between the end of a copy and the next stride are not written, the run's own arrays are only read.  The strides
 *            are BYTES: aln_stride a multiple of 4 and at least n_aln * sizeof(smc_dev_aln), bq_stride a multiple of 16 and at least
 *            2 * n_pairs; d_bq and d_bq_out 16-byte aligned (the pool travels in 16-byte chunks: read once, stored to every copy,
 *            in a launch of its own; the rewrite - a lane per alignment, a row of the grid per copy - follows on the same stream).
 *   smc_spike_rep_counts     what every replicate achieves, with no spiked copy at all.  The covering barcodes of all n_var listed
 *            variants stand one behind the other (variant v's at [cov_off[v], cov_off[v + 1])): d_cov_ident their identities,
 *            d_cov_cnt[e][3] uint32 per barcode its pileup reads at the variant's position, those that show ALT before spiking
 *            and those whose allele key there is a single letter - what the rewrite can touch (smc_allele_carriers' counters on
 *            the run give the first two, its `alt` counter on a copy spiked at threshold 2^32 the third).  d_pos1[n_var]: counter
 *            word 3 of every variant's draw - the 1-based position of the LEADER of its phase set (its own without sets; the
 *            same holds for smc_spike_depth_counts).  d_seeds[n_reps] in device memory; `thr`: HOST memory,
 *            n_targets words in [0, 2^32].  With hit = u_v(b; seeds[j]) < thr[t], u_v smc_spike_alleles' draw:
 *            d_out[v][j][t][3] uint32 = (S: covering b with hit, READS: the sum of single[b] over them, V1: the b with
 *            2 * (hit ? single[b] : alt0[b]) > reads[b]).  One draw per (b, v, j) serves every target.  d_out is zeroed by the call.
 * Enqueued on `stream`; nothing waits.  SMC_E_INPUT, nothing launched and nothing copied: what smc_spike_alleles refuses (but for the
 * variants' thresholds), n_copies below 1 or above SMC_SPIKE_MAX_COPIES, a threshold above 2^32, a stride smaller than a copy,
 * n_copies * n_var * 2 (or n_var * n_reps * n_targets * 3) of 2^32 - 256 words or more, n_targets above
 * SMC_SPIKE_REP_MAX_TARGETS, n_reps above SMC_AF_REP_MAX_REPS, offsets that decrease. */
#define SMC_SPIKE_MAX_COPIES 64        /* (the copies' seeds and thresholds travel in the kernel's argument block) */
#define SMC_SPIKE_REP_MAX_TARGETS 32   /* (= spike targets of one run) */
int smc_spike_alleles_reps(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, const uint8_t* d_bq, int64_t n_pairs,
                           const smc_spike_variant* d_var, const smc_spike_variant* var_host, int32_t n_var, const uint64_t* d_idents,
                           int64_t n_bc, const uint64_t* seeds, const uint64_t* thr, int32_t n_copies, double mismatch_thr,
                           const int32_t* d_nm, const int32_t* d_n_indel, uint8_t* d_aln_out, int64_t aln_stride, uint8_t* d_bq_out,
                           int64_t bq_stride, uint32_t* d_stats, void* stream);
int smc_spike_rep_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint32_t* d_cov_cnt, const uint32_t* d_cov_off,
                         const uint32_t* cov_off_host, const uint32_t* d_pos1, int32_t n_var, const uint64_t* d_seeds, int32_t n_reps,
                         const uint64_t* thr, int32_t n_targets, uint32_t* d_out, void* stream);
/* (ABI 11, additive: one entry more, the version number unchanged) --spikeDepth: the cells (target t, barcode fraction f) of the
 * --spikeAF spike-in.  Cell (t, f) of replicate j is the spike-in at t drawn with seeds[j], of which the barcodes stay that
 * smc_select_alignments' philox rule keeps at f with the same seed: keep = word 0 of Philox4x32-10(counter = (identity lo, identity
 * hi, 0x64734D54 "dsMT", 0), key = (seeds[j] lo, hi)) < depth_thr[f].  `depth_thr`: HOST memory, n_fracs words, floor(f * 2^32) each
 * and 2^32 at f = 1; the other arguments are smc_spike_rep_counts'.  With hit = u_v(b; seeds[j]) < thr[t] as there:
 *   d_out[v][j][t][f][5] uint32 = (N': the covering b with keep, V0': those with 2 * alt0[b] > reads[b], S': those with hit, READS':
 *   the sum of single[b] over the b with keep and hit, V1': the b with keep and 2 * (hit ? single[b] : alt0[b]) > reads[b]).
 * Two draws per (b, v, j) serve every cell; the depth draw is not made when no threshold is below 2^32, and at one fraction of 2^32
 * (S', READS', V1') are smc_spike_rep_counts' numbers.  d_out is zeroed by the call.
 * Enqueued on `stream`; nothing waits.  SMC_E_INPUT, nothing launched and nothing zeroed: what smc_spike_rep_counts refuses, a depth
 * threshold above 2^32, n_fracs below 1, n_targets * n_fracs above SMC_AF_DEPTH_MAX_CELLS, an output of 2^32 - 256 words or more. */
int smc_spike_depth_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint32_t* d_cov_cnt, const uint32_t* d_cov_off,
                           const uint32_t* cov_off_host, const uint32_t* d_pos1, int32_t n_var, const uint64_t* d_seeds, int32_t n_reps,
                           const uint64_t* thr, int32_t n_targets, const uint64_t* depth_thr, int32_t n_fracs, uint32_t* d_out, void* stream);
/* (ABI 11, additive: one entry more, the version number unchanged) --spikePhase: the JOINT numbers of phase sets - groups of listed
 * SNVs of one chromosome that share one draw (smc_spike_variant.lead), so that a barcode carries the whole haplotype or nothing of
 * it.  Per set g its M_g = set_m_host[g] members (1 .. SMC_SPIKE_PHASE_MAX_MEMBERS) and its JOINT barcodes, those that cover every
 * member: d_joint_ident holds the identities of all n_sets sets one behind the other, set g's at [joint_off[g], joint_off[g + 1])
 * (d_joint_off in device memory, `joint_off_host` the same on the host, which is what is checked).  d_joint_cnt: uint32, per set a
 * block of (joint barcodes of g) rows of 3 * M_g words that starts at word d_cnt_off[g] - row e of set g holds, member after member,
 * (reads, alt0, single) of that barcode at that member's position, as smc_spike_rep_counts takes them per variant.  d_set_m /
 * d_cnt_off[n_sets]: device copies of set_m_host and of the word offsets.  d_pos1[n_sets]: counter word 3 of the set's draw, the
 * leader's 1-based position.  d_seeds, `thr`, `depth_thr`: as smc_spike_depth_counts takes them.  With hit = u(b; seeds[j]) <
 * thr[t] and keep = the "dsMT" draw of b with seeds[j] < depth_thr[f] - ONE spike draw per (barcode, set, replicate), the depth draw
 * only when some depth threshold is below 2^32:
 *   d_out[g][j][t][f][4] uint32 = (N_ALL': the joint b with keep, V0_ALL': those that carry EVERY member before spiking - 2 *
 *   alt0 > reads at each -, S_ALL': those with keep and hit, V1_ALL': those with keep and 2 * (hit ? single : alt0) > reads at
 *   every member).  At M_g = 1 these are columns (N', V0', S', V1') of smc_spike_depth_counts.  d_out is zeroed by the call.
 * Enqueued on `stream`; nothing waits.  SMC_E_INPUT, nothing launched and nothing zeroed: a set with M_g outside 1 ..
 * SMC_SPIKE_PHASE_MAX_MEMBERS, offsets that decrease, n_targets * n_fracs above SMC_AF_DEPTH_MAX_CELLS, a threshold above 2^32 on
 * either axis, n_fracs below 1, n_reps above SMC_AF_REP_MAX_REPS, more than SMC_AF_MAX_VARIANTS sets, an output of 2^32 - 256
 * words or more. */
#define SMC_SPIKE_PHASE_MAX_MEMBERS 8
int smc_spike_phase_counts(smc_ctx* ctx, const uint64_t* d_joint_ident, const uint32_t* d_joint_cnt, const uint32_t* d_joint_off,
                           const uint32_t* joint_off_host, const uint32_t* d_set_m, const uint32_t* set_m_host, const uint32_t* d_cnt_off,
                           const uint32_t* d_pos1, int32_t n_sets, const uint64_t* d_seeds, int32_t n_reps, const uint64_t* thr,
                           int32_t n_targets, const uint64_t* depth_thr, int32_t n_fracs, uint32_t* d_out, void* stream);
/* (ABI 11, additive: three entries more, the version number unchanged) --spikeIndelReps / --spikeIndelDepth: replicates and barcode
 * depths of the --spikeIndels spike-in.
 *   smc_spike_indels_reps    n_copies copies (1 .. SMC_SPIKE_MAX_COPIES) of one run from one call.  `seeds` / `thr`: HOST memory, n_copies
 *            words each - copy c is drawn with seeds[c] and EVERY variant at thr[c] (in [0, 2^32]; the variants' own `thr` is not
 *            read).  Copy c is byte for byte what smc_spike_indels writes with seeds[c] and every thr = thr[c]: its records at
 *            d_aln_out + c * aln_stride, its pair pool at d_bq_out + c * bq_stride (up to its totals[0] pairs), its CIGAR pool at
 *            d_cig_out + c * cig_stride (up to its totals[1] words), d_nm_out[c][n_aln], d_n_indel_out[c][n_aln],
 *            d_stats[c][n_var][2] and d_totals[c][3].  cap_pairs / cap_cig hold for every copy; nothing beyond a copy's capacity
 *            is written, the bytes between a copy's end and the next stride are not written, the run's arrays are only read.  A
 *            copy that needs more sets its own totals[c][2] and leaves the records that do not fit as the run has them; the other
 *            copies are not affected.  The strides are BYTES: aln_stride a multiple of 4 and at least n_aln * sizeof(smc_dev_aln),
 *            bq_stride / cig_stride multiples of 16 and at least 2 * cap_pairs / 4 * cap_cig; d_bq, d_cig, d_bq_out and d_cig_out
 *            16-byte aligned (both pools travel in 16-byte chunks: read once, stored to every copy, before the scatter).  The
 *            three launches of smc_spike_indels with a row of the grid per copy, one scan workgroup per copy; nothing waits for
 *            the host.
 *   smc_spike_indel_touch    d_out[v][n_bc] uint32 (zeroed by the call): per listed insertion / deletion v and barcode of the run
 *            the records that take v when the barcode is spiked - smc_spike_indels' eligibility (the same device code), every
 *            variant taken as hit.  An SNV's row stays 0.  Whether a record takes v depends on no other variant's draw as long as
 *            the 16-bit limits of l_seq and n_cig cannot bind: the caller makes sure of that (n_cig + 2 k <= 65535 and l_seq + the
 *            inserted letters <= 65535 for a record that spans k listed indels).  A record that points beyond the pools, or has
 *            bc_gid >= n_bc, counts nowhere.  The variants' thresholds and inserted letters are not read.
 *   smc_spike_indel_counts   smc_spike_rep_counts (depth_thr NULL: d_out[v][j][t][3]) or smc_spike_depth_counts (d_out[v][j][t][f][5])
 *            from FOUR counters per covering barcode, d_cov_cnt[e][4] = (reads, alt0, alt1, touch): alt1 the reads that show ALT
 *            when the barcode is hit (smc_allele_carriers' `alt` on a copy spiked at threshold 2^32), touch the records the rewrite
 *            changes then (an SNV: alt1; an insertion / a deletion: smc_spike_indel_touch).  V1 takes 2 * (hit ? alt1 : alt0) >
 *            reads, READS sums touch.  With alt1 = touch = single the numbers are those of the two entries named.
 * Enqueued on `stream`; nothing waits.  SMC_E_INPUT, nothing launched and nothing copied: what smc_spike_indels (but for the variants'
 * thresholds) and smc_spike_alleles_reps / smc_spike_rep_counts / smc_spike_depth_counts refuse, each for the entry that combines
 * them; n_var * n_bc of 2^32 - 256 counters or more. */
int smc_spike_indels_reps(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, int64_t n_cig_words, const uint8_t* d_bq,
                          int64_t n_pairs, const smc_spike_indel_variant* d_var, const smc_spike_indel_variant* var_host, int32_t n_var,
                          const uint8_t* d_ins, int64_t n_ins, const uint64_t* d_idents, int64_t n_bc, const uint64_t* seeds, const uint64_t* thr,
                          int32_t n_copies, double mismatch_thr, const int32_t* d_nm, const int32_t* d_n_indel, int64_t cap_pairs,
                          int64_t cap_cig, uint8_t* d_aln_out, int64_t aln_stride, uint8_t* d_bq_out, int64_t bq_stride, uint8_t* d_cig_out,
                          int64_t cig_stride, int32_t* d_nm_out, int32_t* d_n_indel_out, uint32_t* d_stats, uint64_t* d_totals, void* stream);
int smc_spike_indel_touch(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, int64_t n_cig_words, int64_t n_pairs,
                          const smc_spike_indel_variant* d_var, const smc_spike_indel_variant* var_host, int32_t n_var, int64_t n_bc,
                          uint32_t* d_out, void* stream);
int smc_spike_indel_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint32_t* d_cov_cnt, const uint32_t* d_cov_off,
                           const uint32_t* cov_off_host, const uint32_t* d_pos1, int32_t n_var, const uint64_t* d_seeds, int32_t n_reps,
                           const uint64_t* thr, int32_t n_targets, const uint64_t* depth_thr, int32_t n_fracs, uint32_t* d_out, void* stream);
/* (ABI 11, additive: one entry more, the version number unchanged) --spikeIndelPhase: the joint numbers of phase sets whose members
 * may be insertions and deletions.  smc_spike_phase_counts on rows of 4 * M_g words per joint barcode: per member (reads, alt0, alt1,
 * touch), the columns of smc_spike_indel_counts - d_joint_cnt holds, per set, a block of (joint barcodes of g) rows of 4 * M_g words
 * from word d_cnt_off[g].  V1_ALL' takes 2 * (hit ? alt1 : alt0) > reads at EVERY member; `touch` is not read (no READS' of a set).
 * Every other argument, d_out[g][j][t][f][4] and every refusal are smc_spike_phase_counts'; with alt1 = touch = single the numbers
 * are its numbers word for word, at M_g = 1 columns (N', V0', S', V1') of smc_spike_indel_counts. */
int smc_spike_indel_phase_counts(smc_ctx* ctx, const uint64_t* d_joint_ident, const uint32_t* d_joint_cnt, const uint32_t* d_joint_off,
                                 const uint32_t* joint_off_host, const uint32_t* d_set_m, const uint32_t* set_m_host, const uint32_t* d_cnt_off,
                                 const uint32_t* d_pos1, int32_t n_sets, const uint64_t* d_seeds, int32_t n_reps, const uint64_t* thr,
                                 int32_t n_targets, const uint64_t* depth_thr, int32_t n_fracs, uint32_t* d_out, void* stream);
/* (ABI 11, additive: two entries more, the version number unchanged) --spikeRpb: the cells (spike target t, reads-per-barcode target
 * r) of the --spikeAF spike-in.  Cell (t, r) of replicate j is the spike-in at t drawn with seeds[j], of which the records stay that
 * smc_read_groups_masks keeps with the same seed at r: a record whose read name is the first of its barcode, file-wide, or whose
 * read draw - word 0 of Philox4x32-10(counter = (name identity lo, name identity hi, 0x64735250 "dsRP", 0), key = (seeds[j] lo, hi)) -
 * is below read_thr[r] = floor(probKeep_r * 2^32).  Thinning reads changes a barcode's counters per r and per seed, so they are
 * counted per record:
 *   smc_spike_read_bits   for the run as smc_spike_indel_touch takes it (d_bq: its pair pool of n_pairs pairs; d_loc[n_loci], start0:
 *            as smc_allele_carriers takes them) and its listed SNVs d_var[n_var] (smc_allele_carriers' records, kind SMC_AF_SNV, `letter`
 *            the ALT): d_out[v][n_aln] uint8, one byte per alignment - bit 0: the record is in the window [w0, w1) of v's locus and
 *            covers its position p (pos <= p < end); bit 1: it shows ALT there as it is (smc_allele_carriers' rule); bit 2: its allele
 *            key there is a single letter (a base, not inside a deletion, no insertion or deletion starting behind it, inside l_seq
 *            and the pools) - exactly the records smc_spike_alleles rewrites when the barcode is spiked.  Every byte of d_out is
 *            written (0 for a record outside the window); plain stores, no atomics.  Summed per barcode the three bits are
 *            smc_spike_rep_counts' (reads, alt0, single).
 *   smc_spike_rpb_counts  the covering barcodes of all n_var variants one behind the other as smc_spike_rep_counts takes them
 *            (d_cov_ident, d_cov_off / cov_off_host); per covering barcode e its covering records [rec_off[e], rec_off[e + 1]) of
 *            d_rec_name (the read-name identity: smc_bam_pair_idents of the record's pair_gid) and d_rec_flag (uint8: bit 0 = the
 *            name is its barcode's first, file-wide; bits 1 and 2 = bits 1 and 2 of smc_spike_read_bits) - d_rec_off: the
 *            cov_off_host[n_var] + 1 offsets in device memory, rec_off_host the same on the host; n_rec records.  d_pos1, d_seeds,
 *            `thr`: smc_spike_rep_counts'; `read_thr`: HOST memory, n_read_thr words in [0, 2^32].  A record is KEPT at r when flag
 *            bit 0 is set or its read draw is below read_thr[r]; with (reads_r, alt_r, single_r) of a barcode over its kept records,
 *            hit = u_v(b; seeds[j]) < thr[t], there = reads_r > 0:
 *            d_out[v][j][t][r][5] uint32 = (N': the b with there, V0': those with 2 * alt_r > reads_r, S': those with hit, READS':
 *            the sum of single_r over the b with there and hit, V1': the b with there and 2 * (hit ? single_r : alt_r) > reads_r).
 *            One spike draw per (b, v, j) and one read draw per (record, j) serve every cell; at one read threshold of 2^32 the
 *            numbers are smc_spike_depth_counts' at one depth threshold of 2^32.  d_out is zeroed by the call; integer atomics
 *            only: two calls give the same words.
 * Enqueued on `stream`; nothing waits.  SMC_E_INPUT, nothing launched and nothing zeroed: more than SMC_AF_MAX_VARIANTS variants, a
 * locus index beyond n_loci, a kind that is not SMC_AF_SNV (smc_spike_read_bits); what smc_spike_depth_counts refuses, a read
 * threshold above 2^32, n_read_thr below 1, n_targets * n_read_thr above SMC_AF_DEPTH_MAX_CELLS, record offsets that decrease or end
 * beyond n_rec (smc_spike_rpb_counts). */
int smc_spike_read_bits(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, int64_t n_cig_words, const uint8_t* d_bq,
                        int64_t n_pairs, const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0, const smc_af_variant* d_var,
                        const smc_af_variant* var_host, int32_t n_var, uint8_t* d_out, void* stream);
int smc_spike_rpb_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint32_t* d_cov_off, const uint32_t* cov_off_host,
                         const uint32_t* d_rec_off, const uint32_t* rec_off_host, const uint64_t* d_rec_name, const uint8_t* d_rec_flag,
                         int64_t n_rec, const uint32_t* d_pos1, int32_t n_var, const uint64_t* d_seeds, int32_t n_reps, const uint64_t* thr,
                         int32_t n_targets, const uint64_t* read_thr, int32_t n_read_thr, uint32_t* d_out, void* stream);
/* (ABI 11, additive: two entries more, the version number unchanged) --spikeGrid: the cells (spike target t, barcode fraction f,
 * reads-per-barcode target r) of the --spikeAF spike-in.  Cell (t, f, r) of replicate j is the spike-in at t drawn with seeds[j], of
 * which the records stay that smc_read_groups_masks_grid keeps with the same seed in cell (f, r): the barcode's draw (smc_select_
 * alignments' philox rule, domain "dsMT") is below bc_thr[f], and the record's name is its barcode's first, file-wide, or its read
 * draw (smc_spike_rpb_counts') is below the cell's read threshold.  probKeep of (f, r) is made from the barcodes kept at f, which move
 * with the seed, so every replicate has read thresholds of its own:
 *   smc_read_groups_counts_frac_seeds  smc_read_groups_counts_frac for n_seeds seeds (HOST memory, at most SMC_AF_REP_MAX_REPS) in one
 *            launch: host counts[j][f][4] uint64 = (barcodes, one, multi, multi_names) of the barcodes seeds[j] keeps at bc_thr[f] - the
 *            four counters probKeep is made from.  Null stream; the table must be finished.  Unlike _counts_frac, which uses the
 *            table's own scratch, every call allocates and frees a device buffer for the seeds and the counters (R reaches 1000) and
 *            copies both ways blocking: meant for one call per run, not for a loop.
 *   smc_spike_grid_counts  smc_spike_rpb_counts' arguments, with `bc_thr`: HOST memory, n_fracs words in [0, 2^32] (2^32 keeps every
 *            barcode), and the read thresholds d_rd_thr[n_reps][n_fracs][n_read_thr] uint64 in DEVICE memory, rd_thr_host the same
 *            words on the host (checked there; each in [0, 2^32]).  With (reads_q, alt_q, single_q) of a barcode over the records
 *            kept at the pair q = (f, r) - flag bit 0 set, or the read draw below d_rd_thr[j][f][r] -, hit as there and
 *            there = the barcode's draw < bc_thr[f] && reads_q > 0:
 *            d_out[v][j][t][f][r][5] uint32 = smc_spike_rpb_counts' five counters with that `there`.  One spike draw and one barcode
 *            draw per (b, v, j), one read draw per (record, j).  With n_fracs = 1, bc_thr[0] = 2^32 and the same thresholds in every
 *            replicate the words are smc_spike_rpb_counts'; with n_read_thr = 1 and a threshold of 2^32 they are smc_spike_depth_
 *            counts' on the per-barcode sums of the flag bits.  d_out is zeroed by the call; integer atomics only: two calls give
 *            the same words.  Enqueued on `stream`; nothing waits.
 * SMC_E_INPUT, nothing launched and nothing zeroed: what smc_spike_rpb_counts refuses, n_fracs or n_read_thr below 1, n_targets *
 * n_fracs * n_read_thr above SMC_AF_DEPTH_MAX_CELLS, a threshold above 2^32 on any axis. */
int smc_read_groups_counts_frac_seeds(smc_read_groups* g, const uint64_t* seeds, int32_t n_seeds, const uint64_t* bc_thr, int32_t n_frac,
                                      uint64_t* counts);
int smc_spike_grid_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint32_t* d_cov_off, const uint32_t* cov_off_host,
                          const uint32_t* d_rec_off, const uint32_t* rec_off_host, const uint64_t* d_rec_name, const uint8_t* d_rec_flag,
                          int64_t n_rec, const uint32_t* d_pos1, int32_t n_var, const uint64_t* d_seeds, int32_t n_reps, const uint64_t* thr,
                          int32_t n_targets, const uint64_t* bc_thr, int32_t n_fracs, const uint64_t* d_rd_thr, const uint64_t* rd_thr_host,
                          int32_t n_read_thr, uint32_t* d_out, void* stream);
/* (ABI 11, additive: two entries more, the version number unchanged) --spikeIndelRpb: the cells (spike target t, reads-per-barcode
 * target r) of the --spikeIndels spike-in.  The cell, the two draws and the kept records are smc_spike_rpb_counts'; what a record
 * contributes is FOUR bits, because for an insertion or a deletion the records that show the key when the barcode is hit (alt1) and the
 * records the rewrite changes then (touch) are two sets (smc_spike_indel_counts).
 *   smc_spike_indel_read_bits   the run, d_loc[n_loci] and start0 as smc_spike_read_bits takes them; d_var[n_var] / d_ins[n_ins]: the
 *            listed variants of the run as smc_spike_indel_touch takes them (SNVs, insertions, deletions; strictly ascending by pos0,
 *            footprints disjoint; `thr` and `lead` are not read), each a locus of the run: 0 <= pos0 - start0 < n_loci.
 *            d_out[v][n_aln] uint8, every byte written (0 for a record outside the window of v's locus):
 *              bit 0  the record is in the window and covers the position - an indel's anchor: pos <= pos0 < end
 *              bit 1  alt0: it shows the variant's key there as it is (smc_allele_carriers' rule, INS / DEL keys included)
 *              bit 2  alt1: it shows the key when its barcode is spiked - an SNV: the single-letter bit of smc_spike_read_bits; an
 *                     insertion / a deletion: touched and the anchor's letter is `ref`, or not touched and bit 1
 *              bit 3  touch: the rewrite changes it when its barcode is spiked - an SNV: bit 2; an insertion / a deletion:
 *                     smc_spike_indels' eligibility (the same device code as smc_spike_indel_touch, the 16-bit limits included)
 *            A record whose CIGAR words or pairs lie beyond the pools covers and shows nothing; bc_gid is not read.  Summed per
 *            barcode the four bits are smc_spike_indel_counts' (reads, alt0, alt1, touch).  Plain stores, no atomics.
 *   smc_spike_indel_rpb_counts  smc_spike_rpb_counts' arguments; d_rec_flag: bit 0 = first name, bits 1 / 2 / 3 = bits 1 / 2 / 3 above.
 *            With (reads_r, alt0_r, alt1_r, touch_r) of a barcode over its kept records, hit and there as in smc_spike_rpb_counts:
 *            d_out[v][j][t][r][5] uint32 = (N': the b with there, V0': those with 2 * alt0_r > reads_r, S': those with hit, READS':
 *            the sum of touch_r over the b with there and hit, V1': the b with there and 2 * (hit ? alt1_r : alt0_r) > reads_r).
 *            With bit 3 = bit 2 in every flag the words are smc_spike_rpb_counts'; at one read threshold of 2^32 they are
 *            smc_spike_indel_counts' at one depth threshold of 2^32.  The same kernel body as smc_spike_rpb_counts; integer atomics
 *            only: two calls give the same words.  d_pos1: the variant's own 1-based position (no phase sets under this axis).
 * Enqueued on `stream`; nothing waits.  SMC_E_INPUT, nothing launched and nothing zeroed: what smc_spike_indel_touch refuses (a kind
 * beyond SMC_AF_DEL, positions not strictly ascending, letters, lengths, overlapping footprints), inserted letters beyond d_ins, a
 * position that is no locus of the run (smc_spike_indel_read_bits); what smc_spike_rpb_counts refuses (smc_spike_indel_rpb_counts). */
int smc_spike_indel_read_bits(smc_ctx* ctx, const smc_dev_aln* d_aln, int64_t n_aln, const uint32_t* d_cig, int64_t n_cig_words,
                              const uint8_t* d_bq, int64_t n_pairs, const smc_dev_locus* d_loc, int64_t n_loci, int32_t start0,
                              const smc_spike_indel_variant* d_var, const smc_spike_indel_variant* var_host, int32_t n_var,
                              const uint8_t* d_ins, int64_t n_ins, uint8_t* d_out, void* stream);
int smc_spike_indel_rpb_counts(smc_ctx* ctx, const uint64_t* d_cov_ident, const uint32_t* d_cov_off, const uint32_t* cov_off_host,
                               const uint32_t* d_rec_off, const uint32_t* rec_off_host, const uint64_t* d_rec_name, const uint8_t* d_rec_flag,
                               int64_t n_rec, const uint32_t* d_pos1, int32_t n_var, const uint64_t* d_seeds, int32_t n_reps,
                               const uint64_t* thr, int32_t n_targets, const uint64_t* read_thr, int32_t n_read_thr, uint32_t* d_out,
                               void* stream);
/* (ABI 11, additive: one entry more, the version number unchanged) --spikePhaseRpb: the JOINT numbers of phase sets in the cells
 * (spike target t, reads-per-barcode target r).  Thinning reads can take a barcode out of one member's pileup, or flip its majority
 * at one member only, so the joint numbers are counted per record.  Per set g its M_g = set_m_host[g] members (1 ..
 * SMC_SPIKE_PHASE_MAX_MEMBERS; d_set_m the device copy) and its joint barcodes - the identities that cover every member in the
 * unthinned run, ascending, as smc_spike_phase_counts takes them (d_joint_ident, d_joint_off / joint_off_host): a barcode that is
 * not joint unthinned cannot become joint.  Per (joint barcode e of g, member m) ONE segment of covering records, segment
 * seg_base[g] + (e - joint_off[g]) * M_g + m: its records are [rec_off[s], rec_off[s + 1]) of d_rec_name / d_rec_flag as
 * smc_spike_indel_rpb_counts takes them (bit 0 = first name, bit 1 = alt0, bit 2 = alt1; bit 3 is not read: a set has no READS').
 * d_seg_base / seg_base_host[n_sets]: the running sums of M_g * (joint barcodes of g), from 0 - the segments lie set after set;
 * d_rec_off / rec_off_host: the n_seg + 1 offsets, n_seg the sum over all sets; n_rec records.  A record that spans several
 * members appears in each of their segments.  d_pos1[n_sets]: the leader's 1-based position, counter word 3 of the set's draw.
 * d_seeds, `thr`, `read_thr`: as smc_spike_rpb_counts takes them.  An SNV-only list passes smc_spike_read_bits' bytes, whose bit 2
 * (single) is an SNV's alt1.  With hit = u(b; seeds[j]) < thr[t] - ONE spike draw per (barcode, set, replicate) -, a record KEPT
 * at r when flag bit 0 is set or its read draw with seeds[j] is below read_thr[r], and (reads, alt0, alt1) of a barcode at member m
 * over the kept records of its segment:
 *   d_out[g][j][t][r][4] uint32 = (N_ALL': the joint b with reads > 0 at EVERY member, V0_ALL': those of N_ALL' with 2 * alt0 >
 *   reads at every member, S_ALL': those of N_ALL' with hit, V1_ALL': those of N_ALL' with 2 * (hit ? alt1 : alt0) > reads at every
 *   member).  At M_g = 1 these are columns (N', V0', S', V1') of smc_spike_indel_rpb_counts; at one read threshold of 2^32 they are
 *   smc_spike_indel_phase_counts' at one depth threshold of 2^32.  d_out is zeroed by the call; integer atomics only: two calls
 *   give the same words.
 * Enqueued on `stream`; nothing waits.  SMC_E_INPUT, nothing launched and nothing zeroed: a set with M_g outside 1 ..
 * SMC_SPIKE_PHASE_MAX_MEMBERS, joint or record offsets that decrease, record offsets that end beyond n_rec, segment bases that
 * are not the running sums, a threshold above 2^32 on either axis, n_read_thr below 1, n_targets * n_read_thr above
 * SMC_AF_DEPTH_MAX_CELLS, n_reps above SMC_AF_REP_MAX_REPS, more than SMC_AF_MAX_VARIANTS sets, an output of 2^32 - 256 words or
 * more. */
int smc_spike_phase_rpb_counts(smc_ctx* ctx, const uint64_t* d_joint_ident, const uint32_t* d_joint_off, const uint32_t* joint_off_host,
                               const uint32_t* d_set_m, const uint32_t* set_m_host, const uint32_t* d_seg_base, const uint32_t* seg_base_host,
                               const uint32_t* d_rec_off, const uint32_t* rec_off_host, const uint64_t* d_rec_name, const uint8_t* d_rec_flag,
                               int64_t n_rec, const uint32_t* d_pos1, int32_t n_sets, const uint64_t* d_seeds, int32_t n_reps,
                               const uint64_t* thr, int32_t n_targets, const uint64_t* read_thr, int32_t n_read_thr, uint32_t* d_out,
                               void* stream);
/* (ABI 11, additive: one entry more, the version number unchanged) --spikeScanMnvRpb: smc_spike_phase_rpb_counts' words without a
 * record CSR made on the host - for a scan, where every locus of the panel is a set.  The segments of a (joint barcode, member) come
 * from what is in HBM already: the run in BARCODE-MAJOR order, made once per decoded run, and smc_spike_read_bits' bytes.
 * Per run, n_aln entries each, stable by bc_gid (file order inside a barcode): d_bm_aln uint32 the alignment's index in the run,
 * d_bm_name uint64 the read-name identity of its pair_gid, d_bm_first uint8 1 when that name is its barcode's first, file-wide;
 * d_bc_start / bc_start_host[n_bc + 1]: where each barcode's records begin (ascending, ending at n_aln); d_idents[n_bc]: the
 * barcode identities smc_spike_alleles takes.
 * Per call: d_bits[n_var][n_aln]: smc_spike_read_bits' output as it is (bit 0 covers, bit 1 alt0, bit 2 single = an SNV's alt1; bit
 * 3 is not read).  The rows: d_row_off / row_off_host[n_rows + 1] over d_row_var / row_var_host - indices of bit rows, a row's
 * members in order, 1 .. SMC_SPIKE_PHASE_MAX_MEMBERS of them (a row of one member is a listed variant).  The joint barcodes of every
 * row: d_joint_off / joint_off_host[n_rows + 1] over d_joint_gid, run-wide barcode ids in any order (the host ANDs
 * smc_allele_carriers' cover rows of the members).  d_pos1[n_rows], d_seeds, `thr`, `read_thr`: smc_spike_phase_rpb_counts'.
 * A lane of row g takes joint barcode b and walks records [bc_start[b], bc_start[b + 1]) once per member m; the record of alignment
 * i is member m's when d_bits[row_var[m] * n_aln + i] has bit 0.  A d_bm_aln that is not below n_aln, and a joint id that is not
 * below n_bc, read nothing.  d_out[row][j][t][r][4] uint32 = (N_ALL', V0_ALL', S_ALL', V1_ALL') under smc_spike_phase_rpb_counts'
 * definitions - one spike draw per (barcode, row, replicate) with the row's pos1, a record kept at r when its first-name flag is set
 * or its read draw is below read_thr[r], (reads, alt0, alt1) per member over the kept records, the members ANDed - and by the same
 * kernel body.  d_out is zeroed by the call; integer atomics only: two calls give the same words.
 * Enqueued on `stream`; nothing waits.  SMC_E_INPUT, nothing launched and nothing zeroed, all on the host copies: row or joint
 * offsets that decrease, a row with members outside 1 .. SMC_SPIKE_PHASE_MAX_MEMBERS, a row_var not below n_var, a bc_start that
 * decreases or does not end at n_aln, more than SMC_AF_MAX_VARIANTS rows, a threshold above 2^32 on either axis, n_read_thr below 1,
 * n_targets * n_read_thr above SMC_AF_DEPTH_MAX_CELLS, n_reps above SMC_AF_REP_MAX_REPS, an output of 2^32 - 256 words or more. */
int smc_scan_phase_rpb_counts(smc_ctx* ctx, const uint32_t* d_bm_aln, const uint64_t* d_bm_name, const uint8_t* d_bm_first, int64_t n_aln,
                              const uint32_t* d_bc_start, const uint32_t* bc_start_host, const uint64_t* d_idents, int64_t n_bc,
                              const uint8_t* d_bits, int32_t n_var, const uint32_t* d_row_off, const uint32_t* row_off_host,
                              const uint32_t* d_row_var, const uint32_t* row_var_host, const uint32_t* d_joint_off,
                              const uint32_t* joint_off_host, const uint32_t* d_joint_gid, const uint32_t* d_pos1, int32_t n_rows,
                              const uint64_t* d_seeds, int32_t n_reps, const uint64_t* thr, int32_t n_targets, const uint64_t* read_thr,
                              int32_t n_read_thr, uint32_t* d_out, void* stream);

/* (ABI 11, additive: one entry more, the version number unchanged) --spikeScan: one verdict per (copy, listed locus) of a called
 * batch whose rows stay in HBM.  d_rows: n_copies x n_loci rows as a plan wrote them, copy c's locus l at c * n_loci + l.  d_listed /
 * listed_host[n_listed]: the loci a pass planted an SNV at - `offset` the locus within a copy (below n_loci), `alt` the fixed allele
 * id of the planted letter (A, T, G, C = 0 .. 3).  `thr`: the truncated-PI threshold of the .cut files (writers.pi_threshold).
 *   d_out[c * n_listed + g] = { pi: cand[0].pi unrounded, vmt: cand[0].vmt, mt_verdict: the verdict in bits 30 - 31 above
 *   min(used_mt, SMC_SCAN_MT_MASK) }.  With lo = thr - 0.005 - 1e-6 and hi = thr - 0.005 + 1e-6 in double:
 *     SMC_SCAN_CALLED  status 0, not bi-allelic, cand[0].allele == alt and cand[0].pi > hi
 *     SMC_SCAN_NOT     status 0, not bi-allelic, and cand[0].allele != alt or cand[0].pi < lo
 *     SMC_SCAN_HOST    the rest: a bi-allelic row, a status that is not 0, a PI in [lo, hi] or NaN - the host prints and cuts the row
 *   d_host_list[0 .. *d_n_host): the indices c * n_listed + g of the SMC_SCAN_HOST records, each once, in no fixed order (room for
 *   n_copies * n_listed words); *d_n_host is zeroed by the call.  Nothing else is written.
 * Enqueued on `stream`; nothing waits.  SMC_E_INPUT, nothing launched: an offset that is not below n_loci, an alt above 3, n_copies
 * above 65535, n_copies * n_listed or n_copies * n_loci of 2^31 or more, a `thr` that is not finite. */
typedef struct smc_scan_locus {
    uint32_t offset;
    uint32_t alt;
} smc_scan_locus;
typedef struct smc_scan_verdict {      /* 16 bytes */
    double pi;
    int32_t vmt;
    uint32_t mt_verdict;
} smc_scan_verdict;
#define SMC_SCAN_NOT 0u
#define SMC_SCAN_CALLED 1u
#define SMC_SCAN_HOST 2u
#define SMC_SCAN_MT_MASK 0x3FFFFFFFu
int smc_scan_detect(smc_ctx* ctx, const smc_row* d_rows, int32_t n_copies, int64_t n_loci, const smc_scan_locus* d_listed,
                    const smc_scan_locus* listed_host, int32_t n_listed, double thr, smc_scan_verdict* d_out, uint32_t* d_host_list,
                    uint32_t* d_n_host, void* stream);
/* (ABI 11, additive: one entry more, the version number unchanged) --spikeScanMnv: smc_scan_detect when the listed records are the
 * members of phase sets, and an MNV is called when every member is.  d_rows .. n_listed, thr: smc_scan_detect's.
 *   d_set_off / set_off_host[n_sets + 1]  the sets tile the listed records in order: set s holds the records set_off[s] ..
 *                              set_off[s + 1] - 1; set_off[0] = 0, set_off[n_sets] = n_listed, every size in 1 ..
 *                              SMC_SPIKE_PHASE_MAX_MEMBERS.
 *   d_out[c * n_listed + g]    byte for byte the record smc_scan_detect writes.
 *   d_joint[c * n_sets + s]    one word: bits 31..30 the joint verdict - SMC_SCAN_NOT when any member is NOT, else SMC_SCAN_HOST when any
 *                              member is HOST, else SMC_SCAN_CALLED; bit m of byte 0 / 1 / 2: member m of the set is CALLED / HOST / NOT.
 *   d_host_list[0 .. *d_n_host)  the indices c * n_listed + g of the HOST member records of the sets whose JOINT verdict is HOST - a HOST
 *                              member beside a NOT member decides nothing -, each once, in no fixed order (room for n_copies *
 *                              n_listed words); *d_n_host is zeroed by the call.  Nothing else is written.
 * Enqueued on `stream`, one launch; nothing waits.  SMC_E_INPUT, nothing launched: what smc_scan_detect refuses; offsets that do not
 * tile the records; a set of 0 members or of more than SMC_SPIKE_PHASE_MAX_MEMBERS; n_copies * n_sets of 2^31 or more. */
int smc_scan_detect_sets(smc_ctx* ctx, const smc_row* d_rows, int32_t n_copies, int64_t n_loci, const smc_scan_locus* d_listed,
                         const smc_scan_locus* listed_host, int32_t n_listed, const uint32_t* d_set_off, const uint32_t* set_off_host,
                         int32_t n_sets, double thr, smc_scan_verdict* d_out, uint32_t* d_joint, uint32_t* d_host_list, uint32_t* d_n_host,
                         void* stream);
/* (ABI 11, additive: one entry more, the version number unchanged) --spikeScanIndel: smc_scan_detect for lists whose members are
 * allele KEYS.  An insertion's or a deletion's allele id is numbered per locus and per build (6 and up, in the order the builder met
 * the keys), so the id to compare cand[0].allele with is resolved per copy from that build's extras list.
 *   d_rows, n_copies, n_loci   as smc_scan_detect takes them.
 *   d_var / var_host[n_listed] the listed variants as smc_allele_carriers takes them, `locus` ascending (equal loci may follow one
 *                              another); d_ins[n_ins]: the pool of inserted letters.
 *   d_aln, d_cig, d_bq         the copies' records, CIGAR words and (letter, quality) pairs: copy c's array at base + c * its BYTE
 *                              stride, as smc_spike_indels_reps lays them out; a stride of 0: every copy shares the array.  n_aln
 *                              records per copy; cap_pairs: the pairs of a copy's pool that may be read.  (The CIGAR words are not
 *                              read: an extras entry holds the query position and the indel the builder's walk resolved.)
 *   d_x, x_stride              the builds' extras lists, copy c's at d_x + c * x_stride WORDS: entries of five words (locus, allele id,
 *                              alignment, query position, indel) as smc_build_planes leaves them; d_xcount[c * xcount_stride]: copy
 *                              c's number of entries, clipped to xcap in the kernel.
 *   d_alt_id[c * n_listed + g] out: an SNV's fixed id (A, T, G, C = 0 .. 3); for an insertion / a deletion the allele id of the one
 *                              entry of copy c at that locus whose alignment shows the key by smc_allele_carriers' rule on the copy's
 *                              own record - the anchor letter the variant's; a deletion: indel == -len; an insertion: the inserted
 *                              letters, clamped at the read's end, the pool's -; SMC_SCAN_ID_NONE when no entry does (and for
 *                              SMC_AF_NONE); SMC_SCAN_ID_HOST when two entries do, or when an entry of the locus names a record
 *                              that cannot be read (an alignment beyond n_aln, a query position beyond l_seq, pairs beyond cap_pairs).
 *   d_out, d_host_list, d_n_host  exactly smc_scan_detect's, by its rule with cand[0].allele == d_alt_id[..] and the same lo / hi:
 *                              SMC_SCAN_ID_NONE gives SMC_SCAN_NOT on a row with status 0 that is not bi-allelic, SMC_SCAN_ID_HOST
 *                              gives SMC_SCAN_HOST.
 * Enqueued on `stream`; nothing waits.  SMC_E_INPUT, nothing launched: what smc_scan_detect refuses; a `locus` that is not below
 * n_loci or stands behind a larger one; a kind beyond SMC_AF_NONE; an SNV whose letter is not A, C, G or T; an insertion / a deletion
 * with a len of 0 or above SMC_AF_MAX_INS; inserted letters beyond the pool; a byte stride that does not keep its array aligned (a
 * multiple of 4 for records and CIGAR words, of 2 for pairs) or is negative. */
#define SMC_SCAN_ID_NONE 0xFFFFFFFFu
#define SMC_SCAN_ID_HOST 0xFFFFFFFEu
int smc_scan_detect_keys(smc_ctx* ctx, const smc_row* d_rows, int32_t n_copies, int64_t n_loci, const smc_af_variant* d_var,
                         const smc_af_variant* var_host, int32_t n_listed, const uint8_t* d_ins, int64_t n_ins, const smc_dev_aln* d_aln,
                         int64_t aln_stride, const uint32_t* d_cig, int64_t cig_stride, const uint8_t* d_bq, int64_t bq_stride, int64_t n_aln,
                         int64_t cap_pairs, const uint32_t* d_x, int64_t x_stride, const uint32_t* d_xcount, int64_t xcount_stride,
                         int64_t xcap, double thr, uint32_t* d_alt_id, smc_scan_verdict* d_out, uint32_t* d_host_list, uint32_t* d_n_host,
                         void* stream);
/* (ABI 11, additive: one entry more, the version number unchanged) --spikeScanFilter: the FILTER column of every listed locus's row
 * as a word of bits, per copy of a called batch whose rows stay in HBM - called right behind smc_scan_detect / smc_scan_detect_keys
 * on the same d_rows; the verdict records are neither read nor written.
 *   d_rows, n_copies, n_loci   as smc_scan_detect takes them.
 *   d_offsets / offsets_host[n_listed]  the listed loci within a copy (below n_loci).
 *   d_gate / gate_host[n_listed]        per listed variant SMC_F_HP and / or SMC_F_LOWC: what hpregion.is_hp_or_lowcomp says of the
 *                              PLANTED variant (chromosome, position, REF, ALT, genome) - they apply where cand[0].vmf_lt_099.
 *   d_always / always_host[n_listed]    the repeat names of the position from the run's BEDs (postfilter._apply_one's first-hit rule):
 *                              SMC_F_REPT, SMC_F_REPS, SMC_F_SL, SMC_F_OTHER_REPEAT, and SMC_F_LOWC for RepeatMasker's Low_complexity.
 *   d_out[c * n_listed + g]    from cand[0] of copy c's row at the locus alone:
 *     bits 0 - 9   flt_applied ? (flt & 0x3FF) | (vmf_lt_099 ? gate : 0) : 0        (rows.filter_string)
 *     bits 0 - 13  additionally `always` where pi > 4.995 + 1e-6: int(float(py2 round(PI, 2))) >= 5 outside the band
 *     bit 31       SMC_SCAN_FLT_HOST: the host has to print the row - a status that is not 0, a bi-allelic row, a pi that is NaN or
 *                  within 4.995 +- 1e-6, a flt_applied that is neither 0 nor 1.
 *   A word means the row's FILTER only where the detect call's verdict is SMC_SCAN_CALLED (cand[0] is the planted variant there, and
 *   it is never DEL).  Nothing but d_out is written.
 * Enqueued on `stream`; nothing waits; no launch for n_listed = 0 or n_copies = 0.  SMC_E_INPUT, nothing launched: a NULL array with
 * n_listed > 0, an offset that is not below n_loci, a gate word outside SMC_F_HP | SMC_F_LOWC, an always word outside SMC_F_LOWC and
 * bits 10 - 13, n_copies above 65535, n_copies * n_listed or n_copies * n_loci of 2^31 or more. */
#define SMC_F_REPT 0x0400u          /* the four names only postfilter adds: never in smc_cand.flt */
#define SMC_F_REPS 0x0800u
#define SMC_F_SL 0x1000u
#define SMC_F_OTHER_REPEAT 0x2000u
#define SMC_SCAN_FLT_DEVICE_MASK 0x3FFu
#define SMC_SCAN_FLT_NAMES_MASK 0x3FFFu
#define SMC_SCAN_FLT_HOST 0x80000000u
int smc_scan_filter(smc_ctx* ctx, const smc_row* d_rows, int32_t n_copies, int64_t n_loci, const uint32_t* d_offsets,
                    const uint32_t* offsets_host, const uint32_t* d_gate, const uint32_t* gate_host, const uint32_t* d_always,
                    const uint32_t* always_host, int32_t n_listed, uint32_t* d_out, void* stream);
/* (ABI 11, additive: one entry more, the version number unchanged) --spikeScanMnvFilter: smc_scan_filter when the listed loci are the
 * members of phase sets, and an MNV is PASS when every member's row is - called right behind smc_scan_detect_sets on the same d_rows.
 *   d_rows .. n_listed         smc_scan_filter's; d_set_off / set_off_host[n_sets + 1]: smc_scan_detect_sets'.
 *   d_members[c * n_listed + g]  word for word what smc_scan_filter writes to its d_out.
 *   d_joint_flt[c * n_sets + s]  one word per (copy, set):
 *     bits 0 - 13  the OR over the members of their name bits (SMC_SCAN_FLT_NAMES_MASK)
 *     bit 16 + m   member m's word has at least one name bit: member m is not PASS
 *     bit 31       SMC_SCAN_FLT_HOST: some member's word has it
 *   A word means the set's FILTER only where smc_scan_detect_sets' joint verdict is SMC_SCAN_CALLED.  Nothing else is written.
 * Enqueued on `stream`, one launch of a few thousand lanes (launch latency, not a hot loop); nothing waits; no launch for n_listed = 0
 * or n_copies = 0.  SMC_E_INPUT, nothing launched: what smc_scan_filter refuses; a NULL set_off_host (whatever n_listed is: it has
 * n_sets + 1 entries), a NULL d_set_off, d_members or d_joint_flt with n_listed > 0; offsets that do not tile the listed loci; a set of
 * 0 members or of more than SMC_SPIKE_PHASE_MAX_MEMBERS; n_copies * n_sets of 2^31 or more. */
#define SMC_SCAN_FLT_MEMBER_SHIFT 16
int smc_scan_filter_sets(smc_ctx* ctx, const smc_row* d_rows, int32_t n_copies, int64_t n_loci, const uint32_t* d_offsets,
                         const uint32_t* offsets_host, const uint32_t* d_gate, const uint32_t* gate_host, const uint32_t* d_always,
                         const uint32_t* always_host, int32_t n_listed, const uint32_t* d_set_off, const uint32_t* set_off_host,
                         int32_t n_sets, uint32_t* d_members, uint32_t* d_joint_flt, void* stream);
/* number of kernel launches one smc_plan_run issues, and bytes of device scratch it holds */
int smc_plan_info(const smc_plan* plan, int32_t* n_launches, int64_t* scratch_bytes);

/* Optional: bracket the dominant k_call_v2 launch (the bin holding most reads) of each
 * smc_plan_run with a HIP event pair on the run's stream, kept in a ring of `slots` pairs
 * (0 disables). smc_plan_kernel_ms synchronises on the recorded pairs and returns that launch's
 * mean duration over the last min(runs, slots) runs, with the loci and reads one launch covers. */
int smc_plan_set_timing(smc_plan* plan, int slots);
int smc_plan_kernel_ms(smc_plan* plan, float* avg_ms, int32_t* n_samples, int64_t* n_loci, int64_t* n_reads);

/* Run the hot path over the batch. meta/umi/frag/dist, umi_start and rows are DEVICE pointers
 * (planes n_slots x uint32 each, umi and dist may be NULL - the kernels do not read them; umi_start sum(n_umi + 1) x uint32; rows n_loci x smc_row). `stream` is a hipStream_t (NULL = default
 * stream). Asynchronous: returns after enqueueing. */
int smc_plan_run(smc_plan* plan, const smc_params* params, const uint32_t* meta,
                 const uint32_t* umi, const uint32_t* frag, const uint32_t* dist,
                 const uint32_t* umi_start, smc_row* rows, void* stream);
/* The same on read words (smc_read_word above; n_slots x uint32): the form the kernels read.  smc_plan_run is
 * smc_pack_words into a buffer the plan keeps + this call.  smc_locus.n_frag is taken as given (allFrag of the row): the
 * words carry the fragment boundaries, not their count. */
int smc_plan_run_words(smc_plan* plan, const smc_params* params, const uint32_t* words, const uint32_t* umi_start,
                       smc_row* rows, void* stream);
/* The same on 16-bit read words (smc_read_word16; n_slots x uint16, a locus's first word 8-byte aligned: read_off4 counts
 * quads of reads as before) - what smc_build_planes_w16 writes. */
int smc_plan_run_words16(smc_plan* plan, const smc_params* params, const uint16_t* words16, const uint32_t* umi_start,
                         smc_row* rows, void* stream);
/* meta + frag planes of the plan's batch -> read words (device pointers; asynchronous on `stream`) */
int smc_pack_words(smc_plan* plan, const uint32_t* meta, const uint32_t* frag, uint32_t* words, void* stream);

/* Convenience for callers without their own device buffers: host pointers in, host rows out
 * (synchronous; does H2D, smc_plan_run, D2H). */
int smc_call_batch_host(smc_ctx* ctx, const smc_params* params, const smc_locus* loci,
                        int64_t n_loci, const uint32_t* meta, const uint32_t* umi,
                        const uint32_t* frag, const uint32_t* dist, int64_t n_slots,
                        const uint32_t* umi_start, int64_t n_umi_start, smc_row* rows_out);

/* Pack n rows (DEVICE pointers) into wire rows on `stream` (asynchronous), for the gather to the writing rank; and the
 * inverse on the HOST (no GPU needed): the printed fields are restored exactly, everything else is zero (p-values NaN,
 * n_touched / max_allele / second_allele / touched_mask / tallies: not carried). */
int smc_wire_row_size(void);
int smc_pack_rows(smc_ctx* ctx, const smc_row* rows, int64_t n, smc_wire_row* wire, void* stream);
int smc_unpack_rows(const smc_wire_row* wire, int64_t n, smc_row* rows);

/* Build the planes of a run ON THE DEVICE from its alignments (the device half of the feature extraction; the host half is
 * smc_bam_alignments): per locus the covering alignments in file order, per read the CIGAR walk, allele, quality, flags,
 * end distances and read class (smCounter.py:316-366, :371-452), barcode / fragment ids by first appearance (:462-471),
 * the barcode-major order, umi_start and the descriptor - byte for byte what smc_bam_planes builds on the host.
 * Everything in `in` and every output is a DEVICE pointer.  Outputs: the read words (the run's slots start at slot_base) and /
 * or the four raw-field planes (any of the five may be NULL - not written then - as long as `words`, or `meta` and `frag`, is
 * there; the raw-field planes are for checks: with only `words` the walk stages and stores a quarter of the bytes), umi_start / u_gid / u_finc (sized slots + loci of the batch; locus l of the run uses
 * [umi_base + slot_off(l) + l, ... + n_umi(l)]; u_gid / u_finc - run-wide barcode id and first INCLUDED pileup index per
 * barcode - are filled only for loci with more barcodes than params->ds: what the host needs for the reference's
 * down-sampling, :496-498), loci[n_loci] (read_off4 / umi_off already batch-relative), and for every allele beyond the six
 * fixed ones five words in xlist (locus, allele id, alignment, query position, indel; smc_bam_allele_key turns them into the
 * key text).  counters[0] = entries appended to xlist, counters[1] = status bits (0 = fine; see csrc/k_build_planes.inc:
 * 1 depth mismatch (a locus's reads differ from loc[].n, or exceed in->max_depth / smc_build_max_depth()), 2 extras overflow, 4 base quality > 126, 8 more
 * than 64 alleles) - the caller falls back to smc_bam_planes for the run when it is not 0.  Asynchronous on `stream`. */
typedef struct smc_build_in {
    const smc_dev_aln* aln; const uint32_t* cig;
    const uint8_t* bq;   /* the bases and their qualities as ONE stream of (letter, quality) byte pairs: base i of the pool (smc_dev_aln.
                          * seq_off counts bases) has its ASCII letter at byte 2i and its quality at byte 2i + 1.  The walk reads the 64
                          * positions of an alignment under a tile as 128 consecutive bytes - one or two cache lines; as two separate
                          * pools it touched two to four (measured: 1.79 -> 1.41 ms on the 3000x shape).  2-byte aligned, and readable
                          * 128 bytes past the last pair */
    const smc_dev_locus* loc; const uint8_t* refseq;
    int32_t start0, n_loci, n_bc, n_pair;
    int32_t max_depth;   /* reads at the run's deepest locus (the caller counted them for loc[].n); checked against
                          * smc_build_max_depth() */
    int32_t n_aln;       /* entries of aln[] (every loc[].w1 must stay within them); < 0: not checked */
    const smc_dev_locus* loc_host; /* the same loc[] in HOST memory (the decoder fills it there): sizes the sort and the launch
                                    * grids without a round trip; NULL = the library copies loc[] back itself (synchronous) */
} smc_build_in;
int smc_build_max_depth(void);
/* Optional: bracket the walk that writes the planes (k_bp_tiles<true>, the dominant kernel of smc_build_planes) with a HIP event
 * pair on the run's stream, in a ring of `slots` pairs (0 disables); smc_build_kernel_ms synchronises on the recorded pairs and
 * returns that launch's mean duration over the last min(runs, slots) calls. */
int smc_build_set_timing(smc_ctx* ctx, int slots);
int smc_build_kernel_ms(smc_ctx* ctx, float* avg_ms, int32_t* n_samples);
/* Checks and measurements: the rows the walks of the context's LAST smc_build_planes / _w16 call took from each sorted list (a list
 * per tile of 64 loci; per segment of several tiles in a deep run built without per-tile lists), after that build has finished.
 * A tile's list is its window of the file, loc[first].w0 .. loc[last].w1, without the alignments that end at or before the tile's
 * first position where one workgroup sorts it (k_bp_sort_seg); every window row elsewhere.  -> *n_lists, and the first
 * min(cap, *n_lists) counts in live[]. */
int smc_build_live_rows(smc_ctx* ctx, uint32_t* live, int32_t cap, int32_t* n_lists);
int smc_build_planes(smc_ctx* ctx, const smc_params* params, const smc_build_in* in, uint32_t slot_base, uint32_t umi_base,
                     uint32_t* words, uint32_t* meta, uint32_t* umi, uint32_t* frag, uint32_t* dist, uint32_t* umi_start,
                     uint32_t* u_gid, uint32_t* u_finc, smc_locus* loci, uint32_t* xlist, uint32_t xcap, uint32_t* counters, void* stream);

/* The same run with the read words in 16 bits (smc_read_word16 above) and nothing else written but umi_start / u_gid / u_finc /
 * loci / xlist: the walk stores half the bytes (the 3000x panel shape: 1.18 -> 1.00 ms) and the locus kernels load half.
 * counters[1] has one more status bit, 32: the run has an allele id beyond 15 at some locus or a base quality beyond 63 - the
 * words are not to be used, the caller builds the run again with smc_build_planes.  params->min_bq must lie in 0 .. 63. */
int smc_build_planes_w16(smc_ctx* ctx, const smc_params* params, const smc_build_in* in, uint32_t slot_base, uint32_t umi_base,
                         uint16_t* words16, uint32_t* umi_start, uint32_t* u_gid, uint32_t* u_finc, smc_locus* loci,
                         uint32_t* xlist, uint32_t xcap, uint32_t* counters, void* stream);

/* Build only LISTED loci of a run, for several copies of it, in one call (--spikeScanBuild listed): for B copies and G listed loci
 * (run offsets `offsets[g]`, strictly ascending, HOST memory) what smc_build_planes / smc_build_planes_w16 write for those loci -
 * the read words, the umi_start / u_gid / u_finc stretch, the descriptor, the extras entries, the status bits: byte for byte - as a
 * dense batch of B x G loci, copy-major: locus g of copy c is batch locus c * G + g.
 * `d_copies` (DEVICE memory): per copy where its records, CIGAR pool, (letter, quality) pool and smc_dev_locus array lie and
 * its counts - the copies of smc_spike_alleles_reps / smc_spike_indels_reps and the selections of smc_select_alignments_copies /
 * _reads_copies all fit it.  `flags` & SMC_LISTED_SHARED_ORDER: the copies have the same spans, barcode ids and pair ids (spiked
 * copies of one run: spiking changes bases, CIGARs and NM only) - the barcode-major order of a locus is then made once, from copy
 * 0 (and a declined copy 0 declines them all).  `flags` & SMC_LISTED_DENSE_LOCUS: the locus field of an extras entry holds g, the
 * locus's place in a copy of the dense batch, not the run offset - what smc_scan_detect_keys needs when it is told that a copy has
 * n_listed rows and its listed variants' `locus` fields are 0 .. n_listed - 1.
 * `caps[g]` (HOST memory; a multiple of 4, below 2^24): the slots listed locus g gets in every copy - at least the 4-aligned depth
 * of the locus in any copy (align4 of loc[offsets[g]].n of the unselected, unspiked run: spiking changes no span, a selection
 * only drops records).  With S the sum of the capacities: the words of batch locus c * G + g start at slot slot_base + c * S +
 * (caps[0] + .. + caps[g - 1]), its umi_start / u_gid / u_finc entries at umi_base + c * (S + G) + (caps[0] + .. + caps[g - 1]) + g
 * (n_umi + 1 of them); loci[B * G] holds the batch-relative read_off4 / umi_off.  `word_bits` 16 or 32 (`words` is then uint16 or
 * uint32; 16: params->min_bq in 0 .. 63).  Copy c's extras entries go to xlist + 5 * xcap * c - five words as smc_build_planes'
 * with the locus field holding the RUN offset offsets[g] (or g: SMC_LISTED_DENSE_LOCUS), in the order of the listed loci and of the allele ids - and
 * counters[2 c] = their number, counters[2 c + 1] = the copy's status bits: smc_build_planes' (1 a locus's reads differ from its
 * copy's loc[].n or exceed caps[g], 2 more than xcap extras, 4 base quality > 126, 8 more than 64 alleles, 32 no room in 16-bit
 * words) and SMC_LISTED_UNFLAGGED: the copy has an alignment flagged neither READ1 nor READ2 - it is declined (such reads need
 * the whole builder's look-back rule) and nothing but its counters is written.  The raw-field planes are the whole builder's.
 * A listed locus may be as deep as smc_build_max_depth().  No atomic operation orders an output: two calls leave the same bytes.
 * Everything is checked before anything is enqueued; asynchronous on `stream`.  (ABI 11, additive.) */
#define SMC_LISTED_MAX_LOCI 64
#define SMC_LISTED_MAX_COPIES 1024
#define SMC_LISTED_UNFLAGGED 64u
#define SMC_LISTED_SHARED_ORDER 1
#define SMC_LISTED_DENSE_LOCUS 2
typedef struct smc_listed_copy {       /* 48 bytes */
    const smc_dev_aln* aln; const uint32_t* cig; const uint8_t* bq; const smc_dev_locus* loc;
    int32_t n_aln, n_bc, n_pair, reserved;
} smc_listed_copy;
int smc_build_listed(smc_ctx* ctx, const smc_params* params, const smc_listed_copy* d_copies, int32_t n_copies, int32_t flags,
                     int32_t start0, int32_t n_loci, const uint8_t* d_refseq, const uint32_t* offsets, const uint32_t* caps,
                     int32_t n_listed, int32_t word_bits, uint32_t slot_base, uint32_t umi_base, void* words, uint32_t* umi_start,
                     uint32_t* u_gid, uint32_t* u_finc, smc_locus* loci, uint32_t* xlist, uint32_t xcap, uint32_t* counters,
                     void* stream);

/* The context keeps the device blocks of destroyed plans for the next plan (at most 64 blocks / 8 GB; the oldest goes first).
 * smc_pool_trim waits for the plans' last runs and returns every pooled block to the runtime. */
int smc_pool_trim(smc_ctx* ctx);

/* Device memory for callers without a GPU runtime of their own (the Python command line uses these instead of importing
 * PyTorch: about a second of start-up): allocation, synchronous copies, device synchronisation. */
/* smc_mem_alloc is hipMalloc.  (For most of round 5 it backed blocks of 256 MB and more by HIP virtual memory over physical
 * handles of 64 MB: such a range can LOSE what is written to it on this ROCm - csrc/host_abi.inc, vmm_alloc; scripts/vmm_stress.py;
 * SMC_VMM_CHUNK_MB=<MB> in the environment brings it back for measurements.)  Pointers from it are freed with smc_mem_free only. */
int smc_mem_alloc(smc_ctx* ctx, int64_t bytes, void** out);
void smc_mem_free(smc_ctx* ctx, void* p);
/* For an array the plane builder's walk WRITES (the read words of a batch): which physical pages hold it moves that kernel by up to
 * 10 % (the same from launch to launch; no counter of translation, L2 or request counts tells a fast allocation from a slow one,
 * but a write-only kernel with the walk's pattern does: smc_mem_write_probe).  smc_mem_alloc_best makes up to `tries` allocations
 * (hipMalloc blocks, all held until the choice is made so that each gets other pages), times that pattern into each (~ 4 ms per candidate)
 * and keeps the fastest.  info (may be NULL): [0] the kept block's probe time in ms, [1] the slowest candidate's, [2] candidates
 * tried.  Freed with smc_mem_free. */
int smc_mem_alloc_best(smc_ctx* ctx, int64_t bytes, int tries, void** out, float* info);
/* (smc_mem_write_probe OVERWRITES [p, p + bytes) with its pattern: for blocks that hold nothing yet.) */
int smc_mem_write_probe(smc_ctx* ctx, void* p, int64_t bytes, float* ms);
/* page-locked host memory: copies to and from it run at the link's rate (pageable memory goes through a staging copy) */
int smc_mem_alloc_host(smc_ctx* ctx, int64_t bytes, void** out);
void smc_mem_free_host(smc_ctx* ctx, void* p);
int smc_mem_h2d(smc_ctx* ctx, void* dst_device, const void* src_host, int64_t bytes);
int smc_mem_d2h(smc_ctx* ctx, void* dst_host, const void* src_device, int64_t bytes);
int smc_device_sync(smc_ctx* ctx);

/* HIP-event timing helpers so a host language without HIP bindings can time the stream the
 * kernels run on. */
int smc_event_create(void** ev);
int smc_event_record(void* ev, void* stream);
int smc_event_elapsed_ms(void* start, void* stop, float* ms); /* synchronises on `stop` */
void smc_event_destroy(void* ev);

#ifdef __cplusplus
}
#endif
#endif /* SMCOUNTER_HIP_H */
