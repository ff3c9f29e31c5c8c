// Included by smcounter_hip.hip (after k_spike_rpb.inc; reads smc_row as k_call_v2 / k_filter_loci leave it).
// ------------------------------------------------------------------------------------------
// --spikeScan: was the planted SNV called?  One verdict per (copy, listed locus) of a called batch, the rows staying in HBM
// (smc_scan_detect)
// ------------------------------------------------------------------------------------------
// A pass of the scan calls B spiked copies of a run with one plan: rows[c * n_loci + l] is locus l of copy c.  Of those n_loci rows
// only the G listed ones - where the pass planted its SNVs - say anything, and of their 432 bytes only five fields: status, biallelic,
// used_mt and cand[0]'s allele, vmt and pi.  The .cut file's rule for "the planted ALT was called" (writers.cut_row behind
// rows.format_row) on such a row is
//     status == 0, the row not bi-allelic, cand[0].allele == ALT's fixed id (A, T, G, C = 0 .. 3), and int(float(py2 round(PI, 2))) >= thr
// and round(PI, 2) >= thr for an integer thr is PI >= thr - 0.005 up to how py2 rounds a double that close to the half.  So
//   k_scan_detect  a lane per (copy = blockIdx.y, listed locus): with lo = thr - 0.005 - 1e-6 and hi = thr - 0.005 + 1e-6 (made once on
//                  the host, passed by value)
//                    CALLED  status 0, not bi-allelic, cand[0].allele == alt, cand[0].pi > hi
//                    NOT     status 0, not bi-allelic, and cand[0].allele != alt or cand[0].pi < lo
//                    HOST    everything else: a bi-allelic row (rows._head_and_filter chooses the candidate with the genome in hand),
//                            a status that is not 0, a PI inside [lo, hi] or NaN - py2's round decides there.
//                  The lane writes one 16-byte record (PI, VMT, and the used MT below the verdict's two bits) with one vector
//                  store, and a HOST lane appends its record's index (copy * G + listed locus) to a list through one atomic cursor:
//                  the host downloads those rows only.  The list's ORDER is that of the atomics - not fixed from call to call; its
//                  CONTENT is.  Nothing else is written.
// Once per called batch, G x B lanes: not on the per-locus hot path.  The gathers are scattered (five dwords of a 432-byte row per
// lane), which at a few thousand lanes is nothing beside the batch's build.
#define SCD_BLOCK 256

__global__ __launch_bounds__(SCD_BLOCK) void k_scan_detect(const smc_row* __restrict__ rows, uint32_t n_loci,
                                                           const smc_scan_locus* __restrict__ listed, uint32_t n_listed, double lo, double hi,
                                                           smc_scan_verdict* __restrict__ out, uint32_t* __restrict__ host_list,
                                                           uint32_t* __restrict__ n_host) {
    const uint32_t c = blockIdx.y;
    for (uint32_t g = blockIdx.x * SCD_BLOCK + threadIdx.x; g < n_listed; g += gridDim.x * SCD_BLOCK) {
        const smc_scan_locus L = listed[g];
        const smc_row* const r = rows + ((size_t)c * n_loci + L.offset);      // (the host checked offset < n_loci on its copy)
        const int32_t status = r->status, bi = r->biallelic, used = r->used_mt;
        const int32_t allele = r->cand[0].allele, vmt = r->cand[0].vmt;
        const double pi = r->cand[0].pi;
        uint32_t v = SMC_SCAN_HOST;
        if (status == 0 && bi == 0) {
            if (allele != (int32_t)L.alt || pi < lo) v = SMC_SCAN_NOT;
            else if (pi > hi) v = SMC_SCAN_CALLED;
        }
        const uint32_t idx = c * n_listed + g;
        smc_scan_verdict rec;
        rec.pi = pi;
        rec.vmt = vmt;
        rec.mt_verdict = (v << 30) | (uint32_t)min(max(used, 0), (int32_t)SMC_SCAN_MT_MASK);
        out[idx] = rec;
        if (v == SMC_SCAN_HOST) host_list[atomicAdd(n_host, 1u)] = idx;       // (at most n_copies * n_listed appends: the list's size)
    }
}
