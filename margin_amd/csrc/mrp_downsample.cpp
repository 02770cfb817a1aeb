/*
 * mrp_downsample.cpp -- the downsampling to maxDepth on the host: the definition of what the aligned composites
 * do with mrp_context_set_downsampling on, restated from downsampleBamChunkReadWithVcfEntrySubstringsViaFullReadLengthLikelihood
 * (impl/htsIntegration.c:1141-1216) branch by branch, with the LP of computeReadProbsByLengthAndSecondMetric (:957-1011) in closed form.
 * Plain C++: no device work, no HIP header.
 */
#include "rphmm_host.h" /* mrp_set_error, the status codes, include/margin_rphmm.h */
#include "mrp_downsample.h"

#include <algorithm>
#include <vector>

namespace {

/* One chunk.  status / l / h: per read of the chunk; keep (required) and prob (may be NULL): per read.  Returns whether the chunk was
 * downsampled (the reference's return value, which phase.c:368 only logs and frees by). */
bool ds_chunk(int64_t n_reads, const uint8_t *status, const int32_t *l, const int32_t *h, int64_t V, int64_t D, uint64_t seed, int64_t overlap_start,
              int64_t overlap_end, uint8_t *keep, double *prob) {
    /* :1153-1161 the totals over `reads`: the MRP_READ_KEPT reads in ascending read index */
    int64_t total = 0;
    for (int64_t r = 0; r < n_reads; r++)
        if (status[r] == MRP_READ_KEPT) total += l[r];
    /* :1163-1170 "do we need to downsample?" */
    if (mrp_ds_shallow(total, V, D)) {
        for (int64_t r = 0; r < n_reads; r++) {
            keep[r] = status[r] == MRP_READ_KEPT;
            if (prob) prob[r] = keep[r] ? 1.0 : 0.0;
        }
        return false;
    }
    /* :1174-1186 "is there something wrong with this chunk?" -- chunkSize == 0 (totalVcfEntries == 0 with V > 0 was shallow) */
    if (V == 0) {
        for (int64_t r = 0; r < n_reads; r++) {
            keep[r] = 0;
            if (prob) prob[r] = 0.0;
        }
        return true;
    }
    /* :1193-1195 the LP's optimum: total_cov = target_coverage * region_length (:964) */
    const int64_t T = D * V;
    std::vector<int64_t> order;
    for (int64_t r = 0; r < n_reads; r++)
        if (status[r] == MRP_READ_KEPT && l[r] > 0) order.push_back(r);
    std::sort(order.begin(), order.end(), [&](int64_t j, int64_t i) { return mrp_ds_before(h[j], l[j], j, h[i], l[i], i); });
    std::vector<double> p((size_t) n_reads, 0.0);
    int64_t B = 0;
    for (int64_t r : order) {
        p[(size_t) r] = mrp_ds_prob(B, l[r], T);
        B += l[r];
    }
    /* :1199-1207 one draw per read of `reads`, in list order */
    int64_t k = 0;
    for (int64_t r = 0; r < n_reads; r++) {
        if (status[r] != MRP_READ_KEPT) {
            keep[r] = 0;
            if (prob) prob[r] = 0.0;
            continue;
        }
        double q = l[r] > 0 ? p[(size_t) r] : (h[r] > 0 ? 1.0 : 0.0); /* a free variable of the LP: its objective coefficient decides */
        if (total <= T) q = 1.0; /* the constraint takes every read whole */
        keep[r] = mrp_ds_draw(seed, overlap_start, overlap_end, k) < q; /* :1201 */
        if (prob) prob[r] = q;
        k++;
    }
    return true;
}

}  // namespace

extern "C" {

double mrp_downsample_draw(uint64_t seed, int64_t overlap_start, int64_t overlap_end, int64_t k) { return mrp_ds_draw(seed, overlap_start, overlap_end, k); }

/* getAlignedReadLength3 with boundaryAtMatch = FALSE (htsIntegration.c:37-107) and countIndels (:113-120), as ex_scan_kernel computes
 * aln_len: soft clips before the first M/=/X/D/N/I op, soft clips from the last op back to the first such op (never op 0), and
 * l_qseq - clips + deletions - insertions -- N ops advance the reference but are not counted (:117-118) */
int mrp_aln_read_lengths(const mrp_aligned_chunk *C, int32_t *out) {
    static const char *who = "mrp_aln_read_lengths";
    if (!C || C->n_reads < 0 || (C->n_reads > 0 && (!out || !C->l_qseq || !C->cigar_first))) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (C->n_reads > 0 && C->cigar_first[C->n_reads] > 0 && !C->cigar) return mrp_set_error(MRP_ERR_ARG, "%s: null cigar", who);
    auto body = [](uint32_t op) { return op == 0 || op == 1 || op == 2 || op == 3 || op == 7 || op == 8; };
    for (int64_t r = 0; r < C->n_reads; r++) {
        const int64_t a = C->cigar_first[r], n = C->cigar_first[r + 1] - a;
        if (C->l_qseq[r] <= 0 || n <= 0) { out[r] = 0; continue; }
        const uint32_t *w = C->cigar + a;
        int64_t clip = 0, eclip = 0, ins = 0, del = 0;
        for (int64_t k = 0; k < n && !body(w[k] & 15u); k++)
            if ((w[k] & 15u) == 4) clip += w[k] >> 4;
        for (int64_t k = n - 1; k > 0 && !body(w[k] & 15u); k--)
            if ((w[k] & 15u) == 4) eclip += w[k] >> 4;
        for (int64_t k = 0; k < n; k++) {
            if ((w[k] & 15u) == 1) ins += w[k] >> 4;
            if ((w[k] & 15u) == 2) del += w[k] >> 4;
        }
        out[r] = (int32_t) ((int64_t) C->l_qseq[r] - clip - eclip + del - ins);
    }
    return MRP_OK;
}

int mrp_downsample_keep_from_extracted(const mrp_extracted_chunk *x, const int32_t *aln_read_length, int64_t max_depth, uint64_t seed, int64_t overlap_start,
                                       int64_t overlap_end, uint8_t *keep_out, double *prob_out, int32_t *downsampled_out) {
    static const char *who = "mrp_downsample_keep_from_extracted";
    if (!x || x->n_reads < 0 || x->n_variants < 0) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (max_depth <= 0) return mrp_set_error(MRP_ERR_ARG, "%s: max_depth must be positive (0 means no downsampling: nothing to decide)", who);
    if (x->n_reads > 0 && (!keep_out || !aln_read_length || !x->read_status || !x->read_n_substrings)) return mrp_set_error(MRP_ERR_ARG, "%s: null array", who);
    for (int64_t r = 0; r < x->n_reads; r++)
        if (x->read_n_substrings[r] < 0) return mrp_set_error(MRP_ERR_ARG, "%s: read %lld has a negative substring count", who, (long long) r);
    const bool did = ds_chunk(x->n_reads, x->read_status, x->read_n_substrings, aln_read_length, x->n_variants, max_depth, seed, overlap_start, overlap_end,
                              keep_out, prob_out);
    if (downsampled_out) *downsampled_out = did;
    return MRP_OK;
}

}  /* extern "C" */
