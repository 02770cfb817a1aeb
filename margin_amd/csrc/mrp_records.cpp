/*
 * mrp_records.cpp -- the phased variant records on the host: mrp_variant_records_from_extracted, the
 * definition of what mrp_phase_aligned_chunks_with_records returns for a chunk, and mrp_variants_from_records, from the records of a
 * contig's chunks to the variants mrp_phase_sets takes.  Plain C++: no device work, no HIP header.
 */
#include "rphmm_host.h" /* mrp_set_error, the status codes, include/margin_rphmm.h */

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct RecordArrays { /* the arrays of one mrp_variant_records while they are made: nothing is handed over before all of them exist */
    mrp_variant_records r{};
    ~RecordArrays() {
        free(r.state); free(r.gt); free(r.genotype_log_prob); free(r.hap1_log_prob); free(r.hap2_log_prob); free(r.read_first); free(r.n_hap1);
        free(r.n_hap2); free(r.reads);
    }
    bool alloc(int64_t n_primary, int64_t n_filtered, int64_t n_reads) {
        const size_t n = (size_t) (n_primary + n_filtered);
        r.n_primary = n_primary;
        r.n_filtered = n_filtered;
        r.state = (uint8_t *) calloc(n ? n : 1, 1);
        r.gt = (int32_t *) malloc(8 * (n ? n : 1));
        r.genotype_log_prob = (float *) calloc(n ? n : 1, 4);
        r.hap1_log_prob = (float *) calloc(n ? n : 1, 4);
        r.hap2_log_prob = (float *) calloc(n ? n : 1, 4);
        r.read_first = (int64_t *) calloc(n + 1, 8);
        r.n_hap1 = (int32_t *) calloc(n ? n : 1, 4);
        r.n_hap2 = (int32_t *) calloc(n ? n : 1, 4);
        r.reads = (int32_t *) malloc(4 * (size_t) (n_reads ? n_reads : 1));
        if (!r.state || !r.gt || !r.genotype_log_prob || !r.hap1_log_prob || !r.hap2_log_prob || !r.read_first || !r.n_hap1 || !r.n_hap2 || !r.reads)
            return false;
        for (size_t i = 0; i < 2 * n; i++) r.gt[i] = -2;
        return true;
    }
    void hand_over(mrp_variant_records *out) {
        *out = r;
        memset(&r, 0, sizeof(r));
    }
};

}  // namespace

extern "C" {

int mrp_variant_records_from_extracted(const mrp_extracted_chunk *x, const mrp_extracted_chunk *xf, const uint8_t *keep,
                                       const int64_t *bubble_variant, int64_t n_bubbles, const mrp_phase_result *result, const int8_t *hap_out,
                                       const int64_t *variant_pos, const int64_t *fvariant_pos, int64_t chunk_start, int64_t chunk_end,
                                       const int32_t *gt, const int32_t *variant_state, mrp_variant_records *out) {
    static const char *who = "mrp_variant_records_from_extracted";
    if (!x || !xf || !result || !out || x->n_variants < 0 || x->n_reads < 0 || xf->n_variants < 0 || n_bubbles < 0)
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (xf->n_reads != x->n_reads)
        return mrp_set_error(MRP_ERR_ARG, "%s: the two extractions are over %lld and %lld reads: not the same reads", who, (long long) x->n_reads, (long long) xf->n_reads);
    const int64_t nr = x->n_reads, np = x->n_variants, nv = xf->n_variants;
    if (nr >= (1ll << 30) || np + nv >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: bad sizes", who);
    if (nr > 0 && (!hap_out || !x->read_status || !xf->read_status)) return mrp_set_error(MRP_ERR_ARG, "%s: null read array", who);
    if (!x->entry_first || !xf->entry_first || !x->allele_first || !xf->allele_first || (n_bubbles > 0 && !bubble_variant) || (np > 0 && !variant_pos) ||
        (nv > 0 && (!fvariant_pos || !gt || !variant_state)))
        return mrp_set_error(MRP_ERR_ARG, "%s: null array", who);
    const int64_t ne = x->entry_first[np], nef = xf->entry_first[nv];
    if ((ne > 0 && !x->entry_read) || (nef > 0 && !xf->entry_read)) return mrp_set_error(MRP_ERR_ARG, "%s: null array", who);
    for (int64_t b = 0; b < n_bubbles; b++)
        if (bubble_variant[b] < 0 || bubble_variant[b] >= np)
            return mrp_set_error(MRP_ERR_ARG, "%s: bubble %lld names variant %lld of %lld", who, (long long) b, (long long) bubble_variant[b], (long long) np);
    for (int64_t e = 0; e < ne; e++)
        if (x->entry_read[e] < 0 || x->entry_read[e] >= nr) return mrp_set_error(MRP_ERR_ARG, "%s: entry %lld names read %d", who, (long long) e, x->entry_read[e]);
    for (int64_t e = 0; e < nef; e++)
        if (xf->entry_read[e] < 0 || xf->entry_read[e] >= nr)
            return mrp_set_error(MRP_ERR_ARG, "%s: entry %lld at the filtered variants names read %d", who, (long long) e, xf->entry_read[e]);
    const int64_t f0 = result->ref_start, fl = result->length;
    if (fl < 0 || (fl > 0 && (f0 < 0 || f0 + fl > n_bubbles)))
        return mrp_set_error(MRP_ERR_ARG, "%s: the fragment [%lld, %lld) leaves the chunk's %lld bubbles", who, (long long) f0, (long long) (f0 + fl), (long long) n_bubbles);
    if (fl > 0 && (!result->haplotype_string1 || !result->haplotype_string2 || !result->genotype_probs || !result->haplotype_probs1 || !result->haplotype_probs2))
        return mrp_set_error(MRP_ERR_ARG, "%s: null array of the fragment", who);
    for (int64_t j = 0; j < fl; j++) {
        const int64_t v = bubble_variant[f0 + j], k = x->allele_first[v + 1] - x->allele_first[v];
        if (result->haplotype_string1[j] >= (uint64_t) k || result->haplotype_string2[j] >= (uint64_t) k)
            return mrp_set_error(MRP_ERR_ARG, "%s: bubble %lld: the fragment's alleles %llu | %llu are outside the variant's %lld", who, (long long) (f0 + j),
                                 (unsigned long long) result->haplotype_string1[j], (unsigned long long) result->haplotype_string2[j], (long long) k);
    }
    for (int64_t v = 0; v < nv; v++) {
        const int64_t k = xf->allele_first[v + 1] - xf->allele_first[v];
        for (int w = 0; w < 2; w++)
            if (gt[2 * v + w] < 0 || gt[2 * v + w] >= k)
                return mrp_set_error(MRP_ERR_ARG, "%s: filtered variant %lld: genotype %d outside its %lld alleles", who, (long long) v, gt[2 * v + w], (long long) k);
        if (variant_state[v] < MRP_VARIANT_NOT_VISITED || variant_state[v] > MRP_VARIANT_TIE)
            return mrp_set_error(MRP_ERR_ARG, "%s: filtered variant %lld: state %d", who, (long long) v, variant_state[v]);
    }
    auto primary = [&](int64_t r) { return x->read_status[r] == MRP_READ_KEPT && (!keep || keep[r]); };
    /* the bubble of a variant (vcfEntriesToBubbleIdx read backwards) */
    std::vector<int64_t> bubble_of((size_t) np, -1);
    for (int64_t b = 0; b < n_bubbles; b++) bubble_of[(size_t) bubble_variant[b]] = b;
    /* a slot per entry of a primary read is enough */
    int64_t cap = 0;
    for (int64_t e = 0; e < ne; e++) cap += primary(x->entry_read[e]);
    for (int64_t e = 0; e < nef; e++) cap += primary(xf->entry_read[e]);
    RecordArrays A;
    if (!A.alloc(np, nv, cap)) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    mrp_variant_records &R = A.r;
    int64_t at = 0;
    /* the two lists of a site: the entries' primary reads with tag 1, ascending (the extraction lists a variant's entries in ascending
     * read order), then those with tag 2 */
    auto lists = [&](int64_t s, const mrp_extracted_chunk *X, int64_t v, bool kept_there) {
        for (int h = 1; h <= 2; h++) {
            int32_t n = 0;
            for (int64_t e = X->entry_first[v]; e < X->entry_first[v + 1]; e++) {
                const int32_t r = X->entry_read[e];
                if (kept_there && X->read_status[r] != MRP_READ_KEPT) continue;
                if (!primary(r) || hap_out[r] != h) continue;
                R.reads[at++] = r;
                n++;
            }
            (h == 1 ? R.n_hap1 : R.n_hap2)[s] = n;
        }
    };
    for (int64_t v = 0; v < np; v++) { /* vcf.c:519-592 */
        const int64_t b = bubble_of[(size_t) v];
        const bool updated = b >= 0 && b >= f0 && b < f0 + fl && variant_pos[v] >= chunk_start && variant_pos[v] < chunk_end; /* :520, :538-540 */
        if (updated) {
            const int64_t j = b - f0;
            R.state[v] = MRP_RECORD_UPDATED; /* :563 */
            R.gt[2 * v] = (int32_t) result->haplotype_string1[j]; /* :558-559 */
            R.gt[2 * v + 1] = (int32_t) result->haplotype_string2[j];
            R.genotype_log_prob[v] = result->genotype_probs[j]; /* :560-562, before fromLog */
            R.hap1_log_prob[v] = result->haplotype_probs1[j];
            R.hap2_log_prob[v] = result->haplotype_probs2[j];
            lists(v, x, v, false); /* :572-582 */
        }
        R.read_first[v + 1] = at;
    }
    for (int64_t v = 0; v < nv; v++) { /* bubbleGraph.c:2298-2343 */
        const int64_t s = np + v;
        const int32_t st = variant_state[v];
        if (st != MRP_VARIANT_NOT_VISITED) {
            R.state[s] = st == MRP_VARIANT_TIE ? MRP_RECORD_CLEARED : MRP_RECORD_UPDATED; /* :2318-2327 */
            R.gt[2 * s] = st == MRP_VARIANT_TIE ? -1 : (st == MRP_VARIANT_CIS ? gt[2 * v] : gt[2 * v + 1]); /* :2298-2309 */
            R.gt[2 * s + 1] = st == MRP_VARIANT_TIE ? -1 : (st == MRP_VARIANT_CIS ? gt[2 * v + 1] : gt[2 * v]);
            R.genotype_log_prob[s] = R.hap1_log_prob[s] = R.hap2_log_prob[s] = -INFINITY; /* probability 0, :2300-2302 */
            if (st != MRP_VARIANT_TIE && fvariant_pos[v] >= chunk_start && fvariant_pos[v] < chunk_end) lists(s, xf, v, true); /* :2330-2343 */
        }
        R.read_first[s + 1] = at;
    }
    A.hand_over(out);
    return MRP_OK;
}

int mrp_variants_from_records(int64_t n_chunks, const mrp_variant_records *records, const int64_t *const *variant_pos, const int32_t *const *n_alleles,
                              const int64_t *const *fvariant_pos, const int32_t *const *fn_alleles, const int32_t *switched,
                              const int32_t *const *read_id, mrp_record_variants *out) {
    static const char *who = "mrp_variants_from_records";
    if (n_chunks < 0 || !out || (n_chunks > 0 && (!records || !variant_pos || !n_alleles || !fvariant_pos || !fn_alleles || !switched || !read_id)))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    struct Kept { int64_t pos; int32_t chunk, site; };
    std::vector<Kept> kept;
    int64_t n_lists = 0, n_ids = 0;
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_variant_records &R = records[c];
        const int64_t n = R.n_primary + R.n_filtered;
        if (R.n_primary < 0 || R.n_filtered < 0 || n >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: bad sizes", who, (long long) c);
        if (n == 0) continue;
        if (!R.state || !R.gt || !R.genotype_log_prob || !R.hap1_log_prob || !R.hap2_log_prob || !R.read_first || !R.n_hap1 || !R.n_hap2 ||
            (R.n_primary > 0 && (!variant_pos[c] || !n_alleles[c])) || (R.n_filtered > 0 && (!fvariant_pos[c] || !fn_alleles[c])))
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null array", who, (long long) c);
        if (R.read_first[n] > 0 && (!R.reads || !read_id[c])) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null read array", who, (long long) c);
        for (int64_t s = 0; s < n; s++) {
            if (R.state[s] > MRP_RECORD_CLEARED) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld, site %lld: state %d", who, (long long) c, (long long) s, R.state[s]);
            if (R.state[s] != MRP_RECORD_UPDATED) continue; /* wasUpdated, vcf.c:863-868 */
            const bool prim = s < R.n_primary;
            const int64_t pos = prim ? variant_pos[c][s] : fvariant_pos[c][s - R.n_primary];
            const int32_t na = prim ? n_alleles[c][s] : fn_alleles[c][s - R.n_primary];
            if (pos < 0 || pos > INT32_MAX) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld, site %lld: position %lld", who, (long long) c, (long long) s, (long long) pos);
            if (na < 1 || R.gt[2 * s] < 0 || R.gt[2 * s] >= na || R.gt[2 * s + 1] < 0 || R.gt[2 * s + 1] >= na)
                return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld, site %lld: genotype %d | %d outside its %d alleles", who, (long long) c, (long long) s, R.gt[2 * s],
                                     R.gt[2 * s + 1], na);
            if (R.n_hap1[s] < 0 || R.n_hap2[s] < 0 || R.read_first[s + 1] - R.read_first[s] != (int64_t) R.n_hap1[s] + R.n_hap2[s])
                return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld, site %lld: list lengths", who, (long long) c, (long long) s);
            kept.push_back(Kept{pos, (int32_t) c, (int32_t) s});
            n_lists += na + 1;
            n_ids += R.n_hap1[s] + R.n_hap2[s];
        }
    }
    /* by position; ties by chunk, then primary before filtered, then site: (chunk, site) ascending, the order they were found in */
    std::stable_sort(kept.begin(), kept.end(), [](const Kept &a, const Kept &b) { return a.pos < b.pos; });
    const size_t n = kept.size();
    /* one block: the variants, allele_read_off (8-byte entries first), then the int32 and float arrays */
    const size_t bytes = sizeof(mrp_variant) * n + 8 * (size_t) n_lists + 4 * ((size_t) n_ids + 2 * n + 3 * n) + 16;
    uint8_t *blk = (uint8_t *) malloc(bytes);
    if (!blk) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    mrp_variant *V = (mrp_variant *) blk;
    int64_t *off = (int64_t *) (V + n);
    int32_t *ids = (int32_t *) (off + n_lists), *chunk = ids + n_ids, *site = chunk + n;
    float *lg = (float *) (site + n), *l1 = lg + n, *l2 = l1 + n;
    int64_t io = 0, ii = 0;
    for (size_t i = 0; i < n; i++) {
        const int64_t c = kept[i].chunk, s = kept[i].site;
        const mrp_variant_records &R = records[c];
        const bool prim = s < R.n_primary, sw = switched[c] != 0;
        const int32_t na = prim ? n_alleles[c][s] : fn_alleles[c][s - R.n_primary];
        const int32_t g1 = R.gt[2 * s], g2 = R.gt[2 * s + 1];
        V[i].pos = (int32_t) kept[i].pos;
        V[i].gt1 = sw ? g2 : g1; /* vcf.c:631-633 */
        V[i].gt2 = sw ? g1 : g2;
        V[i].n_alleles = na;
        V[i].allele_read_off = off + io;
        V[i].allele_reads = ids + ii;
        chunk[i] = (int32_t) c;
        site[i] = (int32_t) s;
        lg[i] = R.genotype_log_prob[s];
        l1[i] = sw ? R.hap2_log_prob[s] : R.hap1_log_prob[s]; /* :634-636 */
        l2[i] = sw ? R.hap1_log_prob[s] : R.hap2_log_prob[s];
        const int32_t *h1 = R.reads + R.read_first[s], *h2 = h1 + R.n_hap1[s];
        int64_t k = 0;
        for (int32_t a = 0; a < na; a++) { /* alleleIdxToReads: sets of read ids under the called alleles, the lists staying with their allele */
            off[io + a] = k;
            const int64_t k0 = k;
            if (a == g1)
                for (int32_t q = 0; q < R.n_hap1[s]; q++) ids[ii + k++] = read_id[c][h1[q]];
            if (a == g2)
                for (int32_t q = 0; q < R.n_hap2[s]; q++) ids[ii + k++] = read_id[c][h2[q]];
            std::sort(ids + ii + k0, ids + ii + k);
            k = k0 + (std::unique(ids + ii + k0, ids + ii + k) - (ids + ii + k0));
        }
        off[io + na] = k;
        io += na + 1;
        ii += k;
    }
    out->n_variants = (int64_t) n;
    out->variants = V;
    out->chunk = chunk;
    out->site = site;
    out->genotype_log_prob = lg;
    out->hap1_log_prob = l1;
    out->hap2_log_prob = l2;
    return MRP_OK;
}

}  // extern "C"
