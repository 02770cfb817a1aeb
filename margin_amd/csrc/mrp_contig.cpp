/*
 * mrp_contig.cpp -- closing a contig on the host: what margin phase does after its chunk loop
 * (phase.c:475-535) over the per-chunk outputs of the aligned calls.  mrp_final_read_tags and mrp_stitch_values define what every
 * read carries into the stitching; mrp_close_contig is the glue between them, mrp_stitch_chunk, mrp_variants_from_records and
 * mrp_phase_sets, none of which is restated here; mrp_close_contigs closes several contigs on the library's host threads
 * (stitching.c:1635).  Plain C++: no device work, no HIP header.
 */
#include "mrp_host_pool.h" /* mrp_parallel_for; rphmm_host.h: mrp_set_error, the status codes, include/margin_rphmm.h */

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

/* the length of a list closed by -1 (NULL: empty) */
int64_t closed_length(const int32_t *list) {
    int64_t n = 0;
    while (list && list[n] != -1) n++;
    return n;
}

struct ContigOut { /* the arrays of one mrp_contig_out while they are made: nothing is handed over before all of them exist */
    mrp_contig_out o{};
    ~ContigOut() { mrp_contig_out_clear(&o); }
    void hand_over(mrp_contig_out *out) {
        *out = o;
        memset(&o, 0, sizeof(o));
    }
};

/* every MRP_ERR_ARG of mrp_close_contig that can be seen before a chunk is stitched; what the chain's own functions refuse
 * (a record's state, a genotype outside its alleles) is theirs to report */
int check_chunks(const char *who, int64_t n_chunks, const mrp_contig_chunk *chunks, const mrp_contig_rules *rules) {
    if (n_chunks < 0 || !rules || (n_chunks > 0 && !chunks)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_contig_chunk &K = chunks[c];
        if (K.n_reads < 0 || K.n_reads >= (1ll << 31) || K.n_variants < 0 || K.n_fvariants < 0)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: negative count", who, (long long) c);
        if (K.n_reads > 0 && (!K.read_names || !K.hap_out || (K.filtered_out && !K.phred_out)))
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null read array", who, (long long) c);
        for (int64_t r = 0; r < K.n_reads; r++)
            if (!K.read_names[r]) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: read %lld has no name", who, (long long) c, (long long) r);
        if (!K.records) continue;
        if (K.records->n_primary != K.n_variants || K.records->n_filtered != K.n_fvariants)
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: records over %lld + %lld sites, position arrays over %lld + %lld", who, (long long) c,
                                 (long long) K.records->n_primary, (long long) K.records->n_filtered, (long long) K.n_variants, (long long) K.n_fvariants);
        if ((K.n_variants > 0 && (!K.variant_pos || !K.n_alleles)) || (K.n_fvariants > 0 && (!K.fvariant_pos || !K.fn_alleles)))
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null position array", who, (long long) c);
        if (K.n_reads > 0 && !K.read_id) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null read ids", who, (long long) c);
    }
    return MRP_OK;
}

/* one contig into a ContigOut; the caller has run check_chunks */
int close_one(const char *who, int64_t n_chunks, const mrp_contig_chunk *chunks, const mrp_contig_rules *rules, ContigOut &A) {
    mrp_contig_out &O = A.o;
    int64_t total_reads = 0;
    for (int64_t c = 0; c < n_chunks; c++) total_reads += chunks[c].n_reads;
    const size_t m = (size_t) (n_chunks > 0 ? n_chunks : 1);
    O.n_chunks = n_chunks;
    O.switched = (int32_t *) calloc(m, sizeof(int32_t));
    O.counts = (int64_t *) calloc(4 * m, sizeof(int64_t));
    /* the pointers, then the block they point into */
    O.final_hap = (int8_t **) calloc(1, sizeof(int8_t *) * m + (size_t) (total_reads > 0 ? total_reads : 1));
    if (!O.switched || !O.counts || !O.final_hap) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    int8_t *block = (int8_t *) (O.final_hap + m);
    for (int64_t c = 0, at = 0; c < n_chunks; at += chunks[c].n_reads, c++) O.final_hap[c] = block + at;

    /* ---- the chunk's reads as the stitching sees them, then chunkToStitch_phaseAdjacentChunks chunk by chunk */
    mrp_stitch *S = nullptr;
    int rc = mrp_stitch_create(&S);
    std::vector<int8_t> tag;
    std::vector<double> value;
    std::vector<const char *> names[2];
    std::vector<double> probs[2];
    for (int64_t c = 0; c < n_chunks && rc == MRP_OK; c++) {
        const mrp_contig_chunk &K = chunks[c];
        tag.assign((size_t) K.n_reads + 1, 0);
        value.assign((size_t) K.n_reads + 1, 0.0);
        rc = mrp_final_read_tags(K.n_reads, K.hap_out, K.filtered_out, K.filtered_read_out, tag.data());
        if (rc == MRP_OK) rc = mrp_stitch_values(K.n_reads, K.filtered_out ? K.hap_out : nullptr, K.phred_out, tag.data(), value.data());
        if (rc != MRP_OK) break;
        for (int h = 0; h < 2; h++) { names[h].clear(); probs[h].clear(); }
        for (int64_t r = 0; r < K.n_reads; r++)
            if (tag[(size_t) r] == 1 || tag[(size_t) r] == 2) {
                names[tag[(size_t) r] - 1].push_back(K.read_names[r]);
                probs[tag[(size_t) r] - 1].push_back(value[(size_t) r]);
            }
        int sw = 0;
        rc = mrp_stitch_chunk(S, (int64_t) names[0].size(), names[0].data(), probs[0].data(), (int64_t) names[1].size(), names[1].data(), probs[1].data(),
                              rules->primary_reads_only != 0, c == 0 || rules->prevent_switching != 0, &sw, O.counts + 4 * c);
        O.switched[c] = sw;
    }
    /* ---- the final read sets (stitching.c:1664-1671): by name, so a read of two chunks gets one value */
    for (int64_t c = 0; c < n_chunks && rc == MRP_OK; c++)
        for (int64_t r = 0; r < chunks[c].n_reads; r++)
            O.final_hap[c][r] = mrp_stitch_lookup(S, 1, chunks[c].read_names[r], nullptr) ? 1 : (mrp_stitch_lookup(S, 2, chunks[c].read_names[r], nullptr) ? 2 : 0);
    mrp_stitch_destroy(S);
    if (rc != MRP_OK) return rc;

    /* ---- updateHaplotypeSwitchingInVcfEntries and the kept variants, then writePhasedVcf's phase set rules */
    std::vector<mrp_variant_records> recs((size_t) n_chunks);
    std::vector<const int64_t *> vp((size_t) n_chunks), fp((size_t) n_chunks);
    std::vector<const int32_t *> na((size_t) n_chunks), fa((size_t) n_chunks), ids((size_t) n_chunks);
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_contig_chunk &K = chunks[c];
        memset(&recs[(size_t) c], 0, sizeof(mrp_variant_records)); /* (no records: no sites) */
        if (K.records) recs[(size_t) c] = *K.records;
        vp[(size_t) c] = K.variant_pos; na[(size_t) c] = K.n_alleles;
        fp[(size_t) c] = K.fvariant_pos; fa[(size_t) c] = K.fn_alleles;
        ids[(size_t) c] = K.read_id;
    }
    rc = mrp_variants_from_records(n_chunks, recs.data(), vp.data(), na.data(), fp.data(), fa.data(), O.switched, ids.data(), &O.variants);
    if (rc != MRP_OK) { memset(&O.variants, 0, sizeof(O.variants)); return rc; }
    const size_t nv = (size_t) (O.variants.n_variants > 0 ? O.variants.n_variants : 1);
    O.phase_set = (int32_t *) calloc(nv, sizeof(int32_t));
    O.reason = (int32_t *) calloc(nv, sizeof(int32_t));
    if (!O.phase_set || !O.reason) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    return mrp_phase_sets(O.variants.n_variants, O.variants.variants, rules->min_spanning_reads, rules->min_binomial_read_split_likelihood,
                          rules->max_discordant_ratio, O.phase_set, O.reason);
}

}  // namespace

extern "C" {

void mrp_contig_out_clear(mrp_contig_out *out) {
    if (!out) return;
    free(out->switched); free(out->counts); free(out->final_hap); free(out->variants.variants); free(out->phase_set); free(out->reason);
    memset(out, 0, sizeof(*out));
}

int mrp_final_read_tags(int64_t n_reads, const int8_t *hap_out, const mrp_filtered_out *filtered_out, const int32_t *filtered_read_out,
                        int8_t *tag_out) {
    static const char *who = "mrp_final_read_tags";
    if (n_reads < 0 || n_reads >= (1ll << 31) || (n_reads > 0 && (!hap_out || !tag_out))) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    for (int64_t r = 0; r < n_reads; r++)
        if (hap_out[r] < -1 || hap_out[r] > 2) return mrp_set_error(MRP_ERR_ARG, "%s: read %lld: tag %d", who, (long long) r, hap_out[r]);
    if (!filtered_out) { /* the haplotag tool: the call's tags are final */
        for (int64_t r = 0; r < n_reads; r++) tag_out[r] = hap_out[r] > 0 ? hap_out[r] : 0;
        return MRP_OK;
    }
    const int64_t nf = closed_length(filtered_read_out), nh = filtered_out->n_reads;
    if (nh != n_reads + nf)
        return mrp_set_error(MRP_ERR_ARG, "%s: filtered_out over %lld reads, the chunk has %lld and %lld filtered", who, (long long) nh, (long long) n_reads, (long long) nf);
    if (nh > 0 && !filtered_out->read_hap) return mrp_set_error(MRP_ERR_ARG, "%s: null read_hap", who);
    for (int64_t i = 0; i < nh; i++)
        if (filtered_out->read_hap[i] < 0 || filtered_out->read_hap[i] > 2)
            return mrp_set_error(MRP_ERR_ARG, "%s: read_hap[%lld] is %d", who, (long long) i, filtered_out->read_hap[i]);
    /* where the back half's result of a read lies: its own index, or behind the chunk's reads when it is a filtered read */
    std::vector<int64_t> at((size_t) n_reads);
    for (int64_t r = 0; r < n_reads; r++) at[(size_t) r] = r;
    for (int64_t k = 0; k < nf; k++) {
        const int64_t r = filtered_read_out[k];
        if (r < 0 || r >= n_reads) return mrp_set_error(MRP_ERR_ARG, "%s: filtered read %lld names read %lld of %lld", who, (long long) k, (long long) r, (long long) n_reads);
        if (at[(size_t) r] != r) return mrp_set_error(MRP_ERR_ARG, "%s: read %lld is a filtered read twice", who, (long long) r);
        at[(size_t) r] = n_reads + k;
    }
    for (int64_t r = 0; r < n_reads; r++)
        tag_out[r] = hap_out[r] == 1 || hap_out[r] == 2 ? hap_out[r] : (int8_t) filtered_out->read_hap[at[(size_t) r]];
    return MRP_OK;
}

int mrp_stitch_values(int64_t n_reads, const int8_t *hap_out, const double *phred_out, const int8_t *final_tag, double *value_out) {
    static const char *who = "mrp_stitch_values";
    if (n_reads < 0 || (n_reads > 0 && (!final_tag || !value_out || (hap_out && !phred_out)))) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    for (int64_t r = 0; r < n_reads; r++) {
        if (final_tag[r] < 0 || final_tag[r] > 2) return mrp_set_error(MRP_ERR_ARG, "%s: read %lld: final tag %d", who, (long long) r, final_tag[r]);
        if (!hap_out) continue;
        if (hap_out[r] < -1 || hap_out[r] > 2) return mrp_set_error(MRP_ERR_ARG, "%s: read %lld: tag %d", who, (long long) r, hap_out[r]);
        if (hap_out[r] > 0 && final_tag[r] != hap_out[r])
            return mrp_set_error(MRP_ERR_ARG, "%s: read %lld: the phasing's tag %d with final tag %d", who, (long long) r, hap_out[r], final_tag[r]);
    }
    char text[400]; /* ("%f" of the largest double: 309 digits, the point, six more) */
    for (int64_t r = 0; r < n_reads; r++) {
        if (final_tag[r] == 0) { value_out[r] = 0.0; continue; }
        if (!hap_out || hap_out[r] <= 0) { value_out[r] = -1.0; continue; } /* stitching.c:901, :914 */
        snprintf(text, sizeof(text), "%f", phred_out[r]);                    /* genomeFragment.c:117 */
        value_out[r] = (double) strtof(text, nullptr);                       /* stitching.c:300 */
    }
    return MRP_OK;
}

int mrp_close_contig(int64_t n_chunks, const mrp_contig_chunk *chunks, const mrp_contig_rules *rules, mrp_contig_out *out) {
    static const char *who = "mrp_close_contig";
    if (!out) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    int rc = check_chunks(who, n_chunks, chunks, rules);
    if (rc != MRP_OK) return rc;
    ContigOut A;
    rc = close_one(who, n_chunks, chunks, rules, A);
    if (rc == MRP_OK) A.hand_over(out);
    return rc;
}

int mrp_close_contigs(int64_t n_contigs, const int64_t *first_chunk, const mrp_contig_chunk *chunks, const mrp_contig_rules *rules,
                      mrp_contig_out *out) {
    static const char *who = "mrp_close_contigs";
    if (n_contigs < 0 || !first_chunk || first_chunk[0] != 0 || (n_contigs > 0 && !out)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    for (int64_t k = 0; k < n_contigs; k++)
        if (first_chunk[k + 1] < first_chunk[k]) return mrp_set_error(MRP_ERR_ARG, "%s: contig %lld ends before it starts", who, (long long) k);
    int rc = check_chunks(who, first_chunk[n_contigs], chunks, rules);
    if (rc != MRP_OK) return rc;
    /* stitching.c:1635: every contig on its own, on the host threads; a thread's error text stays with its thread, so it is kept here */
    std::vector<ContigOut> made((size_t) n_contigs);
    std::vector<int> status((size_t) n_contigs, MRP_OK);
    std::vector<std::string> errs((size_t) n_contigs);
    mrp_pool_set_weight(0); /* (a contig's cost is unknown: the loop is posted whatever the caller's last loops weighed) */
    mrp_parallel_for(n_contigs, 1, [&](int64_t k) {
        status[(size_t) k] = close_one(who, first_chunk[k + 1] - first_chunk[k], chunks + first_chunk[k], rules, made[(size_t) k]);
        if (status[(size_t) k] != MRP_OK) errs[(size_t) k] = mrp_last_error();
    });
    for (int64_t k = 0; k < n_contigs; k++)
        if (status[(size_t) k] != MRP_OK) return mrp_set_error(status[(size_t) k], "contig %lld: %s", (long long) k, errs[(size_t) k].c_str());
    for (int64_t k = 0; k < n_contigs; k++) made[(size_t) k].hand_over(&out[k]);
    return MRP_OK;
}

}  // extern "C"
