/*
 * mrp_poa_consensus.cpp -- poa_getConsensus (impl/poa.c:1350-1588) for one consensus over the arrays of mrp_poa_augment:
 * the forward pass with logAdd (pairwiseAligner.c:282-299) and the C library's log, then the greedy trace back.  Sequential by nature (a
 * chain of logAdd over the nodes, milliseconds per polish chunk), so it stays on the host: plain C++, no HIP.  Every sum is one IEEE
 * operation at a time in the reference's order.  The definition is tests/poa_oracle.py's consensus().
 */
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/margin_rphmm.h"
#include "rphmm_host.h" /* mrp_set_error */

namespace {

const double POC_LOG_ZERO = -INFINITY;

/* lookup, pairwiseAligner.c:282-293: float literals widened to double */
double poc_lookup(double x) {
    if (x <= 1.00f) return ((-0.009350833524763f * x + 0.130659527668286f) * x + 0.498799810682272f) * x + 0.693203116424741f;
    if (x <= 2.50f) return ((-0.014532321752540f * x + 0.139942324101744f) * x + 0.495635523139337f) * x + 0.692140569840976f;
    if (x <= 4.50f) return ((-0.004605031767994f * x + 0.063427417320019f) * x + 0.695956496475118f) * x + 0.514272634594009f;
    return ((-0.000458661602210f * x + 0.009695946122598f) * x + 0.930734667215156f) * x + 0.168037164329057f;
}

/* logAdd, :295-299 */
double poc_log_add(double x, double y) {
    if (x < y) return (x == POC_LOG_ZERO || y - x >= 7.5) ? y : poc_lookup(y - x) + x;
    return (y == POC_LOG_ZERO || x - y >= 7.5) ? x : poc_lookup(x - y) + y;
}

}  // namespace

extern "C" int mrp_poa_consensus(int64_t L, const double *base_weight, const int32_t *base_pick, const int32_t *repeat_count_pick,
                                 const int64_t *insert_first, const int64_t *insert_str_off, const int32_t *insert_str_len,
                                 const double *insert_weight_forward, const double *insert_weight_reverse, const uint8_t *pool_symbols,
                                 const int32_t *pool_counts, int64_t pool_len, const int64_t *delete_first, const int32_t *delete_length,
                                 const double *delete_weight_forward, const double *delete_weight_reverse, int32_t use_rle, uint8_t **symbols_out,
                                 int32_t **counts_out, int64_t *length_out, int64_t **poa_to_consensus_map_out) {
    static const char *who = "mrp_poa_consensus";
    if (!base_weight || !base_pick || !repeat_count_pick || !insert_first || !delete_first || !symbols_out || !counts_out || !length_out ||
        !poa_to_consensus_map_out)
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (L < 0 || L + 1 >= (1ll << 31) || pool_len < 0) return mrp_set_error(MRP_ERR_ARG, "%s: bad sizes", who);
    const int64_t n = L + 1; /* stList_length(poa->nodes) */
    for (int64_t i = 0; i < n; i++)
        if (insert_first[i + 1] < insert_first[i] || delete_first[i + 1] < delete_first[i] || insert_first[i] < 0 || delete_first[i] < 0)
            return mrp_set_error(MRP_ERR_ARG, "%s: node %lld: insert_first or delete_first descends", who, (long long) i);
    if (insert_first[n] > insert_first[0] && (!insert_str_off || !insert_str_len || !insert_weight_forward || !insert_weight_reverse))
        return mrp_set_error(MRP_ERR_ARG, "%s: null insert array", who);
    if (delete_first[n] > delete_first[0] && (!delete_length || !delete_weight_forward || !delete_weight_reverse))
        return mrp_set_error(MRP_ERR_ARG, "%s: null delete array", who);
    for (int64_t i = 0; i < n; i++) {
        for (int64_t j = insert_first[i]; j < insert_first[i + 1]; j++)
            if (insert_str_len[j] < 0 || insert_str_off[j] < 0 || insert_str_off[j] > pool_len - insert_str_len[j] ||
                (insert_str_len[j] > 0 && (!pool_symbols || !pool_counts)))
                return mrp_set_error(MRP_ERR_ARG, "%s: node %lld, insert %lld: its string lies outside the pool", who, (long long) i, (long long) j);
        for (int64_t j = delete_first[i]; j < delete_first[i + 1]; j++)
            if (delete_length[j] < 1 || i + delete_length[j] + 1 > n)
                return mrp_set_error(MRP_ERR_ARG, "%s: node %lld, delete %lld: length %d below 1 or beyond the last node", who, (long long) i, (long long) j,
                                     (int) delete_length[j]);
        if (i > 0 && (base_pick[i] < 0 || base_pick[i] > 4 || repeat_count_pick[i] < 0))
            return mrp_set_error(MRP_ERR_ARG, "%s: node %lld: a pick outside its range", who, (long long) i);
    }
    auto ins_weight = [&](int64_t j) { return insert_weight_forward[j] + insert_weight_reverse[j]; }; /* poaInsert_getWeight */
    auto del_weight = [&](int64_t j) { return delete_weight_forward[j] + delete_weight_reverse[j]; };

    std::vector<double> total_out((size_t) n, 0.0), fwd((size_t) n + 1, POC_LOG_ZERO), match_fwd((size_t) n, 0.0);
    fwd[0] = 0.0;
    /* incoming deletions as a CSR by target node, in the reference's order of appending (:1377-1383) */
    std::vector<int64_t> in_first((size_t) n + 2, 0), in_del, in_src;
    for (int64_t i = 0; i < n; i++)
        for (int64_t j = delete_first[i]; j < delete_first[i + 1]; j++) in_first[(size_t) (i + delete_length[j] + 1) + 1]++;
    for (int64_t i = 0; i <= n; i++) in_first[(size_t) i + 1] += in_first[(size_t) i];
    in_del.resize((size_t) in_first[(size_t) n + 1]);
    in_src.resize(in_del.size());
    {
        std::vector<int64_t> at(in_first.begin(), in_first.end() - 1);
        for (int64_t i = 0; i < n; i++)
            for (int64_t j = delete_first[i]; j < delete_first[i + 1]; j++) {
                const int64_t to = i + delete_length[j] + 1;
                in_del[(size_t) at[(size_t) to]] = j;
                in_src[(size_t) at[(size_t) to]++] = i;
            }
    }
    for (int64_t i = 0; i < n; i++) { /* :1387-1458 */
        double indel = 0.0;
        for (int64_t j = insert_first[i]; j < insert_first[i + 1]; j++) indel += ins_weight(j);
        for (int64_t j = delete_first[i]; j < delete_first[i + 1]; j++) indel += del_weight(j);
        double mt = 0.0;
        if (i == 0) {
            if (n == 1) {
                mt = 1.0;
            } else {
                for (int64_t j = 1; j < n; j++)
                    for (int k = 0; k < 5; k++) mt += base_weight[5 * j + k];
                mt /= (double) n - 1;
                mt -= indel;
            }
        } else {
            for (int k = 0; k < 5; k++) mt += base_weight[5 * i + k];
            mt -= indel;
        }
        mt = mt <= 0.0 ? 0.0001 : mt;
        total_out[(size_t) i] = mt + indel;
        for (int64_t j = insert_first[i]; j < insert_first[i + 1]; j++)
            fwd[(size_t) i + 1] = poc_log_add(fwd[(size_t) i + 1], fwd[(size_t) i] + log(ins_weight(j) / total_out[(size_t) i]));
        for (int64_t j = delete_first[i]; j < delete_first[i + 1]; j++) {
            const size_t to = (size_t) (i + delete_length[j] + 1);
            fwd[to] = poc_log_add(fwd[to], fwd[(size_t) i] + log(del_weight(j) / total_out[(size_t) i]));
        }
        match_fwd[(size_t) i] = fwd[(size_t) i] + log(mt / total_out[(size_t) i]);
        fwd[(size_t) i + 1] = poc_log_add(fwd[(size_t) i + 1], match_fwd[(size_t) i]);
    }
    std::vector<int64_t> cmap((size_t) (n - 1), -1);
    std::vector<uint8_t> back_s; /* the expanded consensus, backwards */
    int64_t running = 0;
    int previous = -1; /* previousBase = '-' */
    auto push = [&](int sym, int64_t count) { back_s.insert(back_s.end(), (size_t) count, (uint8_t) sym); };
    for (int64_t i = n; i > 0;) { /* :1473-1563 */
        if (i < n) {
            const int base = base_pick[i];
            if (use_rle) {
                int64_t count = repeat_count_pick[i];
                count = count == 0 ? 1 : count;
                push(base, count);
                if (previous != base) cmap[(size_t) i - 1] = running++;
                previous = base;
            } else {
                push(base, 1);
                cmap[(size_t) i - 1] = running++;
            }
        }
        double max_ins_p = POC_LOG_ZERO, tot_ins = POC_LOG_ZERO, max_del_p = POC_LOG_ZERO, tot_del = POC_LOG_ZERO;
        int64_t max_ins = -1, max_del = -1;
        for (int64_t j = insert_first[i - 1]; j < insert_first[i]; j++) {
            const double p = log(ins_weight(j) / total_out[(size_t) i - 1]) + fwd[(size_t) i - 1];
            if (p > max_ins_p) {
                max_ins_p = p;
                max_ins = j;
            }
            tot_ins = poc_log_add(tot_ins, p);
        }
        for (int64_t q = in_first[(size_t) i]; q < in_first[(size_t) i + 1]; q++) {
            const int64_t j = in_del[(size_t) q], src = in_src[(size_t) q];
            const double p = log(del_weight(j) / total_out[(size_t) src]) + fwd[(size_t) src];
            if (p > max_del_p) {
                max_del_p = p;
                max_del = j;
            }
            tot_del = poc_log_add(tot_del, p);
        }
        if (match_fwd[(size_t) i - 1] >= tot_del && match_fwd[(size_t) i - 1] >= tot_ins) {
            i--;
        } else if (tot_ins >= tot_del) {
            if (max_ins < 0) return mrp_set_error(MRP_ERR_ARG, "%s: node %lld: no maximal insert (the reference dereferences NULL)", who, (long long) (i - 1));
            const int64_t off = insert_str_off[max_ins], len = insert_str_len[max_ins];
            if (len < 1) return mrp_set_error(MRP_ERR_ARG, "%s: node %lld: the chosen insert is empty", who, (long long) (i - 1));
            int64_t expanded = 0;
            for (int64_t q = 0; q < len; q++) {
                if (pool_symbols[off + q] > 4 || pool_counts[off + q] < 0)
                    return mrp_set_error(MRP_ERR_ARG, "%s: node %lld: the chosen insert holds a symbol above 4 or a negative count", who, (long long) (i - 1));
                expanded += pool_counts[off + q];
            }
            for (int64_t q = len - 1; q >= 0; q--) push(pool_symbols[off + q], pool_counts[off + q]); /* rleString_expand, backwards */
            if (use_rle) {
                const int base = pool_symbols[off + len - 1];
                running += len + (base != previous ? 0 : -1);
                previous = pool_symbols[off];
            } else {
                running += expanded;
            }
            i--;
        } else {
            if (max_del < 0) return mrp_set_error(MRP_ERR_ARG, "%s: node %lld: no maximal delete (the reference dereferences NULL)", who, (long long) i);
            i -= delete_length[max_del] + 1;
        }
    }
    /* rleString_construct (rle.c:8-38) or rleString_construct_no_rle of the expanded string */
    std::vector<uint8_t> sym;
    std::vector<int32_t> cnt;
    for (size_t q = back_s.size(); q-- > 0;) {
        if (use_rle && !sym.empty() && sym.back() == back_s[q]) {
            cnt.back()++;
        } else {
            sym.push_back(back_s[q]);
            cnt.push_back(1);
        }
    }
    const int64_t length = (int64_t) sym.size();
    for (int64_t k = 0; k < n - 1; k++) /* :1573-1578 */
        if (cmap[(size_t) k] != -1) cmap[(size_t) k] = length - 1 - cmap[(size_t) k];
    uint8_t *so = (uint8_t *) malloc((size_t) (length > 0 ? length : 1));
    int32_t *co = (int32_t *) malloc((size_t) (length > 0 ? length : 1) * sizeof(int32_t));
    int64_t *mo = (int64_t *) malloc((size_t) (n > 1 ? n - 1 : 1) * sizeof(int64_t));
    if (!so || !co || !mo) {
        free(so);
        free(co);
        free(mo);
        return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    }
    if (length > 0) {
        memcpy(so, sym.data(), (size_t) length);
        memcpy(co, cnt.data(), (size_t) length * sizeof(int32_t));
    }
    if (n > 1) memcpy(mo, cmap.data(), (size_t) (n - 1) * sizeof(int64_t));
    *symbols_out = so;
    *counts_out = co;
    *length_out = length;
    *poa_to_consensus_map_out = mo;
    return MRP_OK;
}
