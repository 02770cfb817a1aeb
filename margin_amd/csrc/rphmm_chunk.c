/*
 * rphmm_chunk.c -- the per-chunk ("hashing") host path of libmargin_rphmm.so, in C as the reference's host code is.
 *
 * The structural stRPHmm operations of impl/hmm.c, column.c, mergeColumn.c, coordination.c and the phasing driver
 * bubbleGraph.c:2673-2801, on ONE flat structure-of-arrays hmm (struct mrp_hmm, rphmm_common.h) whose arrays are
 * exactly the arrays of mrp_hmm_job: cells are rows of (partition, next, prev), merge cells rows of (from, to),
 * transitions are indices instead of hash lookups.  Nothing is flattened before a sweep; the device batch is a memcpy
 * of these arrays.  Cross products are built on the host by hashing, every forward/backward sweep runs on the GPU via
 * mrp_fb_run / mrp_batch_* (one device sweep per recursion level; there is no CPU sweep), the prune is on the host.
 *
 * This is the path behind mrp_phase_reads, mrp_get_rp_hmms and the mrp_hmm_* entry points.  mrp_phase_reads_many
 * uses it for chunks the device-resident path (rphmm_host.c) cannot take, about 100x slower per chunk, and the tests
 * use it as a second opinion.  Plain heap allocation throughout.
 *
 * Order conventions (DESIGN.md "Order semantics"): cell order is the reference's list order;
 * merge cells keep creation order; stList_sort2 is taken to be stable; stHash/stSet iteration
 * (address dependent in the reference) is creation order.
 */
#define _GNU_SOURCE
#include "rphmm_common.h"

static inline uint64_t mix64(uint64_t x) {
    x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
    return x;
}
/* uint64 -> uint32 open-addressing map (stands in for the stHash of mergeColumn.c:27-31) */
typedef struct { uint64_t *k; uint32_t *v; uint64_t mask; } u64map;
#define U64MAP_EMPTY 0xFFFFFFFFu
static void u64map_init(u64map *m, int64_t expect) {
    uint64_t cap = 16;
    while (cap < (uint64_t) expect * 2) cap *= 2;
    m->mask = cap - 1;
    m->k = xmalloc(sizeof(uint64_t) * cap);
    m->v = xmalloc(sizeof(uint32_t) * cap);
    memset(m->v, 0xFF, sizeof(uint32_t) * cap);
}
static void u64map_free(u64map *m) { free(m->k); free(m->v); m->k = NULL; m->v = NULL; }
static inline uint32_t u64map_get(const u64map *m, uint64_t key) {
    uint64_t i = mix64(key) & m->mask;
    while (m->v[i] != U64MAP_EMPTY) {
        if (m->k[i] == key) return m->v[i];
        i = (i + 1) & m->mask;
    }
    return U64MAP_EMPTY;
}
static inline void u64map_put(u64map *m, uint64_t key, uint32_t val) { /* caller sized the map */
    uint64_t i = mix64(key) & m->mask;
    while (m->v[i] != U64MAP_EMPTY) {
        if (m->k[i] == key) { m->v[i] = val; return; }
        i = (i + 1) & m->mask;
    }
    m->k[i] = key; m->v[i] = val;
}

/* partitions.c */
static inline uint64_t accept_mask(int64_t depth) { /* :13-19 */
    return depth < 64 ? ~(0xFFFFFFFFFFFFFFFFULL << depth) : 0xFFFFFFFFFFFFFFFFULL;
}
static inline uint64_t merge_bits(uint64_t p1, uint64_t p2, int64_t d1) { /* :21-28 */
    return d1 < 64 ? ((p2 << d1) | p1) : p1;
}
static inline uint64_t invert_partition(uint64_t p, int64_t depth) { return accept_mask(depth) & ~p; } /* :37-42 */

/* begin a column; cells are appended afterwards */
static void hmm_begin_column(mrp_hmm *h, const world *w, int32_t start, int32_t len, int32_t depth,
                             const int32_t *col_reads) {
    VEC_PUSH(h->col_start, start);
    VEC_PUSH(h->col_len, len);
    VEC_PUSH(h->col_depth, depth);
    for (int32_t i = 0; i < depth; i++) {
        VEC_PUSH(h->col_reads, col_reads[i]);
        VEC_PUSH(h->read_byte_off, read_byte_offset(w, col_reads[i], start));
    }
    if (depth > h->max_depth) h->max_depth = depth;
}
static void hmm_end_column(mrp_hmm *h) {
    VEC_PUSH(h->cell_off, h->part.n);
    VEC_PUSH(h->read_off, h->col_reads.n);
}
static void hmm_begin_merge(mrp_hmm *h, uint64_t mask_from, uint64_t mask_to) {
    VEC_PUSH(h->mask_from, mask_from);
    VEC_PUSH(h->mask_to, mask_to);
}
static void hmm_end_merge(mrp_hmm *h) { VEC_PUSH(h->mcell_off, h->mfrom.n); }

/* stRPHmm_construct hmm.c:97-133: one column, cells {1, 0} */
static mrp_hmm *hmm_from_read(const world *w, int32_t read) {
    mrp_hmm *h = hmm_new();
    const mrp_read *r = &w->reads[read];
    h->ref_start = r->ref_start;
    h->ref_length = r->length;
    VEC_PUSH(h->reads, read);
    hmm_begin_column(h, w, r->ref_start, r->length, 1, &read);
    hmm_add_cell(h, 1, 0);
    hmm_add_cell(h, 0, 0);
    hmm_end_column(h);
    return h;
}

#define HMM_T mrp_hmm
#define PFX(x) x
#define H_NAME_READ(h) ((h)->reads.n > 0 ? (h)->reads.a[0] : -1)
#include "rphmm_paths.inc"
#undef HMM_T
#undef PFX
#undef H_NAME_READ

/* ------------------------------------------------------------------------------------------ */
/* fuse + align + cross product in one pass                                                    */
/* ------------------------------------------------------------------------------------------ */
/* A piece is a column of a source hmm (or a gap) restricted to a site interval; a connector is
 * the merge column that leads out of it.  stRPHmm_fuse (hmm.c:283-372) contributes ZERO
 * connectors and gap pieces, stRPHmm_alignColumns (hmm.c:374-507) the prefix/suffix gaps and,
 * through stRPColumn_split (column.c:70-130), the IDENT connectors. */
typedef enum { CONN_NONE = 0, CONN_REAL, CONN_ZERO, CONN_IDENT } conn_kind;
typedef struct {
    const mrp_hmm *h; /* NULL = gap column (depth 0, one cell, partition 0) */
    int32_t k;        /* column in h */
    int32_t start, len;
    conn_kind out;    /* connector to the next piece */
} piece;
typedef VEC(piece) piece_vec;

static void pieces_of_path(const hmm_vec *tp, int32_t S, int32_t E, piece_vec *out) {
    int32_t pos = S;
    for (int64_t i = 0; i < tp->n; i++) {
        const mrp_hmm *h = tp->a[i];
        if (h->ref_start > pos) { /* gap (hmm.c:335-359, :396-424) */
            piece g = {NULL, 0, pos, h->ref_start - pos, CONN_ZERO};
            VEC_PUSH(*out, g);
        }
        const int64_t K = hmm_K(h);
        for (int64_t k = 0; k < K; k++) {
            piece p = {h, (int32_t) k, h->col_start.a[k], h->col_len.a[k], k + 1 < K ? CONN_REAL : CONN_ZERO};
            VEC_PUSH(*out, p);
        }
        pos = h->ref_start + h->ref_length;
    }
    if (pos < E) { /* suffix gap (hmm.c:435-462) */
        piece g = {NULL, 0, pos, E - pos, CONN_ZERO};
        VEC_PUSH(*out, g);
    }
    out->a[out->n - 1].out = CONN_NONE;
}
/* cut both piece lists at the union of their boundaries (hmm.c:476-504) */
static void align_pieces(const piece_vec *a, const piece_vec *b, piece_vec *oa, piece_vec *ob) {
    int64_t i = 0, j = 0;
    piece pa = a->a[0], pb = b->a[0];
    while (1) {
        const int32_t len = pa.len < pb.len ? pa.len : pb.len;
        piece ca = pa, cb = pb;
        ca.len = len; cb.len = len;
        if (pa.len > len) ca.out = CONN_IDENT;
        if (pb.len > len) cb.out = CONN_IDENT;
        VEC_PUSH(*oa, ca);
        VEC_PUSH(*ob, cb);
        if (pa.len > len) { pa.start += len; pa.len -= len; } else { i++; if (i < a->n) pa = a->a[i]; }
        if (pb.len > len) { pb.start += len; pb.len -= len; } else { j++; if (j < b->n) pb = b->a[j]; }
        if (i >= a->n || j >= b->n) break;
    }
}

static const uint64_t ZERO_PART[1] = {0};
static inline int64_t piece_cells(const piece *p) { return p->h ? p->h->cell_off.a[p->k + 1] - p->h->cell_off.a[p->k] : 1; }
static inline const uint64_t *piece_parts(const piece *p) { return p->h ? p->h->part.a + p->h->cell_off.a[p->k] : ZERO_PART; }
static inline int32_t piece_depth(const piece *p) { return p->h ? p->h->col_depth.a[p->k] : 0; }
static inline const int32_t *piece_reads(const piece *p) { return p->h ? p->h->col_reads.a + p->h->read_off.a[p->k] : NULL; }

/* connector accessors */
typedef struct {
    uint64_t mask_from, mask_to;
    int64_t M;
    const uint64_t *from, *to;
} conn_view;
static void conn_of(const piece *p, conn_view *c) {
    switch (p->out) {
        case CONN_REAL: {
            const mrp_hmm *h = p->h;
            c->mask_from = h->mask_from.a[p->k]; c->mask_to = h->mask_to.a[p->k];
            c->M = h->mcell_off.a[p->k + 1] - h->mcell_off.a[p->k];
            c->from = h->mfrom.a + h->mcell_off.a[p->k]; c->to = h->mto.a + h->mcell_off.a[p->k];
            break;
        }
        case CONN_IDENT: { /* column.c:86-101 */
            c->mask_from = c->mask_to = accept_mask(piece_depth(p));
            c->M = piece_cells(p);
            c->from = c->to = piece_parts(p);
            break;
        }
        default: /* ZERO: hmm.c:324-331 */
            c->mask_from = c->mask_to = 0; c->M = 1; c->from = c->to = ZERO_PART;
    }
}

/* stRPHmm_createCrossProductOfTwoAlignedHmm hmm.c:534-750 over two aligned piece lists */
static mrp_hmm *cross_product(const world *w, const piece_vec *A, const piece_vec *B, const hmm_vec *tpA,
                              const hmm_vec *tpB, const mrp_params *params, int32_t S, int32_t E) {
    mrp_hmm *h = hmm_new();
    h->ref_start = S; h->ref_length = E - S;
    for (int64_t i = 0; i < tpA->n; i++) for (int64_t r = 0; r < tpA->a[i]->reads.n; r++) VEC_PUSH(h->reads, tpA->a[i]->reads.a[r]);
    for (int64_t i = 0; i < tpB->n; i++) for (int64_t r = 0; r < tpB->a[i]->reads.n; r++) VEC_PUSH(h->reads, tpB->a[i]->reads.a[r]);
    const int inv = params->include_inverted_partitions != 0;
    const int64_t n = A->n;
    u64map prev_to = {0}; /* toPartition -> merge index of the merge column before the current column */
    int have_prev = 0;
    uint64_t prev_mask_to = 0;
    int32_t colreads[MRP_MAX_READ_PARTITIONING_DEPTH];
    for (int64_t s = 0; s < n; s++) {
        const piece *pa = &A->a[s], *pb = &B->a[s];
        const int32_t d1 = piece_depth(pa), d2 = piece_depth(pb), depth = d1 + d2;
        if (depth > MRP_MAX_READ_PARTITIONING_DEPTH) {
            mrp_hmm_destroy(h); u64map_free(&prev_to);
            mrp_set_error(MRP_ERR_ARG, "cross product column depth %d exceeds %d", depth, MRP_MAX_READ_PARTITIONING_DEPTH);
            return NULL;
        }
        if (d1) memcpy(colreads, piece_reads(pa), sizeof(int32_t) * (size_t) d1);
        if (d2) memcpy(colreads + d1, piece_reads(pb), sizeof(int32_t) * (size_t) d2);
        hmm_begin_column(h, w, pa->start, pa->len, depth, colreads);
        const int64_t C1 = piece_cells(pa), C2 = piece_cells(pb);
        const uint64_t *P1 = piece_parts(pa), *P2 = piece_parts(pb);
        const int64_t cell0 = h->part.n;
        VEC_RESERVE(h->part, 2 * C1 * C2); VEC_RESERVE(h->prev, 2 * C1 * C2); VEC_RESERVE(h->next, 2 * C1 * C2);
        if (inv) { /* hmm.c:627-655 */
            u64map seen; u64map_init(&seen, 2 * C1 * C2);
            for (int64_t c1 = 0; c1 < C1; c1++)
                for (int64_t c2 = 0; c2 < C2; c2++) {
                    const uint64_t p = merge_bits(P1[c1], P2[c2], d1);
                    if (u64map_get(&seen, p) == U64MAP_EMPTY) {
                        u64map_put(&seen, p, 1);
                        hmm_add_cell(h, p, 0);
                        if (depth > 0) {
                            const uint64_t ip = invert_partition(p, depth);
                            u64map_put(&seen, ip, 1);
                            hmm_add_cell(h, ip, 0);
                        }
                    }
                }
            u64map_free(&seen);
        } else { /* hmm.c:657-668 */
            for (int64_t c1 = 0; c1 < C1; c1++)
                for (int64_t c2 = 0; c2 < C2; c2++) hmm_add_cell(h, merge_bits(P1[c1], P2[c2], d1), 0);
        }
        hmm_end_column(h);
        const int64_t nC = h->part.n - cell0;
        /* link to the previous merge column (mergeColumn.c:72-79) */
        if (have_prev) {
            for (int64_t c = 0; c < nC; c++) {
                const uint32_t m = u64map_get(&prev_to, h->part.a[cell0 + c] & prev_mask_to);
                if (m == U64MAP_EMPTY) {
                    mrp_hmm_destroy(h); u64map_free(&prev_to);
                    mrp_set_error(MRP_ERR_LOOKUP, "cross product: cell without previous merge cell");
                    return NULL;
                }
                h->prev.a[cell0 + c] = m;
            }
            u64map_free(&prev_to);
            have_prev = 0;
        }
        if (s + 1 == n) break;
        /* merge column hmm.c:686-740 */
        conn_view ca, cb;
        conn_of(pa, &ca); conn_of(pb, &cb);
        const int32_t d1n = piece_depth(&A->a[s + 1]), d2n = piece_depth(&B->a[s + 1]);
        const uint64_t from_mask = merge_bits(ca.mask_from, cb.mask_from, d1);
        const uint64_t to_mask = merge_bits(ca.mask_to, cb.mask_to, d1n);
        hmm_begin_merge(h, from_mask, to_mask);
        const int64_t m0 = h->mfrom.n;
        u64map from_map; u64map_init(&from_map, 2 * ca.M * cb.M);
        u64map_init(&prev_to, 2 * ca.M * cb.M);
        for (int64_t i = 0; i < ca.M; i++)
            for (int64_t j = 0; j < cb.M; j++) {
                const uint64_t from = merge_bits(ca.from[i], cb.from[j], d1);
                const uint64_t to = merge_bits(ca.to[i], cb.to[j], d1n);
                if (inv) {
                    if (u64map_get(&from_map, from) == U64MAP_EMPTY) {
                        u64map_put(&from_map, from, (uint32_t) (h->mfrom.n - m0));
                        u64map_put(&prev_to, to, (uint32_t) (h->mfrom.n - m0));
                        VEC_PUSH(h->mfrom, from); VEC_PUSH(h->mto, to);
                        if (__builtin_popcountll(from_mask) > 0) {
                            const uint64_t ifrom = from_mask & invert_partition(from, d1 + d2);
                            const uint64_t ito = to_mask & invert_partition(to, d1n + d2n);
                            u64map_put(&from_map, ifrom, (uint32_t) (h->mfrom.n - m0));
                            u64map_put(&prev_to, ito, (uint32_t) (h->mfrom.n - m0));
                            VEC_PUSH(h->mfrom, ifrom); VEC_PUSH(h->mto, ito);
                        }
                    }
                } else {
                    u64map_put(&from_map, from, (uint32_t) (h->mfrom.n - m0));
                    u64map_put(&prev_to, to, (uint32_t) (h->mfrom.n - m0));
                    VEC_PUSH(h->mfrom, from); VEC_PUSH(h->mto, to);
                }
            }
        hmm_end_merge(h);
        /* link this column's cells to it (mergeColumn.c:63-70) */
        for (int64_t c = 0; c < nC; c++) {
            const uint32_t m = u64map_get(&from_map, h->part.a[cell0 + c] & from_mask);
            if (m == U64MAP_EMPTY) {
                mrp_hmm_destroy(h); u64map_free(&from_map); u64map_free(&prev_to);
                mrp_set_error(MRP_ERR_LOOKUP, "cross product: cell without next merge cell");
                return NULL;
            }
            h->next.a[cell0 + c] = m;
        }
        u64map_free(&from_map);
        have_prev = 1;
        prev_mask_to = to_mask;
    }
    return h;
}

/* fuseTilingPath coordination.c:244-261 without a partner: concatenate hmms with ZERO connectors
 * and gap columns (hmm.c:283-372). */
static mrp_hmm *fuse_path(const world *w, const hmm_vec *tp) {
    if (tp->n == 1) return tp->a[0];
    mrp_hmm *h = hmm_new();
    h->ref_start = tp->a[0]->ref_start;
    h->ref_length = tp->a[tp->n - 1]->ref_start + tp->a[tp->n - 1]->ref_length - h->ref_start;
    piece_vec ps = {0};
    pieces_of_path(tp, h->ref_start, h->ref_start + h->ref_length, &ps);
    for (int64_t i = 0; i < tp->n; i++) for (int64_t r = 0; r < tp->a[i]->reads.n; r++) VEC_PUSH(h->reads, tp->a[i]->reads.a[r]);
    for (int64_t s = 0; s < ps.n; s++) {
        const piece *p = &ps.a[s];
        hmm_begin_column(h, w, p->start, p->len, piece_depth(p), piece_reads(p));
        const int64_t C = piece_cells(p);
        const uint64_t *P = piece_parts(p);
        const int real_prev = s > 0 && ps.a[s - 1].out == CONN_REAL;
        const int real_next = p->out == CONN_REAL;
        for (int64_t c = 0; c < C; c++) {
            hmm_add_cell(h, P[c], real_prev ? p->h->prev.a[p->h->cell_off.a[p->k] + c] : 0);
            h->next.a[h->next.n - 1] = real_next ? p->h->next.a[p->h->cell_off.a[p->k] + c] : 0;
        }
        hmm_end_column(h);
        if (p->out == CONN_NONE) break;
        conn_view cv; conn_of(p, &cv);
        hmm_begin_merge(h, cv.mask_from, cv.mask_to);
        for (int64_t m = 0; m < cv.M; m++) { VEC_PUSH(h->mfrom, cv.from[m]); VEC_PUSH(h->mto, cv.to[m]); }
        hmm_end_merge(h);
    }
    free(ps.a);
    for (int64_t i = 0; i < tp->n; i++) mrp_hmm_destroy(tp->a[i]);
    return h;
}

/* ------------------------------------------------------------------------------------------ */
/* sweeps on the device                                                                        */
/* ------------------------------------------------------------------------------------------ */
static void hmm_alloc_results(mrp_hmm *h) {
    hmm_free_results(h);
    const int64_t K = hmm_K(h);
    h->f = xmalloc(sizeof(double) * (size_t) h->part.n);
    h->b = xmalloc(sizeof(double) * (size_t) h->part.n);
    h->mf = xmalloc(sizeof(double) * (size_t) (h->mfrom.n + 1));
    h->mb = xmalloc(sizeof(double) * (size_t) (h->mfrom.n + 1));
    h->total = xmalloc(sizeof(double) * (size_t) K);
    h->has_results = 1;
}
static void hmm_job(const world *w, mrp_hmm *h, uint32_t flags, mrp_hmm_job *j, int with_outputs) {
    memset(j, 0, sizeof(*j));
    j->chunk = w->chunk;
    j->n_columns = (int32_t) hmm_K(h);
    j->flags = flags;
    j->col_ref_start = h->col_start.a; j->col_length = h->col_len.a; j->col_depth = h->col_depth.a;
    j->col_cell_off = h->cell_off.a; j->col_read_off = h->read_off.a; j->read_byte_off = h->read_byte_off.a;
    j->partition = h->part.a; j->mask_from = h->mask_from.a; j->mask_to = h->mask_to.a;
    j->mcol_cell_off = h->mcell_off.a; j->merge_from = h->mfrom.a; j->merge_to = h->mto.a;
    j->cell_next = h->next.a; j->cell_prev = h->prev.a;
    if (with_outputs) {
        j->cell_forward = h->f; j->cell_backward = h->b; j->merge_forward = h->mf; j->merge_backward = h->mb;
        j->col_total = h->total; j->hmm_forward = &h->fwd; j->hmm_backward = &h->bwd;
    }
}
/* stRPHmm_forwardBackward for a set of independent hmms: one device batch */
static int sweep_many(world *w, mrp_hmm **hmms, int64_t n, const mrp_params *params) {
    if (n == 0) return MRP_OK;
    const uint32_t flags = sweep_flags(params);
    mrp_hmm_job *jobs = xcalloc((size_t) n, sizeof(*jobs));
    for (int64_t i = 0; i < n; i++) {
        hmm_alloc_results(hmms[i]);
        hmm_job(w, hmms[i], flags, &jobs[i], 1);
    }
    int rc = mrp_fb_run(w->ctx, n, jobs);
    if (rc == MRP_OK && w->record) {
        for (int64_t i = 0; rc == MRP_OK && i < n; i++) {
            mrp_hmm_job dj;
            hmm_job(w, hmms[i], flags, &dj, 0);
            rc = mrp_batch_add(w->record, &dj);
        }
    }
    w->n_sweeps += n;
    free(jobs);
    return rc;
}

/* ------------------------------------------------------------------------------------------ */
/* prune (hmm.c:944-1163)                                                                      */
/* ------------------------------------------------------------------------------------------ */
static int posterior(double f, double b, double total, double limit, double *out) { /* column.c:177-193, mergeColumn.c:129-146 */
    const double p = exp(f + b - total);
    if (p > limit || p < 0.0) return mrp_set_error(MRP_ERR_ARG, "ERROR: invalid prob %f", p);
    *out = p > 1.0 ? 1.0 : p;
    return MRP_OK;
}

int mrp_hmm_prune(mrp_hmm *h, const mrp_params *P) {
    if (!h || !P) return mrp_set_error(MRP_ERR_ARG, "mrp_hmm_prune: NULL argument");
    if (!h->has_results) return mrp_set_error(MRP_ERR_ARG, "mrp_hmm_prune before a forward/backward sweep");
    const int64_t K = hmm_K(h);
    int64_t max_c = 1, max_m = 1;
    for (int64_t k = 0; k < K; k++) {
        const int64_t c = h->cell_off.a[k + 1] - h->cell_off.a[k];
        if (c > max_c) max_c = c;
        if (k + 1 < K) { const int64_t m = h->mcell_off.a[k + 1] - h->mcell_off.a[k]; if (m > max_m) max_m = m; }
    }
    /* kept cells per column (old cell indices, new order) and kept-flag per merge cell */
    int64_t *keep_off = xmalloc(sizeof(int64_t) * (size_t) (K + 1));
    int64_t *keep_idx = xmalloc(sizeof(int64_t) * (size_t) (h->part.n + 1));
    uint8_t *keep_m = xcalloc((size_t) (h->mfrom.n + 1), 1);
    keyed *ka = xmalloc(sizeof(keyed) * (size_t) (max_c > max_m ? max_c : max_m));
    keyed *kt = xmalloc(sizeof(keyed) * (size_t) (max_c > max_m ? max_c : max_m));
    uint8_t *chosen = xmalloc((size_t) max_m);
    int rc = MRP_OK;
    /* stRPHmm_pruneForwards hmm.c:1049-1109 */
    keep_off[0] = 0;
    for (int64_t k = 0; k < K && rc == MRP_OK; k++) {
        const int64_t c0 = h->cell_off.a[k], nc = h->cell_off.a[k + 1] - c0;
        int64_t n = 0;
        for (int64_t c = 0; c < nc; c++) { /* getLinkedCells :1021-1047 */
            if (k > 0 && !keep_m[h->mcell_off.a[k - 1] + h->prev.a[c0 + c]]) continue;
            ka[n].idx = c;
            rc = posterior(h->f[c0 + c], h->b[c0 + c], h->total[k], 1.1, &ka[n].key);
            if (rc != MRP_OK) break;
            n++;
        }
        if (rc != MRP_OK) break;
        keyed_sort_desc(ka, n, kt);
        while (n > P->min_partitions_in_a_column &&
               (n > P->max_partitions_in_a_column || ka[n - 1].key < P->min_posterior_probability_for_partition))
            n--;
        for (int64_t i = 0; i < n; i++) keep_idx[keep_off[k] + i] = ka[i].idx;
        keep_off[k + 1] = keep_off[k] + n;
        if (k + 1 == K) break;
        /* getLinkedMergeCells :989-1004, sort + shrink :1088-1101 */
        const int64_t m0 = h->mcell_off.a[k], nm = h->mcell_off.a[k + 1] - m0;
        memset(chosen, 0, (size_t) nm);
        int64_t mn = 0;
        for (int64_t i = 0; i < n; i++) {
            const uint32_t m = h->next.a[c0 + keep_idx[keep_off[k] + i]];
            if (!chosen[m]) {
                chosen[m] = 1;
                ka[mn].idx = m;
                rc = posterior(h->mf[m0 + m], h->mb[m0 + m], h->total[k + 1], 1.001, &ka[mn].key);
                if (rc != MRP_OK) break;
                mn++;
            }
        }
        if (rc != MRP_OK) break;
        keyed_sort_desc(ka, mn, kt);
        while (mn > P->min_partitions_in_a_column &&
               (mn > P->max_partitions_in_a_column || ka[mn - 1].key < P->min_posterior_probability_for_partition))
            mn--;
        for (int64_t i = 0; i < mn; i++) keep_m[m0 + ka[i].idx] = 1;
    }
    /* stRPHmm_pruneBackwards hmm.c:1111-1158 */
    for (int64_t k = K - 1; k >= 0 && rc == MRP_OK; k--) {
        const int64_t c0 = h->cell_off.a[k];
        int64_t n = 0;
        for (int64_t i = keep_off[k]; i < keep_off[k + 1]; i++) {
            const int64_t c = keep_idx[i];
            if (k + 1 < K && !keep_m[h->mcell_off.a[k] + h->next.a[c0 + c]]) continue;
            keep_idx[keep_off[k] + n++] = c; /* order kept: the re-sort of an already sorted list is a no-op */
        }
        /* entries past the new length are marked unused */
        for (int64_t i = keep_off[k] + n; i < keep_off[k + 1]; i++) keep_idx[i] = -1;
        if (k == 0) break;
        const int64_t m0 = h->mcell_off.a[k - 1], nm = h->mcell_off.a[k] - m0;
        memset(chosen, 0, (size_t) nm);
        for (int64_t i = 0; i < n; i++) chosen[h->prev.a[c0 + keep_idx[keep_off[k] + i]]] = 1;
        for (int64_t m = 0; m < nm; m++) keep_m[m0 + m] = keep_m[m0 + m] && chosen[m];
    }
    if (rc == MRP_OK) {
        /* rebuild compactly: merge cells keep their relative order (filterMergeCells :964-987),
         * cells are relinked in sorted order (relinkCells :1006-1019) */
        uint32_t *remap = xmalloc(sizeof(uint32_t) * (size_t) (h->mfrom.n + 1));
        int64_t nm_new = 0;
        int64_t *new_moff = xmalloc(sizeof(int64_t) * (size_t) K);
        new_moff[0] = 0;
        for (int64_t k = 0; k + 1 < K; k++) {
            const int64_t m0 = h->mcell_off.a[k], nm = h->mcell_off.a[k + 1] - m0;
            uint32_t local = 0;
            for (int64_t m = 0; m < nm; m++) {
                if (keep_m[m0 + m]) {
                    remap[m0 + m] = local++;
                    h->mfrom.a[nm_new] = h->mfrom.a[m0 + m];
                    h->mto.a[nm_new] = h->mto.a[m0 + m];
                    h->mf[nm_new] = h->mf[m0 + m];
                    h->mb[nm_new] = h->mb[m0 + m];
                    nm_new++;
                } else remap[m0 + m] = U64MAP_EMPTY;
            }
            new_moff[k + 1] = nm_new;
        }
        const int64_t nC_old = h->part.n;
        uint64_t *np = xmalloc(sizeof(uint64_t) * (size_t) (nC_old + 1));
        uint32_t *nn = xmalloc(sizeof(uint32_t) * (size_t) (nC_old + 1)), *npv = xmalloc(sizeof(uint32_t) * (size_t) (nC_old + 1));
        double *nf = xmalloc(sizeof(double) * (size_t) (nC_old + 1)), *nb = xmalloc(sizeof(double) * (size_t) (nC_old + 1));
        int64_t o = 0;
        int64_t *new_coff = xmalloc(sizeof(int64_t) * (size_t) (K + 1));
        new_coff[0] = 0;
        for (int64_t k = 0; k < K; k++) {
            const int64_t c0 = h->cell_off.a[k];
            for (int64_t i = keep_off[k]; i < keep_off[k + 1]; i++) {
                const int64_t c = keep_idx[i];
                if (c < 0) break;
                np[o] = h->part.a[c0 + c];
                nn[o] = k + 1 < K ? remap[h->mcell_off.a[k] + h->next.a[c0 + c]] : 0;
                npv[o] = k > 0 ? remap[h->mcell_off.a[k - 1] + h->prev.a[c0 + c]] : 0;
                nf[o] = h->f[c0 + c]; nb[o] = h->b[c0 + c];
                o++;
            }
            new_coff[k + 1] = o;
        }
        memcpy(h->part.a, np, sizeof(uint64_t) * (size_t) o);
        memcpy(h->next.a, nn, sizeof(uint32_t) * (size_t) o);
        memcpy(h->prev.a, npv, sizeof(uint32_t) * (size_t) o);
        memcpy(h->f, nf, sizeof(double) * (size_t) o);
        memcpy(h->b, nb, sizeof(double) * (size_t) o);
        h->part.n = h->next.n = h->prev.n = o;
        h->mfrom.n = h->mto.n = nm_new;
        memcpy(h->cell_off.a, new_coff, sizeof(int64_t) * (size_t) (K + 1));
        memcpy(h->mcell_off.a, new_moff, sizeof(int64_t) * (size_t) K);
        free(remap); free(new_moff); free(np); free(nn); free(npv); free(nf); free(nb); free(new_coff);
    }
    free(keep_off); free(keep_idx); free(keep_m); free(ka); free(kt); free(chosen);
    return rc;
}

/* ------------------------------------------------------------------------------------------ */
/* coordination.c                                                                              */
/* ------------------------------------------------------------------------------------------ */
/* mergeTwoTilingPaths coordination.c:263-339.  All cross products of the call are swept in one
 * device batch (the components are independent), then pruned. */
static int merge_two_tiling_paths(world *w, hmm_vec *tp1, hmm_vec *tp2, const mrp_params *params, hmm_vec **out) {
    comp_vec comps = overlapping_components(w, tp1, tp2);
    free(tp1->a); free(tp1); free(tp2->a); free(tp2);
    hmm_vec *res = xcalloc(1, sizeof(*res));
    hmm_vec crossed = {0};
    int rc = MRP_OK;
    for (int64_t i = 0; i < comps.n; i++) {
        component *comp = comps.a[i];
        if (rc == MRP_OK) {
            path_vec sub = tiling_paths_from(w, comp->members.a, comp->members.n);
            if (sub.n == 2) {
                hmm_vec *a = sub.a[0], *b = sub.a[1];
                int32_t S = a->a[0]->ref_start < b->a[0]->ref_start ? a->a[0]->ref_start : b->a[0]->ref_start;
                int32_t Ea = a->a[a->n - 1]->ref_start + a->a[a->n - 1]->ref_length;
                int32_t Eb = b->a[b->n - 1]->ref_start + b->a[b->n - 1]->ref_length;
                int32_t E = Ea > Eb ? Ea : Eb;
                piece_vec pa = {0}, pb = {0}, qa = {0}, qb = {0};
                pieces_of_path(a, S, E, &pa);
                pieces_of_path(b, S, E, &pb);
                align_pieces(&pa, &pb, &qa, &qb);
                mrp_hmm *x = cross_product(w, &qa, &qb, a, b, params, S, E);
                free(pa.a); free(pb.a); free(qa.a); free(qb.a);
                for (int64_t t = 0; t < a->n; t++) mrp_hmm_destroy(a->a[t]);
                for (int64_t t = 0; t < b->n; t++) mrp_hmm_destroy(b->a[t]);
                if (x) { VEC_PUSH(crossed, x); VEC_PUSH(*res, x); } else rc = MRP_ERR_ARG;
            } else if (sub.n == 1 && sub.a[0]->n == 1) {
                VEC_PUSH(*res, sub.a[0]->a[0]);
            } else {
                rc = mrp_set_error(MRP_ERR_ARG, "overlap component with %lld tiling paths", (long long) sub.n);
            }
            for (int64_t t = 0; t < sub.n; t++) { free(sub.a[t]->a); free(sub.a[t]); }
            free(sub.a);
        }
        free(comp->members.a); free(comp);
    }
    free(comps.a);
    if (rc == MRP_OK) rc = sweep_many(w, crossed.a, crossed.n, params);       /* coordination.c:312 */
    for (int64_t i = 0; rc == MRP_OK && i < crossed.n; i++) rc = mrp_hmm_prune(crossed.a[i], params); /* :313 */
    free(crossed.a);
    if (rc == MRP_OK) sort_hmms(w, res->a, res->n);                           /* :336 */
    *out = res;
    return rc;
}

static void free_path(hmm_vec *tp, int destroy_hmms) {
    if (!tp) return;
    if (destroy_hmms) for (int64_t i = 0; i < tp->n; i++) mrp_hmm_destroy(tp->a[i]);
    free(tp->a); free(tp);
}

/* mergeTilingPaths coordination.c:341-409 */
static int merge_tiling_paths(world *w, hmm_vec **paths, int64_t n, const mrp_params *params, hmm_vec **out) {
    if (n == 0) { *out = xcalloc(1, sizeof(hmm_vec)); return MRP_OK; }
    if (n == 1) { *out = paths[0]; return MRP_OK; }
    hmm_vec *tp1 = NULL, *tp2 = NULL;
    int rc = MRP_OK;
    if (n > 2) {
        rc = merge_tiling_paths(w, paths, n / 2, params, &tp1);
        if (rc == MRP_OK) rc = merge_tiling_paths(w, paths + n / 2, n - n / 2, params, &tp2);
        else for (int64_t i = n / 2; i < n; i++) free_path(paths[i], 1);
        if (rc != MRP_OK) { free_path(tp1, 1); free_path(tp2, 1); *out = NULL; return rc; }
    } else {
        tp1 = paths[0]; tp2 = paths[1];
    }
    return merge_two_tiling_paths(w, tp1, tp2, params, out);
}

static path_vec tiling_paths2(const world *w, const int32_t *read_index, int64_t n) { /* coordination.c:224-242 */
    mrp_hmm **hmms = xmalloc(sizeof(*hmms) * (size_t) (n + 1));
    for (int64_t i = 0; i < n; i++) hmms[i] = hmm_from_read(w, read_index[i]);
    path_vec paths = tiling_paths_from(w, hmms, n);
    free(hmms);
    return paths;
}

static int get_rp_hmms(world *w, const int32_t *read_index, int64_t n, const mrp_params *params, hmm_vec **out) {
    path_vec paths = tiling_paths2(w, read_index, n); /* coordination.c:498 */
    if (paths.n > MRP_MAX_READ_PARTITIONING_DEPTH || paths.n > params->max_coverage_depth) { /* :500-504 */
        for (int64_t i = 0; i < paths.n; i++) free_path(paths.a[i], 1);
        const int64_t np = paths.n;
        free(paths.a);
        *out = NULL;
        return mrp_set_error(MRP_ERR_ARG,
                             "Coverage depth: read depth of %lld exceeds hard maximum of %d with configured maximum of %lld",
                             (long long) np, MRP_MAX_READ_PARTITIONING_DEPTH, (long long) params->max_coverage_depth);
    }
    int rc = merge_tiling_paths(w, paths.a, paths.n, params, out);
    free(paths.a);
    return rc;
}

int mrp_get_rp_hmms(mrp_context *ctx, const mrp_chunk *chunk, const mrp_read *reads, const int32_t *read_index,
                    int64_t n, const mrp_params *params, mrp_batch *record, mrp_hmm ***hmms_out, int64_t *n_out) {
    if (!params || !hmms_out || !n_out || n < 0 || (n > 0 && !read_index)) return mrp_set_error(MRP_ERR_ARG, "mrp_get_rp_hmms: bad arguments");
    int64_t max_idx = -1;
    for (int64_t i = 0; i < n; i++) { if (read_index[i] < 0) return mrp_set_error(MRP_ERR_ARG, "negative read index"); if (read_index[i] > max_idx) max_idx = read_index[i]; }
    world w;
    int rc = world_init(&w, ctx, chunk, reads, max_idx + 1, record);
    if (rc != MRP_OK) return rc;
    hmm_vec *tp = NULL;
    rc = get_rp_hmms(&w, read_index, n, params, &tp);
    if (rc != MRP_OK) { free_path(tp, 1); return rc; }
    *n_out = tp->n;
    *hmms_out = tp->a ? tp->a : xmalloc(sizeof(mrp_hmm *));
    free(tp);
    return MRP_OK;
}

int mrp_hmm_view(const mrp_hmm *hmm, mrp_hmm_job *view, const int32_t **col_reads_out, int32_t *ref_start,
                 int32_t *ref_length) {
    if (!hmm || !view) return mrp_set_error(MRP_ERR_ARG, "mrp_hmm_view: NULL argument");
    world w; memset(&w, 0, sizeof(w));
    hmm_job(&w, (mrp_hmm *) hmm, 0, view, hmm->has_results);
    if (col_reads_out) *col_reads_out = hmm->col_reads.a;
    if (ref_start) *ref_start = hmm->ref_start;
    if (ref_length) *ref_length = hmm->ref_length;
    return MRP_OK;
}

int mrp_hmm_forward_backward(mrp_context *ctx, const mrp_chunk *chunk, mrp_hmm *hmm, const mrp_params *params,
                             mrp_batch *record) {
    if (!hmm || !params) return mrp_set_error(MRP_ERR_ARG, "mrp_hmm_forward_backward: NULL argument");
    world w;
    int rc = world_init(&w, ctx, chunk, NULL, 0, record);
    if (rc != MRP_OK) return rc;
    return sweep_many(&w, &hmm, 1, params);
}

/* stRPHmm_forwardTraceBack hmm.c:165-219 */
int mrp_hmm_forward_trace_back(const mrp_hmm *h, int32_t *path) {
    if (!h || !path) return mrp_set_error(MRP_ERR_ARG, "mrp_hmm_forward_trace_back: NULL argument");
    if (!h->has_results) return mrp_set_error(MRP_ERR_ARG, "trace back before a forward/backward sweep");
    const int64_t K = hmm_K(h);
    int64_t c0 = h->cell_off.a[K - 1], nc = h->cell_off.a[K] - c0;
    int64_t best = 0;
    double max_prob = h->f[c0];
    for (int64_t c = 1; c < nc; c++) if (h->f[c0 + c] > max_prob) { max_prob = h->f[c0 + c]; best = c; }
    path[K - 1] = (int32_t) best;
    for (int64_t k = K - 1; k > 0; k--) {
        const uint32_t m = h->prev.a[h->cell_off.a[k] + path[k]];
        c0 = h->cell_off.a[k - 1]; nc = h->cell_off.a[k] - c0;
        best = -1; max_prob = -INFINITY;
        for (int64_t c = 0; c < nc; c++)
            if (h->next.a[c0 + c] == m && h->f[c0 + c] > max_prob) { max_prob = h->f[c0 + c]; best = c; }
        if (best < 0) return mrp_set_error(MRP_ERR_LOOKUP, "trace back: no cell feeds the chosen merge cell in column %lld", (long long) (k - 1));
        path[k - 1] = (int32_t) best;
    }
    return MRP_OK;
}

/* ------------------------------------------------------------------------------------------ */
/* split (hmm.c:1192-1383)                                                                      */
/* ------------------------------------------------------------------------------------------ */
/* columns [k0, k1) of src appended to dst; the first one may start later, the last one end earlier (stRPColumn_split
 * column.c:86-101 leaves both halves with the same cells and reads) */
static void hmm_append_columns(const world *w, mrp_hmm *dst, const mrp_hmm *src, int64_t k0, int64_t k1, int32_t first_start,
                               int32_t last_end) {
    for (int64_t k = k0; k < k1; k++) {
        int32_t start = src->col_start.a[k], end = start + src->col_len.a[k];
        if (k == k0 && first_start > start) start = first_start;
        if (k == k1 - 1 && last_end < end) end = last_end;
        hmm_begin_column(dst, w, start, end - start, src->col_depth.a[k], src->col_reads.a + src->read_off.a[k]);
        for (int64_t c = src->cell_off.a[k]; c < src->cell_off.a[k + 1]; c++) {
            hmm_add_cell(dst, src->part.a[c], k == k0 ? 0u : src->prev.a[c]);
            dst->next.a[dst->next.n - 1] = k == k1 - 1 ? 0u : src->next.a[c];
        }
        hmm_end_column(dst);
        if (k + 1 < k1) {
            hmm_begin_merge(dst, src->mask_from.a[k], src->mask_to.a[k]);
            for (int64_t m = src->mcell_off.a[k]; m < src->mcell_off.a[k + 1]; m++) { VEC_PUSH(dst->mfrom, src->mfrom.a[m]); VEC_PUSH(dst->mto, src->mto.a[m]); }
            hmm_end_merge(dst);
        }
    }
}
/* h takes the arrays of `from` (which is consumed); h's own bookkeeping as an allocation stays */
static void hmm_take(mrp_hmm *h, mrp_hmm *from) {
    void *arrays[] = {h->reads.a, h->col_start.a, h->col_len.a, h->col_depth.a, h->cell_off.a, h->read_off.a, h->col_reads.a,
                      h->read_byte_off.a, h->part.a, h->next.a, h->prev.a, h->mask_from.a, h->mask_to.a, h->mcell_off.a,
                      h->mfrom.a, h->mto.a};
    for (size_t i = 0; i < sizeof(arrays) / sizeof(arrays[0]); i++) hmm_free_array(h, arrays[i]);
    hmm_free_results(h);
    h->ref_start = from->ref_start; h->ref_length = from->ref_length; h->max_depth = from->max_depth;
    h->reads = from->reads; h->col_start = from->col_start; h->col_len = from->col_len; h->col_depth = from->col_depth;
    h->cell_off = from->cell_off; h->read_off = from->read_off; h->col_reads = from->col_reads; h->read_byte_off = from->read_byte_off;
    h->part = from->part; h->next = from->next; h->prev = from->prev; h->mask_from = from->mask_from; h->mask_to = from->mask_to;
    h->mcell_off = from->mcell_off; h->mfrom = from->mfrom; h->mto = from->mto;
    free(from);
}
/* stRPHmm_split hmm.c:1231-1300: h keeps [refStart, split_point), the returned hmm holds the rest.  The column that
 * contains the split point is cut in two (both halves keep its cells); the merge column in front of the suffix goes. */
static mrp_hmm *hmm_split(const world *w, mrp_hmm *h, int32_t sp) {
    const int64_t K = hmm_K(h);
    int64_t ks = 0; /* getColumn :1192-1209 */
    while (ks < K && sp >= h->col_start.a[ks] + h->col_len.a[ks]) ks++;
    const int inside = sp > h->col_start.a[ks];
    mrp_hmm *L = hmm_new(), *R = hmm_new();
    for (int64_t i = 0; i < h->reads.n; i++) { /* :1247-1262 */
        const mrp_read *r = &w->reads[h->reads.a[i]];
        if (r->ref_start < sp) VEC_PUSH(L->reads, h->reads.a[i]);
        if (r->ref_start + r->length > sp) VEC_PUSH(R->reads, h->reads.a[i]);
    }
    hmm_append_columns(w, L, h, 0, inside ? ks + 1 : ks, h->col_start.a[0], sp);
    hmm_append_columns(w, R, h, ks, K, sp, h->col_start.a[K - 1] + h->col_len.a[K - 1]);
    L->ref_start = h->ref_start; L->ref_length = sp - h->ref_start;
    R->ref_start = sp; R->ref_length = h->ref_start + h->ref_length - sp;
    hmm_take(h, L);
    return R;
}
static int hmm_reads_known(const mrp_hmm *h, int64_t n_reads) {
    for (int64_t i = 0; i < h->reads.n; i++) if (h->reads.a[i] < 0 || h->reads.a[i] >= n_reads) return 0;
    return 1;
}
int mrp_hmm_split(const mrp_chunk *chunk, const mrp_read *reads, int64_t n_reads, mrp_hmm *hmm, int32_t split_point,
                  mrp_hmm **suffix_out) {
    if (!hmm || !suffix_out) return mrp_set_error(MRP_ERR_ARG, "mrp_hmm_split: bad arguments");
    if (split_point <= hmm->ref_start) return mrp_set_error(MRP_ERR_ARG, "The split point is at or before the start of the reference interval");
    if (split_point >= hmm->ref_start + hmm->ref_length) return mrp_set_error(MRP_ERR_ARG, "The split point is after the last position of the reference interval");
    world w;
    int rc = world_host(&w, chunk, reads, n_reads);
    if (rc != MRP_OK) return rc;
    if (!hmm_reads_known(hmm, n_reads)) return mrp_set_error(MRP_ERR_ARG, "mrp_hmm_split: the hmm names reads beyond n_reads");
    *suffix_out = hmm_split(&w, hmm, split_point);
    return MRP_OK;
}

/* sitesLinkageIsWellSupported hmm.c:1302-1320: reads shared by the columns that hold the two sites */
static int sites_linkage_well_supported(const mrp_hmm *h, const mrp_params *params, int32_t left, int32_t right) {
    const int64_t K = hmm_K(h);
    int64_t kl = 0, kr;
    while (kl < K - 1 && left >= h->col_start.a[kl] + h->col_len.a[kl]) kl++;
    kr = kl;
    while (kr < K - 1 && right >= h->col_start.a[kr] + h->col_len.a[kr]) kr++;
    const int32_t *a = h->col_reads.a + h->read_off.a[kl], *b = h->col_reads.a + h->read_off.a[kr];
    int64_t common = 0;
    for (int32_t i = 0; i < h->col_depth.a[kl]; i++)
        for (int32_t j = 0; j < h->col_depth.a[kr]; j++)
            if (a[i] == b[j]) { common++; break; }
    return common >= params->min_read_coverage_to_support_phasing_between_heterozygous_sites;
}
/* stRPHMM_splitWherePhasingIsUncertain hmm.c:1322-1383: sweep, trace back, predicted haplotypes; between two consecutive
 * heterozygous sites that too few reads span, the hmm is cut half way.  The input hmm becomes the first of the list. */
int mrp_hmm_split_where_phasing_is_uncertain(mrp_context *ctx, const mrp_chunk *chunk, const mrp_read *reads, int64_t n_reads,
                                             mrp_hmm *hmm, const mrp_params *params, mrp_hmm ***hmms_out, int64_t *n_out) {
    if (!hmm || !params || !hmms_out || !n_out) return mrp_set_error(MRP_ERR_ARG, "mrp_hmm_split_where_phasing_is_uncertain: bad arguments");
    world w;
    int rc = world_init(&w, ctx, chunk, reads, n_reads, NULL);
    if (rc != MRP_OK) return rc;
    if (!hmm_reads_known(hmm, n_reads)) return mrp_set_error(MRP_ERR_ARG, "the hmm names reads beyond n_reads");
    mrp_hmm *one = hmm;
    rc = sweep_many(&w, &one, 1, params);
    if (rc != MRP_OK) return rc;
    const int64_t K = hmm_K(hmm);
    int32_t *path = xmalloc(sizeof(int32_t) * (size_t) K);
    rc = mrp_hmm_forward_trace_back(hmm, path);
    if (rc != MRP_OK) { free(path); return rc; }
    uint64_t *chosen = xmalloc(sizeof(uint64_t) * (size_t) K);
    for (int64_t k = 0; k < K; k++) chosen[k] = hmm->part.a[hmm->cell_off.a[k] + path[k]];
    mrp_phase_result *g = result_new(hmm->ref_start, hmm->ref_length, n_reads);
    genome_fragment(&w, g, hmm, chosen, 0); /* stGenomeFragment_construct only, :1330 */
    hmm_vec out = {0};
    int32_t prev_het = -1;
    for (int32_t i = 0; i < g->length; i++) {
        if (g->haplotype_string1[i] == g->haplotype_string2[i]) continue;
        const int32_t site = g->ref_start + i;
        if (prev_het >= 0 && !sites_linkage_well_supported(hmm, params, prev_het, site)) {
            mrp_hmm *right = hmm_split(&w, hmm, prev_het + (site - prev_het + 1) / 2); /* :1361 */
            VEC_PUSH(out, hmm);
            hmm = right;
        }
        prev_het = site;
    }
    VEC_PUSH(out, hmm);
    free(path); free(chosen); mrp_phase_result_destroy(g);
    *hmms_out = out.a;
    *n_out = out.n;
    return MRP_OK;
}

/* filterReadsByCoverageDepth coordination.c:443-488 */
static void filter_reads_by_coverage_depth(const world *w, const mrp_params *params, int32_t *filtered, int64_t *nf,
                                           int32_t *discarded, int64_t *nd) {
    int32_t *all = xmalloc(sizeof(int32_t) * (size_t) (w->n_reads + 1));
    for (int64_t i = 0; i < w->n_reads; i++) all[i] = (int32_t) i;
    path_vec paths = tiling_paths2(w, all, w->n_reads);
    free(all);
    keyed *a = xmalloc(sizeof(keyed) * (size_t) (paths.n + 1)), *t = xmalloc(sizeof(keyed) * (size_t) (paths.n + 1));
    for (int64_t i = 0; i < paths.n; i++) {
        int64_t total = 0;
        for (int64_t j = 0; j < paths.a[i]->n; j++) total += w->reads[paths.a[i]->a[j]->reads.a[0]].length;
        a[i].idx = i; a[i].key = (double) total;
    }
    keyed_sort_desc(a, paths.n, t);
    int64_t np = paths.n;
    *nf = 0; *nd = 0;
    while (np > params->max_coverage_depth) {
        hmm_vec *tp = paths.a[a[--np].idx];
        for (int64_t j = tp->n - 1; j >= 0; j--) discarded[(*nd)++] = tp->a[j]->reads.a[0];
    }
    while (np > 0) {
        hmm_vec *tp = paths.a[a[--np].idx];
        for (int64_t j = tp->n - 1; j >= 0; j--) filtered[(*nf)++] = tp->a[j]->reads.a[0];
    }
    for (int64_t i = 0; i < paths.n; i++) free_path(paths.a[i], 1);
    free(paths.a); free(a); free(t);
}

/* bubbleGraph.c:2755-2779 on a swept host hmm */
static int finish_phase(world *w, mrp_hmm *hmm, const mrp_params *params, const int32_t *discarded, int64_t nd,
                        mrp_phase_result **out) {
    const int64_t K = hmm_K(hmm);
    int32_t *path = xmalloc(sizeof(int32_t) * (size_t) K);
    int rc = mrp_hmm_forward_trace_back(hmm, path); /* :2755 */
    if (rc == MRP_OK) {
        uint64_t *chosen = xmalloc(sizeof(uint64_t) * (size_t) K);
        for (int64_t k = 0; k < K; k++) chosen[k] = hmm->part.a[hmm->cell_off.a[k] + path[k]];
        finish_phase_parts(w, hmm, chosen, hmm->fwd, hmm->bwd, params, discarded, nd, out);
        free(chosen);
    }
    free(path);
    return rc;
}

/* bubbleGraph_phaseBubbleGraph bubbleGraph.c:2673-2801 */
int mrp_phase_reads(mrp_context *ctx, const mrp_chunk *chunk, const mrp_read *reads, int64_t n_reads,
                    const mrp_params *params, mrp_batch *record, mrp_phase_result **out) {
    if (!params || !out || n_reads < 0) return mrp_set_error(MRP_ERR_ARG, "mrp_phase_reads: bad arguments");
    *out = NULL;
    world w;
    int rc = world_init(&w, ctx, chunk, reads, n_reads, record);
    if (rc != MRP_OK) return rc;
    if (n_reads == 0) { *out = result_new(0, 0, 0); return MRP_OK; } /* :2719-2728 */
    int32_t *filtered = xmalloc(sizeof(int32_t) * (size_t) n_reads), *discarded = xmalloc(sizeof(int32_t) * (size_t) n_reads);
    int64_t nf, nd;
    filter_reads_by_coverage_depth(&w, params, filtered, &nf, discarded, &nd); /* :2699 */
    uint8_t *is_disc = xcalloc((size_t) n_reads, 1);
    for (int64_t i = 0; i < nd; i++) is_disc[discarded[i]] = 1;
    int32_t *fwd = xmalloc(sizeof(int32_t) * (size_t) n_reads), *rev = xmalloc(sizeof(int32_t) * (size_t) n_reads);
    int64_t nfwd = 0, nrev = 0;
    for (int64_t i = 0; i < n_reads; i++) { /* :2705-2716 */
        if (is_disc[i]) continue;
        if (reads[i].forward_strand) fwd[nfwd++] = (int32_t) i; else rev[nrev++] = (int32_t) i;
    }
    mrp_params pc = *params;
    pc.include_ancestor_sub_prob = 0; /* :2733 */
    hmm_vec *tpF = NULL, *tpR = NULL, *joined = NULL;
    mrp_hmm *hmm = NULL;
    rc = get_rp_hmms(&w, fwd, nfwd, &pc, &tpF);                  /* :2736 */
    if (rc == MRP_OK) rc = get_rp_hmms(&w, rev, nrev, &pc, &tpR); /* :2740 */
    if (rc == MRP_OK) { rc = merge_two_tiling_paths(&w, tpF, tpR, &pc, &joined); tpF = tpR = NULL; } /* :2745 */
    if (rc == MRP_OK && joined->n > 0) {
        hmm = fuse_path(&w, joined);
        free(joined->a); free(joined); joined = NULL;
        pc.include_ancestor_sub_prob = 1; /* :2748 */
        rc = sweep_many(&w, &hmm, 1, &pc); /* :2749 */
        if (rc == MRP_OK) rc = finish_phase(&w, hmm, params, discarded, nd, out);
    } else if (rc == MRP_OK) {
        *out = result_new(0, 0, n_reads);
    }
    free_path(tpF, 1); free_path(tpR, 1); free_path(joined, 1);
    mrp_hmm_destroy(hmm);
    free(filtered); free(discarded); free(is_disc); free(fwd); free(rev);
    return rc;
}
