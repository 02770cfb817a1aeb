/*
 * rphmm_common.h -- what the translation units of the C host pipeline share: rphmm_chunk.c (per-chunk path), rphmm_host.c
 * (device-resident path), rphmm_many.c (call scheduling) and rphmm_result.c (result building).  Included by those files and by
 * tools/hostbench only; the interface to the C++ side is rphmm_host.h.
 *
 * Functions that cross files are either static inline here or hidden: the library is built without -fvisibility, and the
 * set of exported symbols is the C ABI of include/margin_rphmm.h plus what rphmm_host.h declares.
 */
#ifndef RPHMM_COMMON_H_
#define RPHMM_COMMON_H_

#include "rphmm_host.h"

#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#define RPHMM_HIDDEN __attribute__((visibility("hidden")))

static inline double now_ms(void) {
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return 1e3 * (double) ts.tv_sec + 1e-6 * (double) ts.tv_nsec;
}

/* host worker threads: the structural code is independent per chunk / per merge node */
typedef void (*par_fn)(int64_t i, void *arg);
static inline void parallel_for(int64_t n, par_fn fn, void *arg) { mrp_pool_run(n, 1, fn, arg); } /* persistent pool, mrp_host_pool.cpp */

/* Allocation: out of memory is fatal, like st_malloc.  Every translation unit has the three functions under these names.  The
 * plain ones are defined here; rphmm_host.c defines RPHMM_ARENA_ALLOC before it includes this header and supplies its own,
 * which take from the calling thread's scratch arena while that is switched on. */
#ifdef RPHMM_ARENA_ALLOC
static void *xmalloc(size_t n);
static void *xcalloc(size_t n, size_t s);
static void *xrealloc(void *q, size_t n);
#else
static inline void *xmalloc(size_t n) {
    void *p = malloc(n ? n : 1);
    if (!p) { fprintf(stderr, "margin_rphmm: out of host memory\n"); abort(); }
    return p;
}
static inline void *xcalloc(size_t n, size_t s) {
    void *p = calloc(n ? n : 1, s ? s : 1);
    if (!p) { fprintf(stderr, "margin_rphmm: out of host memory\n"); abort(); }
    return p;
}
static inline void *xrealloc(void *q, size_t n) {
    void *p = realloc(q, n ? n : 1);
    if (!p) { fprintf(stderr, "margin_rphmm: out of host memory\n"); abort(); }
    return p;
}
#endif

#define VEC(T) struct { T *a; int64_t n, cap; }
#define VEC_PUSH(v, x)                                                                        \
    do {                                                                                      \
        if ((v).n == (v).cap) {                                                               \
            (v).cap = (v).cap ? (v).cap * 2 : 16;                                             \
            (v).a = xrealloc((v).a, sizeof(*(v).a) * (size_t) (v).cap);                       \
        }                                                                                     \
        (v).a[(v).n++] = (x);                                                                 \
    } while (0)
#define VEC_RESERVE(v, extra)                                                                 \
    do {                                                                                      \
        if ((v).n + (int64_t) (extra) > (v).cap) {                                            \
            while ((v).n + (int64_t) (extra) > (v).cap) (v).cap = (v).cap ? (v).cap * 2 : 16; \
            (v).a = xrealloc((v).a, sizeof(*(v).a) * (size_t) (v).cap);                       \
        }                                                                                     \
    } while (0)

/* ------------------------------------------------------------------------------------------ */
/* the flat hmm: one structure of arrays whose arrays are exactly the arrays of mrp_hmm_job    */
/* ------------------------------------------------------------------------------------------ */
struct mrp_hmm {
    int32_t ref_start, ref_length; /* stRPHmm.refStart / refLength */
    int32_t max_depth;
    VEC(int32_t) reads;            /* stRPHmm.profileSeqs (read indices) */
    /* columns */
    VEC(int32_t) col_start, col_len, col_depth;
    VEC(int64_t) cell_off, read_off;   /* K+1 */
    VEC(int32_t) col_reads;            /* per column, bit order */
    VEC(int64_t) read_byte_off;        /* per column per read: offset of column->seqs[i] in the pool */
    /* cells */
    VEC(uint64_t) part;
    VEC(uint32_t) next, prev;
    /* merge columns */
    VEC(uint64_t) mask_from, mask_to;  /* K-1 */
    VEC(int64_t) mcell_off;            /* K (first entry 0) */
    VEC(uint64_t) mfrom, mto;
    /* results of the last sweep */
    double *f, *b, *mf, *mb, *total;
    double fwd, bwd;
    int has_results;
};

static inline int64_t hmm_K(const mrp_hmm *h) { return h->col_start.n; }

static inline mrp_hmm *hmm_new(void) {
    mrp_hmm *h = xcalloc(1, sizeof(*h));
    VEC_PUSH(h->cell_off, 0);
    VEC_PUSH(h->read_off, 0);
    VEC_PUSH(h->mcell_off, 0);
    return h;
}
static inline void hmm_free_results(mrp_hmm *h) {
    free(h->f); free(h->b); free(h->mf); free(h->mb); free(h->total);
    h->f = h->b = h->mf = h->mb = h->total = NULL;
    h->has_results = 0;
}
static inline void hmm_free_array(const mrp_hmm *h, void *p) { (void) h; free(p); }

/* per-job view of the reads + chunk the structural code works against */
typedef struct {
    const mrp_chunk *chunk;
    mrp_chunk_host ch;
    const mrp_read *reads;
    int64_t n_reads;
    mrp_context *ctx;
    mrp_batch *record;
    int64_t n_sweeps;
    uint32_t max_alleles;
    int failed; /* resident path: a kernel asked for this chunk to be redone on the hashing path */
} world;
/* checks the arguments and the reads' intervals; world_host: without a context, for host-only entry points (rphmm_result.c) */
RPHMM_HIDDEN int world_init(world *w, mrp_context *ctx, const mrp_chunk *chunk, const mrp_read *reads, int64_t n_reads,
                            mrp_batch *record);
RPHMM_HIDDEN int world_host(world *w, const mrp_chunk *chunk, const mrp_read *reads, int64_t n_reads);

static inline int64_t read_byte_offset(const world *w, int32_t read, int32_t site) { /* profileSeq.c:41-47 */
    const mrp_read *r = &w->reads[read];
    return r->pool_offset + (int64_t) (w->ch.allele_offset[site] - w->ch.allele_offset[r->ref_start]);
}
static inline void hmm_add_cell(mrp_hmm *h, uint64_t p, uint32_t prev) {
    VEC_PUSH(h->part, p);
    VEC_PUSH(h->prev, prev);
    VEC_PUSH(h->next, 0u);
}

static inline uint32_t sweep_flags(const mrp_params *p) {
    return (p->max_not_sum_transitions ? MRP_FLAG_MAX_NOT_SUM : 0u) |
           (p->include_ancestor_sub_prob ? MRP_FLAG_INCLUDE_ANCESTOR_SUB_PROB : 0u);
}

typedef struct { int64_t idx; double key; } keyed;
RPHMM_HIDDEN void keyed_sort_desc(keyed *a, int64_t n, keyed *tmp); /* stable, descending (rphmm_result.c) */

/* result building (rphmm_result.c) */
RPHMM_HIDDEN mrp_phase_result *result_new(int32_t ref_start, int32_t length, int64_t n_reads);
RPHMM_HIDDEN void genome_fragment(const world *w, mrp_phase_result *g, const mrp_hmm *h, const uint64_t *chosen, int64_t max_iterations);
RPHMM_HIDDEN void finish_phase_parts(world *w, const mrp_hmm *hmm, const uint64_t *chosen, double fwd, double bwd, const mrp_params *params,
                                     const int32_t *discarded, int64_t nd, mrp_phase_result **out);

/* one batch of chunks through the device-resident merge levels (rphmm_host.c); rphmm_many.c splits a call into batches */
RPHMM_HIDDEN int phase_many_resident(mrp_context *ctx, int64_t n_chunks, const mrp_chunk *const *chunks, const mrp_read *const *reads,
                                     const int64_t *n_reads, const mrp_params *params, mrp_phase_result **out,
                                     mrp_phase_many_stats *stats);

#endif
