/*
 * rphmm_host.c -- the device-resident host path of libmargin_rphmm.so: the code behind mrp_phase_reads_many's headline.
 *
 * The recursion of mergeTilingPaths (coordination.c:263-409) for any number of chunks at once, with the hmms never
 * leaving HBM.  The host keeps a compact "shadow" of every hmm (struct rhmm: interval, reads, column boundaries, where
 * its pruned form will be on the device) and decides WHICH hmms are merged and where the merged columns begin
 * (r_prepare_merge, r_cross_build); everything else -- cells, connectors, sweep, prune, trace back, genome fragment --
 * is the engine's (mrp_engine.cpp), one batch of kernels per recursion level (r_run_tree).  phase_many_resident is one
 * batch of chunks from reads to results; rphmm_many.c splits a call into such batches.
 *
 * The hot loops run some 10^5 times per call on 16 threads, so two private allocators live here beside their only
 * users: the thread's scratch arena (with the arena-aware xmalloc / xcalloc / xrealloc and this file's free()) and
 * the shadow block pool.  The flat hmm and the per-job view are in rphmm_common.h, results are built in
 * rphmm_result.c, the per-chunk path a chunk falls back to is rphmm_chunk.c.
 */
#define _GNU_SOURCE
#define RPHMM_ARENA_ALLOC /* this file supplies xmalloc / xcalloc / xrealloc */
#include "rphmm_common.h"

/* Scratch arena of the calling thread.  One merge of the resident pipeline (r_prepare_merge) makes some thirty small
 * allocations that all die before it returns -- component lists, tiling paths, piece lists -- and a call makes 10^5 merges on
 * 16 threads: a quarter of the host CPU time of a call went into malloc/free.  While the arena is switched on, xmalloc /
 * xcalloc / xrealloc (hence VEC_PUSH) bump-allocate from it; free() of such a pointer is a no-op (this file's free() checks
 * the range), the arena is rewound when the merge is done.  What outlives the merge (shadows, the result path, the garbage
 * list) is allocated with the arena switched off.  A block never changes threads while the arena owns it.
 * The arena is only ever on inside r_prepare_merge: flat hmms and results (rphmm_result.c, whose free() is the heap's) never
 * come from it.  Its state exists once in the library, in this file. */
typedef struct { char *base; size_t cap, used; int active; } tl_arena;
static __thread tl_arena t_ar;
static pthread_key_t ar_key;
static pthread_once_t ar_once = PTHREAD_ONCE_INIT;
static void ar_release(void *p) { free(p); }
static void ar_make_key(void) { (void) pthread_key_create(&ar_key, ar_release); }
static inline int ar_owns(const void *p) { return t_ar.base && (const char *) p >= t_ar.base && (const char *) p < t_ar.base + t_ar.cap; }
static void *ar_alloc(size_t n) {
    if (!t_ar.base) {
        (void) pthread_once(&ar_once, ar_make_key);
        t_ar.cap = (size_t) 8 << 20;
        t_ar.base = malloc(t_ar.cap);
        if (!t_ar.base) { t_ar.cap = 0; return NULL; }
        (void) pthread_setspecific(ar_key, t_ar.base); /* freed when the thread ends */
    }
    n = (n + 15) & ~(size_t) 15;
    if (t_ar.used + n + 16 > t_ar.cap) return NULL; /* does not fit: the caller takes it from the heap */
    char *q = t_ar.base + t_ar.used;
    *(size_t *) q = n;
    t_ar.used += n + 16;
    return q + 16;
}
static inline void ar_on(void) { t_ar.active = 1; }
static inline void ar_off(void) { t_ar.active = 0; }
static inline void ar_rewind(void) { t_ar.used = 0; t_ar.active = 0; }

static void *xmalloc(size_t n) { /* like st_malloc: out of memory is fatal */
    if (t_ar.active) { void *a = ar_alloc(n ? n : 1); if (a) return a; }
    void *p = malloc(n ? n : 1);
    if (!p) { fprintf(stderr, "margin_rphmm: out of host memory\n"); abort(); }
    return p;
}
static void *xcalloc(size_t n, size_t s) {
    if (t_ar.active) { void *a = ar_alloc((n ? n : 1) * (s ? s : 1)); if (a) { memset(a, 0, (n ? n : 1) * (s ? s : 1)); return a; } }
    void *p = calloc(n ? n : 1, s ? s : 1);
    if (!p) { fprintf(stderr, "margin_rphmm: out of host memory\n"); abort(); }
    return p;
}
static void *xrealloc(void *q, size_t n) {
    if (q && ar_owns(q)) { /* grows inside the arena (or moves to the heap when the arena is full or off) */
        const size_t old = *(size_t *) ((char *) q - 16);
        if (n <= old) return q;
        void *p = xmalloc(n);
        memcpy(p, q, old);
        return p;
    }
    if (!q) return xmalloc(n);
    void *p = realloc(q, n ? n : 1);
    if (!p) { fprintf(stderr, "margin_rphmm: out of host memory\n"); abort(); }
    return p;
}
static inline void tl_free(void *p) { if (p && !ar_owns(p)) free(p); }
#define free(p) tl_free(p) /* from here on: a block of the thread's scratch arena is not given to the heap */

/* Blocks of the shadow hmms of the device-resident merge: tens of thousands per call, a few hundred bytes to a few hundred
 * kilobytes each, all dead by the end of the call.  Through malloc the large ones are mapped and unmapped one by one (and
 * page-faulted in again by the next call); here they are kept on per-size-class stacks (powers of two) and reused warm. */
#define SHADOW_MIN_LOG 9
#define SHADOW_CLASSES 20 /* 512 B .. 256 MB */
static struct { pthread_mutex_t mu; void **stack; int64_t n, cap; } g_shadow[SHADOW_CLASSES];
static pthread_once_t g_shadow_once = PTHREAD_ONCE_INIT;
static int shadow_class(size_t bytes) {
    int c = 0;
    while (((size_t) 1 << (c + SHADOW_MIN_LOG)) < bytes) c++;
    return c;
}
/* per-thread front of the pool: the shared stacks are touched a batch at a time.  The fronts are large for the small classes
 * -- a level of the first merges makes tens of thousands of blocks of 512 B .. 2 KB on the worker threads and the thread that
 * drives the batch gives the parents' blocks back: everything flows through the shared stack, and with fronts of 16 the
 * class mutex was taken every eighth block by 24 threads (a fifth of a call's host CPU time in futex calls). */
#define SHADOW_TL 256
#define SHADOW_TL_LARGE 16
#define SHADOW_SMALL_CLASSES 6 /* up to 16 KB */
static inline int shadow_front(int c) { return c < SHADOW_SMALL_CLASSES ? SHADOW_TL : SHADOW_TL_LARGE; }
typedef struct { void *slot[SHADOW_CLASSES][SHADOW_TL]; int n[SHADOW_CLASSES]; int keyed; } shadow_tl;
static __thread shadow_tl t_shadow;
static pthread_key_t g_shadow_key;
static void shadow_spill(int c, shadow_tl *f, int keep) { /* front -> shared stack */
    pthread_mutex_lock(&g_shadow[c].mu);
    if (g_shadow[c].n + f->n[c] > g_shadow[c].cap) {
        while (g_shadow[c].n + f->n[c] > g_shadow[c].cap) g_shadow[c].cap = g_shadow[c].cap ? 2 * g_shadow[c].cap : 1024;
        void **grown = realloc(g_shadow[c].stack, sizeof(void *) * (size_t) g_shadow[c].cap);
        if (!grown) { fprintf(stderr, "margin_rphmm: out of host memory\n"); abort(); }
        g_shadow[c].stack = grown;
    }
    while (f->n[c] > keep) g_shadow[c].stack[g_shadow[c].n++] = f->slot[c][--f->n[c]];
    pthread_mutex_unlock(&g_shadow[c].mu);
}
static void shadow_thread_exit(void *arg) { /* a thread ends (the threads of a call's concurrent batches do): its front goes back */
    shadow_tl *f = arg;
    for (int c = 0; c < SHADOW_CLASSES; c++) if (f->n[c] > 0) shadow_spill(c, f, 0);
}
static void shadow_pool_init(void) {
    for (int i = 0; i < SHADOW_CLASSES; i++) pthread_mutex_init(&g_shadow[i].mu, NULL);
    (void) pthread_key_create(&g_shadow_key, shadow_thread_exit);
}
static inline void shadow_thread_enter(void) { /* every thread that holds blocks in its front is registered: its front is spilled when it ends */
    if (__builtin_expect(t_shadow.keyed, 1)) return;
    pthread_once(&g_shadow_once, shadow_pool_init);
    t_shadow.keyed = 1;
    (void) pthread_setspecific(g_shadow_key, &t_shadow);
}
static void *shadow_alloc(size_t bytes, int *cls_out) {
    const int c = shadow_class(bytes);
    if (c >= SHADOW_CLASSES) { *cls_out = -1; return xmalloc(bytes); }
    *cls_out = c;
    shadow_thread_enter();
    if (t_shadow.n[c] > 0) return t_shadow.slot[c][--t_shadow.n[c]];
    /* refill: up to half a front from the shared stack */
    pthread_mutex_lock(&g_shadow[c].mu);
    while (t_shadow.n[c] < shadow_front(c) / 2 && g_shadow[c].n > 0) t_shadow.slot[c][t_shadow.n[c]++] = g_shadow[c].stack[--g_shadow[c].n];
    pthread_mutex_unlock(&g_shadow[c].mu);
    if (t_shadow.n[c] > 0) return t_shadow.slot[c][--t_shadow.n[c]];
    const int was = t_ar.active; /* (never from the scratch arena: the block outlives the merge) */
    t_ar.active = 0;
    void *p = xmalloc((size_t) 1 << (c + SHADOW_MIN_LOG));
    t_ar.active = was;
    return p;
}
static void shadow_release(void *p, int cls) {
    if (cls < 0) { free(p); return; }
    shadow_thread_enter(); /* (a thread that only ever releases -- a batch's own thread, the clean-up of a call -- used to keep its front for good) */
    if (t_shadow.n[cls] == shadow_front(cls)) { /* spill half of the front */
        shadow_spill(cls, &t_shadow, shadow_front(cls) / 2);
    }
    t_shadow.slot[cls][t_shadow.n[cls]++] = p;
}

/* ------------------------------------------------------------------------------------------ */
/* device-resident merge                                                     */
/*                                                                                             */
/* The same recursion as merge_tiling_paths / merge_two_tiling_paths of rphmm_chunk.c, but the  */
/* hmms never leave HBM.  The structural decisions depend on read intervals only, split in two: */
/*   host    WHICH hmms are merged -- tiling paths, overlap components (coordination.c:69-339):   */
/*           a few hundred intervals per chunk and level -- and the merged column BOUNDARIES of   */
/*           every cross product (two sorted lists per hmm: 8 bytes per column);                 */
/*   device  everything else a column needs (which parent column each side is cut from, the      */
/*           connector kinds, the column's reads and where their profile bytes start, allele      */
/*           slots): mrp_structure_kernel, one thread per column, from the parents' own column    */
/*           tables, which stay in HBM (mrp_engine.h).                                           */
/* A "shadow" is what the host keeps of an hmm: interval, reads, column boundaries, and WHERE its */
/* pruned form will be on the device (segment, first column).  Cross product, sweep and prune    */
/* of every overlap component of a recursion level -- of every chunk and strand handed in --     */
/* run as ONE batch of kernels (mrp_engine_level_*).                                            */
/* ------------------------------------------------------------------------------------------ */
typedef struct rhmm {
    int32_t ref_start, ref_length;
    int32_t first_read;        /* reads[0]: its name breaks ties in stRPHmm_cmpFn */
    int32_t n_cols, n_reads;
    int32_t seg;               /* segment of the engine that holds the pruned hmm; -1: stRPHmm_construct leaf */
    int64_t col0;              /* first column in the segment; leaf: offset of the read's profile bytes in the pool */
    int32_t *starts;           /* [n_cols] first site of every column */
    int32_t *roff;             /* [n_cols + 1] prefix sums of the column depths */
    int32_t *reads;            /* [n_reads] stRPHmm.profileSeqs; a column's reads are those of them that cover it, in this order */
    mrp_xpar *par;             /* [n_a + n_b] the two tiling paths it is the cross product of */
    int32_t n_a, n_b;
    int64_t bound_cells, bound_merge, depth_sites; /* static bounds, see mrp_xhmm */
    int32_t bound_max_cells, bound_max_merge;
    int32_t pool_class;        /* size class of the block in the shadow pool + 1; 0: lives in a block owned by someone else */
} rhmm;

#define HMM_T rhmm
#define PFX(x) r_##x
#define H_NAME_READ(h) ((h)->first_read)
#include "rphmm_paths.inc"
#undef HMM_T
#undef PFX
#undef H_NAME_READ

static void rhmm_destroy(rhmm *h) {
    if (h && h->pool_class != 0) shadow_release(h, h->pool_class - 1);
}
/* A tiling path is either a vector of its own (heap) or the head of ONE block of the shadow pool that also holds its array and
 * the lists of the merge that made it (level_prepare): cap = -(size class + 2) marks the latter. */
static void r_path_release(r_hmm_vec *tp) {
    if (!tp) return;
    if (tp->cap < -1) { shadow_release(tp, (int) (-tp->cap - 2)); return; }
    free(tp->a); free(tp);
}
static void r_free_path(r_hmm_vec *tp, int destroy_hmms) {
    if (!tp) return;
    if (destroy_hmms) for (int64_t i = 0; i < tp->n; i++) rhmm_destroy(tp->a[i]);
    r_path_release(tp);
}

/* stRPHmm_construct (hmm.c:97-133): one column {1, 0} over the read's sites.  All leaves of a chunk live in one block. */
typedef struct { rhmm h; int32_t starts[1], roff[2], reads[1]; } rleaf;
static void r_leaf_init(rleaf *l, const world *w, int32_t read) {
    const mrp_read *r = &w->reads[read];
    rhmm *h = &l->h;
    memset(h, 0, sizeof(*h));
    h->ref_start = r->ref_start; h->ref_length = r->length; h->first_read = read;
    h->n_cols = 1; h->n_reads = 1;
    h->seg = -1; h->col0 = r->pool_offset; /* profileSeq.c:41-47 at the read's first site */
    l->starts[0] = r->ref_start; l->roff[0] = 0; l->roff[1] = 1; l->reads[0] = read;
    h->starts = l->starts; h->roff = l->roff; h->reads = l->reads;
}
static rleaf *r_leaves_of_chunk(const world *w, int *cls) { /* (a block of the shadow pool: a few hundred KB, warm from the call before) */
    rleaf *lv = shadow_alloc(sizeof(rleaf) * (size_t) (w->n_reads + 1), cls);
    for (int64_t i = 0; i < w->n_reads; i++) r_leaf_init(&lv[i], w, (int32_t) i);
    return lv;
}

/* filterReadsByCoverageDepth coordination.c:443-488 on the chunk's leaves */
static void r_filter_reads_by_coverage_depth(const world *w, rhmm *const *sorted, const mrp_params *params, int32_t *filtered, int64_t *nf,
                                             int32_t *discarded, int64_t *nd) {
    r_path_vec paths = r_tiling_paths_sorted(sorted, w->n_reads);
    keyed *a = xmalloc(sizeof(keyed) * (size_t) (paths.n + 1)), *t = xmalloc(sizeof(keyed) * (size_t) (paths.n + 1));
    for (int64_t i = 0; i < paths.n; i++) {
        int64_t total = 0;
        for (int64_t j = 0; j < paths.a[i]->n; j++) total += paths.a[i]->a[j]->ref_length;
        a[i].idx = i; a[i].key = (double) total;
    }
    keyed_sort_desc(a, paths.n, t);
    int64_t np = paths.n;
    *nf = 0; *nd = 0;
    while (np > params->max_coverage_depth) {
        r_hmm_vec *tp = paths.a[a[--np].idx];
        for (int64_t j = tp->n - 1; j >= 0; j--) discarded[(*nd)++] = tp->a[j]->first_read;
    }
    while (np > 0) {
        r_hmm_vec *tp = paths.a[a[--np].idx];
        for (int64_t j = tp->n - 1; j >= 0; j--) filtered[(*nf)++] = tp->a[j]->first_read;
    }
    for (int64_t i = 0; i < paths.n; i++) r_free_path(paths.a[i], 0);
    free(paths.a); free(a); free(t);
}

/* The pieces of a tiling path between S and E, one after the other: a column of one of its hmms, or a gap between two of
 * them / in front of the first / behind the last (stRPHmm_fuse hmm.c:283-372 and the prefix / suffix gaps of
 * stRPHmm_alignColumns hmm.c:396-462). */
typedef struct { const r_hmm_vec *tp; int64_t i; int32_t k, pos, E; } piter;
typedef struct { int32_t end, depth; uint8_t out; } rpiece; /* out: connector that leaves the piece at its own end */
static inline __attribute__((always_inline)) int piter_next(piter *it, rpiece *p) {
    if (it->i < it->tp->n) {
        const rhmm *h = it->tp->a[it->i];
        if (it->k == 0 && h->ref_start > it->pos) { /* gap: depth 0, one cell; (0, 0) merge column behind it (hmm.c:324-345) */
            p->end = h->ref_start; p->depth = 0; p->out = MRP_CONN_ZERO;
            it->pos = p->end;
            return 1;
        }
        const int32_t k = it->k;
        p->end = k + 1 < h->n_cols ? h->starts[k + 1] : h->ref_start + h->ref_length;
        p->depth = h->roff[k + 1] - h->roff[k];
        p->out = k + 1 < h->n_cols ? MRP_CONN_REAL : MRP_CONN_ZERO;
        it->pos = p->end;
        if (++it->k == h->n_cols) { it->i++; it->k = 0; }
        return 1;
    }
    if (it->pos < it->E) {
        p->end = it->E; p->depth = 0; p->out = MRP_CONN_ZERO;
        it->pos = it->E;
        return 1;
    }
    return 0;
}

/* The shadow of stRPHmm_createCrossProductOfTwoAlignedHmm (hmm.c:534-750) of two tiling paths: both are cut at the union
 * of their column boundaries (hmm.c:476-504, column.c:70-130); per column the host keeps its first site and its depth and
 * sums up the static bounds the engine sizes its launches with.  b may be empty: stRPHmm_fuse of path a alone. */
static int r_cross_build(const world *w, const r_hmm_vec *a, const r_hmm_vec *b, int32_t S, int32_t E, int32_t stride, rhmm **out) {
    (void) w;
    int64_t cap = 2, n_reads = 0;
    /* (the parents were written a level ago, often by another core: their arrays are asked for while the sizes are added up) */
    for (int64_t i = 0; i < a->n; i++) { const rhmm *p = a->a[i]; cap += p->n_cols + 1; n_reads += p->n_reads; __builtin_prefetch(p->starts); __builtin_prefetch(p->roff); __builtin_prefetch(p->reads); }
    for (int64_t i = 0; i < b->n; i++) { const rhmm *p = b->a[i]; cap += p->n_cols + 1; n_reads += p->n_reads; __builtin_prefetch(p->starts); __builtin_prefetch(p->roff); __builtin_prefetch(p->reads); }
    const size_t o_starts = (sizeof(rhmm) + 7) & ~(size_t) 7, o_roff = o_starts + 4 * (size_t) cap, o_reads = o_roff + 4 * (size_t) (cap + 1),
                 o_par = (o_reads + 4 * (size_t) n_reads + 7) & ~(size_t) 7, bytes = o_par + sizeof(mrp_xpar) * (size_t) (a->n + b->n);
    int cls = 0;
    char *blk = shadow_alloc(bytes, &cls);
    rhmm *h = (rhmm *) blk;
    memset(h, 0, sizeof(*h));
    h->pool_class = cls + 1;
    h->starts = (int32_t *) (blk + o_starts); h->roff = (int32_t *) (blk + o_roff); h->reads = (int32_t *) (blk + o_reads);
    h->par = (mrp_xpar *) (blk + o_par);
    h->ref_start = S; h->ref_length = E - S; h->seg = -2; /* set when its level is staged */
    h->n_a = (int32_t) a->n; h->n_b = (int32_t) b->n;
    {   /* stRPHmm.profileSeqs: path A's reads, then path B's (hmm.c:559-566); the parents as the device will look them up */
        int32_t *rd = h->reads;
        mrp_xpar *pr = h->par;
        const r_hmm_vec *side[2] = {a, b};
        for (int q = 0; q < 2; q++)
            for (int64_t i = 0; i < side[q]->n; i++) {
                const rhmm *p = side[q]->a[i];
                memcpy(rd, p->reads, sizeof(int32_t) * (size_t) p->n_reads);
                rd += p->n_reads;
                pr->start = p->ref_start; pr->end = p->ref_start + p->ref_length; pr->n_cols = p->n_cols; pr->seg = p->seg; pr->col0 = p->col0;
                pr++;
            }
        h->n_reads = (int32_t) n_reads;
        h->first_read = n_reads > 0 ? h->reads[0] : -1;
    }
    /* mrp_side_bound for every depth, once per thread and stride */
    static __thread int32_t sb_stride = -1;
    static __thread int32_t sb[MRP_MAX_READ_PARTITIONING_DEPTH + 2];
    if (sb_stride != stride) { for (int d = 0; d <= MRP_MAX_READ_PARTITIONING_DEPTH + 1; d++) sb[d] = (int32_t) mrp_side_bound(d, stride); sb_stride = stride; }
    piter ia = {a, 0, 0, S, E}, ib = {b, 0, 0, S, E};
    rpiece pa, pb;
    if (!piter_next(&ia, &pa) || !piter_next(&ib, &pb)) { rhmm_destroy(h); return mrp_set_error(MRP_ERR_ARG, "cross product of an empty interval"); }
    int32_t pos = S, n = 0;
    int64_t D = 0;
    int rc = MRP_OK;
    for (;;) {
        const int32_t end = pa.end < pb.end ? pa.end : pb.end;
        const int32_t d1 = pa.depth, d2 = pb.depth, depth = d1 + d2;
        if (depth > MRP_MAX_READ_PARTITIONING_DEPTH) {
            rc = mrp_set_error(MRP_ERR_ARG, "cross product column depth %d exceeds %d", depth, MRP_MAX_READ_PARTITIONING_DEPTH);
            break;
        }
        if (n >= cap || end <= pos) { rc = mrp_set_error(MRP_ERR_ARG, "cross product: inconsistent tiling paths"); break; }
        h->starts[n] = pos;
        h->roff[n] = (int32_t) D;
        D += depth;
        const int64_t C = (int64_t) sb[d1] * sb[d2];
        h->bound_cells += C;
        if (C > h->bound_max_cells) h->bound_max_cells = (int32_t) C;
        h->depth_sites += (int64_t) depth * (end - pos);
        if (end < E) { /* merge column hmm.c:686-740: a piece that is cut leaves through an accept-mask connector (column.c:86-101) */
            const uint8_t oa = pa.end > end ? MRP_CONN_IDENT : pa.out, ob = pb.end > end ? MRP_CONN_IDENT : pb.out;
            const int64_t Ma = oa == MRP_CONN_ZERO ? 1 : sb[d1], Mb = ob == MRP_CONN_ZERO ? 1 : sb[d2];
            h->bound_merge += Ma * Mb;
            if (Ma * Mb > h->bound_max_merge) h->bound_max_merge = (int32_t) (Ma * Mb);
        }
        n++;
        pos = end;
        if (pos >= E) break;
        if (pa.end == end && !piter_next(&ia, &pa)) { rc = mrp_set_error(MRP_ERR_ARG, "cross product: tiling path A ends early"); break; }
        if (pb.end == end && !piter_next(&ib, &pb)) { rc = mrp_set_error(MRP_ERR_ARG, "cross product: tiling path B ends early"); break; }
    }
    if (rc == MRP_OK && D > 0x7FFFFFFFll) rc = mrp_set_error(MRP_ERR_UNSUPPORTED, "cross product with %lld column reads", (long long) D);
    if (rc != MRP_OK) { rhmm_destroy(h); return rc; }
    h->roff[n] = (int32_t) D;
    h->n_cols = n;
    if (h->bound_max_cells < 1) h->bound_max_cells = 1;
    if (h->bound_max_merge < 1) h->bound_max_merge = 1;
    *out = h;
    return MRP_OK;
}

/* A shadow as an ordinary flat hmm WITHOUT cells: column intervals, the reads of every column in bit order and where their
 * profile bytes start (profileSeq.c:41-47), and -- with_masks -- the masks of the merge columns (the reads of a column that
 * go on into the next one, in the bit positions of either column: what hmm.c:686-700 computes by merging the parents'
 * masks).  A column's reads are the hmm's reads that cover it, in the order of stRPHmm.profileSeqs: side A's reads precede
 * side B's in both (partitions.c:21-28, hmm.c:559-566), recursively. */
static mrp_hmm *r_expand(const world *w, const rhmm *x, int with_masks) {
    mrp_hmm *h = hmm_new();
    const int64_t K = x->n_cols, D = x->roff[K];
    h->ref_start = x->ref_start; h->ref_length = x->ref_length;
    VEC_RESERVE(h->reads, x->n_reads);
    memcpy(h->reads.a, x->reads, sizeof(int32_t) * (size_t) x->n_reads); h->reads.n = x->n_reads;
    VEC_RESERVE(h->col_start, K); VEC_RESERVE(h->col_len, K); VEC_RESERVE(h->col_depth, K);
    VEC_RESERVE(h->read_off, K + 1); VEC_RESERVE(h->cell_off, K + 1);
    VEC_RESERVE(h->col_reads, D + 1); VEC_RESERVE(h->read_byte_off, D + 1);
    const int32_t E = x->ref_start + x->ref_length;
    h->read_off.n = 0; h->cell_off.n = 0;
    for (int64_t k = 0; k < K; k++) {
        h->col_start.a[k] = x->starts[k];
        h->col_len.a[k] = (k + 1 < K ? x->starts[k + 1] : E) - x->starts[k];
        h->col_depth.a[k] = x->roff[k + 1] - x->roff[k];
        if (h->col_depth.a[k] > h->max_depth) h->max_depth = h->col_depth.a[k];
        h->read_off.a[k] = x->roff[k];
        h->cell_off.a[k] = 0;
    }
    h->read_off.a[K] = D; h->cell_off.a[K] = 0;
    h->col_start.n = h->col_len.n = h->col_depth.n = K;
    h->read_off.n = h->cell_off.n = K + 1;
    h->col_reads.n = h->read_byte_off.n = D;
    int32_t *fill = xmalloc(sizeof(int32_t) * (size_t) (K + 1));
    memcpy(fill, x->roff, sizeof(int32_t) * (size_t) (K + 1));
    int ok = 1;
    for (int64_t i = 0; i < x->n_reads && ok; i++) {
        const int32_t rd = x->reads[i];
        const mrp_read *r = &w->reads[rd];
        int64_t lo = 0, hi = K; /* the column that starts where the read does */
        while (lo < hi) { const int64_t mid = (lo + hi) >> 1; if (x->starts[mid] < r->ref_start) lo = mid + 1; else hi = mid; }
        if (lo >= K || x->starts[lo] != r->ref_start) { ok = 0; break; }
        for (int64_t k = lo; k < K && x->starts[k] < r->ref_start + r->length; k++) {
            if (fill[k] >= x->roff[k + 1]) { ok = 0; break; }
            h->col_reads.a[fill[k]] = rd;
            h->read_byte_off.a[fill[k]] = read_byte_offset(w, rd, x->starts[k]);
            fill[k]++;
        }
    }
    for (int64_t k = 0; k < K && ok; k++) if (fill[k] != x->roff[k + 1]) ok = 0;
    free(fill);
    if (!ok) { mrp_hmm_destroy(h); mrp_set_error(MRP_ERR_ARG, "shadow hmm: the column depths do not match the reads' intervals"); return NULL; }
    if (with_masks)
        for (int64_t k = 0; k + 1 < K; k++) {
            uint64_t mf = 0, mt = 0;
            const int32_t cut = x->starts[k + 1];
            const int32_t *ra = h->col_reads.a + h->read_off.a[k], *rb = h->col_reads.a + h->read_off.a[k + 1];
            for (int32_t i = 0; i < h->col_depth.a[k]; i++) if (w->reads[ra[i]].ref_start + w->reads[ra[i]].length > cut) mf |= (uint64_t) 1 << i;
            for (int32_t i = 0; i < h->col_depth.a[k + 1]; i++) if (w->reads[rb[i]].ref_start < cut) mt |= (uint64_t) 1 << i;
            VEC_PUSH(h->mask_from, mf); VEC_PUSH(h->mask_to, mt);
        }
    return h;
}

/* a cross product of a level: its shadow, its chunk, and -- filled by the thread that built it, while the shadow is in its cache --
 * what the engine is told about it (r_describe) */
typedef struct { rhmm *x; const world *w; mrp_xhmm d; } xbuild;
typedef VEC(xbuild) xbuild_vec;

/* mergeTwoTilingPaths coordination.c:263-339, structure only: the overlap components that need a cross
 * product are appended to xs (and, unpruned, to res); the others pass through */
static int64_t g_ns[6]; /* MRP_TIMING: components, tiling paths, cross shadows, destroy */
/* (only under MRP_TIMING: the thread CPU clock is a system call, and r_prepare_merge would make six of them per overlap
 * component -- 700 000 per call, 0.2 s of CPU) */
static int g_prepare_timing;
static double tcpu_ms(void) {
    if (!g_prepare_timing) return 0.0;
    struct timespec t; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &t); return 1e3 * (double) t.tv_sec + 1e-6 * (double) t.tv_nsec;
}
#define T_ADD(slot, t0) do { if (g_prepare_timing) __atomic_fetch_add(&g_ns[slot], (int64_t) ((tcpu_ms() - (t0)) * 1e6), __ATOMIC_RELAXED); } while (0)
static int r_prepare_merge(const world *w, int32_t stride, r_hmm_vec *tp1, r_hmm_vec *tp2, r_hmm_vec *res, xbuild_vec *xs) {
    double tq = tcpu_ms();
    ar_on();
    r_comp_vec comps = r_overlapping_components(w, tp1, tp2);
    ar_off();
    T_ADD(0, tq);
    r_path_release(tp1); r_path_release(tp2);
    int rc = MRP_OK;
    for (int64_t i = 0; i < comps.n; i++) {
        r_component *comp = comps.a[i];
        if (rc == MRP_OK && comp->members.n == 1) { /* nothing overlaps it: passes through (coordination.c:317-322) */
            VEC_PUSH(*res, comp->members.a[0]);
        } else if (rc == MRP_OK && comp->members.n == 2) {
            /* two hmms that overlap -- the common case -- are two tiling paths of one hmm each, the smaller one by stRPHmm_cmpFn
             * first (getTilingPaths sorts, coordination.c:186-190): no lists to build */
            rhmm *m0 = comp->members.a[0], *m1 = comp->members.a[1];
            if (r_hmm_cmp(w, m0, m1) > 0) { rhmm *t_ = m0; m0 = m1; m1 = t_; }
            rhmm *ma[1] = {m0}, *mb[1] = {m1};
            const r_hmm_vec va = {ma, 1, 1}, vb = {mb, 1, 1};
            const int32_t S = m0->ref_start < m1->ref_start ? m0->ref_start : m1->ref_start;
            const int32_t Ea = m0->ref_start + m0->ref_length, Eb = m1->ref_start + m1->ref_length;
            xbuild xb; xb.x = NULL; xb.w = w;
            tq = tcpu_ms();
            rc = r_cross_build(w, &va, &vb, S, Ea > Eb ? Ea : Eb, stride, &xb.x);
            T_ADD(2, tq);
            /* the parents' shadows are no longer needed (their cells stay in the engine's segments; what the engine was told of
             * them it copied when their level was staged): back to THIS thread's front of the pool, warm for its next hmm */
            rhmm_destroy(m0); rhmm_destroy(m1);
            if (rc == MRP_OK) { VEC_PUSH(*xs, xb); VEC_PUSH(*res, xb.x); }
        } else if (rc == MRP_OK) {
            tq = tcpu_ms();
            ar_on();
            r_path_vec sub = r_tiling_paths_from(w, comp->members.a, comp->members.n);
            ar_off();
            T_ADD(1, tq);
            if (sub.n == 2) {
                r_hmm_vec *a = sub.a[0], *b = sub.a[1];
                int32_t S = a->a[0]->ref_start < b->a[0]->ref_start ? a->a[0]->ref_start : b->a[0]->ref_start;
                int32_t Ea = a->a[a->n - 1]->ref_start + a->a[a->n - 1]->ref_length;
                int32_t Eb = b->a[b->n - 1]->ref_start + b->a[b->n - 1]->ref_length;
                int32_t E = Ea > Eb ? Ea : Eb;
                xbuild xb; xb.x = NULL; xb.w = w;
                tq = tcpu_ms();
                rc = r_cross_build(w, a, b, S, E, stride, &xb.x);
                T_ADD(2, tq);
                for (int64_t t = 0; t < a->n; t++) rhmm_destroy(a->a[t]);
                for (int64_t t = 0; t < b->n; t++) rhmm_destroy(b->a[t]);
                if (rc == MRP_OK) { VEC_PUSH(*xs, xb); VEC_PUSH(*res, xb.x); }
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
    ar_rewind(); /* every temporary of this merge is gone */
    return rc;
}

/* the recursion tree of mergeTilingPaths (coordination.c:341-409) over all problems of a run */
typedef struct {
    int left, right;   /* children (node indices) or -1 */
    int height;        /* 0: a tiling path as it is; h > 0: merged at level h */
    const world *w;
    r_hmm_vec *path;   /* the node's tiling path once its level is done (owned) */
} rnode;
typedef VEC(rnode) rnode_vec;

static int r_leaf_node(rnode_vec *t, const world *w, r_hmm_vec *path) {
    rnode nd = {-1, -1, 0, w, path};
    VEC_PUSH(*t, nd);
    return (int) t->n - 1;
}
static int r_merge_node(rnode_vec *t, const world *w, int l, int r) {
    const int hl = t->a[l].height, hr = t->a[r].height;
    rnode nd = {l, r, 1 + (hl > hr ? hl : hr), w, NULL};
    VEC_PUSH(*t, nd);
    return (int) t->n - 1;
}
static int r_tree_of_paths(rnode_vec *t, const world *w, r_hmm_vec **paths, int64_t n) {
    if (n == 0) return r_leaf_node(t, w, xcalloc(1, sizeof(r_hmm_vec)));
    if (n == 1) return r_leaf_node(t, w, paths[0]);
    if (n == 2) return r_merge_node(t, w, r_leaf_node(t, w, paths[0]), r_leaf_node(t, w, paths[1]));
    const int l = r_tree_of_paths(t, w, paths, n / 2);
    const int r = r_tree_of_paths(t, w, paths + n / 2, n - n / 2);
    return r_merge_node(t, w, l, r);
}
/* getRPHmms coordination.c:490-516 as a subtree over leaves given in stRPHmm_cmpFn order (a chunk's leaves are sorted once:
 * the coverage filter and both strands walk the same order); returns the root node or -1 */
static int r_tree_of_sorted(rnode_vec *t, const world *w, rhmm *const *hmms, int64_t n, const mrp_params *params) {
    r_path_vec paths = r_tiling_paths_sorted(hmms, n);
    if (paths.n > MRP_MAX_READ_PARTITIONING_DEPTH || paths.n > params->max_coverage_depth) { /* :500-504 */
        const int64_t np = paths.n;
        for (int64_t i = 0; i < paths.n; i++) r_free_path(paths.a[i], 0);
        free(paths.a);
        mrp_set_error(MRP_ERR_ARG, "Coverage depth: read depth of %lld exceeds hard maximum of %d with configured maximum of %lld",
                      (long long) np, MRP_MAX_READ_PARTITIONING_DEPTH, (long long) params->max_coverage_depth);
        return -1;
    }
    /* the leaf paths as blocks of the shadow pool: the merge that consumes one (another thread, a level later) gives a block back
     * to its own front instead of freeing into this thread's malloc arena */
    for (int64_t i = 0; i < paths.n; i++) {
        r_hmm_vec *tp = paths.a[i];
        const size_t o_a = (sizeof(r_hmm_vec) + 15) & ~(size_t) 15;
        int cls = 0;
        char *blk = shadow_alloc(o_a + sizeof(rhmm *) * (size_t) (tp->n + 1), &cls);
        if (cls < 0) { free(blk); continue; } /* (beyond the pool's classes: stays as it is) */
        r_hmm_vec *v = (r_hmm_vec *) blk;
        v->a = (rhmm **) (blk + o_a); v->n = tp->n; v->cap = -(int64_t) cls - 2;
        memcpy(v->a, tp->a, sizeof(rhmm *) * (size_t) tp->n);
        free(tp->a); free(tp);
        paths.a[i] = v;
    }
    const int root = r_tree_of_paths(t, w, paths.a, paths.n);
    free(paths.a);
    return root;
}

static void r_free_tree(rnode_vec *t) {
    for (int64_t i = 0; i < t->n; i++) r_free_path(t->a[i].path, 1);
    free(t->a);
    t->a = NULL; t->n = t->cap = 0;
}

/* run every merge node, level by level */
static __thread double g_t_prepare, g_t_level; /* MRP_TIMING diagnostics of the calling thread */
typedef struct {
    rnode_vec *t;
    int64_t node;
    int32_t stride;
    uint32_t flags;    /* sweep_flags of the run: part of what the engine is told about every cross product */
    r_hmm_vec *res;
    xbuild_vec xs;
    int rc, res_class;
    int64_t x0;        /* where the item's cross products start in the level's list */
    void *big_block;
    char err[256];
} level_item;
static void r_describe(const world *w, const rhmm *x, uint32_t flags, mrp_xhmm *d);
static void level_prepare(int64_t i, void *arg) {
    level_item *it = &((level_item *) arg)[i];
    rnode *nd = &it->t->a[it->node];
    r_hmm_vec *l = it->t->a[nd->left].path, *r = it->t->a[nd->right].path;
    it->t->a[nd->left].path = NULL; it->t->a[nd->right].path = NULL;
    {   /* the merged path and the cross products to build: at most one entry per hmm of the two paths each.  ONE block of the
         * shadow pool, owned by the path (released when the next level consumes it; the list of cross products is read by the
         * thread that drives the batch before that) -- no malloc / free across threads */
        const int64_t cap = l->n + r->n + 1;
        const size_t o_res = (sizeof(r_hmm_vec) + 15) & ~(size_t) 15, o_xs = o_res + sizeof(rhmm *) * (size_t) cap,
                     bytes = o_xs + sizeof(xbuild) * (size_t) cap;
        int cls = 0;
        char *blk = shadow_alloc(bytes, &cls);
        it->res = (r_hmm_vec *) blk;
        it->res->a = (rhmm **) (blk + o_res); it->res->n = 0; it->res->cap = cap;
        it->xs.a = (xbuild *) (blk + o_xs); it->xs.n = 0; it->xs.cap = cap;
        it->res_class = cls;
    }
    it->rc = r_prepare_merge(nd->w, it->stride, l, r, it->res, &it->xs);
    for (int64_t j = 0; j < it->xs.n && it->rc == MRP_OK; j++) r_describe(it->xs.a[j].w, it->xs.a[j].x, it->flags, &it->xs.a[j].d);
    if (it->res_class >= 0) it->res->cap = -(int64_t) it->res_class - 2;
    else { /* (a path beyond the pool's largest class: an ordinary vector again) */
        r_hmm_vec *v = xcalloc(1, sizeof(*v));
        v->a = xmalloc(sizeof(rhmm *) * (size_t) (it->res->n + 1)); memcpy(v->a, it->res->a, sizeof(rhmm *) * (size_t) it->res->n);
        v->n = it->res->n; v->cap = it->res->n + 1;
        it->big_block = it->res; it->res = v;
    }
    if (it->rc != MRP_OK) snprintf(it->err, sizeof(it->err), "%s", mrp_last_error());
}
static void level_drop_garbage(int64_t i, void *arg) { /* (the parents' shadows went back to the pool in r_prepare_merge) */
    level_item *it = &((level_item *) arg)[i];
    if (it->big_block) { free(it->big_block); it->big_block = NULL; }
}
static void level_finish(int64_t i, void *arg) {
    level_item *it = &((level_item *) arg)[i];
    rnode *nd = &it->t->a[it->node];
    r_sort_hmms(nd->w, it->res->a, it->res->n); /* coordination.c:336 */
}
/* a shadow as the engine is told about it */
static void r_describe(const world *w, const rhmm *x, uint32_t flags, mrp_xhmm *d) {
    memset(d, 0, sizeof(*d));
    d->chunk = w->chunk; d->flags = flags; d->discarded = &w->failed;
    d->ref_start = x->ref_start; d->ref_end = x->ref_start + x->ref_length;
    d->n_cols = x->n_cols; d->n_a = x->n_a; d->n_b = x->n_b; d->par = x->par;
    d->col_start = x->starts; d->col_read_off = x->roff;
    d->bound_cells = x->bound_cells; d->bound_merge = x->bound_merge; d->depth_sites = x->depth_sites;
    d->bound_max_cells = x->bound_max_cells; d->bound_max_merge = x->bound_max_merge;
    d->n_col_reads = x->roff[x->n_cols];
    d->n_slots = (int64_t) w->ch.allele_offset[x->ref_start + x->ref_length] - (int64_t) w->ch.allele_offset[x->ref_start];
}
typedef struct { rhmm *x; const world *w; } xowner; /* what the host keeps of a cross product while its level is on the device */
typedef struct { level_item *items; mrp_xhmm *xh; xowner *xb; } level_gather_ctl;
static void level_gather(int64_t i, void *arg) { /* (the descriptions were written by level_prepare, one item's side by side: a copy) */
    const level_gather_ctl *g = arg;
    const level_item *it = &g->items[i];
    for (int64_t j = 0; j < it->xs.n; j++) {
        g->xb[it->x0 + j].x = it->xs.a[j].x; g->xb[it->x0 + j].w = it->xs.a[j].w;
        g->xh[it->x0 + j] = it->xs.a[j].d;
    }
}
/* what the host keeps of a level while it is on the device */
typedef struct {
    level_item *items; int64_t n_items;
    mrp_xhmm *xh; xowner *xb; int64_t n_x;
    int cls_items, cls_xh, cls_xb; /* the three lists are blocks of the shadow pool (megabytes per level: warm instead of mapped afresh) */
    int64_t seq;                   /* the level is the seq-th the engine launched: over once mrp_engine_levels_ended() reaches seq */
} level_run;
/* the levels launched and not yet settled, oldest first (the engine ends small levels late: several are in flight at a time) */
#define LEVEL_RUNS_MAX 72
typedef struct { level_run r[LEVEL_RUNS_MAX]; int head, tail; int64_t launched; } level_runs;
static void level_run_settle(level_run *r, int rc_ok) { /* the level has ended: its error flags are in */
    for (int64_t i = 0; i < r->n_x; i++)
        /* outside what the kernels handle (a parent not in complement-pair order, ...): the later levels leave this
         * chunk out, its caller redoes it on the hashing path */
        if (rc_ok && r->xh[i].err != 0) ((world *) r->xb[i].w)->failed = 1;
    if (r->xh) shadow_release(r->xh, r->cls_xh);
    if (r->xb) shadow_release(r->xb, r->cls_xb);
    if (r->items) shadow_release(r->items, r->cls_items);
    memset(r, 0, sizeof(*r));
}
/* the levels the engine has ended (all of them: `all`, after mrp_engine_level_end or a launch that waited) */
static void level_runs_settle(level_runs *q, mrp_engine *e, int rc_ok, int all) {
    const int64_t ended = mrp_engine_levels_ended(e);
    while (q->head < q->tail && (all || q->r[q->head].seq <= ended)) level_run_settle(&q->r[q->head++], rc_ok);
    if (q->head == q->tail) q->head = q->tail = 0;
}
/* pending: if not NULL the levels still in flight are left there (the caller stages what comes next beside them, then launches / ends
 * and settles them); otherwise they are ended here */
static int r_run_tree(mrp_engine *e, rnode_vec *t, const mrp_params *params, level_runs *pending) {
    int max_h = 0;
    for (int64_t i = 0; i < t->n; i++) if (t->a[i].height > max_h) max_h = t->a[i].height;
    /* Level of a merge node = as late as its parent allows (every root at the last level), not its height: the merges
     * near the roots are the expensive ones (a workgroup walks ~10^3 columns of ~10^4 cells one after the other) and a
     * level costs what its longest hmm costs, so they should share their levels -- a problem one merge deeper than the
     * others then adds a level of small leaf merges instead of a level with a single large hmm on an idle device. */
    int *lvl = xmalloc(sizeof(int) * (size_t) (t->n + 1));
    for (int64_t i = 0; i < t->n; i++) lvl[i] = -1;
    for (int64_t i = t->n - 1; i >= 0; i--) { /* children precede their parent */
        if (lvl[i] < 0) lvl[i] = max_h;
        if (t->a[i].left >= 0) { lvl[t->a[i].left] = lvl[i] - 1; lvl[t->a[i].right] = lvl[i] - 1; }
    }
    const uint32_t flags = sweep_flags(params);
    const int32_t stride = mrp_engine_stride(e);
    int rc = MRP_OK;
    /* The host's part of level h -- which hmms are merged, their column boundaries -- needs nothing the device computes
     * (only WHERE level h - 1's results are, fixed when that level was staged): it is done while level h - 1 runs.  The one
     * wait per level is inside mrp_engine_level_launch. */
    level_runs own = {0}, *runs = pending ? pending : &own;
    for (int h = 1; h <= max_h && rc == MRP_OK; h++) {
        const double t0 = now_ms();
        int64_t n_items = 0;
        for (int64_t i = 0; i < t->n; i++) if (t->a[i].height > 0 && lvl[i] == h && !t->a[i].w->failed) n_items++;
        if (n_items == 0) continue;
        int cls_items = -1, cls_xh = -1, cls_xb = -1;
        level_item *items = shadow_alloc(sizeof(*items) * ((size_t) n_items + 1), &cls_items);
        memset(items, 0, sizeof(*items) * ((size_t) n_items + 1));
        n_items = 0;
        for (int64_t i = 0; i < t->n; i++) if (t->a[i].height > 0 && lvl[i] == h && !t->a[i].w->failed) { items[n_items].t = t; items[n_items].node = i; items[n_items].stride = stride; items[n_items].flags = flags; n_items++; }
        /* the merges of a level touch disjoint nodes: structure in parallel, device work as one batch */
        mrp_pool_set_tag(1); mrp_pool_set_weight(8000); mrp_pool_run(n_items, n_items > 512 ? (n_items > 16384 ? 64 : n_items / 256) : 1, level_prepare, items); mrp_pool_set_weight(0); mrp_pool_set_tag(0);
        const double ta = now_ms();
        int64_t n_x = 0;
        for (int64_t i = 0; i < n_items; i++) {
            n_x += items[i].xs.n;
            if (items[i].rc != MRP_OK && rc == MRP_OK) rc = mrp_set_error(items[i].rc, "%s", items[i].err);
        }
        mrp_xhmm *xh = shadow_alloc(sizeof(*xh) * ((size_t) n_x + 1), &cls_xh);
        xowner *xb = shadow_alloc(sizeof(*xb) * ((size_t) n_x + 1), &cls_xb);
        n_x = 0;
        for (int64_t i = 0; i < n_items; i++) { items[i].x0 = n_x; n_x += items[i].xs.n; }
        {   /* the level as the engine is told about it, in node order (worker threads: the shadows are in their caches) */
            level_gather_ctl gc = {items, xh, xb};
            mrp_pool_set_tag(3); mrp_pool_set_weight(400); mrp_pool_run(n_items, n_items > 512 ? n_items / 256 : 1, level_gather, &gc); mrp_pool_set_weight(0); mrp_pool_set_tag(0);
        }
        for (int64_t i = 0; i < n_items; i++) /* coordination.c:312: one forward/backward per overlap component */
            ((world *) t->a[items[i].node].w)->n_sweeps += (int) items[i].xs.n, items[i].xs.a = NULL; /* (the list is part of the path's block) */
        const double tb = now_ms();
        if (rc == MRP_OK) rc = mrp_engine_level_stage(e, n_x, xh);
        const double tc = now_ms();
        /* where the level's results will be is known from here on: the next level can be described against them */
        for (int64_t i = 0; i < n_x && rc == MRP_OK; i++) { xb[i].x->seg = xh[i].seg; xb[i].x->col0 = xh[i].col0; }
        mrp_pool_set_tag(2); mrp_pool_set_weight(300); if (rc == MRP_OK) mrp_pool_run(n_items, n_items > 512 ? (n_items > 16384 ? 64 : n_items / 256) : 1, level_finish, items); mrp_pool_set_weight(0); mrp_pool_set_tag(0);
        for (int64_t i = 0; i < n_items; i++) t->a[items[i].node].path = items[i].res;
        const double t1 = now_ms();
        /* level h goes to the device (a large level first waits for the levels before it, a small one does not) */
        int launched = 0;
        if (rc == MRP_OK) { rc = mrp_engine_level_launch(e); launched = rc == MRP_OK && n_x > 0; /* (an empty level is not staged: the launch only ends what runs) */ }
        else (void) mrp_engine_level_end(e);
        level_runs_settle(runs, e, rc == MRP_OK, rc != MRP_OK);
        const double t2 = now_ms();
        for (int64_t i = 0; i < n_items; i++) level_drop_garbage(i, items);
        (void) t2;
        g_t_prepare += t1 - t0; g_t_level += now_ms() - t1;
        if (getenv("MRP_TIMING"))
            fprintf(stderr, "    host level %d: prepare %.2f ms, gather %.2f, stage %.2f, sort %.2f | launch (waits for the level before) %.2f | settle+garbage %.2f\n",
                    h, ta - t0, tb - ta, tc - tb, t1 - tc, t2 - t1, now_ms() - t2);
        {
            level_run cur = {items, n_items, xh, xb, n_x, cls_items, cls_xh, cls_xb, 0};
            if (launched && runs->tail < LEVEL_RUNS_MAX) { cur.seq = ++runs->launched; runs->r[runs->tail++] = cur; }
            else { /* (not launched: the engine holds nothing of it; a queue that is full cannot happen -- the engine has 64 segments) */
                if (launched) { (void) mrp_engine_level_end(e); level_runs_settle(runs, e, rc == MRP_OK, 1); }
                level_run_settle(&cur, launched && rc == MRP_OK);
            }
        }
    }
    if (!(pending && rc == MRP_OK)) {
        const double t1 = now_ms();
        const int rc2 = mrp_engine_level_end(e);
        if (rc == MRP_OK) rc = rc2;
        level_runs_settle(runs, e, rc == MRP_OK, 1);
        g_t_level += now_ms() - t1;
    }
    free(lvl);
    return rc;
}

/* resident shadow -> ordinary flat hmm on the host; phase 0 queues the copies, phase 1 (after
 * mrp_engine_sync) unpacks them */
typedef struct { mrp_hmm *h; uint64_t *part; uint32_t *np; int32_t *n_cells, *n_merge; int32_t stride; } r_staging;
static int r_download_begin(mrp_engine *e, const world *w, const rhmm *x, r_staging *st) {
    memset(st, 0, sizeof(*st));
    st->h = r_expand(w, x, 1);
    if (!st->h) return MRP_ERR_ARG;
    if (x->seg < 0) return MRP_OK; /* a stRPHmm_construct hmm: nothing to fetch */
    const int64_t K = x->n_cols;
    st->stride = mrp_engine_stride(e);
    const int64_t n = K * st->stride;
    const uint64_t *d_part; const uint32_t *d_np; const int32_t *d_nc, *d_nm;
    int rc = mrp_engine_locate(e, x->seg, x->col0, &d_part, &d_np, &d_nc, &d_nm);
    if (rc != MRP_OK) return rc;
    st->part = xmalloc(sizeof(uint64_t) * (size_t) n);
    st->np = xmalloc(sizeof(uint32_t) * (size_t) n);
    st->n_cells = xmalloc(sizeof(int32_t) * (size_t) K);
    st->n_merge = xmalloc(sizeof(int32_t) * (size_t) K);
    rc = mrp_engine_fetch(e, st->part, d_part, (int64_t) sizeof(uint64_t) * n);
    if (rc == MRP_OK) rc = mrp_engine_fetch(e, st->np, d_np, (int64_t) sizeof(uint32_t) * n);
    if (rc == MRP_OK) rc = mrp_engine_fetch(e, st->n_cells, d_nc, (int64_t) sizeof(int32_t) * K);
    if (rc == MRP_OK) rc = mrp_engine_fetch(e, st->n_merge, d_nm, (int64_t) sizeof(int32_t) * K);
    return rc;
}
static void r_staging_free(r_staging *st) { free(st->part); free(st->np); free(st->n_cells); free(st->n_merge); memset(st, 0, sizeof(*st)); }
static mrp_hmm *r_download_end(r_staging *st) {
    mrp_hmm *h = st->h;
    const int64_t K = hmm_K(h);
    h->cell_off.n = 0; h->mcell_off.n = 0;
    VEC_PUSH(h->cell_off, 0);
    VEC_PUSH(h->mcell_off, 0);
    if (!st->part) { /* hmm.c:97-133 */
        hmm_add_cell(h, 1, 0);
        hmm_add_cell(h, 0, 0);
        VEC_PUSH(h->cell_off, h->part.n);
    } else {
        for (int64_t k = 0; k < K; k++) {
            const int64_t o = k * st->stride;
            for (int32_t i = 0; i < st->n_cells[k]; i++) {
                hmm_add_cell(h, st->part[o + i], st->np[o + i] >> 16);
                h->next.a[h->next.n - 1] = st->np[o + i] & 0xFFFFu;
            }
            VEC_PUSH(h->cell_off, h->part.n);
            if (k + 1 < K) {
                for (int32_t m = 0; m < st->n_merge[k]; m++) { VEC_PUSH(h->mfrom, 0); VEC_PUSH(h->mto, 0); }
                VEC_PUSH(h->mcell_off, h->mfrom.n);
            }
        }
        /* a merge cell's keys are the masked partition of any cell that feeds it / is fed by it
         * (mergeColumn.c:63-79); every merge cell the prune keeps has both */
        for (int64_t k = 0; k < K; k++)
            for (int64_t c = h->cell_off.a[k]; c < h->cell_off.a[k + 1]; c++) {
                if (k + 1 < K) h->mfrom.a[h->mcell_off.a[k] + h->next.a[c]] = h->part.a[c] & h->mask_from.a[k];
                if (k > 0) h->mto.a[h->mcell_off.a[k - 1] + h->prev.a[c]] = h->part.a[c] & h->mask_to.a[k - 1];
            }
    }
    st->h = NULL;
    r_staging_free(st);
    return h;
}
static int r_download_path(mrp_engine *e, const world *w, const r_hmm_vec *tp, mrp_hmm ***out) {
    r_staging *st = xcalloc((size_t) tp->n + 1, sizeof(*st));
    mrp_hmm **res = xcalloc((size_t) tp->n + 1, sizeof(*res));
    int rc = MRP_OK;
    for (int64_t i = 0; i < tp->n && rc == MRP_OK; i++) rc = r_download_begin(e, w, tp->a[i], &st[i]);
    if (rc == MRP_OK) rc = mrp_engine_sync(e);
    for (int64_t i = 0; i < tp->n; i++) {
        if (rc == MRP_OK) res[i] = r_download_end(&st[i]);
        else { mrp_hmm_destroy(st[i].h); st[i].h = NULL; r_staging_free(&st[i]); }
    }
    free(st);
    if (rc != MRP_OK) { free(res); res = NULL; }
    *out = res;
    return rc;
}

int mrp_get_rp_hmms_resident(mrp_context *ctx, const mrp_chunk *chunk, const mrp_read *reads, const int32_t *read_index,
                             int64_t n, const mrp_params *params, mrp_hmm ***hmms_out, int64_t *n_out) {
    if (!params || !hmms_out || !n_out || n < 0 || (n > 0 && !read_index)) return mrp_set_error(MRP_ERR_ARG, "mrp_get_rp_hmms_resident: bad arguments");
    int64_t max_idx = -1;
    for (int64_t i = 0; i < n; i++) { if (read_index[i] < 0) return mrp_set_error(MRP_ERR_ARG, "negative read index"); if (read_index[i] > max_idx) max_idx = read_index[i]; }
    world w;
    int rc = world_init(&w, ctx, chunk, reads, max_idx + 1, NULL);
    if (rc != MRP_OK) return rc;
    mrp_engine *e = NULL;
    rc = mrp_engine_create(ctx, params, &e);
    if (rc != MRP_OK) return rc;
    int leaves_class = -1;
    rleaf *leaves = r_leaves_of_chunk(&w, &leaves_class);
    rnode_vec tree = {0};
    rhmm **picked = xmalloc(sizeof(*picked) * (size_t) (n + 1));
    for (int64_t i = 0; i < n; i++) picked[i] = &leaves[read_index[i]].h;
    r_sort_hmms(&w, picked, n);
    const int root = r_tree_of_sorted(&tree, &w, picked, n, params);
    free(picked);
    rc = root < 0 ? MRP_ERR_ARG : r_run_tree(e, &tree, params, NULL);
    if (rc == MRP_OK && w.failed) rc = mrp_set_error(MRP_ERR_UNSUPPORTED, "device-resident merge: an hmm outside what the kernels handle (pair order / kept merge cells)");
    if (rc == MRP_OK) {
        mrp_hmm **res = NULL;
        rc = r_download_path(e, &w, tree.a[root].path, &res);
        if (rc == MRP_OK) { *n_out = tree.a[root].path->n; *hmms_out = res; }
    }
    r_free_tree(&tree);
    shadow_release(leaves, leaves_class);
    mrp_engine_destroy(e);
    return rc;
}

/* bubbleGraph_phaseBubbleGraph (bubbleGraph.c:2673-2801) for a set of chunks at once: the loop body of
 * phase.c:276-473 that phases one chunk, with the merge levels of all chunks run together */
typedef struct {
    world w;
    int32_t *discarded; int64_t nd;
    int root;            /* node of the joined tiling path (in the chunk's own tree, then in the run's tree) */
    rnode_vec tree;      /* the chunk's subtree while it is being set up */
    rhmm *hmm;           /* shadow of the fused final hmm */
    int32_t *path;       /* traced-back cell per column */
    uint64_t *chosen;    /* and its partition */
    double fwd, bwd;
    int64_t final_index;
    rleaf *leaves;       /* leaf shadows of all reads of the chunk */
    int leaves_class;
    int rc;
    char err[256];
    /* the genome fragment as the device leaves it (mrp_xhmm.frag_*): 20 bytes per site, the two read lists */
    int32_t *by_pool, *frag_reads1, *frag_reads2;
    void *frag_sites;
    int32_t frag_n1, frag_n2, frag_done;
} many_state;

typedef struct {
    many_state *st;
    mrp_context *ctx;
    const mrp_chunk *const *chunks;
    const mrp_read *const *reads;
    const int64_t *n_reads;
    const mrp_params *params, *pc;
    mrp_engine *e;
    rnode_vec *tree;
    mrp_phase_result **out;
    mrp_xhmm *xfinal;
    uint32_t final_flags;
} many_ctl;

/* bubbleGraph.c:2699-2745 for one chunk: coverage filter, strand split, the two getRPHmms subtrees and their join */
static void many_setup(int64_t c, void *arg) {
    many_ctl *ctl = arg;
    many_state *m = &ctl->st[c];
    m->root = -1;
    m->rc = world_init(&m->w, ctl->ctx, ctl->chunks[c], ctl->reads[c], ctl->n_reads[c], NULL);
    if (m->rc == MRP_OK && ctl->n_reads[c] > 0) {
        const int64_t nr = ctl->n_reads[c];
        m->leaves = r_leaves_of_chunk(&m->w, &m->leaves_class);
        /* every getTilingPaths of the chunk (coverage filter, either strand) starts by sorting its hmms with stRPHmm_cmpFn
         * (coordination.c:186-190): the leaves are sorted once, subsets keep the order */
        rhmm **sorted = xmalloc(sizeof(*sorted) * (size_t) (nr + 1));
        for (int64_t i = 0; i < nr; i++) sorted[i] = &m->leaves[i].h;
        r_sort_hmms(&m->w, sorted, nr);
        int32_t *filtered = xmalloc(sizeof(int32_t) * (size_t) nr);
        m->discarded = xmalloc(sizeof(int32_t) * (size_t) nr);
        int64_t nf;
        r_filter_reads_by_coverage_depth(&m->w, sorted, ctl->params, filtered, &nf, m->discarded, &m->nd); /* :2699 */
        uint8_t *is_disc = xcalloc((size_t) nr, 1);
        for (int64_t i = 0; i < m->nd; i++) is_disc[m->discarded[i]] = 1;
        rhmm **fwd = xmalloc(sizeof(*fwd) * (size_t) (nr + 1)), **rev = xmalloc(sizeof(*rev) * (size_t) (nr + 1));
        int64_t nfwd = 0, nrev = 0;
        for (int64_t i = 0; i < nr; i++) { /* :2705-2716 */
            const int32_t rd = sorted[i]->first_read;
            if (is_disc[rd]) continue;
            if (ctl->reads[c][rd].forward_strand) fwd[nfwd++] = sorted[i]; else rev[nrev++] = sorted[i];
        }
        const int rf = r_tree_of_sorted(&m->tree, &m->w, fwd, nfwd, ctl->pc);   /* :2736 */
        const int rr = rf < 0 ? -1 : r_tree_of_sorted(&m->tree, &m->w, rev, nrev, ctl->pc); /* :2740 */
        if (rf < 0 || rr < 0) m->rc = MRP_ERR_ARG;
        else m->root = r_merge_node(&m->tree, &m->w, rf, rr);                         /* :2745 */
        free(filtered); free(is_disc); free(fwd); free(rev); free(sorted);
    }
    if (m->rc != MRP_OK) snprintf(m->err, sizeof(m->err), "%s", mrp_last_error());
}
/* stRPHmm_fuse of the joined tiling path (hmm.c:283-372, gap columns :335-359) = its cross product with nothing:
 * the shadow of the final hmm as the device builds it */
static void many_final_shadow(int64_t c, void *arg) {
    many_ctl *ctl = arg;
    many_state *m = &ctl->st[c];
    if (m->root < 0 || m->rc != MRP_OK || m->w.failed) return;
    r_hmm_vec *joined = ctl->tree->a[m->root].path;
    if (joined->n == 0) return;
    const int32_t S = joined->a[0]->ref_start, E = joined->a[joined->n - 1]->ref_start + joined->a[joined->n - 1]->ref_length;
    r_hmm_vec nothing = {0};
    m->rc = r_cross_build(&m->w, joined, &nothing, S, E, mrp_engine_stride(ctl->e), &m->hmm);
    if (m->rc != MRP_OK) { m->hmm = NULL; snprintf(m->err, sizeof(m->err), "%s", mrp_last_error()); return; }
    const int64_t K = m->hmm->n_cols;
    m->path = xmalloc(sizeof(int32_t) * (size_t) K);
    m->chosen = xmalloc(sizeof(uint64_t) * (size_t) K);
    mrp_xhmm *x = &ctl->xfinal[c];
    r_describe(&m->w, m->hmm, ctl->final_flags, x);
    x->n_cells = m->path;
    x->path_part = m->chosen;
    m->w.n_sweeps += 1; /* bubbleGraph.c:2749 */
    {   /* the genome fragment on the device, behind the trace back: the chunk's reads, their order by pool offset (a column names a
         * read by where its profile bytes are), the reads the coverage filter took out */
        const int64_t nr = m->w.n_reads;
        m->by_pool = xmalloc(sizeof(int32_t) * (size_t) (nr + 1));
        int sorted = 1;
        for (int64_t i = 0; i < nr; i++) { m->by_pool[i] = (int32_t) i; if (i > 0 && m->w.reads[i].pool_offset < m->w.reads[i - 1].pool_offset) sorted = 0; }
        if (!sorted) { /* (rare: callers lay the profiles out in read order) insertion into a keyed array, then a plain sort */
            keyed *a = xmalloc(sizeof(keyed) * (size_t) (nr + 1)), *t = xmalloc(sizeof(keyed) * (size_t) (nr + 1));
            for (int64_t i = 0; i < nr; i++) { a[i].idx = i; a[i].key = -(double) m->w.reads[i].pool_offset; } /* keyed_sort_desc: descending key */
            keyed_sort_desc(a, nr, t);
            for (int64_t i = 0; i < nr; i++) m->by_pool[i] = (int32_t) a[i].idx;
            free(a); free(t);
        }
        const int64_t len = (int64_t) x->ref_end - x->ref_start;
        m->frag_sites = xmalloc(20 * (size_t) (len + 1));
        m->frag_reads1 = xmalloc(sizeof(int32_t) * (size_t) (2 * nr + 2));
        m->frag_reads2 = xmalloc(sizeof(int32_t) * (size_t) (2 * nr + 2));
        x->frag_reads = m->w.reads; x->frag_n_reads = (int32_t) nr; x->frag_by_pool = m->by_pool;
        x->frag_discarded = m->discarded; x->frag_n_discarded = (int32_t) m->nd;
        x->frag_iterations = (int32_t) ctl->params->rounds_of_iterative_refinement;
        x->frag_sites = m->frag_sites; x->frag_reads1 = m->frag_reads1; x->frag_reads2 = m->frag_reads2;
        x->frag_n1 = x->frag_n2 = 0; x->frag_done = 0;
    }
}
static void many_finish(int64_t c, void *arg) {
    many_ctl *ctl = arg;
    many_state *m = &ctl->st[c];
    if (m->w.failed) ctl->out[c] = NULL; /* redone by the caller on the hashing path */
    else if (m->hmm && m->frag_done) { /* the fragment came from the device: widen it into the result's arrays */
        const int32_t start = m->hmm->ref_start, len = m->hmm->ref_length;
        mrp_phase_result *g = result_new(start, len, m->w.n_reads);
        const struct { uint8_t anc, h1, h2, s1, s2, pad[3]; float gp, p1, p2; } *fs = m->frag_sites;
        for (int32_t q = 0; q < len; q++) {
            const uint64_t A = m->w.ch.allele_number[start + q], h1 = fs[q].h1, h2 = fs[q].h2;
            g->ancestor_string[q] = fs[q].anc; g->haplotype_string1[q] = h1; g->haplotype_string2[q] = h2;
            g->genotype_string[q] = h1 < h2 ? h1 * A + h2 : h2 * A + h1;
            g->genotype_probs[q] = fs[q].gp; g->haplotype_probs1[q] = fs[q].p1; g->haplotype_probs2[q] = fs[q].p2;
            g->reads_supporting_haplotype1[q] = fs[q].s1; g->reads_supporting_haplotype2[q] = fs[q].s2;
        }
        memcpy(g->reads1, m->frag_reads1, sizeof(int32_t) * (size_t) m->frag_n1); g->n_reads1 = m->frag_n1;
        memcpy(g->reads2, m->frag_reads2, sizeof(int32_t) * (size_t) m->frag_n2); g->n_reads2 = m->frag_n2;
        g->hmm_forward = m->fwd; g->hmm_backward = m->bwd; g->n_sweeps = m->w.n_sweeps;
        ctl->out[c] = g;
    }
    else if (m->hmm) {
        mrp_hmm *flat = r_expand(&m->w, m->hmm, 0);
        if (!flat) { m->rc = MRP_ERR_ARG; snprintf(m->err, sizeof(m->err), "%s", mrp_last_error()); return; }
        finish_phase_parts(&m->w, flat, m->chosen, m->fwd, m->bwd, ctl->params, m->discarded, m->nd, &ctl->out[c]);
        mrp_hmm_destroy(flat);
    }
    else ctl->out[c] = result_new(0, 0, ctl->n_reads[c]);
}

int phase_many_resident(mrp_context *ctx, int64_t n_chunks, const mrp_chunk *const *chunks, const mrp_read *const *reads,
                               const int64_t *n_reads, const mrp_params *params, mrp_phase_result **out,
                               mrp_phase_many_stats *stats) {
    mrp_params pc = *params;
    pc.include_ancestor_sub_prob = 0; /* bubbleGraph.c:2733 */
    mrp_engine *e = NULL;
    const double t_enter = now_ms();
    if (getenv("MRP_TIMING")) fprintf(stderr, "  batch of %lld chunks enters at %.1f ms on the process clock\n", (long long) n_chunks, fmod(t_enter, 1e5));
    int rc = mrp_engine_create(ctx, &pc, &e);
    if (rc != MRP_OK) return rc;
    many_state *st = xcalloc((size_t) n_chunks + 1, sizeof(*st));
    rnode_vec tree = {0};
    const int timing = getenv("MRP_TIMING") != NULL;
    g_prepare_timing = getenv("MRP_TIMING_PREPARE") != NULL;
    double tt[6];
    tt[0] = now_ms(); g_t_prepare = g_t_level = 0;
    for (int q = 0; q < 6; q++) __atomic_store_n(&g_ns[q], 0, __ATOMIC_RELAXED); /* (diagnostics shared by the concurrent halves) */
    many_ctl ctl = {st, ctx, chunks, reads, n_reads, params, &pc, e, &tree, out, NULL, 0};
    tt[3] = tt[2] = 0;
    mrp_pool_set_tag(4); parallel_for(n_chunks, many_setup, &ctl); mrp_pool_set_tag(0);
    for (int64_t c = 0; c < n_chunks; c++) { /* splice the chunks' subtrees into one tree */
        many_state *m = &st[c];
        if (m->rc != MRP_OK && rc == MRP_OK) rc = mrp_set_error(m->rc, "%s", m->err);
        const int base = (int) tree.n;
        for (int64_t i = 0; i < m->tree.n; i++) {
            rnode nd = m->tree.a[i];
            if (nd.left >= 0) nd.left += base;
            if (nd.right >= 0) nd.right += base;
            VEC_PUSH(tree, nd);
        }
        if (m->root >= 0) m->root += base;
        free(m->tree.a);
        m->tree.a = NULL; m->tree.n = m->tree.cap = 0;
    }
    tt[1] = now_ms();
    level_runs pending = {0}; /* the last merge levels: still on the device while the final stage is described */
    if (rc == MRP_OK) rc = r_run_tree(e, &tree, &pc, &pending);
    tt[2] = now_ms();
    tt[3] = now_ms();
    /* fuse the joined path (:2745-2747), final sweep with the ancestor model (:2748-2749) and trace back (:2755) on
     * the device, all chunks in one batch: only the traced-back partition of every column comes back */
    pc.include_ancestor_sub_prob = 1;
    if (rc == MRP_OK) {
        ctl.final_flags = sweep_flags(&pc);
        ctl.xfinal = xcalloc((size_t) n_chunks + 1, sizeof(*ctl.xfinal));
        mrp_pool_set_tag(5); parallel_for(n_chunks, many_final_shadow, &ctl); mrp_pool_set_tag(0);
        mrp_xhmm *xh = xcalloc((size_t) n_chunks + 1, sizeof(*xh));
        int64_t nj = 0;
        for (int64_t c = 0; c < n_chunks; c++) {
            if (st[c].rc != MRP_OK && rc == MRP_OK) rc = mrp_set_error(st[c].rc, "%s", st[c].err);
            if (st[c].hmm) { st[c].final_index = nj; xh[nj++] = ctl.xfinal[c]; }
        }
        if (rc == MRP_OK) rc = mrp_engine_final_stage(e, nj, xh);
        /* the wait for the last merge level (its error flags mark the chunks to redo), then the final stage goes */
        if (rc == MRP_OK) rc = mrp_engine_level_launch(e);
        else (void) mrp_engine_level_end(e);
        level_runs_settle(&pending, e, rc == MRP_OK, 1); /* (the final level's launch waits for everything before it) */
        if (rc == MRP_OK) rc = mrp_engine_level_end(e);
        for (int64_t c = 0; c < n_chunks; c++)
            if (st[c].hmm) {
                st[c].fwd = xh[st[c].final_index].hmm_forward; st[c].bwd = xh[st[c].final_index].hmm_backward;
                st[c].frag_done = rc == MRP_OK ? xh[st[c].final_index].frag_done : 0;
                st[c].frag_n1 = xh[st[c].final_index].frag_n1; st[c].frag_n2 = xh[st[c].final_index].frag_n2;
                if (rc == MRP_OK && xh[st[c].final_index].err != 0) st[c].w.failed = 1;
            }
        free(xh);
        free(ctl.xfinal);
    } else {
        (void) mrp_engine_level_end(e);
        level_runs_settle(&pending, e, 0, 1);
    }
    tt[4] = now_ms();
    if (rc == MRP_OK) {
        mrp_pool_set_tag(6); parallel_for(n_chunks, many_finish, &ctl); mrp_pool_set_tag(0);
        for (int64_t c = 0; c < n_chunks; c++)
            if (st[c].rc != MRP_OK && rc == MRP_OK) rc = mrp_set_error(st[c].rc, "%s", st[c].err);
    }
    int64_t n_failed = 0;
    for (int64_t c = 0; c < n_chunks && rc == MRP_OK; c++) {
        if (!st[c].w.failed) continue;
        /* bubbleGraph_phaseBubbleGraph of this chunk alone, cross products by hashing and prune on the host (mrp_phase_reads) */
        n_failed++;
        if (timing) fprintf(stderr, "  chunk %lld left the resident path: redone on the hashing path\n", (long long) c);
        rc = mrp_phase_reads(ctx, chunks[c], reads[c], n_reads[c], params, NULL, &out[c]);
    }
    tt[5] = now_ms();
    if (timing)
        fprintf(stderr, "mrp_phase_reads_many: setup %.1f ms, merge levels %.1f ms (host prepare %.1f, engine %.1f), download %.1f, "
                        "final sweep %.1f, trace back + genome fragments %.1f\n", tt[1] - tt[0], tt[2] - tt[1], g_t_prepare, g_t_level,
                tt[3] - tt[2], tt[4] - tt[3], tt[5] - tt[4]);
    if (timing) {
        int64_t cached = 0, held = 0;
        mrp_context_pool_bytes(ctx, &cached, &held);
        fprintf(stderr, "  device memory: %.1f GB idle in this context's pool, %.1f GB held by all pools of the device\n", (double) cached * 1e-9, (double) held * 1e-9);
    }
    if (timing)
        fprintf(stderr, "  prepare (summed over threads): components %.1f ms, tiling paths %.1f, cross shadows %.1f, garbage %.1f\n",
                g_ns[0] * 1e-6, g_ns[1] * 1e-6, g_ns[2] * 1e-6, g_ns[3] * 1e-6);
    if (stats) {
        mrp_engine_stats es;
        mrp_engine_get_stats(e, &es);
        stats->resident = 1;
        stats->fallback_chunks = (int32_t) n_failed;
        stats->levels = es.levels; stats->hmms = es.hmms; stats->columns = es.columns; stats->cells = es.cells;
        stats->merge_cells = es.merge_cells;
        stats->device_ms = es.device_ms; stats->cross_ms = es.cross_ms; stats->sweep_ms = es.sweep_ms; stats->prune_ms = es.prune_ms;
        stats->pack_ms = es.pack_ms; stats->cross_emit_ms = es.cross_emit_ms; stats->recursion_ms = es.recursion_ms; stats->prune_kernel_ms = es.prune_kernel_ms; stats->compact_ms = es.compact_ms;
    }
    const double t_clean = now_ms();
    for (int64_t c = 0; c < n_chunks; c++) {
        rhmm_destroy(st[c].hmm); free(st[c].discarded); free(st[c].tree.a); free(st[c].path); free(st[c].chosen);
        free(st[c].by_pool); free(st[c].frag_sites); free(st[c].frag_reads1); free(st[c].frag_reads2);
    }
    r_free_tree(&tree);
    for (int64_t c = 0; c < n_chunks; c++) if (st[c].leaves) shadow_release(st[c].leaves, st[c].leaves_class);
    free(st);
    const double t_eng = now_ms();
    mrp_engine_destroy(e);
    if (timing)
        fprintf(stderr, "  engine create %.1f ms, host clean-up %.1f, engine destroy %.1f, whole call %.1f (ends at %.1f ms on the process clock)\n", tt[0] - t_enter, t_eng - t_clean,
                now_ms() - t_eng, now_ms() - t_enter, fmod(now_ms(), 1e5));
    return rc;
}

#undef free /* (a file that includes this one -- tools/hostbench -- holds no arena pointers) */
