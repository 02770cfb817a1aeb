/*
 * rphmm_many.c -- mrp_phase_reads_many: how a call is cut up and where its chunks run.  No hot loops.
 *
 * A call runs as consecutive slices that fit the device's memory budget (phase_many_capped); a slice as up to 16
 * concurrent batches, each with a context and a host thread of its own (phase_many_once, mrp_phase_group_assign), so
 * that one batch's host work runs beside another's kernels; a batch is phase_many_resident (rphmm_host.c).  When the
 * resident path refuses the parameters, every chunk of the slice takes the per-chunk path instead (mrp_phase_reads,
 * rphmm_chunk.c), said loudly on stderr and in the stats' note.
 */
#define _GNU_SOURCE
#include "rphmm_common.h"

/* one concurrent batch of mrp_phase_reads_many: while its levels wait for the device, the other batch's host work runs */
typedef struct {
    mrp_context *ctx;
    int64_t n;
    const mrp_chunk **chunks;
    const mrp_read **reads;
    int64_t *n_reads;
    const mrp_params *params;
    mrp_phase_result **out;
    mrp_phase_many_stats stats;
    int rc, index;
    void *pool; /* the caller's host worker pool */
    char err[256];
} phase_group;
long long mrp_pool_task_cpu_ns(void);
long long mrp_pool_task_cpu_ns_this_thread(void);
static double thread_cpu_ms(void) { struct timespec t; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &t); return 1e3 * t.tv_sec + 1e-6 * t.tv_nsec; }
/* The batch (0 .. G - 1) every chunk of a call goes to: a repeating pattern that gives batch g the share w_g / sum w of the chunks.
 * For calls of large chunks the first batches are the smaller ones (shares 2 : 3 : 4 : 5 : 5 ...): every batch starts with merge levels
 * that cost the host more than the device, the batches leave them one after the other (the pool serves batch 0 first), and the device
 * waits for the first batch to reach its large levels -- a small first batch gets there sooner, the later ones are prepared beside its
 * kernels (-1 to -2 % per call of 1 152 configs[1] chunks, A/B on three boxes).  Chunks of a few hundred sites keep equal shares: their
 * calls are the host's time throughout, and a larger last batch only lengthens them (640 chunks of 130 sites: 16.2 ms with equal shares,
 * 17.6 with graded ones).  MRP_GROUP_WEIGHTS=w0:w1:... (development) sets the shares.  A work queue's chunk block is uploaded in the
 * same groups (mrp_chunk_block_create): a batch waits for its own group's copy only. */
void mrp_phase_group_assign(int64_t n_chunks, int G, int64_t total_sites, uint8_t *group_of) {
    int w[16], W = 0, pat[256], np = 0;
    if (G < 1) G = 1;
    if (G > 16) G = 16;
    const int graded = G >= 4 && n_chunks >= 16 * (int64_t) G && total_sites >= 500 * n_chunks;
    for (int g = 0; g < G; g++) w[g] = graded ? (g + 2 < 5 ? g + 2 : 5) : 1;
    const char *we = getenv("MRP_GROUP_WEIGHTS");
    if (we) { int g = 0; for (const char *c = we; *c && g < G; g++) { w[g] = atoi(c); if (w[g] < 1) w[g] = 1; if (w[g] > 8) w[g] = 8; while (*c >= '0' && *c <= '9') c++; if (*c) c++; /* (any separator) */ } }
    for (int g = 0; g < G; g++) W += w[g];
    /* the pattern: round by round, every batch that still has weight left takes one place */
    for (int round = 0; np < W; round++) for (int g = 0; g < G && np < W; g++) if (w[g] > round) pat[np++] = g;
    for (int64_t i = 0; i < n_chunks; i++) group_of[i] = (uint8_t) pat[i % W];
}

static void *phase_group_main(void *p) {
    phase_group *g = p;
    const double cpu0 = thread_cpu_ms();
    const long long pool0 = mrp_pool_task_cpu_ns(), mine0 = mrp_pool_task_cpu_ns_this_thread();
    mrp_pool_adopt(g->pool);
    mrp_pool_set_priority(g->index); /* batch 0's host loops first: the batches reach their device-heavy levels one after the other */
    g->rc = phase_many_resident(g->ctx, g->n, g->chunks, g->reads, g->n_reads, g->params, g->out, &g->stats);
    mrp_pool_set_priority(0);
    if (getenv("MRP_TIMING")) {
        fprintf(stderr, "  batch %d: cpu of its own thread %.1f ms (%.1f of it pool tasks it ran itself); pool tasks (all batches, while it ran) %.1f ms; cumulative by loop:", g->index,
                thread_cpu_ms() - cpu0, (mrp_pool_task_cpu_ns_this_thread() - mine0) * 1e-6, (mrp_pool_task_cpu_ns() - pool0) * 1e-6);
        for (int t = 0; t < 12; t++) fprintf(stderr, " %d:%.0f", t, mrp_pool_tag_cpu_ns(t) * 1e-6);
        fprintf(stderr, "\n");
    }
    if (g->rc != MRP_OK) snprintf(g->err, sizeof(g->err), "%s", mrp_last_error());
    return NULL;
}

/* the chunks of a call that cannot take the resident path, pulled one at a time by up to eight host threads */
typedef struct {
    mrp_context *ctx;
    const mrp_chunk *const *chunks;
    const mrp_read *const *reads;
    const int64_t *n_reads;
    const mrp_params *params;
    mrp_phase_result **out;
    int64_t next;
    int rc;
    char err[256];
    int threads;
    int64_t n;
} hashing_ctl;
typedef struct { hashing_ctl *ctl; mrp_context *ctx; } hashing_arg;
static void *hashing_main(void *p) {
    hashing_arg *a = p;
    hashing_ctl *hc = a->ctl;
    for (;;) {
        const int64_t c = __atomic_fetch_add(&hc->next, 1, __ATOMIC_RELAXED);
        if (c >= hc->n || __atomic_load_n(&hc->rc, __ATOMIC_RELAXED) != MRP_OK) return NULL;
        const int rc = mrp_phase_reads(a->ctx, hc->chunks[c], hc->reads[c], hc->n_reads[c], hc->params, NULL, &hc->out[c]);
        if (rc != MRP_OK) {
            int expect = MRP_OK;
            if (__atomic_compare_exchange_n(&hc->rc, &expect, rc, 0, __ATOMIC_RELAXED, __ATOMIC_RELAXED)) snprintf(hc->err, sizeof(hc->err), "%s", mrp_last_error());
            return NULL;
        }
    }
}

/* the concurrent batches a call over n_chunks chunks is split into (chunk i goes to batch i % G) */
int mrp_phase_groups_for(const mrp_context *ctx, int64_t n_chunks) {
    int G = mrp_context_phase_groups(ctx); /* mrp_context_set_phase_groups; 0 (default): by batch size */
    if (G <= 0) G = n_chunks < 192 ? (int) (n_chunks / 12 > 4 ? 4 : n_chunks / 12) : 8;
    if (G < 1) G = 1;
    if (G > 16) G = 16;
    if (n_chunks < 4 * G) G = 1;
    return G;
}

/* The totals of a call from those of its parts: the slices of phase_many_capped, the concurrent batches of phase_many_once.
 * (A batch that ended well reports resident = 1 and no note, phase_many_resident: for the batches this is the plain sum.) */
static void stats_add(mrp_phase_many_stats *stats, const mrp_phase_many_stats *st, int first) {
    if (first) { *stats = *st; return; }
    stats->resident = stats->resident && st->resident; stats->fallback_chunks += st->fallback_chunks;
    if (st->levels > stats->levels) stats->levels = st->levels;
    stats->hmms += st->hmms; stats->columns += st->columns; stats->cells += st->cells; stats->merge_cells += st->merge_cells;
    stats->device_ms += st->device_ms; stats->cross_ms += st->cross_ms; stats->sweep_ms += st->sweep_ms; stats->prune_ms += st->prune_ms;
    stats->pack_ms += st->pack_ms; stats->cross_emit_ms += st->cross_emit_ms; stats->recursion_ms += st->recursion_ms; stats->prune_kernel_ms += st->prune_kernel_ms; stats->compact_ms += st->compact_ms;
    if (st->note[0] && !stats->note[0]) memcpy(stats->note, st->note, sizeof(stats->note));
}

static int phase_many_once(mrp_context *ctx, int64_t n_chunks, const mrp_chunk *const *chunks, const mrp_read *const *reads,
                           const int64_t *n_reads, const mrp_params *params, mrp_phase_result **out, mrp_phase_many_stats *stats) {
    if (stats) memset(stats, 0, sizeof(*stats));
    for (int64_t c = 0; c < n_chunks; c++) out[c] = NULL;
    /* the levels of a batch alternate host work (structure, descriptors) and device work; two interleaved halves of the
     * chunks, each with its own context and host thread, keep both busy */
    int G = mrp_phase_groups_for(ctx, n_chunks);
    /* measured on MI355X (bench.py --chunks N --phase-groups G, two streams a batch): 48 chunks 45.3 ms with 2 batches, 42.5
     * with 4; 96: 52.3 with 4, 54.8 with 8; 144: 66.4 / 68.0; 192: 80.2 / 78.6; 288: 104.5 / 96.9; 432: 139.9 with 6, 130.5
     * with 8; 576 with 8: 169.5 (2.04e8 units/s, the best rate; 768: 243 ms).  More than 8 would share hardware queues. */
    int rc = MRP_OK;
    if (G == 1) {
        rc = phase_many_resident(ctx, n_chunks, chunks, reads, n_reads, params, out, stats);
    } else {
        phase_group *grp = xcalloc((size_t) G, sizeof(*grp));
        pthread_t th[16];
        int started[16] = {0};
        /* which batch a chunk goes to (mrp_phase_group_assign: graded shares for calls of large chunks) */
        uint8_t *group_of = xmalloc((size_t) n_chunks + 1);
        int first = 1; /* of the batches whose totals are added up */
        {
            int64_t sites = 0;
            for (int64_t i = 0; i < n_chunks; i++) { mrp_chunk_host hv; mrp_chunk_host_view(chunks[i], &hv); sites += hv.n_sites; }
            mrp_phase_group_assign(n_chunks, G, sites, group_of);
        }
        for (int g = 0; g < G; g++) {
            phase_group *q = &grp[g];
            q->index = g;
            q->pool = mrp_pool_current();
            q->ctx = g == 0 ? ctx : mrp_context_sibling(ctx, g - 1);
            q->params = params;
            q->n = 0;
            for (int64_t i = 0; i < n_chunks; i++) if (group_of[i] == g) q->n++;
            q->chunks = xmalloc(sizeof(*q->chunks) * (size_t) (q->n + 1));
            q->reads = xmalloc(sizeof(*q->reads) * (size_t) (q->n + 1));
            q->n_reads = xmalloc(sizeof(*q->n_reads) * (size_t) (q->n + 1));
            q->out = xcalloc((size_t) q->n + 1, sizeof(*q->out));
            q->n = 0;
            for (int64_t i = 0; i < n_chunks; i++)
                if (group_of[i] == g) { q->chunks[q->n] = chunks[i]; q->reads[q->n] = reads[i]; q->n_reads[q->n] = n_reads[i]; q->n++; }
            if (!q->ctx) { q->rc = MRP_ERR_HIP; snprintf(q->err, sizeof(q->err), "%s", mrp_last_error()); }
        }
        const int was_grouped = mrp_context_set_grouped(ctx, 1); /* (the siblings always are) */
        for (int g = 0; g < G; g++) if (grp[g].ctx) mrp_context_set_concurrent_batches(grp[g].ctx, G * mrp_context_calls_sharing_device(ctx));
        mrp_warn_hw_queues_once(G);
        for (int g = 1; g < G; g++)
            if (grp[g].ctx && pthread_create(&th[g], NULL, phase_group_main, &grp[g]) == 0) started[g] = 1;
        if (grp[0].ctx) phase_group_main(&grp[0]);
        for (int g = 1; g < G; g++) {
            if (started[g]) pthread_join(th[g], NULL);
            else if (grp[g].ctx) phase_group_main(&grp[g]); /* thread creation failed: run it here */
        }
        mrp_context_set_grouped(ctx, was_grouped);
        for (int g = 0; g < G; g++) if (grp[g].ctx) mrp_context_set_concurrent_batches(grp[g].ctx, 1);
        for (int g = 0; g < G; g++) {
            phase_group *q = &grp[g];
            if (q->rc != MRP_OK && (rc == MRP_OK || rc == MRP_ERR_UNSUPPORTED)) rc = mrp_set_error(q->rc, "%s", q->err);
            { int64_t k = 0; for (int64_t i = 0; i < n_chunks; i++) if (group_of[i] == g) out[i] = q->out[k++]; }
            if (stats && q->rc == MRP_OK) { stats_add(stats, &q->stats, first); first = 0; }
            free(q->chunks); free(q->reads); free(q->n_reads); free(q->out);
        }
        free(grp);
        free(group_of);
    }
    if (rc == MRP_ERR_UNSUPPORTED) {
        /* Parameters or hmm shapes outside the resident path: the hashing path (mrp_phase_reads), one chunk per host thread,
         * each thread with a context of its own.  Said loudly: this is two orders of magnitude slower than the resident path. */
        char why[160];
        snprintf(why, sizeof(why), "%s", mrp_last_error());
        if (stats) { memset(stats, 0, sizeof(*stats)); snprintf(stats->note, sizeof(stats->note), "%s", why); }
        static int warned;
        if (!__atomic_exchange_n(&warned, 1, __ATOMIC_RELAXED) && !getenv("MRP_QUIET"))
            fprintf(stderr, "margin_rphmm: mrp_phase_reads_many leaves the device-resident path (%s): %lld chunk(s) take the per-chunk hashing path, "
                            "about 100x slower per chunk\n", why, (long long) n_chunks);
        rc = MRP_OK;
        for (int64_t c = 0; c < n_chunks; c++) { mrp_phase_result_destroy(out[c]); out[c] = NULL; }
        int T = mrp_host_threads();
        if (T > 8) T = 8;
        if (T > n_chunks) T = (int) n_chunks;
        if (T < 1) T = 1;
        hashing_ctl hc = {ctx, chunks, reads, n_reads, params, out, 0, MRP_OK, {0}, T, 0};
        for (int t = 1; t < T && rc == MRP_OK; t++)
            if (!mrp_context_sibling(ctx, t - 1)) rc = MRP_ERR_HIP; /* all contexts before the first thread (allocator peers) */
        if (rc == MRP_OK) {
            hc.n = n_chunks;
            pthread_t th[8];
            int started[8] = {0};
            hashing_arg ha[8];
            for (int t = 0; t < T; t++) { ha[t].ctl = &hc; ha[t].ctx = t == 0 ? ctx : mrp_context_sibling(ctx, t - 1); }
            for (int t = 1; t < T; t++) started[t] = pthread_create(&th[t], NULL, hashing_main, &ha[t]) == 0;
            hashing_main(&ha[0]);
            for (int t = 1; t < T; t++) if (started[t]) pthread_join(th[t], NULL);
            rc = hc.rc;
            if (rc != MRP_OK) mrp_set_error(rc, "%s", hc.err);
        }
    }
    if (rc != MRP_OK)
        for (int64_t c = 0; c < n_chunks; c++) { mrp_phase_result_destroy(out[c]); out[c] = NULL; }
    return rc;
}

/* A call of at most `cap` (read, site) units at a time: what a call keeps on the device grows with its units (measured 214 GB
 * for 1 152 chunks of 60 000 units, ~3.1 KB per unit: the cells of the widest merge level of every concurrent batch), so a call
 * beyond the device's budget runs as consecutive slices that fit.  The estimate is only that: when the driver still refuses
 * an allocation (memory held by another process, a pool grown by best-fit reuse) the slice is redone as two halves after
 * every cache of the context has been given back -- down to single chunks -- instead of failing the call. */
static int phase_many_capped(mrp_context *ctx, int64_t n_chunks, const mrp_chunk *const *chunks, const mrp_read *const *reads,
                             const int64_t *n_reads, const mrp_params *params, mrp_phase_result **out, mrp_phase_many_stats *stats,
                             int64_t cap, int depth) {
    int64_t total = 0;
    for (int64_t c = 0; c < n_chunks; c++)
        for (int64_t r = 0; r < n_reads[c]; r++) total += reads[c][r].length;
    if (total <= cap || n_chunks <= 1) {
        const uint64_t oom0 = mrp_context_oom_events(ctx);
        int rc = phase_many_once(ctx, n_chunks, chunks, reads, n_reads, params, out, stats);
        if (rc == MRP_ERR_HIP && n_chunks > 1 && depth < 8 && mrp_context_oom_events(ctx) != oom0) {
            static int warned;
            if (!__atomic_exchange_n(&warned, 1, __ATOMIC_RELAXED) && !getenv("MRP_QUIET"))
                fprintf(stderr, "margin_rphmm: the device refused memory for a call of %lld chunks (%lld units): redone in two halves\n",
                        (long long) n_chunks, (long long) total);
            for (int64_t c = 0; c < n_chunks; c++) { mrp_phase_result_destroy(out[c]); out[c] = NULL; }
            mrp_context_trim(ctx);
            return phase_many_capped(ctx, n_chunks, chunks, reads, n_reads, params, out, stats, total / 2 + 1, depth + 1);
        }
        return rc;
    }
    int rc = MRP_OK;
    int64_t c0 = 0;
    if (stats) memset(stats, 0, sizeof(*stats));
    while (c0 < n_chunks && rc == MRP_OK) {
        int64_t c1 = c0, u = 0;
        while (c1 < n_chunks) {
            int64_t uc = 0;
            for (int64_t r = 0; r < n_reads[c1]; r++) uc += reads[c1][r].length;
            if (c1 > c0 && u + uc > cap) break;
            u += uc; c1++;
        }
        mrp_phase_many_stats st;
        rc = phase_many_capped(ctx, c1 - c0, chunks + c0, reads + c0, n_reads + c0, params, out + c0, &st, cap, depth);
        if (stats && rc == MRP_OK) stats_add(stats, &st, c0 == 0);
        c0 = c1;
    }
    if (rc != MRP_OK)
        for (int64_t c = 0; c < n_chunks; c++) { mrp_phase_result_destroy(out[c]); out[c] = NULL; }
    return rc;
}

int mrp_phase_reads_many(mrp_context *ctx, int64_t n_chunks, const mrp_chunk *const *chunks, const mrp_read *const *reads,
                         const int64_t *n_reads, const mrp_params *params, mrp_phase_result **out,
                         mrp_phase_many_stats *stats) {
    if (!ctx || n_chunks < 0 || !params || (n_chunks > 0 && (!chunks || !reads || !n_reads || !out)))
        return mrp_set_error(MRP_ERR_ARG, "mrp_phase_reads_many: bad arguments");
    if (params->reserved != 0) return mrp_set_error(MRP_ERR_ARG, "mrp_params.reserved must be 0");
    if (stats) memset(stats, 0, sizeof(*stats));
    for (int64_t c = 0; c < n_chunks; c++) out[c] = NULL;
    /* the slice size from the device's budget (free memory when the process's first pool asked, mrp_internal.h); MRP_CALL_UNITS
     * overrides it (tests) */
    const int64_t budget = mrp_context_device_budget(ctx);
    int64_t cap = budget > 0 ? budget / 3400 : (int64_t) 7e7;
    const char *ce = getenv("MRP_CALL_UNITS");
    if (ce && atoll(ce) > 0) cap = atoll(ce);
    return phase_many_capped(ctx, n_chunks, chunks, reads, n_reads, params, out, stats, cap, 0);
}
