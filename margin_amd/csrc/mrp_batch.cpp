/*
 * mrp_batch.cpp -- the recursion batch behind mrp_fb_run, and the emission-only seam.
 *
 * Validates and concatenates flattened stRPHmm jobs into batch-wide arrays (mrp_device.h), moves them to HBM, launches the plane
 * and sweep kernels on the context's stream and scatters the post-conditions of stRPHmm_forwardBackward (hmm.c:931-942) back into
 * the caller's arrays.  The resident engine (mrp_engine.cpp) fills a batch's device arrays itself and comes here for the launch.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <mutex>
#include <new>
#include <vector>

#include "mrp_internal.h"
#include "mrp_level_order.h" /* sweep_class */

extern "C" {

int mrp_batch_create(mrp_context *ctx, mrp_batch **out) {
    if (!ctx || !out) return mrp_set_error(MRP_ERR_ARG, "mrp_batch_create: bad arguments");
    mrp_batch *b = new (std::nothrow) mrp_batch();
    if (!b) return mrp_set_error(MRP_ERR_NOMEM, "out of host memory");
    b->ctx = ctx;
    b->bind_pool(&ctx->pool);
    *out = b;
    return MRP_OK;
}

void mrp_batch_destroy(mrp_batch *batch) {
    if (!batch) return;
    (void) hipSetDevice(batch->ctx->device);
    mrp_context *ctx = batch->ctx;
    (void) hipStreamSynchronize(ctx->stream); /* the auxiliary streams were joined into it */
    for (auto &slot : batch->ev_ring)
        for (hipEvent_t ev : slot) {
            if (ev == ctx->last_emission) ctx->last_emission = nullptr;
            if (ev) (void) hipEventDestroy(ev);
        }
    delete batch;
    ctx->pool.reclaim();
}

/* resolve cell -> merge cell indices from keys: stHash_search of mergeColumn.c:63-79 */
static int resolve_column(const uint64_t *part, int64_t n_cells, uint64_t mask, const uint64_t *keys,
                          int64_t n_keys, uint32_t *out) {
    size_t cap = 16;
    while (cap < (size_t) n_keys * 2) cap *= 2;
    std::vector<uint64_t> hk(cap);
    std::vector<uint32_t> hv(cap, 0xFFFFFFFFu);
    auto mix = [](uint64_t x) {
        x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
        return x;
    };
    for (int64_t i = 0; i < n_keys; i++) {
        size_t s = mix(keys[i]) & (cap - 1);
        while (hv[s] != 0xFFFFFFFFu) {
            if (hk[s] == keys[i]) return MRP_ERR_ARG; /* duplicate key: mergeColumn.c:104-107 asserts */
            s = (s + 1) & (cap - 1);
        }
        hk[s] = keys[i];
        hv[s] = (uint32_t) i;
    }
    for (int64_t c = 0; c < n_cells; c++) {
        const uint64_t key = part[c] & mask;
        size_t s = mix(key) & (cap - 1);
        uint32_t found = 0xFFFFFFFFu;
        while (hv[s] != 0xFFFFFFFFu) {
            if (hk[s] == key) { found = hv[s]; break; }
            s = (s + 1) & (cap - 1);
        }
        if (found == 0xFFFFFFFFu) return MRP_ERR_LOOKUP;
        out[c] = found;
    }
    return MRP_OK;
}

/* appends one hmm to a host-fed batch (a resident level's batch is described on the device: mrp_engine.cpp) */
int mrp_batch_add(mrp_batch *b, const mrp_hmm_job *job) {
    if (!b || !job) return mrp_set_error(MRP_ERR_ARG, "mrp_batch_add: NULL argument");
    if (b->uploaded) return mrp_set_error(MRP_ERR_ARG, "mrp_batch_add: batch already uploaded");
    const int K = job->n_columns;
    if (K < 1) return mrp_set_error(MRP_ERR_ARG, "hmm has %d columns", K);
    if (!job->chunk || !job->col_ref_start || !job->col_length || !job->col_depth || !job->col_cell_off ||
        !job->col_read_off || !job->partition)
        return mrp_set_error(MRP_ERR_ARG, "hmm job is missing required arrays");
    if (K > 1 && (!job->mcol_cell_off || ((!job->cell_next || !job->cell_prev) &&
                                          (!job->mask_from || !job->mask_to || !job->merge_from || !job->merge_to))))
        return mrp_set_error(MRP_ERR_ARG, "hmm job is missing its merge column arrays");
    const bool device_only = !job->cell_forward && !job->cell_backward && !job->col_total && !job->hmm_forward &&
                             !job->hmm_backward && !job->merge_forward && !job->merge_backward;
    if (!device_only && (!job->cell_forward || !job->cell_backward || !job->col_total || !job->hmm_forward ||
                         !job->hmm_backward || (K > 1 && (!job->merge_forward || !job->merge_backward))))
        return mrp_set_error(MRP_ERR_ARG, "hmm job is missing output arrays");
    const mrp_chunk *ch = job->chunk;
    if (ch->host_wait() != hipSuccess) return mrp_set_error(MRP_ERR_HIP, "chunk upload failed");
    if (ch->ctx->device != b->ctx->device) return mrp_set_error(MRP_ERR_ARG, "chunk lives on a different device");
    std::lock_guard<std::mutex> lock(b->mu);
    const bool ancestor = (job->flags & MRP_FLAG_INCLUDE_ANCESTOR_SUB_PROB) != 0;

    int chunk_index = -1;
    for (size_t i = 0; i < b->chunks.size(); i++)
        if (b->chunks[i] == ch) chunk_index = (int) i;
    if (chunk_index < 0) {
        chunk_index = (int) b->chunks.size();
        b->chunks.push_back(ch);
    }

    /* validate before touching the batch */
    if (job->col_cell_off[0] != 0 || job->col_read_off[0] != 0 || (K > 1 && job->mcol_cell_off[0] != 0))
        return mrp_set_error(MRP_ERR_ARG, "prefix-sum arrays must start at 0");
    for (int k = 0; k < K; k++) {
        const int64_t nc = job->col_cell_off[k + 1] - job->col_cell_off[k];
        const int64_t nd = job->col_read_off[k + 1] - job->col_read_off[k];
        if (nc < 1 || nc > 0x7FFFFFFF) return mrp_set_error(MRP_ERR_ARG, "column %d has %lld cells", k, (long long) nc);
        if (job->col_depth[k] < 0 || job->col_depth[k] > MRP_MAX_READ_PARTITIONING_DEPTH || nd != job->col_depth[k])
            return mrp_set_error(MRP_ERR_ARG, "column %d: depth %d inconsistent", k, job->col_depth[k]);
        if (job->col_length[k] < 1 || job->col_ref_start[k] < 0 ||
            (int64_t) job->col_ref_start[k] + job->col_length[k] > ch->n_sites)
            return mrp_set_error(MRP_ERR_ARG, "column %d: site interval [%d,+%d) outside the reference", k,
                        job->col_ref_start[k], job->col_length[k]);
        if (nd > 0 && !job->read_byte_off) return mrp_set_error(MRP_ERR_ARG, "read_byte_off is NULL");
        const uint32_t slots = ch->allele_offset[job->col_ref_start[k] + job->col_length[k]] -
                               ch->allele_offset[job->col_ref_start[k]];
        for (int64_t i = 0; i < nd; i++) {
            const int64_t o = job->read_byte_off[job->col_read_off[k] + i];
            if (o < 0 || o + (int64_t) slots > ch->pool_bytes)
                return mrp_set_error(MRP_ERR_ARG, "column %d read %lld: profile bytes outside the pool", k, (long long) i);
        }
        if (ancestor) {
            for (int s = 0; s < job->col_length[k]; s++)
                if (ch->allele_number[job->col_ref_start[k] + s] > MRP_MAX_ALLELES)
                    return mrp_set_error(MRP_ERR_UNSUPPORTED, "site %d has more than %d alleles (ancestor mode)",
                                job->col_ref_start[k] + s, MRP_MAX_ALLELES);
        }
        if (k + 1 < K) {
            const int64_t nm = job->mcol_cell_off[k + 1] - job->mcol_cell_off[k];
            if (nm < 1 || nm > 0x7FFFFFFF) return mrp_set_error(MRP_ERR_ARG, "merge column %d has %lld cells", k, (long long) nm);
        }
    }

    const int64_t n_cells = job->col_cell_off[K];
    const int64_t n_merge = K > 1 ? job->mcol_cell_off[K - 1] : 0;
    /* every hmm starts at a multiple of 4 cells: the recursion kernel moves 4 cells per lane (16 B) */
    while (b->n_cells_total % 4 != 0) {
        b->n_cells_total++;
        b->partition.push_back(0);
        if (b->need_wide) { b->cell_next.push_back(0); b->cell_prev.push_back(0); }
        b->cell_np.push_back(0);
    }
    const int64_t cell0 = b->n_cells_total;
    const int64_t mcell0 = b->n_merge;
    const int64_t col0 = (int64_t) b->cols.size();
    const int64_t read0 = (int64_t) b->read_byte_off.size();

    std::vector<uint32_t> nxt((size_t) n_cells, 0), prv((size_t) n_cells, 0);
    for (int k = 0; k < K; k++) {
        const int64_t c0 = job->col_cell_off[k], nc = job->col_cell_off[k + 1] - c0;
        if (k + 1 < K) {
            const int64_t m0 = job->mcol_cell_off[k], nm = job->mcol_cell_off[k + 1] - m0;
            if (job->cell_next) {
                for (int64_t c = 0; c < nc; c++) {
                    if (job->cell_next[c0 + c] >= (uint64_t) nm) return mrp_set_error(MRP_ERR_ARG, "cell_next out of range");
                    nxt[c0 + c] = job->cell_next[c0 + c];
                }
            } else {
                int rc = resolve_column(job->partition + c0, nc, job->mask_from[k], job->merge_from + m0, nm, &nxt[c0]);
                if (rc != MRP_OK) return mrp_set_error(rc, "column %d: a cell has no next merge cell (mergeColumn.c:63)", k);
            }
        }
        if (k > 0) {
            const int64_t m0 = job->mcol_cell_off[k - 1], nm = job->mcol_cell_off[k] - m0;
            if (job->cell_prev) {
                for (int64_t c = 0; c < nc; c++) {
                    if (job->cell_prev[c0 + c] >= (uint64_t) nm) return mrp_set_error(MRP_ERR_ARG, "cell_prev out of range");
                    prv[c0 + c] = job->cell_prev[c0 + c];
                }
            } else {
                int rc = resolve_column(job->partition + c0, nc, job->mask_to[k - 1], job->merge_to + m0, nm, &prv[c0]);
                if (rc != MRP_OK) return mrp_set_error(rc, "column %d: a cell has no previous merge cell (mergeColumn.c:72)", k);
            }
        }
    }

    DevHmm h{};
    h.col0 = col0;
    h.n_cols = K;
    h.flags = job->flags;
    h.max_merge = 1;
    h.max_cells = 1;
    h.cost_bound = 0;
    for (int k = 0; k < K; k++) {
        DevCol c{};
        c.cell_off = cell0 + job->col_cell_off[k];
        c.n_cells = (int32_t) (job->col_cell_off[k + 1] - job->col_cell_off[k]);
        c.mcell_off = k + 1 < K ? mcell0 + job->mcol_cell_off[k] : 0;
        c.n_merge = k + 1 < K ? (int32_t) (job->mcol_cell_off[k + 1] - job->mcol_cell_off[k]) : 0;
        c.slot_off = b->n_slots;
        c.read_off = read0 + job->col_read_off[k];
        c.site_start = job->col_ref_start[k];
        c.n_sites = job->col_length[k];
        c.depth = job->col_depth[k];
        c.n_slots = (int32_t) (ch->allele_offset[c.site_start + c.n_sites] - ch->allele_offset[c.site_start]);
        c.chunk = chunk_index;
        c.flags = job->flags;
        b->n_slots += c.n_slots;
        int32_t uniform = (int32_t) ch->allele_number[c.site_start];
        for (int s2 = 1; s2 < c.n_sites; s2++)
            if ((int32_t) ch->allele_number[c.site_start + s2] != uniform) uniform = 0;
        for (int t0 = 0; t0 < c.n_cells; t0 += MRP_EMIT_TILE) {
            EmitTile t{};
            t.cell_off = c.cell_off + t0;
            t.slot_off = c.slot_off;
            t.n = std::min<int32_t>(MRP_EMIT_TILE, c.n_cells - t0);
            t.col = (int32_t) b->cols.size();
            t.n_sites = c.n_sites;
            t.uniform_alleles = uniform;
            t.depth = c.depth;
            t.flags = job->flags;
            b->tiles.push_back(t);
        }
        SweepCol sc{};
        sc.cell_off = c.cell_off;
        sc.mcell_off = c.mcell_off;
        sc.n_cells = c.n_cells;
        sc.n_merge = c.n_merge;
        b->scols.push_back(sc);
        PlaneCol pc{};
        pc.pool = ch->dev.pool;
        pc.read_off = c.read_off;
        pc.slot_off = c.slot_off;
        pc.depth = c.depth;
        pc.n_slots = c.n_slots;
        pc.need_planes = (uniform == 0 || ancestor) ? 1 : 0;
        b->pcols.push_back(pc);
        b->cols.push_back(c);
        h.max_merge = std::max(h.max_merge, c.n_merge);
        h.max_cells = std::max(h.max_cells, c.n_cells);
        int64_t per_site = 255ll * c.depth;
        if (ancestor) per_site += 2ll * ch->max_sub + ch->max_prior;
        h.cost_bound += per_site * c.n_sites;
        /* statistics: SURVEY.md 8(d) algorithmic bytes and the CPU formulation's popcount count */
        b->stats.profile_bytes += (int64_t) c.depth * c.n_slots;
        b->stats.algorithmic_bytes += 24ll * c.n_cells + 32ll * c.n_merge + (int64_t) c.depth * c.n_slots + 8;
        b->stats.popcount_ops += (int64_t) c.n_cells * 2 * c.n_slots * 8;
    }
    h.n_cells = n_cells;
    h.n_merge = n_merge;
    h.wide_idx = h.max_merge > 65535 ? 1 : 0;
    if (h.wide_idx && !b->need_wide) {
        /* the first hmm whose transitions do not fit 16 bits: from now on the full indices are kept too; those of the
         * hmms added so far are recovered from their packed form (they fit) */
        b->need_wide = true;
        const size_t have = b->cell_np.size();
        b->cell_next.resize(have);
        b->cell_prev.resize(have);
        for (size_t c = 0; c < have; c++) { b->cell_next[c] = b->cell_np[c] & 0xFFFFu; b->cell_prev[c] = b->cell_np[c] >> 16; }
    }
    b->hmms.push_back(h);
    b->n_cells_total += n_cells;
    b->partition.insert(b->partition.end(), job->partition, job->partition + n_cells);
    if (b->need_wide) {
        b->cell_next.insert(b->cell_next.end(), nxt.begin(), nxt.end());
        b->cell_prev.insert(b->cell_prev.end(), prv.begin(), prv.end());
    }
    const size_t base = b->cell_np.size();
    b->cell_np.resize(base + (size_t) n_cells);
    for (int64_t c = 0; c < n_cells; c++) b->cell_np[base + c] = (nxt[c] & 0xFFFFu) | (prv[c] << 16);
    if (job->col_read_off[K] > 0)
        b->read_byte_off.insert(b->read_byte_off.end(), job->read_byte_off, job->read_byte_off + job->col_read_off[K]);
    b->n_merge += n_merge;
    JobOut o{job->cell_forward, job->cell_backward, job->merge_forward, job->merge_backward, job->col_total,
             job->hmm_forward, job->hmm_backward, cell0, n_cells, mcell0, n_merge, col0, K};
    b->outs.push_back(o);
    b->stats.n_hmms += 1;
    b->stats.n_columns += K;
    b->stats.n_cells += n_cells;
    b->stats.n_merge_cells += n_merge;
    return MRP_OK;
}

/* Host-fed batches only: the resident engine sets `uploaded` itself when it has sized and described a level's batch on the device
 * (launch_size_batch), so mrp_batch_launch never comes here for a batch the engine owns. */
int mrp_batch_upload(mrp_batch *b) {
    if (!b) return mrp_set_error(MRP_ERR_ARG, "batch is NULL");
    if (b->uploaded) return MRP_OK;
    mrp_context *ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;

    const bool timing_ = getenv("MRP_TIMING") != nullptr;
    auto now_ = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return 1e3 * ts.tv_sec + 1e-6 * ts.tv_nsec; };
    const double u0 = now_();
    /* launch plan: int32/LDS path for max-plus HMMs that fit, fp64 path otherwise.  The int32 path is
     * split into size classes (LDS per workgroup = 2 * largest merge column * 4 B) that are launched
     * on separate streams so that small hmms do not inherit the residency of the largest one. */
    std::vector<std::pair<int64_t, int32_t>> wide, mid, narrow, generic, lse, lse_big;
    for (size_t i = 0; i < b->hmms.size(); i++) {
        const DevHmm &h = b->hmms[i];
        const int64_t work = b->outs[i].n_cells;
        const bool max_mode = (h.flags & MRP_FLAG_MAX_NOT_SUM) != 0;
        const size_t lds = (size_t) (2 * (int64_t) std::max(h.max_merge, 64) + 4) * sizeof(int32_t) + 128 * 8;
        if (max_mode && !h.wide_idx && b->outs[i].n_cells < (1ll << 30) && h.cost_bound < (1ll << 30) && lds <= (size_t) MRP_LDS_BUDGET) {
            b->outs[i].int_path = true;
            const SweepClass k = sweep_class(h.max_cells, h.max_merge);
            (k == SWEEP_NARROW ? narrow : k == SWEEP_MID ? mid : wide).push_back({-work, (int32_t) i});
        } else {
            generic.push_back({-work, (int32_t) i});
            /* sum mode with merge columns that fit LDS: the reproducible log-sum-exp kernel.  Its sums are 64-bit fixed point
             * in units of 2^-50 with every term <= 1: fewer than 2^14 terms per sum (a column's cells also sum into the
             * hmm's / column's total), and its reference points are floats: |log p| has to stay below 2^27, where a float
             * still resolves 8 -- beyond either bound the generic fp64 kernel takes the hmm */
            const bool lse_ok = !max_mode && !h.wide_idx && h.max_cells < MRP_LSE_MAX_TERMS && h.cost_bound < MRP_LSE_MAX_COST;
            if (lse_ok && h.max_merge <= MRP_LSE_CUR_LDS_MAX_MERGE) lse.push_back({-work, (int32_t) i});
            else if (lse_ok && h.max_merge <= MRP_LSE_MAX_MERGE) lse_big.push_back({-work, (int32_t) i});
        }
    }
    auto plan = [&](std::vector<std::pair<int64_t, int32_t>> &v, std::vector<int32_t> &order, int *max_merge) {
        std::sort(v.begin(), v.end()); /* largest first */
        order.clear();
        int mm = 1;
        for (auto &p : v) {
            order.push_back(p.second);
            mm = std::max(mm, b->hmms[p.second].max_merge);
        }
        if (max_merge) *max_merge = mm;
    };
    plan(wide, b->order_wide, &b->max_merge_wide);
    plan(mid, b->order_mid, &b->max_merge_mid);
    plan(narrow, b->order_narrow, &b->max_merge_narrow);
    plan(generic, b->order_f64, nullptr); /* every hmm with fp64 results */
    plan(lse, b->order_lse, &b->max_merge_lse);
    plan(lse_big, b->order_lse_big, &b->max_merge_lse_big);
    b->order_gen.clear();                  /* ... of which the generic kernel takes what the LDS ones do not */
    {
        std::vector<char> in_lse(b->hmms.size(), 0);
        for (int32_t i : b->order_lse) in_lse[(size_t) i] = 1;
        for (int32_t i : b->order_lse_big) in_lse[(size_t) i] = 1;
        for (int32_t i : b->order_f64)
            if (!in_lse[(size_t) i]) b->order_gen.push_back(i);
    }

    const double u1 = now_();
    std::vector<DevChunk> chunks;
    for (auto *c : b->chunks) chunks.push_back(c->dev);
    std::vector<int32_t> pack_list, plane_list;
    /* declared after the staging vectors: an early return drains the stream before they are destroyed */
    Drain drain{s};

    HIP_TRY(b->d_hmms.upload(b->hmms, s));
    HIP_TRY(b->d_cols.upload(b->cols, s));
    HIP_TRY(b->d_chunks.upload(chunks, s));
    HIP_TRY(b->d_read_byte_off.upload(b->read_byte_off, s));
    HIP_TRY(b->d_partition.upload(b->partition, s));
    HIP_TRY(b->d_np.upload(b->cell_np, s));
    HIP_TRY(b->d_scols.upload(b->scols, s));
    HIP_TRY(b->d_pcols.upload(b->pcols, s));
    if (b->need_wide) {
        HIP_TRY(b->d_next.upload(b->cell_next, s));
        HIP_TRY(b->d_prev.upload(b->cell_prev, s));
    }
    HIP_TRY(b->d_order_wide.upload(b->order_wide, s));
    HIP_TRY(b->d_order_mid.upload(b->order_mid, s));
    HIP_TRY(b->d_order_narrow.upload(b->order_narrow, s));
    HIP_TRY(b->d_order_f64.upload(b->order_gen, s));
    HIP_TRY(b->d_order_lse.upload(b->order_lse, s));
    HIP_TRY(b->d_order_lse_big.upload(b->order_lse_big, s));
    const double u2 = now_();
    {   /* fast tiles first */
        auto is_fast = [](const EmitTile &t) { return t.uniform_alleles != 0 && !(t.flags & MRP_FLAG_INCLUDE_ANCESTOR_SUB_PROB); };
        auto mid_it = std::stable_partition(b->tiles.begin(), b->tiles.end(), is_fast);
        b->n_fast_tiles = mid_it - b->tiles.begin();
    }
    b->n_tiles_dev = (int64_t) b->tiles.size();
    HIP_TRY(b->d_tiles.upload(b->tiles, s));
    pack_list.reserve(b->pcols.size());
    for (size_t i = 0; i < b->pcols.size(); i++) (b->pcols[i].need_planes ? plane_list : pack_list).push_back((int32_t) i);
    HIP_TRY(b->d_pack_list.upload(pack_list, s));
    HIP_TRY(b->d_plane_list.upload(plane_list, s));
    const double u3 = now_();
    const size_t nC = (size_t) b->n_cells_total;
    HIP_TRY(b->d_planes.alloc((size_t) b->n_slots * 8));
    HIP_TRY(b->d_slot_total.alloc((size_t) b->n_slots));
    HIP_TRY(b->d_slot_bytes.alloc((size_t) b->n_slots * 16));
    HIP_TRY(b->d_cost.alloc(nC));
    HIP_TRY(b->d_f32.alloc(nC));
    HIP_TRY(b->d_b32.alloc(nC));
    HIP_TRY(b->d_mf32.alloc((size_t) b->n_merge));
    HIP_TRY(b->d_mb32.alloc((size_t) b->n_merge));
    if (!b->order_f64.empty()) { /* fp64 result arrays only when some hmm takes the fp64 path */
        HIP_TRY(b->d_f.alloc(nC));
        HIP_TRY(b->d_b.alloc(nC));
        HIP_TRY(b->d_mf.alloc((size_t) b->n_merge));
        HIP_TRY(b->d_mb.alloc((size_t) b->n_merge));
    }
    HIP_TRY(b->d_total.alloc(b->cols.size()));
    HIP_TRY(b->d_hmm_fb.alloc(2 * b->hmms.size()));
    const double u4 = now_();
    HIP_TRY(hipStreamSynchronize(s));
    if (timing_)
        fprintf(stderr, "      upload: plan %.2f ms, arrays %.2f, tiles+lists %.2f, allocs %.2f, sync %.2f\n", u1 - u0, u2 - u1, u3 - u2, u4 - u3, now_() - u4);

    b->dev = b->view();
    /* host copies of the bulky inputs are no longer needed */
    HostVec<int64_t>().swap(b->read_byte_off);
    HostVec<uint64_t>().swap(b->partition);
    HostVec<uint32_t>().swap(b->cell_next);
    HostVec<uint32_t>().swap(b->cell_prev);
    HostVec<uint32_t>().swap(b->cell_np);
    b->uploaded = true;
    return MRP_OK;
}

int mrp_batch_launch(mrp_batch *b) {
    if (!b) return mrp_set_error(MRP_ERR_ARG, "batch is NULL");
    if (!b->uploaded) {
        int rc = mrp_batch_upload(b);
        if (rc != MRP_OK) return rc;
    }
    mrp_context *ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const MrpBatchDev &d = b->dev;
    hipStream_t ps = s; /* byte packing / bit planes ahead of the emission kernel, on the same stream */
    const size_t slot = (size_t) (b->n_launches % mrp_batch::EV_RING);
    if (slot >= b->ev_ring.size()) {
        std::array<hipEvent_t, 5> fresh{};
        for (auto &ev : fresh) HIP_TRY(hipEventCreate(&ev));
        b->ev_ring.push_back(fresh);
    }
    const std::array<hipEvent_t, 5> &ev = b->ev_ring[slot];
    if (b->n_launches >= mrp_batch::EV_RING) HIP_TRY(hipEventSynchronize(ev[2])); /* the launch that used these events has to be over */
    if (ps != s && ctx->last_emission) HIP_TRY(hipStreamWaitEvent(ps, ctx->last_emission, 0));
    HIP_TRY(hipEventRecord(ev[0], ps));
    HIP_TRY(mrp_launch_planes(d, ps));
    if (b->resident && mrp_dup('p')) HIP_TRY(mrp_launch_planes(d, ps));
    HIP_TRY(hipEventRecord(ev[1], ps));
    if (ps != s) HIP_TRY(hipStreamWaitEvent(s, ev[1], 0));
    HIP_TRY(hipEventRecord(ev[4], s));
    if (b->pre_sweep) HIP_TRY(b->pre_sweep(s)); /* resident merge levels: cross product + emission in one pass */
    if (b->pre_sweep && mrp_dup('x')) HIP_TRY(b->pre_sweep(s));
    HIP_TRY(mrp_launch_emission(d, b->d_tiles.p, b->n_fast_tiles, b->n_tiles_dev - b->n_fast_tiles, s));
    HIP_TRY(hipEventRecord(ev[3], s));
    ctx->last_emission = ev[3];
    if (!b->order_f64.empty()) {
        /* stRPHmm_initialiseProbs (hmm.c:752-789) for the accumulate-in-place fp64 path */
        const double neg = -__builtin_inf();
        HIP_TRY(mrp_launch_fill_f64(b->d_mf.p, d.n_merge, neg, s));
        HIP_TRY(mrp_launch_fill_f64(b->d_mb.p, d.n_merge, neg, s));
        HIP_TRY(mrp_launch_fill_f64(b->d_total.p, d.n_cols, neg, s));
        HIP_TRY(mrp_launch_fill_f64(b->d_hmm_fb.p, 2 * d.n_hmms, neg, s));
    }
    /* size classes side by side: wide on the main stream, mid and narrow on the auxiliary streams */
    hipStream_t a0 = s, a1 = s;
    if (s == ctx->stream) HIP_TRY(ctx->side_streams(&a0, &a1));
    const bool side = a0 != s;
    if (side) {
        HIP_TRY(hipEventRecord(ctx->fork, s));
        HIP_TRY(hipStreamWaitEvent(a0, ctx->fork, 0));
        HIP_TRY(hipStreamWaitEvent(a1, ctx->fork, 0));
    }
    /* Wide and mid hmms: 512 threads walk an hmm fastest, but the kernel's 128 registers then allow two workgroups to a CU.  When the
     * concurrent batches of a call together bring more such workgroups than the device has slots for (the top levels of a
     * 1 152-chunk call: 2 304 on 512 slots), 256 threads -- four to a CU -- get them through sooner: -3 % per call, A/B on one box;
     * a single batch, whose hmms all find a slot, stays at 512 (+4 % with 256). */
    const int64_t chains = 2 * (int64_t) (b->order_wide.size() + b->order_mid.size()) * (int64_t) ctx->concurrent_batches;
    const int t_chain = ctx->concurrent_batches > 1 && chains > 2 * 256 ? 256 : 512; /* (a batch on its own -- the kernel replay of bench.py too: 512, as measured in rounds 1-3) */
    const int t_wide = t_chain, t_mid = t_chain, t_narrow = 64;
    /* workgroup sizes of the recursion kernel's classes (measured; in the
                                                         * concurrent batches of a call 64 to 512 threads for the mid class make no difference) */
    HIP_TRY(mrp_launch_sweep_i32(d, b->d_order_wide.p, (int64_t) b->order_wide.size(), t_wide, b->max_merge_wide, s));
    HIP_TRY(mrp_launch_sweep_i32(d, b->d_order_mid.p, (int64_t) b->order_mid.size(), t_mid, b->max_merge_mid, a0));
    HIP_TRY(mrp_launch_sweep_i32(d, b->d_order_narrow.p, (int64_t) b->order_narrow.size(), t_narrow, b->max_merge_narrow, a1));
    if (b->resident) { /* the launch census counts the resident path's classes (a class without hmms is not launched) */
        if (!b->order_wide.empty()) ctx->census.bump(census_sweep_slot(SWEEP_WIDE));
        if (!b->order_mid.empty()) ctx->census.bump(census_sweep_slot(SWEEP_MID));
        if (!b->order_narrow.empty()) ctx->census.bump(census_sweep_slot(SWEEP_NARROW));
    }
    if (b->resident && mrp_dup('s')) {
        HIP_TRY(mrp_launch_sweep_i32(d, b->d_order_wide.p, (int64_t) b->order_wide.size(), t_wide, b->max_merge_wide, s));
        HIP_TRY(mrp_launch_sweep_i32(d, b->d_order_mid.p, (int64_t) b->order_mid.size(), t_mid, b->max_merge_mid, a0));
        HIP_TRY(mrp_launch_sweep_i32(d, b->d_order_narrow.p, (int64_t) b->order_narrow.size(), t_narrow, b->max_merge_narrow, a1));
    }
    HIP_TRY(mrp_launch_sweep_f64(d, b->d_order_f64.p, (int64_t) b->order_gen.size(), 256, s));
    HIP_TRY(mrp_launch_sweep_lse(d, b->d_order_lse.p, (int64_t) b->order_lse.size(), b->max_merge_lse, s));
    HIP_TRY(mrp_launch_sweep_lse(d, b->d_order_lse_big.p, (int64_t) b->order_lse_big.size(), std::max(b->max_merge_lse_big, MRP_LSE_CUR_LDS_MAX_MERGE + 2), s));
    if (side) {
        HIP_TRY(hipEventRecord(ctx->join[0], a0));
        HIP_TRY(hipEventRecord(ctx->join[1], a1));
        HIP_TRY(hipStreamWaitEvent(s, ctx->join[0], 0));
        HIP_TRY(hipStreamWaitEvent(s, ctx->join[1], 0));
    }
    HIP_TRY(hipEventRecord(ev[2], s));
    b->n_launches++;
    b->launched = true;
    return MRP_OK;
}

int mrp_batch_stats(mrp_batch *b, mrp_launch_stats *out) {
    if (!b || !out) return mrp_set_error(MRP_ERR_ARG, "mrp_batch_stats: NULL argument");
    *out = b->stats;
    out->n_hmms_lse = (int64_t) (b->order_lse.size() + b->order_lse_big.size());
    out->n_hmms_generic = (int64_t) b->order_gen.size();
    out->n_hmms_int32 = (int64_t) (b->order_wide.size() + b->order_mid.size() + b->order_narrow.size());
    if (b->launched) {
        mrp_context *ctx = b->ctx;
        HIP_TRY(hipSetDevice(ctx->device));
        /* the launches since the previous call (the most recent one at least), as far back as the ring reaches */
        const int64_t k = std::min<int64_t>(std::max<int64_t>(b->n_launches - b->stats_mark, 1), std::min<int64_t>(b->n_launches, mrp_batch::EV_RING));
        b->stats_mark = b->n_launches;
        double sa = 0, se = 0, sc = 0;
        float a = 0, e = 0, c = 0;
        for (int64_t j = 0; j < k; j++) { /* oldest first; the last one is the most recent launch */
            const auto &ev = b->ev_ring[(size_t) ((b->n_launches - k + j) % mrp_batch::EV_RING)];
            HIP_TRY(hipEventSynchronize(ev[2]));
            HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
            HIP_TRY(hipEventElapsedTime(&e, ev[4], ev[3]));
            HIP_TRY(hipEventElapsedTime(&c, ev[3], ev[2]));
            sa += a; se += e; sc += c;
        }
        out->planes_ms = a;
        out->emission_ms = e;
        out->sweep_ms = c;
        out->avg_planes_ms = k ? sa / (double) k : 0.0;
        out->avg_emission_ms = k ? se / (double) k : 0.0;
        out->avg_sweep_ms = k ? sc / (double) k : 0.0;
        out->launches_averaged = k;
    }
    return MRP_OK;
}

/* the most recent launch by kernel family (ms): packing / bit planes, cross product + emission, recursion.  Called after the
 * stream the launch ran on has been waited for. */
void mrp_batch_last_launch_ms(mrp_batch *b, float *pack, float *emission, float *recursion) {
    *pack = *emission = *recursion = 0.f;
    if (!b || !b->launched || b->n_launches < 1) return;
    const auto &ev = b->ev_ring[(size_t) ((b->n_launches - 1) % mrp_batch::EV_RING)];
    (void) hipEventElapsedTime(pack, ev[0], ev[1]);
    (void) hipEventElapsedTime(emission, ev[4], ev[3]);
    (void) hipEventElapsedTime(recursion, ev[3], ev[2]);
}

int mrp_batch_download(mrp_batch *b) {
    if (!b) return mrp_set_error(MRP_ERR_ARG, "batch is NULL");
    if (!b->launched) return mrp_set_error(MRP_ERR_ARG, "mrp_batch_download before mrp_batch_launch");
    mrp_context *ctx = b->ctx;
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const MrpBatchDev &d = b->dev;
    const bool any_out = std::any_of(b->outs.begin(), b->outs.end(), [](const JobOut &o) { return o.cell_f != nullptr; });
    if (!any_out) {
        HIP_TRY(hipStreamSynchronize(s));
        return MRP_OK;
    }
    const bool has_f64 = !b->order_f64.empty();
    std::vector<double> f, bb, mf, mb, tot((size_t) d.n_cols), fb((size_t) (2 * d.n_hmms));
    std::vector<int32_t> f32((size_t) d.n_cells), b32((size_t) d.n_cells), mf32((size_t) d.n_merge), mb32((size_t) d.n_merge);
    if (has_f64) { f.resize((size_t) d.n_cells); bb.resize((size_t) d.n_cells); mf.resize((size_t) d.n_merge); mb.resize((size_t) d.n_merge); }
    auto pull = [&](void *h, const void *p, size_t bytes) -> hipError_t {
        if (bytes == 0) return hipSuccess;
        return hipMemcpyAsync(h, p, bytes, hipMemcpyDeviceToHost, s);
    };
    HIP_TRY(pull(f32.data(), d.cell_f32, f32.size() * 4));
    HIP_TRY(pull(b32.data(), d.cell_b32, b32.size() * 4));
    HIP_TRY(pull(mf32.data(), d.merge_f32, mf32.size() * 4));
    HIP_TRY(pull(mb32.data(), d.merge_b32, mb32.size() * 4));
    if (has_f64) {
        HIP_TRY(pull(f.data(), d.cell_f, f.size() * 8));
        HIP_TRY(pull(bb.data(), d.cell_b, bb.size() * 8));
        HIP_TRY(pull(mf.data(), d.merge_f, mf.size() * 8));
        HIP_TRY(pull(mb.data(), d.merge_b, mb.size() * 8));
    }
    HIP_TRY(pull(tot.data(), d.col_total, tot.size() * 8));
    HIP_TRY(pull(fb.data(), d.hmm_fb, fb.size() * 8));
    HIP_TRY(hipStreamSynchronize(s));
    /* widen the max-plus integers to the reference's doubles (exact); MRP_NEG_I32 is log(0) */
    auto widen = [](double *dst, const int32_t *src, int64_t n) {
        for (int64_t i = 0; i < n; i++) dst[i] = src[i] == MRP_NEG_I32 ? -__builtin_inf() : (double) src[i];
    };
    for (size_t i = 0; i < b->outs.size(); i++) {
        const JobOut &o = b->outs[i];
        if (!o.cell_f) continue; /* device-only job */
        if (o.int_path) {
            widen(o.cell_f, f32.data() + o.cell0, o.n_cells);
            widen(o.cell_b, b32.data() + o.cell0, o.n_cells);
            if (o.n_merge > 0) {
                widen(o.merge_f, mf32.data() + o.mcell0, o.n_merge);
                widen(o.merge_b, mb32.data() + o.mcell0, o.n_merge);
            }
        } else {
            memcpy(o.cell_f, f.data() + o.cell0, sizeof(double) * (size_t) o.n_cells);
            memcpy(o.cell_b, bb.data() + o.cell0, sizeof(double) * (size_t) o.n_cells);
            if (o.n_merge > 0) {
                memcpy(o.merge_f, mf.data() + o.mcell0, sizeof(double) * (size_t) o.n_merge);
                memcpy(o.merge_b, mb.data() + o.mcell0, sizeof(double) * (size_t) o.n_merge);
            }
        }
        memcpy(o.col_total, tot.data() + o.col0, sizeof(double) * (size_t) o.n_cols);
        *o.hmm_f = fb[2 * i];
        *o.hmm_b = fb[2 * i + 1];
    }
    return MRP_OK;
}

int mrp_fb_run(mrp_context *ctx, int64_t n_jobs, const mrp_hmm_job *jobs) {
    if (!ctx || n_jobs < 0 || (n_jobs > 0 && !jobs)) return mrp_set_error(MRP_ERR_ARG, "mrp_fb_run: bad arguments");
    if (n_jobs == 0) return MRP_OK;
    mrp_batch *b = nullptr;
    int rc = mrp_batch_create(ctx, &b);
    for (int64_t i = 0; rc == MRP_OK && i < n_jobs; i++) rc = mrp_batch_add(b, &jobs[i]);
    if (rc == MRP_OK) rc = mrp_batch_upload(b);
    if (rc == MRP_OK) rc = mrp_batch_launch(b);
    if (rc == MRP_OK) rc = mrp_batch_download(b);
    mrp_batch_destroy(b);
    return rc;
}

/* ---- emission-only seam -------------------------------------------------------------------- */
static int one_column(mrp_context *ctx, const mrp_chunk *chunk, int32_t first_site, int32_t n_sites, int32_t depth,
                      const int64_t *read_byte_off, DevCol *col) {
    if (!ctx || !chunk || chunk->ctx != ctx) return mrp_set_error(MRP_ERR_ARG, "bad context/chunk");
    if (chunk->host_wait() != hipSuccess) return mrp_set_error(MRP_ERR_HIP, "chunk upload failed");
    if (depth < 0 || depth > MRP_MAX_READ_PARTITIONING_DEPTH || n_sites < 0 || first_site < 0 ||
        (int64_t) first_site + n_sites > chunk->n_sites || (depth > 0 && !read_byte_off))
        return mrp_set_error(MRP_ERR_ARG, "bad column description");
    memset(col, 0, sizeof(*col));
    col->n_cells = 0;
    col->site_start = first_site;
    col->n_sites = n_sites;
    col->depth = depth;
    col->n_slots = (int32_t) (chunk->allele_offset[first_site + n_sites] - chunk->allele_offset[first_site]);
    for (int i = 0; i < depth; i++)
        if (read_byte_off[i] < 0 || read_byte_off[i] + col->n_slots > chunk->pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "read %d: profile bytes outside the pool", i);
    return MRP_OK;
}

static int run_planes(mrp_context *ctx, const mrp_chunk *chunk, const DevCol &col, const int64_t *read_byte_off,
                      DevBuf<DevCol> &d_col, DevBuf<DevChunk> &d_chunk, DevBuf<int64_t> &d_off,
                      DevBuf<uint64_t> &d_planes, DevBuf<uint32_t> &d_tot) {
    hipStream_t s = ctx->stream;
    DevBuf<uint32_t> d_bytes;
    DevBuf<PlaneCol> d_pcol;
    PlaneCol pc{};
    pc.pool = chunk->dev.pool;
    pc.read_off = 0;
    pc.slot_off = 0;
    pc.depth = col.depth;
    pc.n_slots = col.n_slots;
    pc.need_planes = 1;
    /* host staging of the queued uploads */
    std::vector<DevCol> hc(1, col);
    std::vector<DevChunk> hch(1, chunk->dev);
    std::vector<int64_t> ho(read_byte_off, read_byte_off + col.depth);
    std::vector<PlaneCol> hpc(1, pc);
    /* declared last, so it runs first: whatever way this function is left, the stream is drained before the staging vectors
     * above and the scratch buffers (written by the kernel) go */
    Drain drain{s};
    HIP_TRY(d_col.upload(hc, s));
    HIP_TRY(d_chunk.upload(hch, s));
    HIP_TRY(d_off.upload(ho, s));
    HIP_TRY(d_planes.alloc((size_t) col.n_slots * 8));
    HIP_TRY(d_tot.alloc((size_t) col.n_slots));
    HIP_TRY(d_bytes.alloc((size_t) col.n_slots * 16));
    HIP_TRY(d_pcol.upload(hpc, s));
    MrpBatchDev d{};
    d.pcols = d_pcol.p;
    d.cols = d_col.p;
    d.chunks = d_chunk.p;
    d.read_byte_off = d_off.p;
    d.planes = d_planes.p;
    d.slot_total = d_tot.p;
    d.slot_bytes = d_bytes.p;
    d.n_cols = 1;
    HIP_TRY(mrp_launch_planes(d, s));
    return MRP_OK;
}

int mrp_count_bit_vectors(mrp_context *ctx, const mrp_chunk *chunk, int32_t first_site, int32_t n_sites, int32_t depth,
                          const int64_t *read_byte_off, uint64_t *planes_out) {
    DevCol col;
    int rc = one_column(ctx, chunk, first_site, n_sites, depth, read_byte_off, &col);
    if (rc != MRP_OK) return rc;
    if (col.n_slots == 0) return MRP_OK;
    if (!planes_out) return mrp_set_error(MRP_ERR_ARG, "planes_out is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<DevCol> d_col; DevBuf<DevChunk> d_chunk; DevBuf<int64_t> d_off; DevBuf<uint64_t> d_planes; DevBuf<uint32_t> d_tot;
    rc = run_planes(ctx, chunk, col, read_byte_off, d_col, d_chunk, d_off, d_planes, d_tot);
    if (rc != MRP_OK) return rc;
    HIP_TRY(hipMemcpyAsync(planes_out, d_planes.p, sizeof(uint64_t) * 8 * (size_t) col.n_slots, hipMemcpyDeviceToHost,
                           ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MRP_OK;
}

int mrp_emissions(mrp_context *ctx, const mrp_chunk *chunk, int32_t first_site, int32_t n_sites, int32_t depth,
                  const int64_t *read_byte_off, uint32_t flags, int64_t n_cells, const uint64_t *partitions,
                  double *out) {
    DevCol col;
    int rc = one_column(ctx, chunk, first_site, n_sites, depth, read_byte_off, &col);
    if (rc != MRP_OK) return rc;
    if (n_cells < 0 || (n_cells > 0 && (!partitions || !out))) return mrp_set_error(MRP_ERR_ARG, "bad cell arrays");
    if (n_cells == 0) return MRP_OK;
    if (flags & MRP_FLAG_INCLUDE_ANCESTOR_SUB_PROB)
        for (int s = 0; s < n_sites; s++)
            if (chunk->allele_number[first_site + s] > MRP_MAX_ALLELES)
                return mrp_set_error(MRP_ERR_UNSUPPORTED, "site %d has more than %d alleles (ancestor mode)", first_site + s,
                            MRP_MAX_ALLELES);
    HIP_TRY(hipSetDevice(ctx->device));
    DevBuf<DevCol> d_col; DevBuf<DevChunk> d_chunk; DevBuf<int64_t> d_off; DevBuf<uint64_t> d_planes; DevBuf<uint32_t> d_tot;
    rc = run_planes(ctx, chunk, col, read_byte_off, d_col, d_chunk, d_off, d_planes, d_tot);
    if (rc != MRP_OK) return rc;
    DevBuf<uint64_t> d_part; DevBuf<double> d_out;
    std::vector<uint64_t> hp(partitions, partitions + n_cells);
    HIP_TRY(d_part.upload(hp, ctx->stream));
    HIP_TRY(d_out.alloc((size_t) n_cells));
    HIP_TRY(mrp_launch_emissions(d_col.p, d_chunk.p, d_planes.p, d_tot.p, flags, n_cells, d_part.p, d_out.p, ctx->stream));
    HIP_TRY(hipMemcpyAsync(out, d_out.p, sizeof(double) * (size_t) n_cells, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return MRP_OK;
}

}  /* extern "C" */
