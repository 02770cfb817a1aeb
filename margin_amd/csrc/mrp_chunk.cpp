/*
 * mrp_chunk.cpp -- a chunk's reference tables and profile bytes: validated and copied on the host, then uploaded either on their
 * own (mrp_chunk_create) or with the other chunks of a work queue's batch in one block (mrp_chunk_block_create).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "mrp_internal.h"
#include "mrp_level_order.h" /* BlockCarver, carve_chunk */

extern "C" {

void mrp_chunk_host_view(const mrp_chunk *chunk, mrp_chunk_host *out) {
    if (chunk->pool_host_pending.load() && hipEventSynchronize(chunk->pool_host_ready) == hipSuccess) chunk->pool_host_pending.store(false);
    out->n_sites = chunk->n_sites;
    out->allele_number = chunk->allele_number.data();
    out->allele_offset = chunk->allele_offset.data();
    out->sub_offset = chunk->sub_offset.data();
    out->sub = chunk->sub.data();
    out->prior = chunk->prior.data();
    out->pool = chunk->pool_host;
    out->pool_bytes = chunk->pool_bytes;
}
mrp_context *mrp_chunk_context(const mrp_chunk *chunk) { return chunk->ctx; }

}  /* extern "C" */

/* host half of a chunk: validation, prefix sums, host copies of everything (the caller's arrays may go after the call) */
static int chunk_host_init(mrp_context *ctx, int64_t n_sites, const uint32_t *allele_number, const uint16_t *substitution_log_probs,
                           const uint16_t *allele_prior_log_probs, const uint8_t *profile_pool, int64_t pool_bytes, mrp_chunk **out,
                           bool copy_pool = true) {
    if (!ctx || !out || n_sites < 0 || pool_bytes < 0 || (n_sites > 0 && !allele_number) ||
        (pool_bytes > 0 && !profile_pool))
        return mrp_set_error(MRP_ERR_ARG, "mrp_chunk_create: bad arguments");
    *out = nullptr;
    mrp_chunk *ch = new (std::nothrow) mrp_chunk();
    if (!ch) return mrp_set_error(MRP_ERR_NOMEM, "out of host memory");
    ch->ctx = ctx;
    ch->n_sites = n_sites;
    ch->pool_bytes = pool_bytes;
    ch->allele_number.assign(allele_number, allele_number + n_sites);
    ch->allele_offset.resize(n_sites + 1);
    ch->sub_offset.resize(n_sites + 1);
    uint64_t off = 0, soff = 0;
    for (int64_t i = 0; i < n_sites; i++) {
        ch->allele_offset[i] = (uint32_t) off;
        ch->sub_offset[i] = (uint32_t) soff;
        uint64_t A = allele_number[i];
        if (A == 0 || A > 65535) {
            delete ch;
            return mrp_set_error(MRP_ERR_ARG, "site %lld has %llu alleles", (long long) i, (unsigned long long) A);
        }
        off += A;
        soff += A * A;
        ch->max_alleles = std::max<uint32_t>(ch->max_alleles, (uint32_t) A);
        if (off > 0xFFFFFFFFull || soff > 0xFFFFFFFFull) {
            delete ch;
            return mrp_set_error(MRP_ERR_ARG, "allele tables exceed 32-bit offsets");
        }
    }
    ch->allele_offset[n_sites] = (uint32_t) off;
    ch->same_until.resize((size_t) n_sites);
    for (int64_t i = n_sites - 1; i >= 0; i--)
        ch->same_until[(size_t) i] = (i + 1 < n_sites && allele_number[i + 1] == allele_number[i]) ? ch->same_until[(size_t) i + 1] : (int32_t) (i + 1);
    ch->sub_offset[n_sites] = (uint32_t) soff;
    std::vector<uint16_t> &sub = ch->sub, &prior = ch->prior;
    sub.assign(soff, 0);
    prior.assign(off, 0);
    if (pool_bytes > 0 && copy_pool) ch->pool.assign(profile_pool, profile_pool + pool_bytes);
    ch->pool_host = ch->pool.data(); /* (copy_pool = false: set by the caller, who keeps the bytes elsewhere) */
    if (substitution_log_probs) sub.assign(substitution_log_probs, substitution_log_probs + soff);
    if (allele_prior_log_probs) prior.assign(allele_prior_log_probs, allele_prior_log_probs + off);
    for (uint16_t v : sub) ch->max_sub = std::max<uint32_t>(ch->max_sub, v);
    for (uint16_t v : prior) ch->max_prior = std::max<uint32_t>(ch->max_prior, v);
    *out = ch;
    return MRP_OK;
}

extern "C" {
int mrp_chunk_create(mrp_context *ctx, int64_t n_sites, const uint32_t *allele_number,
                     const uint16_t *substitution_log_probs, const uint16_t *allele_prior_log_probs,
                     const uint8_t *profile_pool, int64_t pool_bytes, mrp_chunk **out) {
    mrp_chunk *ch = nullptr;
    int rc = chunk_host_init(ctx, n_sites, allele_number, substitution_log_probs, allele_prior_log_probs, profile_pool, pool_bytes, &ch);
    if (rc != MRP_OK) return rc;
    *out = nullptr;
    hipError_t e = hipSetDevice(ctx->device);
    hipStream_t s = ctx->stream;
    ch->arrays.bind(&ctx->pool); /* from the context's caching allocator */
    if (e == hipSuccess) e = ch->d_allele_number.upload(ch->allele_number, s);
    if (e == hipSuccess) e = ch->d_allele_offset.upload(ch->allele_offset, s);
    if (e == hipSuccess) e = ch->d_sub_offset.upload(ch->sub_offset, s);
    if (e == hipSuccess) e = ch->d_same_until.upload(ch->same_until, s);
    if (e == hipSuccess) e = ch->d_sub.upload(ch->sub, s);
    if (e == hipSuccess) e = ch->d_prior.upload(ch->prior, s);
    if (e == hipSuccess) e = ch->d_pool.alloc((size_t) pool_bytes + MRP_POOL_TAIL_PAD);
    if (e == hipSuccess && pool_bytes > 0)
        e = hipMemcpyAsync(ch->d_pool.p, ch->pool.data(), (size_t) pool_bytes, hipMemcpyHostToDevice, s); /* (the chunk's own copy: the caller's may go) */
    if (e == hipSuccess) e = ctx->wait_stream(s);
    if (e != hipSuccess) {
        delete ch;
        return mrp_set_error(MRP_ERR_HIP, "chunk upload failed: %s", hipGetErrorString(e));
    }
    ch->dev.allele_number = ch->d_allele_number.p;
    ch->dev.allele_offset = ch->d_allele_offset.p;
    ch->dev.sub_offset = ch->d_sub_offset.p;
    ch->dev.sub = ch->d_sub.p;
    ch->dev.prior = ch->d_prior.p;
    ch->dev.pool = ch->d_pool.p;
    ch->dev.same_until = ch->d_same_until.p;
    *out = ch;
    return MRP_OK;
}
}  /* extern "C" */

/* The chunks of one batch of a work queue, uploaded TOGETHER: every array of every chunk is copied (by the calling thread's
 * host pool) into one page-locked block, which goes to one device block with one asynchronous copy on the context's stream;
 * one event ends it.  Nothing is waited for here: the first device work that reads a chunk waits for the event on its stream
 * (mrp_engine.cpp) or on the host (mrp_chunk::host_wait).  Per chunk this replaces seven allocations and seven pageable
 * copies (30 ms for 288 chunks) by a share of one. */
int mrp_chunk_block_create(mrp_context *ctx, int64_t n, const mrp_chunk_desc *const *descs, mrp_chunk **out, mrp_chunk_block *blk, int groups,
                           const uint8_t *const *device_pools) {
    if (!ctx || n < 0 || !blk || (n > 0 && (!descs || !out))) return mrp_set_error(MRP_ERR_ARG, "mrp_chunk_block_create: bad arguments");
    for (int64_t i = 0; i < n; i++) out[i] = nullptr;
    HIP_TRY(hipSetDevice(ctx->device));
    std::vector<int> rcs((size_t) n, MRP_OK);
    std::vector<std::string> msgs((size_t) n);
    mrp_parallel_for(n, 4, [&](int64_t i) {
        const mrp_chunk_desc &c = *descs[i];
        /* (the profile bytes -- nine tenths of a chunk -- are copied ONCE, into the page-locked block below, which outlives the chunk) */
        rcs[(size_t) i] = chunk_host_init(ctx, c.n_sites, c.allele_number, c.substitution_log_probs, c.allele_prior_log_probs, c.profile_pool, c.pool_bytes, &out[i], false);
        if (rcs[(size_t) i] != MRP_OK) msgs[(size_t) i] = mrp_last_error();
    });
    int rc = MRP_OK;
    for (int64_t i = 0; i < n && rc == MRP_OK; i++)
        if (rcs[(size_t) i] != MRP_OK) rc = mrp_set_error(rcs[(size_t) i], "%s", msgs[(size_t) i].c_str());
    if (groups < 1 || n < 4 * (int64_t) groups) groups = 1;
    if (groups > 16) groups = 16;
    /* the order of the chunks in the block: group 0's, then group 1's, ... -- the groups are the concurrent batches mrp_phase_reads_many
     * will deal the chunks to (mrp_phase_group_assign: not always i % groups) */
    std::vector<uint8_t> group_of((size_t) n + 1, 0);
    {
        int64_t sites = 0;
        for (int64_t i = 0; i < n; i++) sites += descs[i]->n_sites;
        mrp_phase_group_assign(n, groups, sites, group_of.data());
    }
    std::vector<int64_t> order; order.reserve((size_t) n);
    std::vector<int64_t> group_first((size_t) groups + 1, 0);
    for (int g = 0; g < groups; g++) { group_first[(size_t) g] = (int64_t) order.size(); for (int64_t i = 0; i < n; i++) if (group_of[(size_t) i] == g) order.push_back(i); }
    group_first[(size_t) groups] = n;
    std::vector<size_t> off((size_t) n + 1, 0), at_of((size_t) n, 0); /* off: by position in the block; at_of: by chunk */
    auto carve = [&](BlockCarver &c, const mrp_chunk *ch) {
        return carve_chunk(c, (size_t) ch->n_sites, ch->prior.size(), ch->sub.size(), (size_t) ch->pool_bytes, device_pools == nullptr);
    };
    BlockCarver sizes(nullptr, MRP_CHUNK_BLOCK_ALIGN);
    for (int64_t k = 0; k < n && rc == MRP_OK; k++) {
        at_of[(size_t) order[(size_t) k]] = off[(size_t) k];
        carve(sizes, out[order[(size_t) k]]);
        off[(size_t) k + 1] = sizes.used;
    }
    hipError_t e = hipSuccess;
    if (rc == MRP_OK) {
        blk->dev.pool = &ctx->pool;
        e = blk->host.reserve(chunk_block_bytes(off[(size_t) n]));
        if (e == hipSuccess) e = blk->dev.alloc(chunk_block_bytes(off[(size_t) n]));
        if (e == hipSuccess && !blk->ready) e = hipEventCreateWithFlags(&blk->ready, hipEventBlockingSync | hipEventDisableTiming);
        while (e == hipSuccess && (int) blk->group_ready.size() < groups) {
            hipEvent_t ev = nullptr;
            e = hipEventCreateWithFlags(&ev, hipEventBlockingSync | hipEventDisableTiming);
            if (e == hipSuccess) blk->group_ready.push_back(ev);
        }
    }
    if (rc == MRP_OK && e == hipSuccess) {
        char *hb = (char *) blk->host.p;
        uint8_t *db = blk->dev.p;
        for (int g = 0; g < groups && e == hipSuccess; g++) { /* group by group: the copy of one runs beside the staging of the next */
            const int64_t g_n = group_first[(size_t) g + 1] - group_first[(size_t) g];
            mrp_parallel_for(g_n, 4, [&](int64_t k) {
                const int64_t i = order[(size_t) (group_first[(size_t) g] + k)];
                mrp_chunk *ch = out[i];
                BlockCarver c(hb + at_of[(size_t) i], MRP_CHUNK_BLOCK_ALIGN);
                const ChunkSlices h = carve(c, ch); /* in the page-locked block; the device's copy of a slice is as far into the device block */
                auto put = [&](auto *dst, const void *src, size_t count) { if (count) memcpy(dst, src, count * sizeof(*dst)); return (decltype(dst)) (db + ((char *) dst - hb)); };
                ch->dev.allele_number = put(h.allele_number, ch->allele_number.data(), ch->allele_number.size());
                ch->dev.allele_offset = put(h.allele_offset, ch->allele_offset.data(), ch->allele_offset.size());
                ch->dev.sub_offset = put(h.sub_offset, ch->sub_offset.data(), ch->sub_offset.size());
                ch->dev.same_until = put(h.same_until, ch->same_until.data(), ch->same_until.size());
                ch->dev.sub = put(h.sub, ch->sub.data(), ch->sub.size());
                ch->dev.prior = put(h.prior, ch->prior.data(), ch->prior.size());
                if (device_pools) {
                    ch->pool_host = descs[i]->profile_pool;
                    ch->dev.pool = device_pools[i];
                } else {
                    ch->pool_host = h.pool;
                    ch->dev.pool = put(h.pool, descs[i]->profile_pool, (size_t) ch->pool_bytes);
                }
            });
            const size_t lo = off[(size_t) group_first[(size_t) g]], hi = off[(size_t) group_first[(size_t) g + 1]];
            if (hi > lo) e = hipMemcpyAsync(db + lo, hb + lo, hi - lo, hipMemcpyHostToDevice, ctx->stream);
            if (e == hipSuccess) e = hipEventRecord(blk->group_ready[(size_t) g], ctx->stream);
        }
        if (e == hipSuccess) e = hipEventRecord(blk->ready, ctx->stream);
        if (e == hipSuccess && getenv("MRP_TIMING_UPLOAD")) { /* diagnosis only: waits for the copy */
            const auto t0 = std::chrono::steady_clock::now();
            e = hipEventSynchronize(blk->ready);
            fprintf(stderr, "  chunk block: %lld chunks, %.1f MB, copy waited %.2f ms\n", (long long) n, (double) off[(size_t) n] / 1e6,
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        }
        if (e == hipSuccess)
            for (int64_t i = 0; i < n; i++) { out[i]->ready = blk->group_ready[(size_t) group_of[(size_t) i]]; out[i]->owns_ready = false; out[i]->ready_pending.store(true); }
    }
    if (rc == MRP_OK && e != hipSuccess) rc = mrp_set_error(MRP_ERR_HIP, "chunk block upload failed: %s", hipGetErrorString(e));
    if (rc != MRP_OK)
        for (int64_t i = 0; i < n; i++) { delete out[i]; out[i] = nullptr; }
    return rc;
}

extern "C" {

void mrp_chunk_destroy(mrp_chunk *chunk) {
    if (!chunk) return;
    (void) hipSetDevice(chunk->ctx->device);
    delete chunk;
}

}  /* extern "C" */
