/*
 * mrp_downsample.hip -- the downsampling to maxDepth on the device: ds_reads_kernel makes, a workgroup per
 * chunk, the mask the owners kernel of the aligned composites reads as `take`, from the extraction's per-read state where it lies in
 * HBM; mrp_downsample_reads is the same kernel over host arrays, its public seam.  The definition is mrp_downsample.cpp's; the draw,
 * the decision and the probability are the shared text of mrp_downsample.h.  gfx950 only.
 */
#include "mrp_internal.h"
#include "mrp_downsample.h"

#pragma clang fp contract(off)

namespace {

constexpr int DS_NT = 256, DS_WAVES = DS_NT / 64, DS_TILE = 1024;

__device__ inline int32_t ds_l(const MrpDsIn &in, int64_t r) { return in.l ? in.l[r] : (int32_t) (in.entry_first[r + 1] - in.entry_first[r]); }
/* (the extraction keeps alnReadLength + 1, its walk bound, htsIntegration.c:1901; the reference's (int), :1160) */
__device__ inline int32_t ds_h(const MrpDsIn &in, int64_t r) { return in.h ? in.h[r] : (int32_t) (in.limit[r * in.limit_stride] - 1); }

/* One workgroup per chunk.  (1) the chunk's total over its kept reads, a wave sum and a sum over the waves; (2) the fp64 decision -- a
 * shallow chunk (and one without variants) writes its mask and leaves; (3) batch by batch of DS_NT reads: the kept-rank of every read
 * by ballot / popcount with a running base, then B = the l of the reads ordered before it, by an all-pairs pass -- the workgroup streams
 * tiles of (h, l) of ALL the chunk's reads through LDS (a read that is not kept as (0, 0): it adds nothing), every thread compares its
 * own read with the tile's by the exact 64-bit cross product and the index tie-break; (4) p, the draw, the mask byte.  Exact integer
 * work, no sort, no scratch, no atomics, no limit on a chunk's reads; every store is a plain vector store to the thread's own read.
 * Every barrier is reached by the whole workgroup: the loop bounds, `all` and the early exit depend on the chunk alone. */
__global__ void __launch_bounds__(DS_NT) ds_reads_kernel(MrpDsIn in, const uint8_t *__restrict__ status, const MrpDsChunk *__restrict__ chunks,
                                                         int64_t D, uint64_t seed, double *__restrict__ prob, uint8_t *__restrict__ keep,
                                                         int32_t *__restrict__ downsampled) {
    __shared__ int64_t s_part[DS_WAVES];
    __shared__ int32_t s_cnt[DS_WAVES];
    __shared__ int2 s_tile[DS_TILE];
    const MrpDsChunk c = chunks[blockIdx.x];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    int64_t mine = 0;
    for (int64_t i = tid; i < c.n_reads; i += DS_NT)
        if (status[c.first + i] == MRP_READ_KEPT) mine += ds_l(in, c.first + i);
    for (int d = 32; d >= 1; d >>= 1) mine += __shfl_xor(mine, d, 64);
    if (lane == 0) s_part[wv] = mine;
    __syncthreads();
    int64_t total = 0;
    for (int w = 0; w < DS_WAVES; w++) total += s_part[w];
    const bool shallow = mrp_ds_shallow(total, c.V, D);
    if (shallow || c.V == 0) { /* htsIntegration.c:1166-1170: everybody stays; :1174-1186: everybody goes */
        for (int64_t i = tid; i < c.n_reads; i += DS_NT) {
            const bool stays = shallow && status[c.first + i] == MRP_READ_KEPT;
            keep[c.first + i] = stays;
            if (prob) prob[c.first + i] = stays ? 1.0 : 0.0;
        }
        if (tid == 0) downsampled[blockIdx.x] = !shallow;
        return;
    }
    const int64_t T = D * c.V;
    const bool all = total <= T;
    int64_t rank_base = 0;
    for (int64_t i0 = 0; i0 < c.n_reads; i0 += DS_NT) {
        const int64_t i = i0 + tid, r = c.first + i;
        const bool in_chunk = i < c.n_reads, kept = in_chunk && status[r] == MRP_READ_KEPT;
        const int32_t li = kept ? ds_l(in, r) : 0, hi = kept ? ds_h(in, r) : 0;
        const uint64_t kb = __ballot(kept);
        if (lane == 0) s_cnt[wv] = __popcll(kb);
        __syncthreads();
        int64_t k = rank_base + __popcll(kb & ((1ull << lane) - 1ull)), batch = 0;
        for (int w = 0; w < DS_WAVES; w++) {
            if (w < wv) k += s_cnt[w];
            batch += s_cnt[w];
        }
        int64_t B = 0;
        for (int64_t j0 = 0; !all && j0 < c.n_reads; j0 += DS_TILE) {
            __syncthreads(); /* the tile before has been read */
            for (int t = tid; t < DS_TILE; t += DS_NT) {
                const int64_t j = j0 + t;
                int2 v = make_int2(0, 0);
                if (j < c.n_reads && status[c.first + j] == MRP_READ_KEPT) v = make_int2(ds_h(in, c.first + j), ds_l(in, c.first + j));
                s_tile[t] = v;
            }
            __syncthreads();
            if (li > 0) {
                const int m = (int) min((int64_t) DS_TILE, c.n_reads - j0);
                for (int t = 0; t < m; t++) {
                    const int2 v = s_tile[t];
                    B += mrp_ds_before(v.x, v.y, j0 + t, hi, li, i) ? v.y : 0;
                }
            }
        }
        if (kept) {
            double q = li > 0 ? mrp_ds_prob(B, li, T) : (hi > 0 ? 1.0 : 0.0);
            if (all) q = 1.0;
            keep[r] = mrp_ds_draw(seed, c.overlap_start, c.overlap_end, k) < q; /* :1201 */
            if (prob) prob[r] = q;
        } else if (in_chunk) {
            keep[r] = 0;
            if (prob) prob[r] = 0.0;
        }
        rank_base += batch;
        __syncthreads(); /* before the next batch counts */
    }
    if (tid == 0) downsampled[blockIdx.x] = 1;
}

}  // namespace

hipError_t mrp_downsample_launch(hipStream_t s, int64_t n_chunks, const MrpDsChunk *d_chunks, const MrpDsIn &in, const uint8_t *d_status, int64_t max_depth,
                                 uint64_t seed, double *d_prob, uint8_t *d_keep, int32_t *d_downsampled) {
    if (n_chunks <= 0) return hipSuccess;
    hipLaunchKernelGGL(ds_reads_kernel, dim3((unsigned) n_chunks), dim3(DS_NT), 0, s, in, d_status, d_chunks, max_depth, seed, d_prob, d_keep, d_downsampled);
    return hipGetLastError();
}

/* ds_reads_kernel over host arrays: upload, one launch, 9 B per read and 4 B per chunk back */
extern "C" int mrp_downsample_reads(mrp_context *ctx, int64_t n_chunks, const int64_t *n_reads, const int64_t *first, const int32_t *l, const int32_t *h,
                                    const uint8_t *status, const int64_t *V, int64_t max_depth, uint64_t seed, const int64_t *overlap_start,
                                    const int64_t *overlap_end, double *prob_out, uint8_t *keep_out, mrp_downsampling_stats *stats) {
    static const char *who = "mrp_downsample_reads";
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_chunks < 0 || n_chunks >= (1ll << 31) || (n_chunks > 0 && (!n_reads || !first || !V || !overlap_start || !overlap_end)))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (max_depth <= 0) return mrp_set_error(MRP_ERR_ARG, "%s: max_depth must be positive", who);
    int64_t n_total = 0;
    for (int64_t c = 0; c < n_chunks; c++) { /* ascending, disjoint ranges: a read is written by one workgroup */
        if (n_reads[c] < 0 || V[c] < 0 || V[c] >= (1ll << 31) || first[c] < n_total || n_reads[c] >= (1ll << 31))
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: negative size, or its reads begin before the chunk before ends", who, (long long) c);
        n_total = first[c] + n_reads[c];
    }
    if (n_total >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 reads in one call", who);
    if (n_total > 0 && (!l || !h || !status || !keep_out)) return mrp_set_error(MRP_ERR_ARG, "%s: null read array", who);
    for (int64_t c = 0; c < n_chunks; c++)
        for (int64_t r = first[c]; r < first[c] + n_reads[c]; r++)
            if (l[r] < 0) return mrp_set_error(MRP_ERR_ARG, "%s: read %lld has a negative substring count", who, (long long) r);
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the seam runs the kernel; the host definition is mrp_downsample_keep_from_extracted)", who);
    ctx->last_downsampling = mrp_downsampling_stats{};
    if (n_chunks == 0) return MRP_OK;
    float ms = 0.f;
    HostVec<uint8_t> back_keep((size_t) n_total); /* (the outputs are written only on success) */
    HostVec<double> back_prob((size_t) n_total);
    HostVec<int32_t> flag((size_t) n_chunks);
    {
        HIP_TRY(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        HostVec<MrpDsChunk> hc((size_t) n_chunks);
        for (int64_t c = 0; c < n_chunks; c++) hc[(size_t) c] = MrpDsChunk{first[c], n_reads[c], V[c], overlap_start[c], overlap_end[c]};
        DevBuf<MrpDsChunk> d_chunks;
        DevBuf<int32_t> d_l, d_h, d_flag;
        DevBuf<uint8_t> d_status, d_keep;
        DevBuf<double> d_prob;
        d_chunks.pool = &ctx->pool;
        d_l.pool = d_h.pool = d_flag.pool = &ctx->pool;
        d_status.pool = d_keep.pool = &ctx->pool;
        d_prob.pool = &ctx->pool;
        hipEvent_t ev[2] = {nullptr, nullptr};
        struct Events { hipEvent_t *e; ~Events() { for (int i = 0; i < 2; i++) if (e[i]) (void) hipEventDestroy(e[i]); } } events{ev};
        Drain drain{s};
        for (hipEvent_t &x : ev) HIP_TRY(hipEventCreate(&x));
        HIP_TRY(d_chunks.upload(hc, s));
        HIP_TRY(d_l.alloc((size_t) n_total));
        HIP_TRY(d_h.alloc((size_t) n_total));
        HIP_TRY(d_status.alloc((size_t) n_total));
        HIP_TRY(d_keep.alloc((size_t) n_total));
        HIP_TRY(d_prob.alloc((size_t) n_total));
        HIP_TRY(d_flag.alloc((size_t) n_chunks));
        if (n_total > 0) {
            HIP_TRY(hipMemcpyAsync(d_l.p, l, 4 * (size_t) n_total, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_h.p, h, 4 * (size_t) n_total, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(d_status.p, status, (size_t) n_total, hipMemcpyHostToDevice, s));
            /* (reads between two chunks' ranges belong to nobody: they come back as 0) */
            HIP_TRY(hipMemsetAsync(d_keep.p, 0, (size_t) n_total, s));
            HIP_TRY(hipMemsetAsync(d_prob.p, 0, 8 * (size_t) n_total, s));
        }
        HIP_TRY(hipEventRecord(ev[0], s));
        HIP_TRY(mrp_downsample_launch(s, n_chunks, d_chunks.p, MrpDsIn{d_l.p, d_h.p, nullptr, nullptr, 0}, d_status.p, max_depth, seed, d_prob.p, d_keep.p, d_flag.p));
        HIP_TRY(hipEventRecord(ev[1], s));
        if (n_total > 0) {
            HIP_TRY(hipMemcpyAsync(back_keep.data(), d_keep.p, (size_t) n_total, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(back_prob.data(), d_prob.p, 8 * (size_t) n_total, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipMemcpyAsync(flag.data(), d_flag.p, 4 * (size_t) n_chunks, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
    }
    ctx->pool.reclaim();
    mrp_downsampling_stats &st = ctx->last_downsampling;
    st.chunks = n_chunks;
    for (int64_t c = 0; c < n_chunks; c++) {
        st.chunks_downsampled += flag[(size_t) c] != 0;
        for (int64_t r = first[c]; r < first[c] + n_reads[c]; r++) st.reads_discarded += status[r] == MRP_READ_KEPT && !back_keep[(size_t) r];
    }
    st.bytes_downloaded = 9 * n_total + 4 * n_chunks;
    st.downsample_ms = ms;
    if (n_total > 0) {
        memcpy(keep_out, back_keep.data(), (size_t) n_total);
        if (prob_out) memcpy(prob_out, back_prob.data(), 8 * (size_t) n_total);
    }
    if (stats) *stats = st;
    return MRP_OK;
}
