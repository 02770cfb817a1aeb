/*
 * mrp_anchors.hip -- getKmerAlignmentAnchors (impl/pairwiseAligner.c:1519-1627, KMER_SIZE 20) for any number of (x, y) string pairs
 * over a symbol pool that lies on the device: the k-mer chain the reference anchors long (structural variant) alleles with.  The
 * host function kmer_anchors() of mrp_pairhmm.hip (mrp_kmer_alignment_anchors) is the specification, quirks included; the public
 * entry is mrp_kmer_alignment_anchors_many, the composite mrp_phase_aligned_chunks (mrp_aligned.hip) calls mrp_kmer_anchors_on_device.  gfx950 only.
 *
 * ak_chain_kernel, a wave per pair (the waves stride over the pairs; no wave waits for another):
 *   search   a lane per y position, 64 at a time: the first x whose 20 symbols equal the y k-mer (getKmers :1543-1555 keeps the first
 *            occurrence).  The 20 bytes of the x window are the same for every lane, so the window is rolled a byte at a time in
 *            uniform registers and each lane compares it with the 20 bytes of its own k-mer held in five dwords: lx - 19 steps of
 *            one uniform byte load and five compares for 64 y positions -- the O(lx ly / 64) part.
 *   chain    the matches of the 64 positions are compacted in y order (ballot + popcount) and chained one after the other (:1580-1600):
 *            record i looks back over the records before it for those with a smaller x; the walk stops behind the first of them that
 *            was a running maximum (:1592).  The last 64 records live one per lane in registers (record j in lane j mod 64), so the walk
 *            is a ballot (where it stops), a wave maximum (the best score inside the stop) and a second ballot (the nearest record
 *            with that score: the walk updates on > only); only a walk that finds no stop among 64 records goes on over the records
 *            in the global workspace, 64 at a time.
 *   The score of the last running maximum is the length of its chain (score = 1 + the score of the record it points back to), so the
 *   count of a pair is known without a walk.
 * ak_trace_kernel, a lane per pair, twice: the trace back from the last maximum (:1605-1617), which first counts and then writes the
 * chain as diagonal runs -- (x + 10, y + 10, length) for anchors that follow each other by (+1, +1), which is how shared stretches of
 * two strings show up -- at the pair's offset (the scan of the run counts, made on the host between the two passes).  An SV pair has
 * an anchor per shared 20-mer, 16 B each as (x, y), many times the symbols of its strings; as runs the anchors of a call are a
 * fraction of them.  The host expands the runs.
 *
 * Every loop is bounded by lx, ly or the record count.  Workspace: 16 B per y position with a k-mer, i.e. sum(ly - 19).
 */
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstring>
#include <vector>

#include "../../include/margin_rphmm.h"
#include "mrp_internal.h"
#include "mrp_wave.h"

namespace {

constexpr int AK_WAVE = 64;
constexpr int AK_K = 20; /* KMER_SIZE, pairwiseAligner.c:1519 */

struct AkPair {
    int64_t x_off, y_off;
    int64_t rec_off; /* the pair's records in the workspace arrays */
    int32_t lx, ly;
};

static __device__ __forceinline__ uint32_t ak_dword(const uint8_t *p) {
    return (uint32_t) p[0] | (uint32_t) p[1] << 8 | (uint32_t) p[2] << 16 | (uint32_t) p[3] << 24;
}
/* the lanes' ballot with bit d = the lane at distance d behind lane r (lane (r - d) mod 64) */
static __device__ __forceinline__ uint64_t ak_by_distance(uint64_t ballot, int r) {
    const uint64_t rev = __brevll(ballot);
    const int sh = (63 - r) & 63;
    return sh ? (rev >> sh | rev << (64 - sh)) : rev;
}

__global__ void __launch_bounds__(AK_WAVE) ak_chain_kernel(const AkPair *__restrict__ pairs, int64_t n_pairs, const uint8_t *__restrict__ pool,
                                                           int32_t *rec_x, int32_t *rec_y, int32_t *rec_score, int32_t *rec_back,
                                                           int32_t *__restrict__ count, int32_t *__restrict__ last) {
    __shared__ int32_t found_x[AK_WAVE];
    const int lane = (int) threadIdx.x;
    for (int64_t pi = blockIdx.x; pi < n_pairs; pi += gridDim.x) {
        const AkPair p = pairs[pi];
        if (p.lx < AK_K || p.ly < AK_K) { /* :1567 */
            if (lane == 0) { count[pi] = 0; last[pi] = -1; }
            continue;
        }
        const uint8_t *__restrict__ sx = pool + p.x_off;
        const uint8_t *__restrict__ sy = pool + p.y_off;
        const int nx = p.lx - AK_K + 1, ny = p.ly - AK_K + 1;
        int32_t *rx = rec_x + p.rec_off, *ry = rec_y + p.rec_off, *rs = rec_score + p.rec_off, *rb = rec_back + p.rec_off;
        int n = 0, max_score = 0, max_rec = -1; /* the same in every lane */
        int ring_x = 0, ring_s = 0;             /* the lane's record of the last 64: x, score * 2 + (was a running maximum) */
        for (int yb = 0; yb < ny; yb += AK_WAVE) {
            const int y = yb + lane;
            const bool have = y < ny;
            uint32_t k0 = 0, k1 = 0, k2 = 0, k3 = 0, k4 = 0;
            if (have) {
                const uint8_t *q = sy + y;
                k0 = ak_dword(q); k1 = ak_dword(q + 4); k2 = ak_dword(q + 8); k3 = ak_dword(q + 12); k4 = ak_dword(q + 16);
            }
            /* the x window, rolled a byte at a time: the same in every lane */
            uint32_t w0 = ak_dword(sx), w1 = ak_dword(sx + 4), w2 = ak_dword(sx + 8), w3 = ak_dword(sx + 12), w4 = ak_dword(sx + 16);
            int m = -1;
            for (int x = 0; x < nx; x++) {
                const bool eq = w0 == k0 && w1 == k1 && w2 == k2 && w3 == k3 && w4 == k4;
                if (have && m < 0 && eq) m = x;
                if (__ballot(have && m < 0) == 0) break;
                if (x + 1 < nx) {
                    const uint32_t in = sx[x + AK_K];
                    w0 = w0 >> 8 | w1 << 24; w1 = w1 >> 8 | w2 << 24; w2 = w2 >> 8 | w3 << 24; w3 = w3 >> 8 | w4 << 24; w4 = w4 >> 8 | in << 24;
                }
            }
            const uint64_t found = __ballot(m >= 0);
            const int cnt = __popcll(found);
            if (cnt == 0) continue;
            const int rank = __popcll(found & ((1ull << lane) - 1ull));
            if (m >= 0) {
                found_x[rank] = m;
                rx[n + rank] = m;
                ry[n + rank] = y;
            }
            __syncthreads();
            const int cx = lane < cnt ? found_x[lane] : 0;
            __syncthreads(); /* found_x is rewritten in the next pass */
            for (int t = 0; t < cnt; t++) {
                const int i = n + t;
                const int xi = __shfl(cx, t, AK_WAVE);
                int score = 1, back = -1;
                /* the records i - 1 .. i - 64 in the lanes' registers: lane (i - 1 - d) mod 64 holds the one at distance d */
                const int r = (i - 1) & 63;
                const int d = (r - lane) & 63;
                const bool chainable = i - 1 - d >= 0 && ring_x < xi;
                const uint64_t stops = ak_by_distance(__ballot(chainable && (ring_s & 1)), r);
                const int d_stop = stops ? (int) __builtin_ctzll(stops) : 64;
                const bool in_walk = chainable && d <= d_stop;
                const int best = wave_max_i32(in_walk ? ring_s >> 1 : -1);
                if (best >= 0) {
                    const uint64_t who = ak_by_distance(__ballot(in_walk && (ring_s >> 1) == best), r);
                    score = best + 1;
                    back = i - 1 - (int) __builtin_ctzll(who);
                }
                if (d_stop == 64 && i > 64) {
                    /* no stop among the last 64: on over the older records where the kernel wrote them */
                    __syncthreads();
                    bool stopped = false;
                    for (int top = i - 65; top >= 0 && !stopped; top -= AK_WAVE) {
                        const int j = top - lane;
                        int gx = 0, gs = 0;
                        if (j >= 0) { gx = rx[j]; gs = rs[j]; }
                        const bool ch = j >= 0 && gx < xi;
                        const uint64_t st = __ballot(ch && (gs & 1));
                        const int l_stop = st ? (int) __builtin_ctzll(st) : 64;
                        const bool in = ch && lane <= l_stop;
                        const int b = wave_max_i32(in ? gs >> 1 : -1);
                        if (b >= 0 && b + 1 > score) {
                            score = b + 1;
                            back = top - (int) __builtin_ctzll(__ballot(in && (gs >> 1) == b));
                        }
                        stopped = st != 0;
                    }
                }
                const bool high = score >= max_score; /* :1596: the last of equal scores wins */
                if (high) { max_score = score; max_rec = i; }
                const int packed = score * 2 + (high ? 1 : 0);
                if (lane == 0) { rs[i] = packed; rb[i] = back; }
                if (lane == (i & 63)) { ring_x = xi; ring_s = packed; }
            }
            n += cnt;
        }
        if (lane == 0) { count[pi] = max_score; last[pi] = max_rec; }
    }
}

struct AkRun {
    int32_t x, y, n; /* anchors (x + t, y + t), t < n */
};

/* WRITE false: n_runs[pi] = the diagonal runs of the pair's chain; true: the runs themselves at run_off[pi], ascending */
template <bool WRITE>
__global__ void __launch_bounds__(256) ak_trace_kernel(const AkPair *__restrict__ pairs, int64_t n_pairs, const int32_t *__restrict__ rec_x,
                                                       const int32_t *__restrict__ rec_y, const int32_t *__restrict__ rec_back,
                                                       const int32_t *__restrict__ count, const int32_t *__restrict__ last, int32_t *n_runs,
                                                       const int64_t *__restrict__ run_off, AkRun *__restrict__ runs) {
    const int64_t pi = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (pi >= n_pairs) return;
    const int64_t ro = pairs[pi].rec_off;
    const int32_t n = count[pi];
    int32_t q = last[pi];
    if (n == 0 || q < 0) {
        if (!WRITE) n_runs[pi] = 0;
        return;
    }
    AkRun *out = WRITE ? runs + run_off[pi] : nullptr;
    int32_t r = WRITE ? n_runs[pi] - 1 : 0; /* writing: the run being walked, from the last one down; counting: the breaks so far */
    int32_t x = rec_x[ro + q], y = rec_y[ro + q], len = 1;
    for (int32_t k = 1; k < n; k++) { /* the chain has n records (n = the score of the last maximum) */
        q = rec_back[ro + q];
        if (q < 0) break;
        const int32_t bx = rec_x[ro + q], by = rec_y[ro + q];
        if (bx + 1 == x && by + 1 == y) {
            len++;
        } else {
            if (WRITE) {
                if (r >= 0) out[r] = AkRun{x + AK_K / 2, y + AK_K / 2, len};
                r--;
            } else {
                r++;
            }
            len = 1;
        }
        x = bx;
        y = by;
    }
    if (WRITE) {
        if (r >= 0) out[r] = AkRun{x + AK_K / 2, y + AK_K / 2, len};
    } else {
        n_runs[pi] = r + 1;
    }
}

double ak_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

struct AkEvents {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    ~AkEvents() {
        for (hipEvent_t x : ev)
            if (x) (void) hipEventDestroy(x);
    }
};

}  // namespace

int mrp_kmer_anchors_on_device(mrp_context *ctx, const char *who, const uint8_t *device_pool, int64_t n_pairs, const int64_t *x_off,
                               const int32_t *x_len, const int64_t *y_off, const int32_t *y_len, int64_t *anchor_off, std::vector<int64_t> &anchors,
                               double *kernel_ms, int64_t *bytes_downloaded, int64_t *n_runs_out) {
    anchor_off[0] = 0;
    if (n_runs_out) *n_runs_out = 0;
    anchors.clear();
    if (kernel_ms) *kernel_ms = 0;
    if (bytes_downloaded) *bytes_downloaded = 0;
    if (n_pairs == 0) return MRP_OK;
    if (n_pairs >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 pairs to anchor in one call", who);
    HostVec<AkPair> hp((size_t) n_pairs);
    int64_t n_rec = 0;
    for (int64_t i = 0; i < n_pairs; i++) {
        if (x_len[i] >= (1 << 30) || y_len[i] >= (1 << 30)) return mrp_set_error(MRP_ERR_ARG, "%s: strings too long", who);
        hp[(size_t) i] = AkPair{x_off[i], y_off[i], n_rec, x_len[i], y_len[i]};
        if (x_len[i] >= AK_K && y_len[i] >= AK_K) n_rec += y_len[i] - AK_K + 1;
    }
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    Drain drain{s};
    AkEvents E;
    for (hipEvent_t &x : E.ev) HIP_TRY(hipEventCreate(&x));
    DevBuf<AkPair> d_pairs;
    DevBuf<int32_t> d_rec, d_count;
    DevBuf<int64_t> d_off;
    DevBuf<AkRun> d_runs;
    d_pairs.pool = d_rec.pool = d_count.pool = d_off.pool = d_runs.pool = &ctx->pool;
    HIP_TRY(d_pairs.upload(hp, s));
    HIP_TRY(d_rec.alloc(4 * (size_t) n_rec));
    HIP_TRY(d_count.alloc(3 * (size_t) n_pairs));
    int32_t *d_last = d_count.p + n_pairs, *d_nruns = d_last + n_pairs;
    int32_t *rx = d_rec.p, *ry = rx + n_rec, *rs = ry + n_rec, *rb = rs + n_rec;
    const dim3 trace_grid((unsigned) ((n_pairs + 255) / 256));
    HIP_TRY(hipEventRecord(E.ev[0], s));
    hipLaunchKernelGGL(ak_chain_kernel, dim3((unsigned) std::min<int64_t>(n_pairs, 65536)), dim3(AK_WAVE), 0, s, d_pairs.p, n_pairs, device_pool, rx, ry, rs, rb,
                       d_count.p, d_last);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(ak_trace_kernel<false>, trace_grid, dim3(256), 0, s, d_pairs.p, n_pairs, rx, ry, rb, d_count.p, d_last, d_nruns, (const int64_t *) nullptr,
                       (AkRun *) nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(E.ev[1], s));
    HostVec<int32_t> n_runs((size_t) n_pairs);
    HIP_TRY(hipMemcpyAsync(n_runs.data(), d_nruns, sizeof(int32_t) * (size_t) n_pairs, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    HostVec<int64_t> run_off((size_t) n_pairs + 1);
    run_off[0] = 0;
    for (int64_t i = 0; i < n_pairs; i++) run_off[(size_t) i + 1] = run_off[(size_t) i] + n_runs[(size_t) i];
    const int64_t total_runs = run_off[(size_t) n_pairs];
    float a = 0.f, b = 0.f;
    HostVec<AkRun> runs((size_t) total_runs);
    if (total_runs > 0) {
        HIP_TRY(d_off.upload(run_off, s));
        HIP_TRY(d_runs.alloc((size_t) total_runs));
        HIP_TRY(hipEventRecord(E.ev[2], s));
        hipLaunchKernelGGL(ak_trace_kernel<true>, trace_grid, dim3(256), 0, s, d_pairs.p, n_pairs, rx, ry, rb, d_count.p, d_last, d_nruns, d_off.p, d_runs.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(E.ev[3], s));
        HIP_TRY(hipMemcpyAsync(runs.data(), d_runs.p, sizeof(AkRun) * (size_t) total_runs, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipEventElapsedTime(&b, E.ev[2], E.ev[3]));
    }
    HIP_TRY(hipEventElapsedTime(&a, E.ev[0], E.ev[1]));
    /* the runs as the anchors they stand for */
    for (int64_t i = 0; i < n_pairs; i++) {
        int64_t n = 0;
        for (int64_t q = run_off[(size_t) i]; q < run_off[(size_t) i + 1]; q++) {
            const AkRun &R = runs[(size_t) q];
            for (int32_t t = 0; t < R.n; t++) { anchors.push_back((int64_t) R.x + t); anchors.push_back((int64_t) R.y + t); }
            n += R.n;
        }
        anchor_off[i + 1] = anchor_off[i] + n;
    }
    if (n_runs_out) *n_runs_out = total_runs;
    if (kernel_ms) *kernel_ms = (double) a + (double) b;
    if (bytes_downloaded) *bytes_downloaded = 4 * n_pairs + (int64_t) sizeof(AkRun) * total_runs;
    return MRP_OK;
}

extern "C" int mrp_kmer_alignment_anchors_many(mrp_context *ctx, int64_t n_pairs, const uint8_t *pool, int64_t pool_bytes, const int64_t *x_off,
                                               const int32_t *x_len, const int64_t *y_off, const int32_t *y_len, int64_t *anchor_off_out,
                                               int64_t **anchors_out, mrp_pairhmm_stats *stats) {
    static const char *who = "mrp_kmer_alignment_anchors_many";
    const double t_begin = ak_now_ms();
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_pairs < 0 || pool_bytes < 0 || !anchor_off_out || !anchors_out || (pool_bytes > 0 && !pool)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (n_pairs > 0 && (!x_off || !x_len || !y_off || !y_len)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    for (int64_t i = 0; i < n_pairs; i++)
        if (x_len[i] < 0 || y_len[i] < 0 || x_off[i] < 0 || y_off[i] < 0 || x_off[i] + x_len[i] > pool_bytes || y_off[i] + y_len[i] > pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "%s: pair %lld lies outside the symbol pool", who, (long long) i);
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the device path has no CPU fallback; mrp_kmer_alignment_anchors is the host function)", who);
    std::vector<int64_t> off((size_t) n_pairs + 1, 0), anchors;
    double kernel_ms = 0;
    {
        HIP_TRY(hipSetDevice(ctx->device));
        DevBuf<uint8_t> d_pool;
        d_pool.pool = &ctx->pool;
        Drain drain{ctx->stream};
        HIP_TRY(d_pool.alloc((size_t) pool_bytes));
        if (pool_bytes) HIP_TRY(hipMemcpyAsync(d_pool.p, pool, (size_t) pool_bytes, hipMemcpyHostToDevice, ctx->stream));
        const int rc = mrp_kmer_anchors_on_device(ctx, who, d_pool.p, n_pairs, x_off, x_len, y_off, y_len, off.data(), anchors, &kernel_ms, nullptr, nullptr);
        if (rc != MRP_OK) return rc;
    }
    ctx->pool.reclaim();
    int64_t *res = (int64_t *) malloc(std::max<size_t>(anchors.size() * sizeof(int64_t), 8));
    if (!res) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    if (!anchors.empty()) memcpy(res, anchors.data(), anchors.size() * sizeof(int64_t));
    memcpy(anchor_off_out, off.data(), sizeof(int64_t) * ((size_t) n_pairs + 1));
    *anchors_out = res;
    if (stats) {
        stats->kernel_ms = kernel_ms;
        stats->total_ms = ak_now_ms() - t_begin;
    }
    return MRP_OK;
}
