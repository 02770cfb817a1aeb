/*
 * mrp_repeat_counts.hip -- the ML repeat counts of a run-length consensus from the posterior matches:
 * poa_estimateRepeatCountsUsingBayesianModel / poa_estimatePhasedRepeatCountsUsingBayesianModel (impl/poa.c:1715-1756) over
 * repeatSubMatrix_getMLRepeatCount / _getPhasedMLRepeatCount (impl/repeatSubMatrix.c:65-238), and mrp_rle_expand (rleString_expand,
 * impl/rle.c:145-155).  The host checks, uploads the raw lists once and downloads the outputs; two stages run on the device:
 *
 *   regroup   rc_count_kernel    a lane per match: the node's counter, an integer atomic
 *             rc_scan_kernel     one workgroup: every node's range in the record array
 *             rc_claim_kernel    a lane per match: claims a slot of its node's range in whatever order the atomics land and writes the
 *                                record with its sequence number (read-major, walk order)
 *             rc_order_kernel    a wave per node: the rank of every record among its node's by sequence number, all pairs over an LDS
 *                                tile, and the record stored at its rank -- the definition's order, whatever the claim did
 *   estimate  rc_estimate_kernel a wave per node: min and max by wave reductions, a lane per candidate u (rounds of 64), the records
 *                                walked in order through an LDS tile (same-address reads), one accumulator unphased and two phased,
 *                                the reference's scan over the candidates by one lane
 *             rc_sums_kernel     a workgroup per consensus: nonRleLength and the stats' integer sums
 *
 * Compiled with -ffp-contract=off: the sum is a multiply and an add, two IEEE operations, as in the reference's build.  gfx950 only.
 */
#include "mrp_repeat_counts.h"

#include <chrono>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int RC_NT = 256;   /* the lane-per-match kernels and the sums */
constexpr int RC_WAVE = 64;  /* the wave-per-node kernels: one wave per workgroup, so a workgroup barrier is a wave's */
constexpr int RC_SCAN_NT = 1024;

double rc_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

/* the read of match i: the last r with first[r] <= i (reads without matches share their first with the next) */
__device__ inline int rc_read_of(const int64_t *__restrict__ first, int n_reads, int64_t i) {
    int lo = 0, hi = n_reads;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(RC_NT) rc_count_kernel(int64_t n_matches, int n_reads, const int64_t *__restrict__ first, const RcRead *__restrict__ reads,
                                                         const int32_t *__restrict__ x, uint32_t *__restrict__ cnt) {
    const int64_t i = (int64_t) blockIdx.x * RC_NT + threadIdx.x;
    if (i >= n_matches) return;
    const int r = rc_read_of(first, n_reads, i);
    atomicAdd(&cnt[reads[r].node_base + x[i]], 1u);
}

/* off[k] = the sum of cnt[0 .. k), off[n] the total.  One workgroup: a thread sums a stretch, the stretches' sums are scanned in LDS,
 * the thread writes its stretch. */
__global__ void __launch_bounds__(RC_SCAN_NT) rc_scan_kernel(int64_t n, const uint32_t *__restrict__ cnt, uint32_t *__restrict__ off) {
    __shared__ uint32_t s_sum[RC_SCAN_NT];
    const int tid = threadIdx.x;
    const int64_t stretch = (n + RC_SCAN_NT - 1) / RC_SCAN_NT;
    const int64_t lo = (int64_t) tid * stretch < n ? (int64_t) tid * stretch : n, hi = lo + stretch < n ? lo + stretch : n;
    uint32_t mine = 0;
    for (int64_t k = lo; k < hi; k++) mine += cnt[k];
    s_sum[tid] = mine;
    __syncthreads();
    for (int d = 1; d < RC_SCAN_NT; d <<= 1) {
        const uint32_t v = tid >= d ? s_sum[tid - d] : 0u;
        __syncthreads();
        s_sum[tid] += v;
        __syncthreads();
    }
    uint32_t at = s_sum[tid] - mine;
    for (int64_t k = lo; k < hi; k++) {
        off[k] = at;
        at += cnt[k];
    }
    if (tid == RC_SCAN_NT - 1) off[n] = s_sum[tid];
}

/* cnt counts down to 0 here: the slot a match gets depends on the order of the atomics, its record does not */
__global__ void __launch_bounds__(RC_NT) rc_claim_kernel(int64_t n_matches, int n_reads, const int64_t *__restrict__ first, const RcRead *__restrict__ reads,
                                                         const int32_t *__restrict__ x, const int32_t *__restrict__ y, const int32_t *__restrict__ weight,
                                                         const uint8_t *__restrict__ counts, int R, int backwards, const uint32_t *__restrict__ off,
                                                         uint32_t *__restrict__ cnt, RcRecord *__restrict__ rec) {
    const int64_t i = (int64_t) blockIdx.x * RC_NT + threadIdx.x;
    if (i >= n_matches) return;
    const int r = rc_read_of(first, n_reads, i);
    const RcRead rd = reads[r];
    const int64_t node = rd.node_base + x[i];
    const uint32_t c = counts[rd.y_off + y[i]];
    const uint32_t slot = off[node] + (atomicSub(&cnt[node], 1u) - 1u);
    RcRecord o;
    o.weight = (double) weight[i];
    o.seq = (uint32_t) rc_sequence_number(first[r], first[r + 1], i, backwards);
    o.bits = (c < (uint32_t) R ? (c | RC_BELOW_R) : (uint32_t) (R - 1)) | rd.flags;
    rec[slot] = o;
}

/* A wave per node.  The sequence numbers of a call are distinct, so the ranks of a node's n records are 0 .. n - 1, each once: every
 * slot of the node's range in `sorted` is written by exactly one lane.  n is the node's alone, so the whole wave reaches every barrier. */
__global__ void __launch_bounds__(RC_WAVE) rc_order_kernel(const uint32_t *__restrict__ off, const RcRecord *__restrict__ rec, RcRecord *__restrict__ sorted) {
    __shared__ uint32_t s_seq[RC_WAVE];
    const int lane = threadIdx.x;
    const uint32_t b = off[blockIdx.x], n = off[blockIdx.x + 1] - b;
    for (uint32_t i0 = 0; i0 < n; i0 += RC_WAVE) {
        const bool have = i0 + lane < n;
        RcRecord me{0.0, 0u, 0u};
        if (have) me = rec[b + i0 + lane];
        uint32_t rank = 0;
        for (uint32_t j0 = 0; j0 < n; j0 += RC_WAVE) {
            __syncthreads(); /* the tile before has been read */
            if (j0 + lane < n) s_seq[lane] = rec[b + j0 + lane].seq;
            __syncthreads();
            const int m = (int) min((uint32_t) RC_WAVE, n - j0);
            for (int t = 0; t < m; t++) rank += s_seq[t] < me.seq;
        }
        if (have) sorted[b + rank] = me;
    }
}

__device__ inline int rc_wave_min(int v) {
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}
__device__ inline int rc_wave_max(int v) {
    for (int d = 32; d >= 1; d >>= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

/* The reference's scan over the candidates, by one lane.  Unphased: getMax, :153-167, the first that is strictly greater.  Phased:
 * getRepeatLengthProbForHaplotype, :145-151, and the scan of :208-220, which takes the last that is not smaller. */
__device__ inline int rc_pick(const double *lp1, const double *lp2, int len, int phased, double s, double *best_out) {
    double best;
    int at = 0;
    if (!phased) {
        best = lp1[0];
        for (int i = 1; i < len; i++) {
            if (lp1[i] > best) {
                best = lp1[i];
                at = i;
            }
        }
    } else {
        double ml2 = lp2[0];
        for (int i = 1; i < len; i++)
            if (lp2[i] > ml2) ml2 = lp2[i];
        best = lp1[0] + ((lp2[0] > ml2 + s) ? lp2[0] : ml2 + s);
        for (int i = 1; i < len; i++) {
            const double p = lp1[i] + ((lp2[i] > ml2 + s) ? lp2[i] : ml2 + s);
            if (p >= best) {
                best = p;
                at = i;
            }
        }
    }
    *best_out = best;
    return at;
}

/* A wave per node over its ordered records.  tt is the transposed table: lanes with consecutive u read consecutive doubles. */
__global__ void __launch_bounds__(RC_WAVE) rc_estimate_kernel(const uint8_t *__restrict__ symbols, const uint32_t *__restrict__ off,
                                                              const RcRecord *__restrict__ rec, const double *__restrict__ tt, int R, int phased, double s,
                                                              int32_t *__restrict__ count_out, double *__restrict__ lp_out, int32_t *__restrict__ range_out) {
    __shared__ RcRecord s_rec[RC_WAVE];
    __shared__ double s_lp1[RC_MAX_R + 1], s_lp2[RC_MAX_R + 1];
    const int lane = threadIdx.x;
    const int64_t node = blockIdx.x;
    const uint32_t b = off[node], n = off[node + 1] - b;
    /* repeatSubMatrix_getMinAndMaxRepeatCountObservations, :86-113: an overlong count never lowers min and is R - 1 in max */
    int mn = R, mx = 0;
    for (uint32_t i = lane; i < n; i += RC_WAVE) {
        const uint32_t bits = rec[b + i].bits;
        const int o = (int) (bits & RC_COUNT_MASK);
        if (bits & RC_BELOW_R) mn = min(mn, o);
        mx = max(mx, o);
    }
    mn = rc_wave_min(mn);
    mx = rc_wave_max(mx);
    if (mn == R) { /* :133-136, :177-180, and the fix-up of poa.c:1721-1723 */
        if (lane == 0) {
            count_out[node] = 1;
            lp_out[node] = -INFINITY;
            range_out[node] = 0;
        }
        return;
    }
    int base = symbols[node];
    if (base > 3) base = 0; /* N as A, repeatSubMatrix.c:16-27 */
    const double *t_forward = tt + (size_t) base * R * R, *t_reverse = tt + (size_t) (3 - base) * R * R;
    for (int u0 = mn; u0 <= mx; u0 += RC_WAVE) {
        const int u = u0 + lane;
        const bool active = u <= mx;
        double lp1 = 0.0, lp2 = 0.0; /* LOG_ONE */
        for (uint32_t j0 = 0; j0 < n; j0 += RC_WAVE) {
            __syncthreads(); /* the tile before has been read */
            if (j0 + lane < n) s_rec[lane] = rec[b + j0 + lane];
            __syncthreads();
            const int m = (int) min((uint32_t) RC_WAVE, n - j0);
            if (active) {
                for (int t = 0; t < m; t++) { /* repeatSubMatrix_getLogProbForGivenRepeatCount, :70-81 */
                    const RcRecord r = s_rec[t];
                    const double *tab = (r.bits & RC_STRAND) ? t_forward : t_reverse;
                    const double term = tab[(size_t) (r.bits & RC_COUNT_MASK) * R + u] * r.weight;
                    if (!phased || (r.bits & RC_IN_HAP)) lp1 = lp1 + term;
                    else lp2 = lp2 + term;
                }
            }
        }
        if (active) {
            s_lp1[u - mn] = lp1 / RC_PAIR_ALIGNMENT_PROB_1;
            s_lp2[u - mn] = lp2 / RC_PAIR_ALIGNMENT_PROB_1;
        }
    }
    __syncthreads();
    if (lane != 0) return;
    const int len = mx - mn + 1;
    double best;
    const int at = rc_pick(s_lp1, s_lp2, len, phased, s, &best);
    const int ml = at + mn;
    count_out[node] = ml == 0 ? 1 : ml; /* poa.c:1721-1723 */
    lp_out[node] = best;
    range_out[node] = len;
}

/* per consensus: sums[3c] = nonRleLength, sums[3c + 1] = nodes with an observation, sums[3c + 2] = candidates.  Integer sums. */
__global__ void __launch_bounds__(RC_NT) rc_sums_kernel(const int64_t *__restrict__ node_first, const uint32_t *__restrict__ off,
                                                        const int32_t *__restrict__ count_out, const int32_t *__restrict__ range_out,
                                                        int64_t *__restrict__ sums) {
    __shared__ int64_t s_part[RC_NT / 64][3];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int64_t lo = node_first[blockIdx.x], hi = node_first[blockIdx.x + 1];
    int64_t v[3] = {0, 0, 0};
    for (int64_t k = lo + tid; k < hi; k += RC_NT) {
        v[0] += count_out[k];
        v[1] += off[k + 1] > off[k];
        v[2] += range_out[k];
    }
    for (int q = 0; q < 3; q++) {
        for (int d = 32; d >= 1; d >>= 1) v[q] += __shfl_xor(v[q], d, 64);
        if (lane == 0) s_part[wv][q] = v[q];
    }
    __syncthreads();
    if (tid < 3) {
        int64_t t = 0;
        for (int w = 0; w < RC_NT / 64; w++) t += s_part[w][tid];
        sums[3 * (int64_t) blockIdx.x + tid] = t;
    }
}

}  // namespace

int rc_check_and_build(const char *who, const double *log_prob, int32_t max_repeat, int64_t n_consensus, const int64_t *node_first,
                       const uint8_t *symbols, const int64_t *read_first, const uint8_t *counts, int64_t counts_bytes, const int64_t *y_off,
                       const int32_t *y_len, const uint8_t *read_forward_strand, const int32_t *x_shift, const uint8_t *read_in_hap,
                       const mrp_posterior_pairs *matches, const mrp_repeat_count_options *opt, const int32_t *repeat_count_out,
                       const int64_t *non_rle_length_out, HostVec<RcRead> &reads) {
    if (!log_prob || !node_first || !read_first || !matches || !matches->first || !opt) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (n_consensus < 0 || counts_bytes < 0) return mrp_set_error(MRP_ERR_ARG, "%s: bad sizes", who);
    if (max_repeat < 2 || max_repeat > RC_MAX_R) return mrp_set_error(MRP_ERR_ARG, "%s: max_repeat %d outside [2, %d]", who, (int) max_repeat, RC_MAX_R);
    if (opt->reserved != 0 || opt->reserved2 != 0) return mrp_set_error(MRP_ERR_ARG, "%s: reserved must be 0", who);
    if (opt->walk_backwards != 0 && opt->walk_backwards != 1) return mrp_set_error(MRP_ERR_ARG, "%s: walk_backwards must be 0 or 1", who);
    if (read_in_hap && std::isnan(opt->log_het_substitution)) return mrp_set_error(MRP_ERR_ARG, "%s: log_het_substitution is NaN", who);
    const int R = max_repeat;
    for (int64_t k = 0; k < (int64_t) 4 * R * R; k++)
        if (std::isnan(log_prob[k]) || log_prob[k] == INFINITY)
            return mrp_set_error(MRP_ERR_ARG, "%s: log_prob[%d][%d][%d] is %s", who, (int) (k / ((int64_t) R * R)), (int) (k / R % R), (int) (k % R),
                                 std::isnan(log_prob[k]) ? "NaN" : "+inf");
    if (node_first[0] != 0 || read_first[0] != 0) return mrp_set_error(MRP_ERR_ARG, "%s: node_first and read_first must begin at 0", who);
    for (int64_t c = 0; c < n_consensus; c++)
        if (node_first[c + 1] < node_first[c] || read_first[c + 1] < read_first[c])
            return mrp_set_error(MRP_ERR_ARG, "%s: consensus %lld: node_first or read_first descends", who, (long long) c);
    const int64_t n_nodes = node_first[n_consensus], n_reads = read_first[n_consensus];
    if (n_nodes >= (1ll << 31) || n_reads >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: 2^31 or more nodes or reads in one call", who);
    if (n_consensus > 0 && !non_rle_length_out) return mrp_set_error(MRP_ERR_ARG, "%s: null argument (non_rle_length_out)", who);
    if (n_nodes > 0 && (!symbols || !repeat_count_out)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument (symbols or repeat_count_out)", who);
    if (n_reads > 0 && (!y_off || !y_len || !read_forward_strand)) return mrp_set_error(MRP_ERR_ARG, "%s: null read array", who);
    for (int64_t k = 0; k < n_nodes; k++)
        if (symbols[k] > 4) return mrp_set_error(MRP_ERR_ARG, "%s: node %lld: symbol %d above 4", who, (long long) k, (int) symbols[k]);
    const int64_t *first = matches->first;
    if (first[0] != 0) return mrp_set_error(MRP_ERR_ARG, "%s: matches->first must begin at 0", who);
    for (int64_t r = 0; r < n_reads; r++)
        if (first[r + 1] < first[r]) return mrp_set_error(MRP_ERR_ARG, "%s: read %lld: matches->first descends (it holds one range per read)", who, (long long) r);
    const int64_t n_matches = first[n_reads];
    if (n_matches >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: 2^31 or more matches in one call", who);
    if (n_matches > 0 && (!matches->x || !matches->y || !matches->weight || !counts)) return mrp_set_error(MRP_ERR_ARG, "%s: null match array or counts", who);
    reads.resize((size_t) n_reads);
    for (int64_t c = 0; c < n_consensus; c++) {
        const int64_t n_lo = node_first[c], n_hi = node_first[c + 1];
        for (int64_t r = read_first[c]; r < read_first[c + 1]; r++) {
            if (y_len[r] < 0 || y_off[r] < 0 || y_off[r] > counts_bytes - y_len[r])
                return mrp_set_error(MRP_ERR_ARG, "%s: consensus %lld, read %lld: its counts lie outside the pool", who, (long long) c, (long long) r);
            const int64_t shift = x_shift ? x_shift[r] : 0;
            for (int64_t i = first[r]; i < first[r + 1]; i++) {
                const int64_t node = n_lo + shift + matches->x[i];
                if (matches->y[i] < 0 || matches->y[i] >= y_len[r])
                    return mrp_set_error(MRP_ERR_ARG, "%s: consensus %lld, read %lld, match %lld: y %d outside the read (%d counts)", who, (long long) c,
                                         (long long) r, (long long) i, (int) matches->y[i], (int) y_len[r]);
                if (node < n_lo || node >= n_hi)
                    return mrp_set_error(MRP_ERR_ARG, "%s: consensus %lld, read %lld, match %lld: x %d + x_shift %lld outside the consensus (%lld nodes)", who,
                                         (long long) c, (long long) r, (long long) i, (int) matches->x[i], (long long) shift, (long long) (n_hi - n_lo));
                if (matches->weight[i] < 0)
                    return mrp_set_error(MRP_ERR_ARG, "%s: consensus %lld, read %lld, match %lld: negative weight %d", who, (long long) c, (long long) r,
                                         (long long) i, (int) matches->weight[i]);
            }
            reads[(size_t) r] = RcRead{n_lo + shift, y_off[r], (read_forward_strand[r] ? RC_STRAND : 0u) | (read_in_hap && read_in_hap[r] ? RC_IN_HAP : 0u), 0u};
        }
    }
    return MRP_OK;
}

extern "C" int mrp_ml_repeat_counts(mrp_context *ctx, const double *log_prob, int32_t max_repeat, int64_t n_consensus, const int64_t *node_first,
                                    const uint8_t *symbols, const int64_t *read_first, const uint8_t *counts, int64_t counts_bytes, const int64_t *y_off,
                                    const int32_t *y_len, const uint8_t *read_forward_strand, const int32_t *x_shift, const uint8_t *read_in_hap,
                                    const mrp_posterior_pairs *matches, const mrp_repeat_count_options *opt, int32_t *repeat_count_out,
                                    double *log_prob_out, int64_t *non_rle_length_out, mrp_repeat_count_stats *stats) {
    static const char *who = "mrp_ml_repeat_counts";
    const double t_begin = rc_now_ms();
    HostVec<RcRead> reads;
    const int rc = rc_check_and_build(who, log_prob, max_repeat, n_consensus, node_first, symbols, read_first, counts, counts_bytes, y_off, y_len,
                                      read_forward_strand, x_shift, read_in_hap, matches, opt, repeat_count_out, non_rle_length_out, reads);
    if (rc != MRP_OK) return rc;
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context", who);
    mrp_repeat_count_stats st;
    memset(&st, 0, sizeof(st));
    const int R = max_repeat;
    const int64_t n_nodes = node_first[n_consensus], n_reads = read_first[n_consensus], n_matches = matches->first[n_reads];
    HostVec<int32_t> back_count((size_t) n_nodes); /* (the outputs are written only on success) */
    HostVec<double> back_lp(log_prob_out ? (size_t) n_nodes : 0);
    HostVec<int64_t> back_sums((size_t) (3 * n_consensus));
    float ms[3] = {0.f, 0.f, 0.f};
    if (n_consensus > 0) {
        HIP_TRY(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        HostVec<double> tt;
        rc_transpose_table(log_prob, R, tt);
        DevBufGroup arrays;
        DevBuf<double> d_tt{arrays}, d_lp{arrays};
        DevBuf<uint8_t> d_symbols{arrays}, d_counts{arrays};
        DevBuf<int64_t> d_node_first{arrays}, d_first{arrays}, d_sums{arrays};
        DevBuf<RcRead> d_reads{arrays};
        DevBuf<int32_t> d_x{arrays}, d_y{arrays}, d_w{arrays}, d_count{arrays}, d_range{arrays};
        DevBuf<uint32_t> d_cnt{arrays}, d_off{arrays};
        DevBuf<RcRecord> d_rec{arrays}, d_sorted{arrays};
        arrays.bind(&ctx->pool);
        hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
        struct Events { hipEvent_t *e; ~Events() { for (int i = 0; i < 4; i++) if (e[i]) (void) hipEventDestroy(e[i]); } } events{ev};
        Drain drain{s};
        for (hipEvent_t &e : ev) HIP_TRY(hipEventCreate(&e));
        auto up = [&](void *dst, const void *src, size_t bytes) {
            st.bytes_uploaded += (int64_t) bytes;
            return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
        };
        HIP_TRY(hipEventRecord(ev[0], s));
        HIP_TRY(d_tt.alloc(tt.size()));
        HIP_TRY(up(d_tt.p, tt.data(), 8 * tt.size()));
        HIP_TRY(d_symbols.alloc((size_t) n_nodes));
        HIP_TRY(up(d_symbols.p, symbols, (size_t) n_nodes));
        HIP_TRY(d_counts.alloc((size_t) counts_bytes));
        HIP_TRY(up(d_counts.p, counts, n_matches > 0 ? (size_t) counts_bytes : 0));
        HIP_TRY(d_node_first.alloc((size_t) n_consensus + 1));
        HIP_TRY(up(d_node_first.p, node_first, 8 * ((size_t) n_consensus + 1)));
        HIP_TRY(d_first.alloc((size_t) n_reads + 1));
        HIP_TRY(up(d_first.p, matches->first, 8 * ((size_t) n_reads + 1)));
        HIP_TRY(d_reads.alloc((size_t) n_reads));
        HIP_TRY(up(d_reads.p, reads.data(), sizeof(RcRead) * (size_t) n_reads));
        HIP_TRY(d_x.alloc((size_t) n_matches));
        HIP_TRY(d_y.alloc((size_t) n_matches));
        HIP_TRY(d_w.alloc((size_t) n_matches));
        HIP_TRY(up(d_x.p, matches->x, 4 * (size_t) n_matches));
        HIP_TRY(up(d_y.p, matches->y, 4 * (size_t) n_matches));
        HIP_TRY(up(d_w.p, matches->weight, 4 * (size_t) n_matches));
        HIP_TRY(d_cnt.alloc((size_t) n_nodes));
        HIP_TRY(d_off.alloc((size_t) n_nodes + 1));
        HIP_TRY(d_rec.alloc((size_t) n_matches));
        HIP_TRY(d_sorted.alloc((size_t) n_matches));
        HIP_TRY(d_count.alloc((size_t) n_nodes));
        HIP_TRY(d_range.alloc((size_t) n_nodes));
        HIP_TRY(d_lp.alloc((size_t) n_nodes));
        HIP_TRY(d_sums.alloc((size_t) (3 * n_consensus)));
        HIP_TRY(hipEventRecord(ev[1], s));
        /* regroup */
        const unsigned match_blocks = (unsigned) ((n_matches + RC_NT - 1) / RC_NT);
        if (n_nodes > 0) HIP_TRY(hipMemsetAsync(d_cnt.p, 0, 4 * (size_t) n_nodes, s));
        if (n_matches > 0) {
            hipLaunchKernelGGL(rc_count_kernel, dim3(match_blocks), dim3(RC_NT), 0, s, n_matches, (int) n_reads, d_first.p, d_reads.p, d_x.p, d_cnt.p);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(rc_scan_kernel, dim3(1), dim3(RC_SCAN_NT), 0, s, n_nodes, d_cnt.p, d_off.p);
        HIP_TRY(hipGetLastError());
        if (n_matches > 0) {
            hipLaunchKernelGGL(rc_claim_kernel, dim3(match_blocks), dim3(RC_NT), 0, s, n_matches, (int) n_reads, d_first.p, d_reads.p, d_x.p, d_y.p, d_w.p,
                               d_counts.p, R, (int) opt->walk_backwards, d_off.p, d_cnt.p, d_rec.p);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(rc_order_kernel, dim3((unsigned) n_nodes), dim3(RC_WAVE), 0, s, d_off.p, d_rec.p, d_sorted.p);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(ev[2], s));
        /* estimate */
        if (n_nodes > 0) {
            hipLaunchKernelGGL(rc_estimate_kernel, dim3((unsigned) n_nodes), dim3(RC_WAVE), 0, s, d_symbols.p, d_off.p, d_sorted.p, d_tt.p, R,
                               read_in_hap ? 1 : 0, opt->log_het_substitution, d_count.p, d_lp.p, d_range.p);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(rc_sums_kernel, dim3((unsigned) n_consensus), dim3(RC_NT), 0, s, d_node_first.p, d_off.p, d_count.p, d_range.p, d_sums.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[3], s));
        if (n_nodes > 0) {
            HIP_TRY(hipMemcpyAsync(back_count.data(), d_count.p, 4 * (size_t) n_nodes, hipMemcpyDeviceToHost, s));
            if (log_prob_out) HIP_TRY(hipMemcpyAsync(back_lp.data(), d_lp.p, 8 * (size_t) n_nodes, hipMemcpyDeviceToHost, s));
        }
        HIP_TRY(hipMemcpyAsync(back_sums.data(), d_sums.p, 24 * (size_t) n_consensus, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        for (int k = 0; k < 3; k++) HIP_TRY(hipEventElapsedTime(&ms[k], ev[k], ev[k + 1]));
        st.bytes_downloaded = (log_prob_out ? 12 : 4) * n_nodes + 24 * n_consensus;
    }
    if (n_consensus > 0) ctx->pool.reclaim();
    for (int64_t c = 0; c < n_consensus; c++) {
        non_rle_length_out[c] = back_sums[(size_t) (3 * c)];
        st.nodes_observed += back_sums[(size_t) (3 * c + 1)];
        st.candidates += back_sums[(size_t) (3 * c + 2)];
    }
    if (n_nodes > 0) {
        memcpy(repeat_count_out, back_count.data(), 4 * (size_t) n_nodes);
        if (log_prob_out) memcpy(log_prob_out, back_lp.data(), 8 * (size_t) n_nodes);
    }
    st.observations = n_matches;
    st.upload_ms = ms[0];
    st.ordering_ms = ms[1];
    st.estimate_ms = ms[2];
    st.total_ms = rc_now_ms() - t_begin;
    if (stats) *stats = st;
    return MRP_OK;
}

extern "C" int64_t mrp_rle_expand(const uint8_t *symbols, const uint8_t *counts8, const int32_t *counts32, int64_t n, char *out, int64_t capacity) {
    if (n < 0 || (n > 0 && (!symbols || (counts8 != nullptr) == (counts32 != nullptr)))) return -1;
    int64_t len = 0;
    for (int64_t i = 0; i < n; i++) {
        if (symbols[i] > 4 || (counts32 && counts32[i] < 0)) return -1;
        len += counts8 ? (int64_t) counts8[i] : (int64_t) counts32[i];
    }
    if (!out) return len;
    if (capacity < len) return -1;
    int64_t j = 0;
    for (int64_t i = 0; i < n; i++) { /* rleString_expand, rle.c:148-152 */
        const int64_t c = counts8 ? (int64_t) counts8[i] : (int64_t) counts32[i];
        for (int64_t k = 0; k < c; k++) out[j++] = "ACGTN"[symbols[i]];
    }
    return len;
}
