/*
 * mrp_poa.hip -- the POA weights, inserts and deletes of run-length consensus strings from their reads' three posterior lists (DESIGN.md
 * section 9.19): poa_augment (impl/poa.c:317-543) over every read, getMaxWeight (:1335-1348) per node and the totals of :794-839.  The host
 * checks, sizes the tables, uploads the raw lists once and downloads the outputs; the stages on the device:
 *
 *   sets       po_sets_kernel       a lane per entry of a list: its key into the read's open-addressing table (a 64-bit compare-and-swap);
 *                                   a key met twice raises a flag
 *              po_match_kernel      a lane per match: int64 atomic adds to the node's base slot and repeat-count slot
 *   enumerate  po_enumerate_kernel  a lane per gap entry, the start k of candidate complete indels: the left flank, the walk along the
 *                                   run through the gap table with the running minimum, an emission where the right flank holds.
 *                                   Run twice: <false> counts records and string symbols, <true> claims slots and writes the records
 *                                   (shift, common suffix, rotation with end merging) and counts per node
 *   group      po_scan_kernel       one workgroup: every node's range
 *              po_scatter_kernel    a lane per record: into its node's range, in whatever order the atomics land
 *              po_leader_kernel     a lane per record: over its node's range, whether an equal record has a smaller key (then it is not
 *                                   the leader); the leader sums its group's weights per strand and its observations
 *              po_place_kernel      a lane per leader: its rank among the node's leaders by key is its place in the node's list
 *              po_pool_kernel       a lane per distinct insert: its string from the scratch pool to its place in the output pool
 *   picks      po_picks_kernel      a lane per node: the doubles and the two getMaxWeight
 *              po_node_totals_kernel a workgroup per consensus: the reference match weight and the disagreement, summed without atomics
 *              po_totals_kernel     a lane per total: the bound and the double
 *
 * A lane per record, not section 9.18's wave per node over an LDS tile: a node of a polish chunk holds a handful of records, so a wave per
 * node would idle nearly all of its lanes; the record loop reads a range that its neighbours read too (L2 hits), needs no LDS and no barrier,
 * and the ranks are by key, so the result does not depend on the order of any atomic.
 *
 * Vector integer atomics and plain stores only.  The one floating-point operation besides int64 -> double is getMaxWeight's
 * weights[ref] * penalty >= max: compiled with -ffp-contract=off.  gfx950 only.
 */
#include "mrp_poa.h"

#include <chrono>
#include <cmath>

#pragma clang fp contract(off)

namespace {

constexpr int PO_NT = 256;
constexpr int PO_SCAN_NT = 1024;

double po_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

/* the read of entry i: the last r with first[r] <= i (reads without entries share their first with the next) */
__device__ inline int po_read_of(const int64_t *__restrict__ first, int n_reads, int64_t i) {
    int lo = 0, hi = n_reads;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

/* the slot of key in the read's table of a list, or -1.  The table has at least twice as many slots as keys: the walk ends. */
__device__ inline int64_t po_find(const unsigned long long *__restrict__ keys, const PoaRead &rd, int list, uint64_t key) {
    const int lg = rd.lg[list];
    if (lg < 0) return -1;
    const uint64_t mask = (1ull << lg) - 1;
    uint64_t slot = poa_slot(key, lg);
    for (;;) {
        const uint64_t k = keys[rd.table[list] + (int64_t) slot];
        if (k == key) return rd.table[list] + (int64_t) slot;
        if (k == 0) return -1;
        slot = (slot + 1) & mask;
    }
}

__global__ void __launch_bounds__(PO_NT) po_sets_kernel(int list, int64_t n, int n_reads, const int64_t *__restrict__ first, const PoaRead *__restrict__ reads,
                                                        const int32_t *__restrict__ x, const int32_t *__restrict__ y, unsigned long long *__restrict__ keys,
                                                        int32_t *__restrict__ vals, uint32_t *__restrict__ flags) {
    const int64_t i = (int64_t) blockIdx.x * PO_NT + threadIdx.x;
    if (i >= n) return;
    const PoaRead rd = reads[po_read_of(first, n_reads, i)];
    const uint64_t key = poa_key((int64_t) x[i] + rd.shift, y[i]);
    const int lg = rd.lg[list];
    const uint64_t mask = (1ull << lg) - 1;
    uint64_t slot = poa_slot(key, lg);
    for (;;) {
        const unsigned long long old = atomicCAS(&keys[rd.table[list] + (int64_t) slot], 0ull, (unsigned long long) key);
        if (old == 0ull) {
            vals[rd.table[list] + (int64_t) slot] = (int32_t) i;
            return;
        }
        if (old == key) {
            atomicOr(flags, POA_FLAG_DUPLICATE << list);
            return;
        }
        slot = (slot + 1) & mask;
    }
}

/* poa.c:324-340 */
__global__ void __launch_bounds__(PO_NT) po_match_kernel(int64_t n, int n_reads, const int64_t *__restrict__ first, const PoaRead *__restrict__ reads,
                                                         const int32_t *__restrict__ x, const int32_t *__restrict__ y, const int32_t *__restrict__ w,
                                                         const uint8_t *__restrict__ read_s, const uint8_t *__restrict__ read_c, int R,
                                                         unsigned long long *__restrict__ base_w, unsigned long long *__restrict__ count_w) {
    const int64_t i = (int64_t) blockIdx.x * PO_NT + threadIdx.x;
    if (i >= n) return;
    const PoaRead rd = reads[po_read_of(first, n_reads, i)];
    const int64_t node = rd.node_base + x[i] + rd.shift + 1;
    const int sym = read_s[rd.y_off + y[i]], c = read_c[rd.y_off + y[i]];
    atomicAdd(&base_w[node * 5 + sym], (unsigned long long) w[i]);
    atomicAdd(&count_w[node * R + (c < R ? c : R - 1)], (unsigned long long) w[i]);
}

__device__ inline bool po_eq(const uint8_t *sa, const uint8_t *ca, int64_t i, const uint8_t *sb, const uint8_t *cb, int64_t j, int cmp) {
    return sa[i] == sb[j] && (!cmp || ca[i] == cb[j]);
}

/* getShift (:269-298), then getMaxCommonSuffixLength (:300-315) at the shifted position.  rs / rc: the consensus' reference; s / c: the
 * n symbols of the indel.  The minimal internal repeat p: s[i] == s[i - p] for every i >= p is hasInternalRepeat's s[j] == s[j + i]. */
__device__ inline int32_t po_shift(const uint8_t *rs, const uint8_t *rc, int32_t start, const uint8_t *s, const uint8_t *c, int32_t n, int cmp, int32_t *suffix) {
    int32_t p = 1;
    for (; p < n; p++) {
        if (n % p) continue;
        bool ok = true;
        for (int32_t i = p; i < n && ok; i++) ok = po_eq(s, c, i, s, c, i - p, cmp);
        if (ok) break;
    }
    for (int32_t k = start - p; k >= 0; k -= p) {
        bool ok = true;
        for (int32_t l = 0; l < p && ok; l++) ok = po_eq(rs, rc, k + l, s, c, l, cmp);
        if (!ok) break;
        start = k;
    }
    if (n == 1 && cmp && start > 0 && rs[start - 1] == s[0]) start--; /* :292-295 */
    int32_t i = 0;
    while (start - i - 1 >= 0 && n - i - 1 >= 0 && po_eq(rs, rc, start - 1 - i, s, c, n - 1 - i, cmp)) i++;
    *suffix = i;
    return start;
}

/* counters: [0] records, [1] string symbols, [2] the longest maximal run (counting pass); cursors: the same two as 32-bit claims.
 * u is the coordinate that runs (an insert's y, a delete's x); the other one stays. */
template <bool EMIT>
__global__ void __launch_bounds__(PO_NT) po_enumerate_kernel(int kind, int64_t n, int n_reads, const int64_t *__restrict__ first, const PoaRead *__restrict__ reads,
                                                             const int32_t *__restrict__ x, const int32_t *__restrict__ y, const int32_t *__restrict__ w,
                                                             const unsigned long long *__restrict__ keys, const int32_t *__restrict__ vals,
                                                             const uint8_t *__restrict__ ref_s, const uint8_t *__restrict__ ref_c,
                                                             const uint8_t *__restrict__ read_s, const uint8_t *__restrict__ read_c, int cmp, int merge,
                                                             unsigned long long *__restrict__ counters, uint32_t *__restrict__ cursors, uint32_t rec_cap,
                                                             uint32_t str_cap, PoaRecord *__restrict__ rec, uint8_t *__restrict__ sp_s, int32_t *__restrict__ sp_c,
                                                             uint32_t *__restrict__ node_cnt, uint32_t *__restrict__ flags) {
    const int64_t i = (int64_t) blockIdx.x * PO_NT + threadIdx.x;
    if (i >= n) return;
    const int r = po_read_of(first, n_reads, i);
    const PoaRead rd = reads[r];
    const bool ins = kind == POA_INSERT;
    const int32_t xs = x[i] + rd.shift, ys = y[i];
    const int32_t u0 = ins ? ys : xs, end = ins ? rd.y_len : rd.L;
    auto gap_key = [&](int32_t u) { return ins ? poa_key(xs, u) : poa_key(u, ys); };
    /* :389-392, :487-490: the match before the first entry, or the beginning */
    const bool left = u0 - 1 <= -1 || po_find(keys, rd, POA_MATCH, ins ? poa_key(xs, u0 - 1) : poa_key(u0 - 1, ys)) >= 0;
    /* (a run at the first possible coordinate has no predecessor: its key would be 0, the empty slot's mark, which po_find must not be asked for) */
    const bool run_start = !EMIT && (u0 - 1 < 0 || po_find(keys, rd, kind, gap_key(u0 - 1)) < 0);
    if (!left && !run_start) return;
    const uint8_t *rs = ref_s + rd.ref_base, *rc = ref_c + rd.ref_base;
    int32_t wmin = INT32_MAX; /* the reference starts at UINT_MAX, above every weight */
    int64_t e = i;
    unsigned long long n_rec = 0, n_sym = 0;
    for (int32_t u = u0;; u++) {
        wmin = min(wmin, w[e]);
        /* :397-401, :495-499: the match behind the last entry, or the end of the whole read / reference */
        if (left && (u + 1 >= end || po_find(keys, rd, POA_MATCH, ins ? poa_key(xs + 1, u + 1) : poa_key(u + 1, ys + 1)) >= 0)) {
            const int32_t len = u - u0 + 1;
            if (!EMIT) {
                n_rec++;
                n_sym += ins ? (unsigned long long) len : 0ull;
            } else {
                const uint32_t at = atomicAdd(&cursors[0], 1u);
                const uint32_t sat = ins ? atomicAdd(&cursors[1], (uint32_t) len) : 0u;
                if (at >= rec_cap || (ins && (uint64_t) sat + (uint64_t) len > (uint64_t) str_cap)) {
                    atomicOr(flags, POA_FLAG_CAPACITY);
                } else {
                    PoaRecord o;
                    o.key_hi = ((uint64_t) r << 32) | (uint32_t) ((ins ? xs : ys) + 1);
                    o.key_lo = ((uint64_t) (uint32_t) u0 << 32) | (uint32_t) u;
                    o.weight = wmin;
                    o.strand_cons = ((uint32_t) rd.cons << 1) | rd.strand;
                    o.str_at = sat;
                    int32_t suffix;
                    if (ins) {
                        const uint8_t *s = read_s + rd.y_off + u0, *c = read_c + rd.y_off + u0;
                        const int32_t pos = po_shift(rs, rc, xs + 1, s, c, len, cmp, &suffix);
                        uint32_t j = 0;
                        if (suffix == 0) {
                            for (int32_t q = 0; q < len; q++) {
                                sp_s[sat + q] = s[q];
                                sp_c[sat + q] = c[q];
                            }
                            j = (uint32_t) len;
                        } else { /* rleString_rotateString, rle.c:157-176 */
                            int prev = -1;
                            for (int32_t q = 0; q < len; q++) {
                                int32_t src = q - suffix;
                                if (src < 0) src += len;
                                const int sym = s[src];
                                if (!merge || q == 0 || sym != prev) {
                                    sp_s[sat + j] = (uint8_t) sym;
                                    sp_c[sat + j] = c[src];
                                    j++;
                                } else {
                                    sp_c[sat + j - 1] += c[src];
                                }
                                prev = sym;
                            }
                        }
                        uint64_t h = 14695981039346656037ull;
                        for (uint32_t q = 0; q < j; q++) h = (h ^ ((uint64_t) sp_s[sat + q] | ((uint64_t) (uint32_t) sp_c[sat + q] << 8))) * 1099511628211ull;
                        o.hash = (uint32_t) (h ^ (h >> 32));
                        o.len = j;
                        o.node = (int32_t) (rd.node_base + pos - suffix);
                    } else {
                        const int32_t pos = po_shift(rs, rc, u0, rs + u0, rc + u0, len, cmp, &suffix);
                        o.hash = 0;
                        o.len = (uint32_t) len;
                        o.node = (int32_t) (rd.node_base + pos - suffix);
                    }
                    rec[at] = o;
                    atomicAdd(&node_cnt[o.node], 1u);
                }
            }
        }
        const int64_t slot = po_find(keys, rd, kind, gap_key(u + 1));
        if (slot < 0) {
            if (run_start) atomicMax(&counters[2], (unsigned long long) (u - u0 + 1));
            break;
        }
        e = vals[slot];
    }
    if (!EMIT) {
        if (n_rec) atomicAdd(&counters[0], n_rec);
        if (n_sym) atomicAdd(&counters[1], n_sym);
    }
}

/* off[k] = the sum of cnt[0 .. k), off[n] the total.  One workgroup: a thread sums a stretch, the stretches' sums are scanned in LDS,
 * the thread writes its stretch. */
__global__ void __launch_bounds__(PO_SCAN_NT) po_scan_kernel(int64_t n, const uint32_t *__restrict__ cnt, uint32_t *__restrict__ off) {
    __shared__ uint32_t s_sum[PO_SCAN_NT];
    const int tid = threadIdx.x;
    const int64_t stretch = (n + PO_SCAN_NT - 1) / PO_SCAN_NT;
    const int64_t lo = (int64_t) tid * stretch < n ? (int64_t) tid * stretch : n, hi = lo + stretch < n ? lo + stretch : n;
    uint32_t mine = 0;
    for (int64_t k = lo; k < hi; k++) mine += cnt[k];
    s_sum[tid] = mine;
    __syncthreads();
    for (int d = 1; d < PO_SCAN_NT; d <<= 1) {
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
    if (tid == PO_SCAN_NT - 1) off[n] = s_sum[tid];
}

/* cur starts at 0: the slot a record gets depends on the order of the atomics, nothing later does */
__global__ void __launch_bounds__(PO_NT) po_scatter_kernel(uint32_t n, const PoaRecord *__restrict__ rec, const uint32_t *__restrict__ off, uint32_t *__restrict__ cur,
                                                           PoaRecord *__restrict__ sorted) {
    const uint32_t i = blockIdx.x * PO_NT + threadIdx.x;
    if (i >= n) return;
    const PoaRecord o = rec[i];
    sorted[off[o.node] + atomicAdd(&cur[o.node], 1u)] = o;
}

__device__ inline bool po_same(const PoaRecord &a, const PoaRecord &b, int ins, const uint8_t *__restrict__ sp_s, const int32_t *__restrict__ sp_c) {
    if (a.len != b.len) return false; /* addToDeletes, :213-219 */
    if (!ins) return true;
    if (a.hash != b.hash) return false;
    for (uint32_t q = 0; q < a.len; q++) /* rleString_eq, rle.c:115-128 */
        if (sp_s[a.str_at + q] != sp_s[b.str_at + q] || sp_c[a.str_at + q] != sp_c[b.str_at + q]) return false;
    return true;
}

/* addToInserts / addToDeletes (:176-233) without their order: the leader of a group of equal records is the one with the smallest key */
__global__ void __launch_bounds__(PO_NT) po_leader_kernel(uint32_t n, int ins, const PoaRecord *__restrict__ sorted, const uint32_t *__restrict__ off,
                                                          const uint8_t *__restrict__ sp_s, const int32_t *__restrict__ sp_c, uint8_t *__restrict__ leader,
                                                          int64_t *__restrict__ sums, uint32_t *__restrict__ grp_cnt) {
    const uint32_t q = blockIdx.x * PO_NT + threadIdx.x;
    if (q >= n) return;
    const PoaRecord me = sorted[q];
    const uint32_t b = off[me.node], e = off[me.node + 1];
    int64_t wf = 0, wr = 0, obs = 0;
    bool lead = true;
    for (uint32_t t = b; t < e; t++) {
        const PoaRecord o = sorted[t];
        if (!po_same(o, me, ins, sp_s, sp_c)) continue;
        if (poa_key_less(o, me)) {
            lead = false;
            break;
        }
        if (o.strand_cons & 1u) wf += o.weight;
        else wr += o.weight;
        obs++;
    }
    leader[q] = lead ? 1 : 0;
    if (!lead) return;
    sums[3 * (int64_t) q] = wf;
    sums[3 * (int64_t) q + 1] = wr;
    sums[3 * (int64_t) q + 2] = obs;
    atomicAdd(&grp_cnt[me.node], 1u);
}

/* a total's accumulator is a pair: the sum of the terms' low 32 bits and the sum of their high parts, so that no sum of fewer than 2^31
 * terms below 2^53 can wrap */
__device__ inline void po_total_add(unsigned long long *__restrict__ acc, int64_t which, uint64_t term) {
    atomicAdd(&acc[2 * which], (unsigned long long) (term & 0xffffffffull));
    atomicAdd(&acc[2 * which + 1], (unsigned long long) (term >> 32));
}

__global__ void __launch_bounds__(PO_NT) po_place_kernel(uint32_t n, int ins, const PoaRecord *__restrict__ sorted, const uint32_t *__restrict__ off,
                                                         const uint8_t *__restrict__ leader, const int64_t *__restrict__ sums, const uint32_t *__restrict__ grp_first,
                                                         uint32_t *__restrict__ g_len, uint32_t *__restrict__ g_src, double *__restrict__ g_wf, double *__restrict__ g_wr,
                                                         int64_t *__restrict__ g_obs, unsigned long long *__restrict__ tot_acc, uint32_t *__restrict__ flags) {
    const uint32_t q = blockIdx.x * PO_NT + threadIdx.x;
    if (q >= n || !leader[q]) return;
    const PoaRecord me = sorted[q];
    const uint32_t b = off[me.node], e = off[me.node + 1];
    uint32_t rank = 0;
    for (uint32_t t = b; t < e; t++)
        if (leader[t] && poa_key_less(sorted[t], me)) rank++;
    const uint32_t g = grp_first[me.node] + rank;
    const int64_t wf = sums[3 * (int64_t) q], wr = sums[3 * (int64_t) q + 1];
    g_len[g] = me.len;
    g_src[g] = me.str_at;
    g_wf[g] = (double) wf;
    g_wr[g] = (double) wr;
    g_obs[g] = sums[3 * (int64_t) q + 2];
    /* poaInsert_getWeight(insert) * insert->length, :823, :835 */
    const uint64_t both = (uint64_t) wf + (uint64_t) wr;
    const uint64_t lo = both * (uint64_t) me.len, hi = __umul64hi(both, (uint64_t) me.len);
    if (wf >= POA_EXACT_LIMIT || wr >= POA_EXACT_LIMIT || both >= (uint64_t) POA_EXACT_LIMIT || hi != 0 || lo >= (uint64_t) POA_EXACT_LIMIT) {
        atomicOr(flags, POA_FLAG_INEXACT);
        return;
    }
    po_total_add(tot_acc, 4 * (int64_t) (me.strand_cons >> 1) + (ins ? 2 : 3), lo);
}

__global__ void __launch_bounds__(PO_NT) po_pool_kernel(uint32_t n_groups, const uint32_t *__restrict__ g_len, const uint32_t *__restrict__ g_src,
                                                        const uint32_t *__restrict__ g_off, const uint8_t *__restrict__ sp_s, const int32_t *__restrict__ sp_c,
                                                        uint8_t *__restrict__ pool_s, int32_t *__restrict__ pool_c) {
    const uint32_t g = blockIdx.x * PO_NT + threadIdx.x;
    if (g >= n_groups) return;
    const uint32_t len = g_len[g], src = g_src[g], dst = g_off[g];
    for (uint32_t q = 0; q < len; q++) {
        pool_s[dst + q] = sp_s[src + q];
        pool_c[dst + q] = sp_c[src + q];
    }
}

/* getMaxWeight, :1335-1348: the last of the largest weights beside the reference's, unless the reference's times the penalty reaches it */
__device__ inline int po_max_weight(const unsigned long long *__restrict__ wt, int n, int ref, double penalty, double *__restrict__ out, bool *inexact) {
    double max_weight = 0.0;
    int max_index = -1;
    for (int j = 0; j < n; j++) {
        const unsigned long long v = wt[j];
        if (v >= (unsigned long long) POA_EXACT_LIMIT) *inexact = true;
        const double d = (double) v;
        if (out) out[j] = d;
        if (j != ref && d >= max_weight) {
            max_weight = d;
            max_index = j;
        }
    }
    return (double) wt[ref] * penalty >= max_weight ? ref : max_index;
}

__global__ void __launch_bounds__(PO_NT) po_picks_kernel(int64_t n_nodes, int64_t n_consensus, const int64_t *__restrict__ poa_first, const uint8_t *__restrict__ ref_s,
                                                         const uint8_t *__restrict__ ref_c, int R, double penalty, const unsigned long long *__restrict__ base_w,
                                                         const unsigned long long *__restrict__ count_w, double *__restrict__ base_out, double *__restrict__ count_out,
                                                         int32_t *__restrict__ base_pick, int32_t *__restrict__ count_pick, uint32_t *__restrict__ flags) {
    const int64_t k = (int64_t) blockIdx.x * PO_NT + threadIdx.x;
    if (k >= n_nodes) return;
    const int64_t c = po_read_of(poa_first, (int) n_consensus, k); /* the consensus of node k: the last c with poa_first[c] <= k */
    const bool prefix = k == poa_first[c];
    const int sym = prefix ? 4 : ref_s[k - c - 1], cnt = prefix ? 1 : ref_c[k - c - 1]; /* :120, :123 */
    bool inexact = false;
    base_pick[k] = po_max_weight(base_w + 5 * k, 5, sym, penalty, base_out + 5 * k, &inexact);
    count_pick[k] = po_max_weight(count_w + (int64_t) R * k, R, cnt, penalty, count_out ? count_out + (int64_t) R * k : nullptr, &inexact);
    if (inexact) atomicOr(flags, POA_FLAG_INEXACT);
}

/* A workgroup per consensus: the reference match weight and the disagreement of :794-815 over its nodes, each as the pair po_total_add
 * keeps (low 32 bits, high parts), summed in registers, across the wave and across the waves through LDS; no atomics.  Nobody else writes
 * these four words. */
__global__ void __launch_bounds__(PO_NT) po_node_totals_kernel(const int64_t *__restrict__ poa_first, const uint8_t *__restrict__ ref_s,
                                                               const unsigned long long *__restrict__ base_w, unsigned long long *__restrict__ tot_acc) {
    __shared__ long long s_part[PO_NT / 64][4];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    const int64_t c = blockIdx.x, lo = poa_first[c], hi = poa_first[c + 1];
    long long v[4] = {0, 0, 0, 0};
    for (int64_t k = lo + tid; k < hi; k += PO_NT) {
        const int sym = k == lo ? 4 : ref_s[k - c - 1];
        unsigned long long others = 0;
        for (int j = 0; j < 5; j++)
            if (j != sym) others += base_w[5 * k + j];
        const unsigned long long match = base_w[5 * k + sym];
        v[0] += (long long) (match & 0xffffffffull);
        v[1] += (long long) (match >> 32);
        v[2] += (long long) (others & 0xffffffffull);
        v[3] += (long long) (others >> 32);
    }
    for (int q = 0; q < 4; q++) {
        for (int d = 32; d >= 1; d >>= 1) v[q] += __shfl_xor(v[q], d, 64);
        if (lane == 0) s_part[wv][q] = v[q];
    }
    __syncthreads();
    if (tid < 4) {
        long long t = 0;
        for (int w = 0; w < PO_NT / 64; w++) t += s_part[w][tid];
        tot_acc[8 * c + tid] = (unsigned long long) t;
    }
}

__global__ void __launch_bounds__(PO_NT) po_totals_kernel(int64_t n, const unsigned long long *__restrict__ tot_acc, double *__restrict__ totals, uint32_t *__restrict__ flags) {
    const int64_t k = (int64_t) blockIdx.x * PO_NT + threadIdx.x;
    if (k >= n) return;
    const unsigned long long lo = tot_acc[2 * k], hi = tot_acc[2 * k + 1];
    if (hi >= (1ull << 21) || (hi << 32) + lo >= (unsigned long long) POA_EXACT_LIMIT) {
        atomicOr(flags, POA_FLAG_INEXACT);
        totals[k] = 0.0;
        return;
    }
    totals[k] = (double) ((hi << 32) + lo);
}

unsigned po_blocks(int64_t n) { return (unsigned) ((n + PO_NT - 1) / PO_NT); }

int po_check_list(const char *who, const char *name, const mrp_posterior_pairs *l, int64_t n_reads) {
    if (!l->first) return mrp_set_error(MRP_ERR_ARG, "%s: %s->first is NULL", who, name);
    if (l->first[0] != 0) return mrp_set_error(MRP_ERR_ARG, "%s: %s->first must begin at 0", who, name);
    for (int64_t r = 0; r < n_reads; r++)
        if (l->first[r + 1] < l->first[r]) return mrp_set_error(MRP_ERR_ARG, "%s: read %lld: %s->first descends (it holds one range per read)", who, (long long) r, name);
    if (l->first[n_reads] >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: 2^31 or more %s in one call", who, name);
    if (l->first[n_reads] > 0 && (!l->x || !l->y || !l->weight)) return mrp_set_error(MRP_ERR_ARG, "%s: null array of %s", who, name);
    return MRP_OK;
}

template <class T>
bool po_alloc(T *&p, int64_t n) {
    p = (T *) malloc((size_t) (n > 0 ? n : 1) * sizeof(T));
    return p != nullptr;
}

}  // namespace

int poa_check_and_build(const char *who, int32_t max_repeat, int64_t n_consensus, const int64_t *node_first, const uint8_t *symbols,
                        const uint8_t *ref_counts, const int64_t *read_first, const uint8_t *read_symbols, const uint8_t *read_counts,
                        int64_t pool_bytes, const int64_t *y_off, const int32_t *y_len, const uint8_t *read_forward_strand, const int32_t *x_shift,
                        const mrp_posterior_pairs *matches, const mrp_posterior_pairs *deletes, const mrp_posterior_pairs *inserts,
                        const mrp_poa_options *opt, const mrp_poa *out, HostVec<PoaRead> &reads, int64_t *table_slots) {
    if (!node_first || !read_first || !matches || !deletes || !inserts || !opt || !out) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    if (n_consensus < 0 || pool_bytes < 0) return mrp_set_error(MRP_ERR_ARG, "%s: bad sizes", who);
    if (max_repeat < 2 || max_repeat > POA_MAX_R) return mrp_set_error(MRP_ERR_ARG, "%s: max_repeat %d outside [2, %d]", who, (int) max_repeat, POA_MAX_R);
    if ((opt->compare_repeat_counts | 1) != 1 || (opt->merge_ends | 1) != 1 || (opt->want_repeat_count_weight | 1) != 1)
        return mrp_set_error(MRP_ERR_ARG, "%s: compare_repeat_counts, merge_ends and want_repeat_count_weight must be 0 or 1", who);
    if (std::isnan(opt->reference_base_penalty) || opt->reference_base_penalty < 0.0)
        return mrp_set_error(MRP_ERR_ARG, "%s: reference_base_penalty is NaN or negative", who);
    if (opt->reserved != 0 || opt->reserved2 != 0) return mrp_set_error(MRP_ERR_ARG, "%s: reserved must be 0", who);
    if (node_first[0] != 0 || read_first[0] != 0) return mrp_set_error(MRP_ERR_ARG, "%s: node_first and read_first must begin at 0", who);
    for (int64_t c = 0; c < n_consensus; c++)
        if (node_first[c + 1] < node_first[c] || read_first[c + 1] < read_first[c])
            return mrp_set_error(MRP_ERR_ARG, "%s: consensus %lld: node_first or read_first descends", who, (long long) c);
    const int64_t n_ref = node_first[n_consensus], n_reads = read_first[n_consensus];
    if (n_ref + n_consensus >= (1ll << 31) || n_reads >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: 2^31 or more nodes or reads in one call", who);
    if (n_ref > 0 && (!symbols || !ref_counts)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument (symbols or ref_counts)", who);
    if (n_reads > 0 && (!y_off || !y_len || !read_forward_strand)) return mrp_set_error(MRP_ERR_ARG, "%s: null read array", who);
    const int R = max_repeat;
    for (int64_t k = 0; k < n_ref; k++)
        if (symbols[k] > 4) return mrp_set_error(MRP_ERR_ARG, "%s: reference position %lld: symbol %d above 4", who, (long long) k, (int) symbols[k]);
    for (int64_t k = 0; k < n_ref; k++)
        if (ref_counts[k] == 0 || ref_counts[k] >= R)
            return mrp_set_error(MRP_ERR_ARG, "%s: reference position %lld: count %d outside [1, %d]", who, (long long) k, (int) ref_counts[k], R - 1);
    for (int64_t r = 0; r < n_reads; r++) {
        if (y_len[r] < 0 || y_off[r] < 0 || y_off[r] > pool_bytes - y_len[r])
            return mrp_set_error(MRP_ERR_ARG, "%s: read %lld lies outside the pools", who, (long long) r);
        if (y_len[r] > 0 && (!read_symbols || !read_counts)) return mrp_set_error(MRP_ERR_ARG, "%s: null read pool", who);
        for (int64_t k = y_off[r]; k < y_off[r] + y_len[r]; k++)
            if (read_symbols[k] > 4) return mrp_set_error(MRP_ERR_ARG, "%s: read %lld, position %lld: symbol %d above 4", who, (long long) r, (long long) (k - y_off[r]), (int) read_symbols[k]);
    }
    const mrp_posterior_pairs *lists[3] = {matches, deletes, inserts};
    static const char *names[3] = {"matches", "deletes", "inserts"};
    for (int q = 0; q < 3; q++) {
        const int rc = po_check_list(who, names[q], lists[q], n_reads);
        if (rc != MRP_OK) return rc;
    }
    reads.resize((size_t) n_reads);
    int64_t slots = 0;
    for (int64_t c = 0; c < n_consensus; c++) {
        const int64_t L = node_first[c + 1] - node_first[c];
        for (int64_t r = read_first[c]; r < read_first[c + 1]; r++) {
            const int64_t shift = x_shift ? x_shift[r] : 0;
            for (int q = 0; q < 3; q++) {
                const mrp_posterior_pairs *l = lists[q];
                /* a match's x in [0, L - 1], y in [0, len - 1]; a delete's y from -1; an insert's x from -1 */
                const int64_t x_lo = q == POA_INSERT ? -1 : 0, y_lo = q == POA_DELETE ? -1 : 0;
                for (int64_t i = l->first[r]; i < l->first[r + 1]; i++) {
                    const int64_t xs = shift + l->x[i];
                    if (l->y[i] < y_lo || l->y[i] >= y_len[r])
                        return mrp_set_error(MRP_ERR_ARG, "%s: consensus %lld, read %lld, %s entry %lld: y %d outside [%lld, %d)", who, (long long) c, (long long) r,
                                             names[q], (long long) i, (int) l->y[i], (long long) y_lo, (int) y_len[r]);
                    if (xs < x_lo || xs >= L)
                        return mrp_set_error(MRP_ERR_ARG, "%s: consensus %lld, read %lld, %s entry %lld: x %d + x_shift %lld outside [%lld, %lld)", who, (long long) c,
                                             (long long) r, names[q], (long long) i, (int) l->x[i], (long long) shift, (long long) x_lo, (long long) L);
                    if (l->weight[i] < 0)
                        return mrp_set_error(MRP_ERR_ARG, "%s: consensus %lld, read %lld, %s entry %lld: negative weight %d", who, (long long) c, (long long) r,
                                             names[q], (long long) i, (int) l->weight[i]);
                }
            }
            PoaRead rd;
            rd.node_base = node_first[c] + c;
            rd.ref_base = node_first[c];
            rd.y_off = y_off[r];
            for (int q = 0; q < 3; q++) {
                rd.lg[q] = poa_table_lg(lists[q]->first[r + 1] - lists[q]->first[r]);
                rd.table[q] = slots;
                if (rd.lg[q] >= 0) slots += 1ll << rd.lg[q];
            }
            rd.L = (int32_t) L;
            rd.y_len = y_len[r];
            rd.shift = (int32_t) shift;
            rd.strand = read_forward_strand[r] ? 1u : 0u;
            rd.cons = (int32_t) c;
            reads[(size_t) r] = rd;
        }
    }
    *table_slots = slots;
    return MRP_OK;
}

extern "C" void mrp_poa_free(mrp_poa *p) {
    if (!p) return;
    free(p->base_weight);
    free(p->repeat_count_weight);
    free(p->base_pick);
    free(p->repeat_count_pick);
    free(p->insert_first);
    free(p->insert_str_off);
    free(p->insert_str_len);
    free(p->insert_weight_forward);
    free(p->insert_weight_reverse);
    free(p->insert_n_observations);
    free(p->pool_symbols);
    free(p->pool_counts);
    free(p->delete_first);
    free(p->delete_length);
    free(p->delete_weight_forward);
    free(p->delete_weight_reverse);
    free(p->delete_n_observations);
    free(p->totals);
    memset(p, 0, sizeof(*p));
}

extern "C" int mrp_poa_augment(mrp_context *ctx, int32_t max_repeat, int64_t n_consensus, const int64_t *node_first, const uint8_t *symbols,
                               const uint8_t *ref_counts, const int64_t *read_first, const uint8_t *read_symbols, const uint8_t *read_counts, int64_t pool_bytes,
                               const int64_t *y_off, const int32_t *y_len, const uint8_t *read_forward_strand, const int32_t *x_shift,
                               const mrp_posterior_pairs *matches, const mrp_posterior_pairs *deletes, const mrp_posterior_pairs *inserts,
                               const mrp_poa_options *opt, mrp_poa *out, mrp_poa_stats *stats) {
    static const char *who = "mrp_poa_augment";
    const double t_begin = po_now_ms();
    HostVec<PoaRead> reads;
    int64_t table_slots = 0;
    const int rc = poa_check_and_build(who, max_repeat, n_consensus, node_first, symbols, ref_counts, read_first, read_symbols, read_counts, pool_bytes, y_off,
                                       y_len, read_forward_strand, x_shift, matches, deletes, inserts, opt, out, reads, &table_slots);
    if (rc != MRP_OK) return rc;
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context", who);
    mrp_poa_stats st;
    memset(&st, 0, sizeof(st));
    st.check_ms = po_now_ms() - t_begin;
    st.table_slots = table_slots;
    const int R = max_repeat;
    const int64_t n_ref = node_first[n_consensus], n_reads = read_first[n_consensus], n_nodes = n_ref + n_consensus;
    const mrp_posterior_pairs *lists[3] = {matches, deletes, inserts};
    int64_t n_list[3];
    for (int q = 0; q < 3; q++) n_list[q] = lists[q]->first[n_reads];
    st.matches = n_list[POA_MATCH];
    st.deletes = n_list[POA_DELETE];
    st.inserts = n_list[POA_INSERT];
    mrp_poa res;
    memset(&res, 0, sizeof(res));
    struct Guard { mrp_poa *p; ~Guard() { if (p) mrp_poa_free(p); } } guard{&res}; /* an early return frees what was allocated */
    res.n_nodes = n_nodes;
    res.n_consensus = n_consensus;
    res.max_repeat = R;
    HostVec<int64_t> poa_first((size_t) n_consensus + 1);
    for (int64_t c = 0; c <= n_consensus; c++) poa_first[(size_t) c] = node_first[c] + c;
    HostVec<uint32_t> h_first[2], h_len[2], h_off; /* [0] deletes, [1] inserts */
    uint32_t n_groups[2] = {0, 0}, pool_len = 0;
    float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
    if (n_consensus > 0) {
        const int rc_device = [&]() -> int {
        HIP_TRY(hipSetDevice(ctx->device));
        hipStream_t s = ctx->stream;
        DevBufGroup arrays;
        DevBuf<uint8_t> d_ref_s{arrays}, d_ref_c{arrays}, d_read_s{arrays}, d_read_c{arrays}, d_sp_s{arrays}, d_pool_s{arrays}, d_leader{arrays};
        DevBuf<int64_t> d_poa_first{arrays}, d_first[3] = {DevBuf<int64_t>{arrays}, DevBuf<int64_t>{arrays}, DevBuf<int64_t>{arrays}}, d_sums{arrays}, d_g_obs[2] = {DevBuf<int64_t>{arrays}, DevBuf<int64_t>{arrays}};
        DevBuf<PoaRead> d_reads{arrays};
        DevBuf<int32_t> d_x[3] = {DevBuf<int32_t>{arrays}, DevBuf<int32_t>{arrays}, DevBuf<int32_t>{arrays}}, d_y[3] = {DevBuf<int32_t>{arrays}, DevBuf<int32_t>{arrays}, DevBuf<int32_t>{arrays}},
                        d_w[3] = {DevBuf<int32_t>{arrays}, DevBuf<int32_t>{arrays}, DevBuf<int32_t>{arrays}}, d_vals{arrays}, d_sp_c{arrays}, d_pool_c{arrays}, d_base_pick{arrays}, d_count_pick{arrays};
        DevBuf<unsigned long long> d_keys{arrays}, d_base_w{arrays}, d_count_w{arrays}, d_counters{arrays}, d_tot_acc{arrays};
        DevBuf<uint32_t> d_flags{arrays}, d_cursors{arrays}, d_node_cnt{arrays}, d_off{arrays}, d_cur{arrays}, d_grp_cnt{arrays},
            d_grp_first[2] = {DevBuf<uint32_t>{arrays}, DevBuf<uint32_t>{arrays}}, d_g_len[2] = {DevBuf<uint32_t>{arrays}, DevBuf<uint32_t>{arrays}}, d_g_src{arrays}, d_g_off{arrays};
        DevBuf<PoaRecord> d_rec{arrays}, d_sorted{arrays};
        DevBuf<double> d_base_out{arrays}, d_count_out{arrays}, d_totals{arrays}, d_g_wf[2] = {DevBuf<double>{arrays}, DevBuf<double>{arrays}}, d_g_wr[2] = {DevBuf<double>{arrays}, DevBuf<double>{arrays}};
        arrays.bind(&ctx->pool);
        hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
        struct Events { hipEvent_t *e; ~Events() { for (int i = 0; i < 6; i++) if (e[i]) (void) hipEventDestroy(e[i]); } } events{ev};
        Drain drain{s};
        for (hipEvent_t &e : ev) HIP_TRY(hipEventCreate(&e));
        auto up = [&](void *dst, const void *src, size_t bytes) {
            st.bytes_uploaded += (int64_t) bytes;
            return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, s) : hipSuccess;
        };
        auto down = [&](void *dst, const void *src, size_t bytes) {
            st.bytes_downloaded += (int64_t) bytes;
            return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s) : hipSuccess;
        };
        /* upload */
        HIP_TRY(hipEventRecord(ev[0], s));
        HIP_TRY(d_ref_s.alloc((size_t) n_ref));
        HIP_TRY(d_ref_c.alloc((size_t) n_ref));
        HIP_TRY(up(d_ref_s.p, symbols, (size_t) n_ref));
        HIP_TRY(up(d_ref_c.p, ref_counts, (size_t) n_ref));
        HIP_TRY(d_read_s.alloc((size_t) pool_bytes));
        HIP_TRY(d_read_c.alloc((size_t) pool_bytes));
        HIP_TRY(up(d_read_s.p, read_symbols, read_symbols ? (size_t) pool_bytes : 0));
        HIP_TRY(up(d_read_c.p, read_counts, read_counts ? (size_t) pool_bytes : 0));
        HIP_TRY(d_poa_first.alloc(poa_first.size()));
        HIP_TRY(up(d_poa_first.p, poa_first.data(), 8 * poa_first.size()));
        HIP_TRY(d_reads.alloc((size_t) n_reads));
        HIP_TRY(up(d_reads.p, reads.data(), sizeof(PoaRead) * (size_t) n_reads));
        for (int q = 0; q < 3; q++) {
            HIP_TRY(d_first[q].alloc((size_t) n_reads + 1));
            HIP_TRY(up(d_first[q].p, lists[q]->first, 8 * ((size_t) n_reads + 1)));
            HIP_TRY(d_x[q].alloc((size_t) n_list[q]));
            HIP_TRY(d_y[q].alloc((size_t) n_list[q]));
            HIP_TRY(d_w[q].alloc((size_t) n_list[q]));
            HIP_TRY(up(d_x[q].p, lists[q]->x, 4 * (size_t) n_list[q]));
            HIP_TRY(up(d_y[q].p, lists[q]->y, 4 * (size_t) n_list[q]));
            HIP_TRY(up(d_w[q].p, lists[q]->weight, 4 * (size_t) n_list[q]));
        }
        HIP_TRY(d_keys.alloc((size_t) table_slots));
        HIP_TRY(d_vals.alloc((size_t) table_slots));
        HIP_TRY(d_base_w.alloc((size_t) (5 * n_nodes)));
        HIP_TRY(d_count_w.alloc((size_t) (R * n_nodes)));
        HIP_TRY(d_flags.alloc(1));
        HIP_TRY(d_counters.alloc(6)); /* three per kind */
        HIP_TRY(d_cursors.alloc(4));  /* two per kind */
        HIP_TRY(d_tot_acc.alloc((size_t) (8 * n_consensus)));
        HIP_TRY(hipMemsetAsync(d_keys.p, 0, 8 * (size_t) table_slots, s));
        HIP_TRY(hipMemsetAsync(d_base_w.p, 0, 8 * (size_t) (5 * n_nodes), s));
        HIP_TRY(hipMemsetAsync(d_count_w.p, 0, 8 * (size_t) (R * n_nodes), s));
        HIP_TRY(hipMemsetAsync(d_flags.p, 0, 4, s));
        HIP_TRY(hipMemsetAsync(d_counters.p, 0, 48, s));
        HIP_TRY(hipMemsetAsync(d_cursors.p, 0, 16, s));
        HIP_TRY(hipMemsetAsync(d_tot_acc.p, 0, 8 * (size_t) (8 * n_consensus), s));
        HIP_TRY(hipEventRecord(ev[1], s));
        /* sets, match weights, the counting pass */
        for (int q = 0; q < 3; q++)
            if (n_list[q] > 0) {
                hipLaunchKernelGGL(po_sets_kernel, dim3(po_blocks(n_list[q])), dim3(PO_NT), 0, s, q, n_list[q], (int) n_reads, d_first[q].p, d_reads.p, d_x[q].p, d_y[q].p,
                                   d_keys.p, d_vals.p, d_flags.p);
                HIP_TRY(hipGetLastError());
            }
        if (n_list[POA_MATCH] > 0) {
            hipLaunchKernelGGL(po_match_kernel, dim3(po_blocks(n_list[POA_MATCH])), dim3(PO_NT), 0, s, n_list[POA_MATCH], (int) n_reads, d_first[POA_MATCH].p, d_reads.p,
                               d_x[POA_MATCH].p, d_y[POA_MATCH].p, d_w[POA_MATCH].p, d_read_s.p, d_read_c.p, R, d_base_w.p, d_count_w.p);
            HIP_TRY(hipGetLastError());
        }
        for (int q = POA_DELETE; q <= POA_INSERT; q++)
            if (n_list[q] > 0) {
                hipLaunchKernelGGL(po_enumerate_kernel<false>, dim3(po_blocks(n_list[q])), dim3(PO_NT), 0, s, q, n_list[q], (int) n_reads, d_first[q].p, d_reads.p, d_x[q].p,
                                   d_y[q].p, d_w[q].p, d_keys.p, d_vals.p, d_ref_s.p, d_ref_c.p, d_read_s.p, d_read_c.p, (int) opt->compare_repeat_counts,
                                   (int) opt->merge_ends, d_counters.p + 3 * (q - 1), (uint32_t *) nullptr, 0u, 0u, (PoaRecord *) nullptr, (uint8_t *) nullptr,
                                   (int32_t *) nullptr, (uint32_t *) nullptr, d_flags.p);
                HIP_TRY(hipGetLastError());
            }
        uint32_t h_flags = 0;
        unsigned long long h_counters[6];
        HIP_TRY(down(&h_flags, d_flags.p, 4));
        HIP_TRY(down(h_counters, d_counters.p, 48));
        HIP_TRY(hipEventRecord(ev[2], s));
        HIP_TRY(hipStreamSynchronize(s));
        if (h_flags & (7u * POA_FLAG_DUPLICATE)) {
            const int q = (h_flags & 1u) ? 0 : (h_flags & 2u) ? 1 : 2;
            static const char *names[3] = {"matches", "deletes", "inserts"};
            return mrp_set_error(MRP_ERR_ARG, "%s: an (x, y) occurs twice in the %s of one read (the reference asserts)", who, names[q]);
        }
        const unsigned long long n_rec[2] = {h_counters[0], h_counters[3]}, n_sym = h_counters[4];
        if (n_rec[0] >= (1ull << 31) || n_rec[1] >= (1ull << 31) || n_sym >= (1ull << 31)) {
            return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: %llu complete deletes, %llu complete inserts of %llu symbols (limit 2^31 - 1 each)", who, n_rec[0], n_rec[1], n_sym);
        }
        st.complete_deletes = (int64_t) n_rec[0];
        st.complete_inserts = (int64_t) n_rec[1];
        st.longest_run = (int64_t) std::max(h_counters[2], h_counters[5]);
        /* the emitting pass and the regrouping, deletes then inserts over the same arrays */
        const uint32_t rec_cap = (uint32_t) std::max(n_rec[0], n_rec[1]);
        HIP_TRY(d_rec.alloc(rec_cap));
        HIP_TRY(d_sorted.alloc(rec_cap));
        HIP_TRY(d_leader.alloc(rec_cap));
        HIP_TRY(d_sums.alloc(3 * (size_t) rec_cap));
        HIP_TRY(d_sp_s.alloc((size_t) n_sym));
        HIP_TRY(d_sp_c.alloc((size_t) n_sym));
        HIP_TRY(d_node_cnt.alloc((size_t) n_nodes));
        HIP_TRY(d_off.alloc((size_t) n_nodes + 1));
        HIP_TRY(d_cur.alloc((size_t) n_nodes));
        HIP_TRY(d_grp_cnt.alloc((size_t) n_nodes));
        HIP_TRY(d_g_src.alloc((size_t) rec_cap)); /* written by the leaders of either kind */
        HIP_TRY(d_g_off.alloc((size_t) n_rec[1] + 1));
        HIP_TRY(d_pool_s.alloc((size_t) n_sym));
        HIP_TRY(d_pool_c.alloc((size_t) n_sym));
        for (int k = 0; k < 2; k++) {
            HIP_TRY(d_grp_first[k].alloc((size_t) n_nodes + 1));
            HIP_TRY(d_g_len[k].alloc((size_t) n_rec[k]));
            HIP_TRY(d_g_wf[k].alloc((size_t) n_rec[k]));
            HIP_TRY(d_g_wr[k].alloc((size_t) n_rec[k]));
            HIP_TRY(d_g_obs[k].alloc((size_t) n_rec[k]));
        }
        float ms_enum = 0.f, ms_group = 0.f;
        hipEvent_t ev_k[5] = {nullptr, nullptr, nullptr, nullptr, nullptr}; /* [3], [4]: around the pool packing, read after the last wait */
        struct Events3 { hipEvent_t *e; ~Events3() { for (int i = 0; i < 5; i++) if (e[i]) (void) hipEventDestroy(e[i]); } } events3{ev_k};
        for (hipEvent_t &e : ev_k) HIP_TRY(hipEventCreate(&e));
        for (int k = 0; k < 2; k++) {
            const int q = k == 0 ? POA_DELETE : POA_INSERT;
            const uint32_t n = (uint32_t) n_rec[k];
            HIP_TRY(hipEventRecord(ev_k[0], s));
            HIP_TRY(hipMemsetAsync(d_node_cnt.p, 0, 4 * (size_t) n_nodes, s));
            HIP_TRY(hipMemsetAsync(d_cur.p, 0, 4 * (size_t) n_nodes, s));
            HIP_TRY(hipMemsetAsync(d_grp_cnt.p, 0, 4 * (size_t) n_nodes, s));
            if (n_list[q] > 0 && n > 0) {
                hipLaunchKernelGGL(po_enumerate_kernel<true>, dim3(po_blocks(n_list[q])), dim3(PO_NT), 0, s, q, n_list[q], (int) n_reads, d_first[q].p, d_reads.p, d_x[q].p,
                                   d_y[q].p, d_w[q].p, d_keys.p, d_vals.p, d_ref_s.p, d_ref_c.p, d_read_s.p, d_read_c.p, (int) opt->compare_repeat_counts,
                                   (int) opt->merge_ends, d_counters.p + 3 * k, d_cursors.p + 2 * k, n, (uint32_t) n_sym, d_rec.p, d_sp_s.p, d_sp_c.p, d_node_cnt.p,
                                   d_flags.p);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(hipEventRecord(ev_k[1], s));
            hipLaunchKernelGGL(po_scan_kernel, dim3(1), dim3(PO_SCAN_NT), 0, s, n_nodes, d_node_cnt.p, d_off.p);
            HIP_TRY(hipGetLastError());
            if (n > 0) {
                hipLaunchKernelGGL(po_scatter_kernel, dim3(po_blocks(n)), dim3(PO_NT), 0, s, n, d_rec.p, d_off.p, d_cur.p, d_sorted.p);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(po_leader_kernel, dim3(po_blocks(n)), dim3(PO_NT), 0, s, n, k, d_sorted.p, d_off.p, d_sp_s.p, d_sp_c.p, d_leader.p, d_sums.p, d_grp_cnt.p);
                HIP_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL(po_scan_kernel, dim3(1), dim3(PO_SCAN_NT), 0, s, n_nodes, d_grp_cnt.p, d_grp_first[k].p);
            HIP_TRY(hipGetLastError());
            if (n > 0) {
                hipLaunchKernelGGL(po_place_kernel, dim3(po_blocks(n)), dim3(PO_NT), 0, s, n, k, d_sorted.p, d_off.p, d_leader.p, d_sums.p, d_grp_first[k].p, d_g_len[k].p,
                                   d_g_src.p, d_g_wf[k].p, d_g_wr[k].p, d_g_obs[k].p, d_tot_acc.p, d_flags.p);
                HIP_TRY(hipGetLastError());
            }
            HIP_TRY(down(&n_groups[k], d_grp_first[k].p + n_nodes, 4));
            HIP_TRY(hipEventRecord(ev_k[2], s));
            HIP_TRY(hipStreamSynchronize(s)); /* the group count sizes the next launches; the arrays of this kind are reused by the next */
            if (k == 1) {
                HIP_TRY(hipEventRecord(ev_k[3], s));
                hipLaunchKernelGGL(po_scan_kernel, dim3(1), dim3(PO_SCAN_NT), 0, s, (int64_t) n_groups[1], d_g_len[1].p, d_g_off.p);
                HIP_TRY(hipGetLastError());
                if (n_groups[1] > 0) {
                    hipLaunchKernelGGL(po_pool_kernel, dim3(po_blocks(n_groups[1])), dim3(PO_NT), 0, s, n_groups[1], d_g_len[1].p, d_g_src.p, d_g_off.p, d_sp_s.p, d_sp_c.p,
                                       d_pool_s.p, d_pool_c.p);
                    HIP_TRY(hipGetLastError());
                }
                HIP_TRY(hipEventRecord(ev_k[4], s));
                HIP_TRY(down(&pool_len, d_g_off.p + n_groups[1], 4));
            }
            float a = 0.f, b = 0.f;
            HIP_TRY(hipEventElapsedTime(&a, ev_k[0], ev_k[1]));
            HIP_TRY(hipEventElapsedTime(&b, ev_k[1], ev_k[2]));
            ms_enum += a;
            ms_group += b;
        }
        /* picks and totals */
        HIP_TRY(d_base_out.alloc((size_t) (5 * n_nodes)));
        if (opt->want_repeat_count_weight) HIP_TRY(d_count_out.alloc((size_t) (R * n_nodes)));
        HIP_TRY(d_base_pick.alloc((size_t) n_nodes));
        HIP_TRY(d_count_pick.alloc((size_t) n_nodes));
        HIP_TRY(d_totals.alloc((size_t) (4 * n_consensus)));
        HIP_TRY(hipEventRecord(ev[3], s));
        hipLaunchKernelGGL(po_picks_kernel, dim3(po_blocks(n_nodes)), dim3(PO_NT), 0, s, n_nodes, n_consensus, d_poa_first.p, d_ref_s.p, d_ref_c.p, R,
                           opt->reference_base_penalty, d_base_w.p, d_count_w.p, d_base_out.p, opt->want_repeat_count_weight ? d_count_out.p : (double *) nullptr,
                           d_base_pick.p, d_count_pick.p, d_flags.p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(po_node_totals_kernel, dim3((unsigned) n_consensus), dim3(PO_NT), 0, s, d_poa_first.p, d_ref_s.p, d_base_w.p, d_tot_acc.p);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(po_totals_kernel, dim3(po_blocks(4 * n_consensus)), dim3(PO_NT), 0, s, 4 * n_consensus, d_tot_acc.p, d_totals.p, d_flags.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(ev[4], s));
        HIP_TRY(down(&h_flags, d_flags.p, 4));
        HIP_TRY(hipStreamSynchronize(s));
        if (h_flags & POA_FLAG_CAPACITY) {
            return mrp_set_error(MRP_ERR_HIP, "%s: the emitting pass met more complete indels than the counting pass", who);
        }
        if (h_flags & POA_FLAG_INEXACT) {
            return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: an accumulator or a total reaches 2^53: the reference's doubles would round", who);
        }
        /* download */
        const bool ok = po_alloc(res.base_weight, 5 * n_nodes) && (!opt->want_repeat_count_weight || po_alloc(res.repeat_count_weight, (int64_t) R * n_nodes)) &&
                        po_alloc(res.base_pick, n_nodes) && po_alloc(res.repeat_count_pick, n_nodes) && po_alloc(res.insert_first, n_nodes + 1) &&
                        po_alloc(res.insert_str_off, n_groups[1]) && po_alloc(res.insert_str_len, n_groups[1]) && po_alloc(res.insert_weight_forward, n_groups[1]) &&
                        po_alloc(res.insert_weight_reverse, n_groups[1]) && po_alloc(res.insert_n_observations, n_groups[1]) && po_alloc(res.pool_symbols, pool_len) &&
                        po_alloc(res.pool_counts, pool_len) && po_alloc(res.delete_first, n_nodes + 1) && po_alloc(res.delete_length, n_groups[0]) &&
                        po_alloc(res.delete_weight_forward, n_groups[0]) && po_alloc(res.delete_weight_reverse, n_groups[0]) &&
                        po_alloc(res.delete_n_observations, n_groups[0]) && po_alloc(res.totals, 4 * n_consensus);
        if (!ok) {
            return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory for the outputs", who);
        }
        for (int k = 0; k < 2; k++) {
            h_first[k].resize((size_t) n_nodes + 1);
            h_len[k].resize(n_groups[k]);
            HIP_TRY(down(h_first[k].data(), d_grp_first[k].p, 4 * ((size_t) n_nodes + 1)));
            HIP_TRY(down(h_len[k].data(), d_g_len[k].p, 4 * (size_t) n_groups[k]));
        }
        h_off.resize((size_t) n_groups[1] + 1);
        HIP_TRY(down(h_off.data(), d_g_off.p, 4 * ((size_t) n_groups[1] + 1)));
        HIP_TRY(down(res.base_weight, d_base_out.p, 8 * (size_t) (5 * n_nodes)));
        if (opt->want_repeat_count_weight) HIP_TRY(down(res.repeat_count_weight, d_count_out.p, 8 * (size_t) (R * n_nodes)));
        HIP_TRY(down(res.base_pick, d_base_pick.p, 4 * (size_t) n_nodes));
        HIP_TRY(down(res.repeat_count_pick, d_count_pick.p, 4 * (size_t) n_nodes));
        HIP_TRY(down(res.insert_weight_forward, d_g_wf[1].p, 8 * (size_t) n_groups[1]));
        HIP_TRY(down(res.insert_weight_reverse, d_g_wr[1].p, 8 * (size_t) n_groups[1]));
        HIP_TRY(down(res.insert_n_observations, d_g_obs[1].p, 8 * (size_t) n_groups[1]));
        HIP_TRY(down(res.pool_symbols, d_pool_s.p, (size_t) pool_len));
        HIP_TRY(down(res.pool_counts, d_pool_c.p, 4 * (size_t) pool_len));
        HIP_TRY(down(res.delete_weight_forward, d_g_wf[0].p, 8 * (size_t) n_groups[0]));
        HIP_TRY(down(res.delete_weight_reverse, d_g_wr[0].p, 8 * (size_t) n_groups[0]));
        HIP_TRY(down(res.delete_n_observations, d_g_obs[0].p, 8 * (size_t) n_groups[0]));
        HIP_TRY(down(res.totals, d_totals.p, 8 * (size_t) (4 * n_consensus)));
        HIP_TRY(hipEventRecord(ev[5], s));
        HIP_TRY(hipStreamSynchronize(s));
        HIP_TRY(hipEventElapsedTime(&ms[0], ev[0], ev[1]));
        HIP_TRY(hipEventElapsedTime(&ms[1], ev[1], ev[2]));
        HIP_TRY(hipEventElapsedTime(&ms[4], ev[3], ev[4]));
        ms[2] = ms_enum;
        float ms_pool = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms_pool, ev_k[3], ev_k[4]));
        ms[3] = ms_group + ms_pool;
        /* the device's 32-bit offsets as the header's types */
        for (int64_t k = 0; k <= n_nodes; k++) {
            res.delete_first[k] = h_first[0][(size_t) k];
            res.insert_first[k] = h_first[1][(size_t) k];
        }
        for (uint32_t g = 0; g < n_groups[0]; g++) res.delete_length[g] = (int32_t) h_len[0][g];
        for (uint32_t g = 0; g < n_groups[1]; g++) {
            res.insert_str_len[g] = (int32_t) h_len[1][g];
            res.insert_str_off[g] = h_off[g];
        }
        return MRP_OK;
        }();
        ctx->pool.reclaim(); /* (the device arrays have gone back to the pool and the stream has drained) */
        if (rc_device != MRP_OK) return rc_device;
    } else {
        if (!po_alloc(res.base_weight, 0) || !po_alloc(res.base_pick, 0) || !po_alloc(res.repeat_count_pick, 0) || !po_alloc(res.insert_first, 1) ||
            !po_alloc(res.delete_first, 1) || !po_alloc(res.totals, 0))
            return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory for the outputs", who);
        res.insert_first[0] = res.delete_first[0] = 0;
    }
    res.n_deletes = n_groups[0];
    res.n_inserts = n_groups[1];
    res.pool_len = pool_len;
    st.distinct_deletes = n_groups[0];
    st.distinct_inserts = n_groups[1];
    st.upload_ms = ms[0];
    st.sets_ms = ms[1];
    st.enumerate_ms = ms[2];
    st.group_ms = ms[3];
    st.picks_ms = ms[4];
    *out = res;
    guard.p = nullptr;
    st.total_ms = po_now_ms() - t_begin;
    if (stats) *stats = st;
    return MRP_OK;
}
