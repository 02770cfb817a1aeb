/*
 * mrp_extract.hip -- read substrings at variant sites from alignments: extractReadSubstringsAtVariantPositions
 * (impl/htsIntegration.c:1758-1989) with the VCF entries' windows and allele strings of getAlleleSubstrings2
 * (impl/vcf.c:394-462).  gfx950 only.
 *
 * The reference walks every read's CIGAR one base at a time and, after every step, starts the next VCF entries of its list
 * whose window has begun (saveStartingVcfEntries, :1589-1607) and finishes the open ones whose window has ended
 * (saveFinishedVcfEntries, :1610-1680).  The walk's state after any step is a piecewise-linear function of the CIGAR, so here
 * it becomes prefix sums and searches:
 *
 *   ex_scan_kernel     a wave per read: the read filters (:1816-1842), the clips of getAlignedReadLength3 (:37-111,
 *                      boundaryAtMatch = FALSE), alnReadLength, the first VCF entry at or after the read (vcf.c:238-258),
 *                      and the reference / sequence advance before every op (wave-wide scans) into an op table in HBM;
 *   ex_locate_kernel   a wave per read, a lane per (read, candidate entry): the running maximum of the window starts (the
 *                      delayed start), binary searches of the op table for the steps that reach the window's start and
 *                      end, the dropping rules; counted once, then written after a scan of the counts;
 *   ex_var_count_kernel / ex_bucket_kernel / ex_rank_kernel   a stable counting sort of the substrings by entry: counts,
 *                      scan, buckets, and inside a bucket the rank of each substring's (read, entry) index, so the order
 *                      does not depend on the order of the atomics;
 *   ex_gather_kernel   a wave per substring: read bases (seq_nt16_str codes) to symbols into the output pool.
 *
 * With indelSizeForSVHandling > 0 (on a context that admits it, mrp_context_set_sv_split) the reference makes the walk twice, over the
 * small entries and over the structural ones, and merges the two per read (:1725-1755).  Here the entries are staged class-major and
 * the scan and locate kernels are instantiated for two classes: a first-entry search and a running maximum per class, one count and
 * one run of write offsets per read over both; an entry carries its original index, so the sort gives the caller's variant order
 * (DESIGN.md section 9.11).  Without the split the one-class instantiations run: the launches and the bytes of before.
 *
 * The windows are computed on the host while checking the arguments; the allele strings on the worker pool while the
 * device runs.  One total (the substrings and their bases) comes back between the two halves to size the buffers.
 *
 * The call is one mrp_extract_run taken through steps (mrp_internal.h): check, stage and upload, first half, totals, second
 * half, download.  mrp_extract_read_substrings is all of them; mrp_haplotag_aligned_chunks (mrp_aligned.hip) stops before the
 * download and reads the result in HBM.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <climits>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/margin_rphmm.h"
#include "mrp_internal.h"

namespace {

enum : uint32_t { OP_M = 0, OP_I = 1, OP_D = 2, OP_N = 3, OP_S = 4, OP_H = 5, OP_P = 6, OP_EQ = 7, OP_X = 8 };

__host__ __device__ inline bool ex_ref_op(uint32_t op) { return op == OP_M || op == OP_D || op == OP_N || op == OP_EQ || op == OP_X; }
__host__ __device__ inline bool ex_seq_op(uint32_t op) { return op == OP_M || op == OP_I || op == OP_EQ || op == OP_X; }
/* the ops at which getAlignedReadLength3 (boundaryAtMatch = FALSE) stops looking for clips */
__host__ __device__ inline bool ex_body_op(uint32_t op) { return ex_ref_op(op) || op == OP_I; }

struct ExRead {
    int64_t pos;
    int64_t cig;     /* first CIGAR word (and op table row) of the read in the call */
    int64_t seq_nib; /* nibble index of the read's first base in the call's packed sequence */
    int32_t n_cig, l_qseq, chunk;
    uint16_t flag;
    uint8_t mapq, pad;
};

struct ExChunk {
    int64_t ovl, cs, ce;
    int64_t var0; /* first variant of the chunk in the call */
    int64_t n_var;
    /* the two classes of the split walk (indelSizeForSVHandling > 0, :1725-1755): records [0, n_small) are the chunk's small variants,
     * [n_small, n_var) its structural ones; without the split one class holds everything (n_small = n_var) */
    int64_t n_small;
};

/* staged in the caller's order -- or, for the split walk, class-major (small ascending, then structural ascending) beside a table of
 * every record's original index in the call */
struct ExVar {
    int64_t pos;          /* 0-based genome */
    int64_t start, stop;  /* refAlnStart / refAlnStopIncl, 0-based in the overlap slice */
};

struct ExOpt {
    int64_t min_mapq;
    int32_t secondary, supplementary;
};

struct ExState {
    int64_t r0;          /* pos - chunkOverlapStart: ref - overlap start before the first step */
    int64_t limit;       /* alnReadLength + 1 reference steps at most (:1901) */
    int64_t tot_ref, tot_seq;
    int32_t clip;        /* start soft clip */
    int32_t var_first[2]; /* per class: record of the call's first entry at or after the read (the class's end: none) */
    int16_t s1, r1;      /* sequence / reference advance of the first step */
};

struct ExOp {
    int64_t rb; /* reference steps before the op */
    int32_t sb; /* sequence advance before the op */
    uint32_t word;
};

struct ExEntry {
    int64_t src; /* nibble index of the substring's first base */
    int32_t var, read, len, pad;
};

constexpr int EX_WAVE = 64;

__device__ inline int64_t wave_incl_sum(int64_t v) {
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < EX_WAVE; d <<= 1) {
        const int64_t t = __shfl_up(v, d, EX_WAVE);
        if (lane >= d) v += t;
    }
    return v;
}

__device__ inline int64_t wave_incl_max(int64_t v) {
    const int lane = threadIdx.x & 63;
    for (int d = 1; d < EX_WAVE; d <<= 1) {
        const int64_t t = __shfl_up(v, d, EX_WAVE);
        if (lane >= d) v = max(v, t);
    }
    return v;
}

__device__ inline int64_t wave_sum(int64_t v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, EX_WAVE);
    return v;
}

/* NCLS: 1, or 2 for the split walk -- one first-entry search per class (each walk's own, :1852-1855) */
template <int NCLS>
__global__ __launch_bounds__(64) void ex_scan_kernel(const ExRead *__restrict__ reads, const uint32_t *__restrict__ cigar,
                                                     const ExChunk *__restrict__ chunks, const ExVar *__restrict__ vars, ExOpt o,
                                                     ExOp *__restrict__ ops, ExState *__restrict__ state, uint8_t *__restrict__ status) {
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x;
    const ExRead rd = reads[r];
    uint8_t st = MRP_READ_DROPPED;
    if (rd.l_qseq <= 0 || rd.n_cig == 0 || (rd.flag & 0x4) || (!o.secondary && (rd.flag & 0x100)) || (!o.supplementary && (rd.flag & 0x800))) {
        if (lane == 0) status[r] = st;
        return;
    }
    const uint32_t *w = cigar + rd.cig;
    const int n = rd.n_cig;
    /* start clip: soft clips before the first M, =, X, D, N or I (:52-73) */
    int64_t clip = 0;
    for (int base = 0; base < n; base += EX_WAVE) {
        const int k = base + lane;
        const uint32_t op = k < n ? (w[k] & 15u) : 0u, ln = k < n ? (w[k] >> 4) : 0u;
        const uint64_t b = __ballot(k < n && ex_body_op(op));
        const int lim = b ? __ffsll((unsigned long long) b) - 1 : EX_WAVE;
        clip += wave_sum((k < n && lane < lim && op == OP_S) ? (int64_t) ln : 0);
        if (b) break;
    }
    /* end clip: from the last op back, never the first (:76-97) */
    int64_t eclip = 0;
    for (int base = 0; base < n - 1; base += EX_WAVE) {
        const int k = n - 1 - (base + lane);
        const bool in = k >= 1;
        const uint32_t op = in ? (w[k] & 15u) : 0u, ln = in ? (w[k] >> 4) : 0u;
        const uint64_t b = __ballot(in && ex_body_op(op));
        const int lim = b ? __ffsll((unsigned long long) b) - 1 : EX_WAVE;
        eclip += wave_sum((in && lane < lim && op == OP_S) ? (int64_t) ln : 0);
        if (b) break;
    }
    /* op table, countIndels (:113-120) */
    int64_t cr = 0, cs = 0, ins = 0, del = 0;
    for (int base = 0; base < n; base += EX_WAVE) {
        const int k = base + lane;
        const uint32_t word = k < n ? w[k] : 0u, op = word & 15u;
        const int64_t ln = word >> 4;
        const int64_t ra = (k < n && ex_ref_op(op)) ? ln : 0, sa = (k < n && ex_seq_op(op)) ? ln : 0;
        const int64_t ir = wave_incl_sum(ra), is = wave_incl_sum(sa);
        if (k < n) ops[rd.cig + k] = ExOp{cr + ir - ra, (int32_t) (cs + is - sa), word};
        cr += __shfl(ir, EX_WAVE - 1, EX_WAVE);
        cs += __shfl(is, EX_WAVE - 1, EX_WAVE);
        ins += wave_sum((k < n && op == OP_I) ? ln : 0);
        del += wave_sum((k < n && op == OP_D) ? ln : 0);
    }
    const int64_t aln_len = (int64_t) rd.l_qseq - clip - eclip + del - ins;
    const ExChunk ch = chunks[rd.chunk];
    if (aln_len <= 0 || rd.pos >= ch.ce || rd.pos + aln_len <= ch.cs) { /* :1832, :1840-1842 */
        if (lane == 0) status[r] = st;
        return;
    }
    /* binarySearchVcfListForFirstIndexAtOrAfterRefPos on refPos = pos - overlap + 1: the first entry with pos >= read pos */
    int32_t first[2] = {0, 0};
    bool listed = false;
#pragma unroll
    for (int c = 0; c < NCLS; c++) {
        const int64_t end = (c == NCLS - 1) ? ch.n_var : ch.n_small;
        int64_t lo = c ? ch.n_small : 0, hi = end;
        while (lo < hi) {
            const int64_t mid = (lo + hi) / 2;
            if (vars[ch.var0 + mid].pos < rd.pos) lo = mid + 1;
            else hi = mid;
        }
        first[c] = (int32_t) (ch.var0 + lo);
        listed = listed || lo < end;
    }
    if (!listed) { /* :1855 all entries before the read: not listed (split: by neither walk) */
        if (lane == 0) status[r] = st;
        return;
    }
    if (lane == 0) {
        const uint32_t op0 = w[0] & 15u;
        ExState s;
        s.r0 = rd.pos - ch.ovl;
        s.limit = aln_len + 1;
        s.tot_ref = cr;
        s.tot_seq = cs;
        s.clip = (int32_t) clip;
        s.var_first[0] = first[0];
        s.var_first[1] = first[1];
        s.s1 = ex_seq_op(op0) ? 1 : 0;
        s.r1 = ex_ref_op(op0) ? 1 : 0;
        state[r] = s;
        status[r] = (int64_t) rd.mapq < o.min_mapq ? MRP_READ_FILTERED : MRP_READ_KEPT;
    }
}

/* sequence advance right after the t-th reference step (1 <= t <= the read's reference steps) */
__device__ inline int64_t ex_seq_after(const ExOp *__restrict__ op, int n, int64_t t) {
    int lo = 0, hi = n - 1; /* the last op with rb < t: a reference op */
    while (lo < hi) {
        const int mid = (lo + hi + 1) / 2;
        if (op[mid].rb < t) lo = mid;
        else hi = mid - 1;
    }
    const ExOp o = op[lo];
    return (int64_t) o.sb + (ex_seq_op(o.word & 15u) ? t - o.rb : 0);
}

/* NCLS: 1, or 2 for the split walk -- one pass per class, each with its own running maximum; vorig (NCLS == 2): a record's original
 * index in the call, which the entry carries, so that the sort and the gather below see the caller's variant order */
template <bool WRITE, int NCLS>
__global__ __launch_bounds__(64) void ex_locate_kernel(const ExRead *__restrict__ reads, const uint8_t *__restrict__ status,
                                                       const ExState *__restrict__ state, const ExOp *__restrict__ ops,
                                                       const ExChunk *__restrict__ chunks, const ExVar *__restrict__ vars,
                                                       const int32_t *__restrict__ vorig, int64_t *__restrict__ count, unsigned long long *__restrict__ total_bases,
                                                       const int64_t *__restrict__ entry_off, ExEntry *__restrict__ entries) {
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x;
    if (status[r] == MRP_READ_DROPPED) {
        if (!WRITE && lane == 0) count[r] = 0;
        return;
    }
    const ExRead rd = reads[r];
    const ExState s = state[r];
    const ExChunk ch = chunks[rd.chunk];
    const ExOp *op = ops + rd.cig;
    const int n = rd.n_cig;
    const bool cut = s.tot_ref >= s.limit; /* the loop bound ends the walk before the CIGAR does */
    const int64_t r0 = s.r0, r_end = r0 + (cut ? s.limit : s.tot_ref);
    const int64_t seq_end = cut ? ex_seq_after(op, n, s.limit) : s.tot_seq;
    int64_t kept = 0, bases = 0;
#pragma unroll
    for (int c = 0; c < NCLS; c++) {
        const int64_t vend = ch.var0 + ((c == NCLS - 1) ? ch.n_var : ch.n_small);
        int64_t run_max = LLONG_MIN;
        for (int64_t j0 = s.var_first[c]; j0 < vend; j0 += EX_WAVE) {
            const int64_t j = j0 + lane;
            const bool in = j < vend;
            ExVar v{0, LLONG_MAX, 0};
            if (in) v = vars[j];
            const int64_t m = max(run_max, wave_incl_max(v.start)); /* the entry starts once every earlier one has */
            const bool cand = in && m <= r_end;
            bool keep = false;
            int64_t ss = 0, len = 0;
            if (cand) {
                const bool pre = m <= r0 && s.clip == 0; /* started before the first step (:1895-1899), checked after it */
                int64_t rs;
                if (m <= r0) { rs = r0; ss = 0; }
                else { rs = m; ss = ex_seq_after(op, n, m - r0); }
                bool decided = false;
                if (pre && v.stop <= r0 + s.r1) { len = s.s1; keep = len != 0; decided = true; }
                else if (!pre && v.stop <= rs) { decided = true; } /* finished in the step that started it: no base */
                if (!decided) {
                    if (v.stop <= r_end) {
                        len = ex_seq_after(op, n, v.stop - r0) - ss;
                        keep = len != 0;
                    } else { /* open at the end of the read (:1961-1962) */
                        len = seq_end - ss;
                        keep = len != 0 && !(r_end < v.pos - ch.ovl + 1);
                    }
                }
            }
            const uint64_t kb = __ballot(keep);
            if (WRITE && keep) {
                const int rank = __popcll(kb & ((1ull << lane) - 1ull));
                entries[entry_off[r] + kept + rank] = ExEntry{rd.seq_nib + s.clip + ss, NCLS == 2 ? vorig[j] : (int32_t) j, (int32_t) r, (int32_t) len, 0};
            }
            kept += __popcll(kb);
            bases += wave_sum(keep ? len : 0);
            run_max = __shfl(m, EX_WAVE - 1, EX_WAVE);
            if (__ballot(!cand)) break; /* the running maximum only grows: no later entry starts either */
        }
    }
    if (!WRITE && lane == 0) {
        count[r] = kept;
        atomicAdd(total_bases, (unsigned long long) bases);
    }
}

/* exclusive scan of n values into out[0..n], out[n] = total (one workgroup; the arrays of a call are at most ~10^7) */
__global__ __launch_bounds__(1024) void ex_scan_i64(const int64_t *__restrict__ in, int64_t n, int64_t *__restrict__ out) {
    __shared__ int64_t part[16];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63;
    int64_t carry = 0;
    for (int64_t base = 0; base < n; base += 1024) {
        const int64_t i = base + tid;
        const int64_t v = i < n ? in[i] : 0;
        const int64_t incl = wave_incl_sum(v);
        if (lane == 63) part[wv] = incl;
        __syncthreads();
        if (wv == 0) {
            int64_t p = lane < 16 ? part[lane] : 0;
            p = wave_incl_sum(p);
            if (lane < 16) part[lane] = p;
        }
        __syncthreads();
        const int64_t before = wv ? part[wv - 1] : 0;
        if (i < n) out[i] = carry + before + incl - v;
        carry += part[15];
        __syncthreads();
    }
    if (tid == 0) out[n] = carry;
}

__global__ void ex_var_count_kernel(const ExEntry *__restrict__ e, int64_t n, unsigned long long *__restrict__ cnt) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) atomicAdd(&cnt[e[i].var], 1ull);
}

__global__ void ex_bucket_kernel(const ExEntry *__restrict__ e, int64_t n, const int64_t *__restrict__ first, unsigned long long *__restrict__ fill,
                                 int32_t *__restrict__ bucket) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const int32_t v = e[i].var;
        bucket[first[v] + (int64_t) atomicAdd(&fill[v], 1ull)] = (int32_t) i;
    }
}

/* a wave per entry: the substrings of a bucket in the order of their index (= read order, the locate pass writes by read) */
__global__ __launch_bounds__(64) void ex_rank_kernel(const int64_t *__restrict__ first, int64_t n_var, const int32_t *__restrict__ bucket,
                                                     const ExEntry *__restrict__ e, int32_t *__restrict__ order, int64_t *__restrict__ len) {
    const int lane = threadIdx.x;
    for (int64_t v = blockIdx.x; v < n_var; v += gridDim.x) {
        const int64_t a = first[v], b = first[v + 1];
        for (int64_t i = a + lane; i < b; i += EX_WAVE) {
            const int32_t id = bucket[i];
            int64_t rank = 0;
            for (int64_t k = a; k < b; k++) rank += bucket[k] < id;
            order[a + rank] = id;
            len[a + rank] = e[id].len;
        }
    }
}

__global__ __launch_bounds__(64) void ex_gather_kernel(const int32_t *__restrict__ order, int64_t n, const ExEntry *__restrict__ e,
                                                       const int64_t *__restrict__ off, const uint8_t *__restrict__ seq, uint8_t *__restrict__ pool,
                                                       int64_t base, int32_t *__restrict__ read) {
    const int lane = threadIdx.x;
    for (int64_t p = blockIdx.x; p < n; p += gridDim.x) {
        const ExEntry x = e[order[p]];
        if (lane == 0) read[p] = x.read;
        uint8_t *dst = pool + base + off[p]; /* base: where the call's substrings begin in pool */
        for (int t = lane; t < x.len; t += EX_WAVE) {
            const int64_t i = x.src + t;
            const uint32_t code = (seq[i >> 1] >> ((~i & 1) << 2)) & 15u;
            /* seq_nt16_str: A = 1, C = 2, G = 4, T = 8; IUPAC codes and '=' become 4 (mrp_symbols_from_chars) */
            dst[t] = code == 1 ? 0 : code == 2 ? 1 : code == 4 ? 2 : code == 8 ? 3 : 4;
        }
    }
}

/* ---------------- host ---------------- */

double ex_now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

#define EX_HIP(expr)                                                                                                   \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess) return mrp_set_error(MRP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));       \
    } while (0)

uint8_t ex_symbol(char c) {
    switch (c) {
        case 'A': case 'a': return 0;
        case 'C': case 'c': return 1;
        case 'G': case 'g': return 2;
        case 'T': case 't': return 3;
        default: return 4;
    }
}

char ex_upper(char c) { return (c >= 'a' && c <= 'z') ? (char) (c - 'a' + 'A') : c; }

/* getAlleleSubstrings2 (vcf.c:394-462) with putRefPosInPOASpace = FALSE for one entry: the window, and the prefix / suffix
 * of the allele strings (ref[pre_at, pre_at + pre_len) and ref[suf_at, suf_at + suf_len)) */
struct ExWindow {
    int64_t start, stop, pre_at, pre_len, suf_at, suf_len;
};

int ex_window(const mrp_aligned_chunk &C, int64_t v, const mrp_extract_options &o, ExWindow &w, std::string &msg) {
    const int64_t n = C.reference_len, pos = C.variant_pos[v] - C.overlap_start;
    const int64_t e = C.is_sv[v] ? o.expansion_sv : o.expansion_small;
    const char *ra = C.allele_chars + C.allele_off[C.allele_first[v]];
    int64_t rl = C.allele_len[C.allele_first[v]];
    for (int64_t i = 0; i < rl; i++) {
        if (pos + i >= n) { rl = i; break; } /* a REF past the slice stops at its end (:418-421) */
        const char rc = ex_upper(C.reference[pos + i]), ac = ex_upper(ra[i]);
        if (!(rc == ac || (rc != 'A' && rc != 'C' && rc != 'G' && rc != 'T'))) { /* :423 */
            msg = "variant " + std::to_string(v) + ": REF allele disagrees with the reference at slice position " + std::to_string(pos + i) + " (vcf.c:423)";
            return MRP_ERR_ARG;
        }
    }
    const int64_t p_start = pos - e;
    int64_t s_start = pos + rl;
    int64_t s_len = s_start + e >= n ? n - s_start : e;
    if (s_start >= n) { s_start = n - 1; s_len = 0; }
    w.start = p_start < 0 ? 0 : p_start;
    w.stop = s_start + e >= n ? n - 1 : s_start + e;
    w.pre_at = w.start;
    w.pre_len = p_start < 0 ? pos : e;
    w.suf_at = s_start;
    w.suf_len = s_len;
    return MRP_OK;
}

/* argument checks of one chunk (and its windows); aligned_bases: M/=/X/I bases of its reads */
int ex_check_chunk(const mrp_aligned_chunk &C, const mrp_extract_options &o, std::vector<ExWindow> &win, int64_t &aligned_bases, std::string &msg) {
    auto bad = [&](const std::string &m) { msg = m; return MRP_ERR_ARG; };
    if (C.n_variants < 0 || C.n_reads < 0 || C.reference_len < 0 || C.allele_bytes < 0) return bad("bad sizes");
    if (C.n_variants >= (1ll << 31) || C.n_reads >= (1ll << 31)) return bad("more than 2^31 variants or reads");
    if (C.overlap_end < C.overlap_start || C.reference_len != C.overlap_end - C.overlap_start)
        return bad("the reference slice is not overlap_end - overlap_start long");
    if (C.reference_len > 0 && !C.reference) return bad("null reference");
    if (C.n_variants > 0 && (!C.variant_pos || !C.allele_first || !C.allele_off || !C.allele_len || !C.is_sv || (C.allele_bytes > 0 && !C.allele_chars)))
        return bad("null variant array");
    if (C.n_reads > 0 && (!C.pos || !C.flag || !C.mapq || !C.l_qseq || !C.cigar_first || !C.seq_first)) return bad("null read array");
    if (C.n_variants > 0 && C.allele_first[0] != 0) return bad("allele offsets must start at 0");
    for (int64_t v = 0; v < C.n_variants; v++) {
        if (C.variant_pos[v] < C.overlap_start || C.variant_pos[v] >= C.overlap_end) return bad("variant " + std::to_string(v) + " lies outside the overlap");
        if (v > 0 && C.variant_pos[v] < C.variant_pos[v - 1]) return bad("variants not ascending at " + std::to_string(v));
        if (C.allele_first[v + 1] <= C.allele_first[v]) return bad("variant " + std::to_string(v) + " has no allele or offsets not ascending");
        for (int64_t a = C.allele_first[v]; a < C.allele_first[v + 1]; a++)
            if (C.allele_len[a] < 0 || C.allele_off[a] < 0 || C.allele_off[a] + C.allele_len[a] > C.allele_bytes)
                return bad("allele " + std::to_string(a) + " lies outside allele_chars");
    }
    win.resize((size_t) C.n_variants);
    for (int64_t v = 0; v < C.n_variants; v++) {
        const int rc = ex_window(C, v, o, win[(size_t) v], msg);
        if (rc != MRP_OK) return rc;
    }
    if (C.n_reads == 0) return MRP_OK;
    if (C.cigar_first[0] != 0 || C.seq_first[0] != 0) return bad("read offsets must start at 0");
    if (C.cigar_first[C.n_reads] > 0 && !C.cigar) return bad("null cigar");
    if (C.seq_first[C.n_reads] > 0 && !C.seq) return bad("null seq");
    aligned_bases = 0;
    for (int64_t r = 0; r < C.n_reads; r++) {
        const int64_t a = C.cigar_first[r], b = C.cigar_first[r + 1];
        if (b < a || b - a >= (1ll << 31)) return bad("cigar offsets not ascending at read " + std::to_string(r));
        if (C.seq_first[r + 1] < C.seq_first[r]) return bad("seq offsets not ascending at read " + std::to_string(r));
        const bool walked = C.l_qseq[r] > 0 && b > a;
        if (walked && C.seq_first[r + 1] - C.seq_first[r] < ((int64_t) C.l_qseq[r] + 1) / 2)
            return bad("read " + std::to_string(r) + " has fewer packed bases than l_qseq");
        int64_t qlen = 0;
        for (int64_t k = a; k < b; k++) {
            const uint32_t op = C.cigar[k] & 15u, ln = C.cigar[k] >> 4;
            if (op > 8) return bad("read " + std::to_string(r) + ": CIGAR op code " + std::to_string(op) + " (htsIntegration.c:70)");
            if (walked && ln == 0 && op != OP_S && op != OP_H && op != OP_P) return bad("read " + std::to_string(r) + ": CIGAR op of length 0");
            if (ex_seq_op(op) || op == OP_S) qlen += ln;
            if (ex_seq_op(op)) aligned_bases += ln;
        }
        if (walked && qlen != C.l_qseq[r]) return bad("read " + std::to_string(r) + ": CIGAR query length is not l_qseq");
    }
    return MRP_OK;
}

template <class T> size_t ex_align(size_t x) { return (x + alignof(T) - 1) / alignof(T) * alignof(T); }

void ex_free_chunks(mrp_extracted_chunk *res, int64_t n_chunks) {
    if (!res) return;
    for (int64_t c = 0; c < n_chunks; c++) {
        mrp_extracted_chunk &X = res[c];
        void *ps[] = {X.ref_aln_start, X.ref_aln_stop_incl, X.allele_first, X.allele_off, X.allele_len, X.read_status,
                      X.read_n_substrings, X.entry_first, X.entry_read, X.entry_off, X.entry_len, X.pool};
        for (void *p : ps) free(p);
    }
    free(res);
}

}  // namespace

/* One extraction taken through steps (mrp_internal.h): everything the queued work reads or writes until the stream has drained -- the
 * windows, the staging block, the device arrays, the events -- and the allele strings made beside the first half.  The destructor
 * drains the stream before the buffers go back to the pool; whoever ran it reclaims the pool afterwards. */
struct mrp_extract_run {
    const char *const who;
    const int64_t n_chunks;
    const mrp_aligned_chunk *const chunks;
    const mrp_extract_options *const options;
    mrp_extract_stats *const stats;
    const double t_begin;
    mrp_extract_options o{};
    std::vector<std::vector<ExWindow>> win;
    std::vector<int64_t> aligned;
    std::vector<int64_t> rb, vb, cb, sb; /* n_chunks + 1: chunk c's share of the call's reads, variants, CIGAR words, packed bases */
    int64_t n_reads = 0, n_var = 0, n_ops = 0, n_seq = 0, n_ent = 0, n_bases = 0;
    size_t o_cig = 0, o_read = 0, o_chunk = 0, o_var = 0, o_vorig = 0, o_seq = 0, in_bytes = 0;
    bool split = false; /* check_modes: the walk runs per class of variant (indelSizeForSVHandling > 0 on a context that admits it) */
    mrp_context *ctx = nullptr;
    hipStream_t s = nullptr; /* set once the device is current: from then on the destructor drains it */
    DevBuf<uint8_t> d_in, d_status, d_pool;
    DevBuf<ExOp> d_ops;
    DevBuf<ExState> d_state;
    DevBuf<int64_t> d_count, d_eoff, d_vcnt, d_vfirst, d_vfill, d_flen, d_foff;
    DevBuf<unsigned long long> d_tot;
    DevBuf<ExEntry> d_entries;
    DevBuf<int32_t> d_bucket, d_order, d_fread;
    uint8_t *g_pool = nullptr; /* where the gather wrote: d_pool, or the caller's pool + its base */
    PinnedBuf h_in, h_back;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    double t_dev0 = 0, t_dev2 = 0, t_end = 0;
    /* the allele strings (prefix + allele + suffix), symbols, per chunk */
    std::vector<HostVec<uint8_t>> apool;
    std::vector<std::vector<int64_t>> aoff;

    mrp_extract_run(const char *w, int64_t n, const mrp_aligned_chunk *c, const mrp_extract_options *op, mrp_extract_stats *st)
        : who(w), n_chunks(n), chunks(c), options(op), stats(st), t_begin(ex_now_ms()) {
        if (stats) memset(stats, 0, sizeof(*stats));
    }
    ~mrp_extract_run() {
        if (s) (void) hipStreamSynchronize(s);
        for (hipEvent_t x : ev)
            if (x) (void) hipEventDestroy(x);
    }
    void bind(DevPool *pl) {
        d_in.pool = d_status.pool = d_pool.pool = pl;
        d_ops.pool = pl;
        d_state.pool = pl;
        d_count.pool = d_eoff.pool = d_vcnt.pool = d_vfirst.pool = d_vfill.pool = d_flen.pool = d_foff.pool = pl;
        d_tot.pool = pl;
        d_entries.pool = pl;
        d_bucket.pool = d_order.pool = d_fread.pool = pl;
    }
};

mrp_extract_run *mrp_extract_run_create(const char *who, int64_t n_chunks, const mrp_aligned_chunk *chunks, const mrp_extract_options *options,
                                        mrp_extract_stats *stats) {
    return new (std::nothrow) mrp_extract_run(who, n_chunks, chunks, options, stats);
}

void mrp_extract_run_destroy(mrp_extract_run *R) { delete R; }

int mrp_extract_run_check_args(mrp_extract_run *R, bool have_out) {
    if (R->n_chunks < 0 || (R->n_chunks > 0 && !R->chunks) || !R->options || !have_out) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", R->who);
    R->o = *R->options;
    if (R->o.expansion_small < 0 || R->o.expansion_sv < 0) return mrp_set_error(MRP_ERR_ARG, "%s: negative reference expansion", R->who);
    return MRP_OK;
}

int mrp_extract_run_check_modes(mrp_extract_run *R, int sv_split) {
    /* only the sign is read: the threshold was applied when is_sv was made (mrp_mark_structural_variants) */
    R->split = sv_split && R->o.indel_size_for_sv_handling > 0;
    if (R->o.indel_size_for_sv_handling != 0 && !R->split)
        return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: indelSizeForSVHandling > 0 (htsIntegration.c:1724-1755) is not supported", R->who);
    if (R->o.use_run_length_encoding != 0) return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: run-length encoding is not supported", R->who);
    return MRP_OK;
}

/* the chunks' own checks, and the windows */
int mrp_extract_run_check_chunks(mrp_extract_run *R) {
    const int64_t n_chunks = R->n_chunks;
    R->win.resize((size_t) n_chunks);
    R->aligned.assign((size_t) n_chunks, 0);
    std::vector<int> rcs((size_t) n_chunks, MRP_OK);
    std::vector<std::string> msgs((size_t) n_chunks);
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) { rcs[(size_t) c] = ex_check_chunk(R->chunks[c], R->o, R->win[(size_t) c], R->aligned[(size_t) c], msgs[(size_t) c]); });
    for (int64_t c = 0; c < n_chunks; c++)
        if (rcs[(size_t) c] != MRP_OK) return mrp_set_error(rcs[(size_t) c], "%s: chunk %lld: %s", R->who, (long long) c, msgs[(size_t) c].c_str());
    return MRP_OK;
}

/* the call's reads, ops, bases and variants in one staging buffer, and its upload */
int mrp_extract_run_stage(mrp_extract_run *R, mrp_context *ctx) {
    const char *who = R->who;
    const int64_t n_chunks = R->n_chunks;
    const mrp_aligned_chunk *chunks = R->chunks;
    std::vector<int64_t> &rb = R->rb, &vb = R->vb, &cb = R->cb, &sb = R->sb;
    rb.assign((size_t) n_chunks + 1, 0); vb.assign((size_t) n_chunks + 1, 0); cb.assign((size_t) n_chunks + 1, 0); sb.assign((size_t) n_chunks + 1, 0);
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_aligned_chunk &C = chunks[c];
        rb[(size_t) c + 1] = rb[(size_t) c] + C.n_reads;
        vb[(size_t) c + 1] = vb[(size_t) c] + C.n_variants;
        cb[(size_t) c + 1] = cb[(size_t) c] + (C.n_reads ? C.cigar_first[C.n_reads] : 0);
        sb[(size_t) c + 1] = sb[(size_t) c] + (C.n_reads ? C.seq_first[C.n_reads] : 0);
    }
    const int64_t n_reads = R->n_reads = rb[(size_t) n_chunks], n_var = R->n_var = vb[(size_t) n_chunks], n_ops = R->n_ops = cb[(size_t) n_chunks],
                  n_seq = R->n_seq = sb[(size_t) n_chunks];
    if (n_reads >= (1ll << 31) || n_var >= (1ll << 31)) return mrp_set_error(MRP_ERR_ARG, "%s: more than 2^31 reads or variants in one call", who);
    size_t at = 0;
    const size_t o_cig = R->o_cig = at; at = ex_align<ExRead>(at + sizeof(uint32_t) * (size_t) n_ops);
    const size_t o_read = R->o_read = at; at = ex_align<ExChunk>(at + sizeof(ExRead) * (size_t) n_reads);
    const size_t o_chunk = R->o_chunk = at; at = ex_align<ExVar>(at + sizeof(ExChunk) * (size_t) n_chunks);
    const size_t o_var = R->o_var = at; at += sizeof(ExVar) * (size_t) n_var;
    const bool split = R->split;
    const size_t o_vorig = R->o_vorig = at; at += split ? sizeof(int32_t) * (size_t) n_var : 0; /* (then bytes: no alignment to keep) */
    const size_t o_seq = R->o_seq = at; at += (size_t) n_seq;
    const size_t in_bytes = R->in_bytes = at;

    EX_HIP(hipSetDevice(ctx->device));
    R->ctx = ctx;
    R->bind(&ctx->pool);
    hipStream_t s = R->s = ctx->stream;
    for (hipEvent_t &x : R->ev) EX_HIP(hipEventCreate(&x));

    EX_HIP(R->h_in.reserve(std::max<size_t>(in_bytes, 1)));
    uint8_t *hin = (uint8_t *) R->h_in.p;
    ExChunk *hch = (ExChunk *) (hin + o_chunk);
    const std::vector<std::vector<ExWindow>> &win = R->win;
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) {
        const mrp_aligned_chunk &C = chunks[c];
        ExVar *hv = (ExVar *) (hin + o_var) + vb[(size_t) c];
        int64_t n_small = C.n_variants;
        if (!split) {
            for (int64_t v = 0; v < C.n_variants; v++) hv[v] = ExVar{C.variant_pos[v], win[(size_t) c][(size_t) v].start, win[(size_t) c][(size_t) v].stop};
        } else { /* class-major, each class ascending as the caller's list is (:1727-1732) */
            int32_t *ho = (int32_t *) (hin + o_vorig) + vb[(size_t) c];
            int64_t k = 0;
            for (int cls = 0; cls < 2; cls++) {
                for (int64_t v = 0; v < C.n_variants; v++) {
                    if ((C.is_sv[v] != 0) != (cls != 0)) continue;
                    hv[k] = ExVar{C.variant_pos[v], win[(size_t) c][(size_t) v].start, win[(size_t) c][(size_t) v].stop};
                    ho[k] = (int32_t) (vb[(size_t) c] + v);
                    k++;
                }
                if (cls == 0) n_small = k;
            }
        }
        hch[c] = ExChunk{C.overlap_start, C.chunk_start, C.chunk_end, vb[(size_t) c], C.n_variants, n_small};
        ExRead *hr = (ExRead *) (hin + o_read) + rb[(size_t) c];
        for (int64_t r = 0; r < C.n_reads; r++) {
            ExRead &x = hr[r];
            x.pos = C.pos[r];
            x.cig = cb[(size_t) c] + C.cigar_first[r];
            x.seq_nib = 2 * (sb[(size_t) c] + C.seq_first[r]);
            x.n_cig = (int32_t) (C.cigar_first[r + 1] - C.cigar_first[r]);
            x.l_qseq = C.l_qseq[r];
            x.chunk = (int32_t) c;
            x.flag = C.flag[r];
            x.mapq = C.mapq[r];
            x.pad = 0;
        }
        if (C.n_reads) {
            if (C.cigar_first[C.n_reads]) memcpy(hin + o_cig + sizeof(uint32_t) * (size_t) cb[(size_t) c], C.cigar, sizeof(uint32_t) * (size_t) C.cigar_first[C.n_reads]);
            if (C.seq_first[C.n_reads]) memcpy(hin + o_seq + (size_t) sb[(size_t) c], C.seq, (size_t) C.seq_first[C.n_reads]);
        }
    });
    EX_HIP(R->d_in.alloc(in_bytes));
    if (in_bytes) EX_HIP(hipMemcpyAsync(R->d_in.p, hin, in_bytes, hipMemcpyHostToDevice, s));
    if (R->stats) EX_HIP(hipStreamSynchronize(s)); /* kernel_ms must not contain the tail of the upload */
    R->t_dev0 = ex_now_ms();
    return MRP_OK;
}

/* first half: scan, count, scan of the counts; one total (the substrings and their bases) starts on its way back */
int mrp_extract_run_first_half(mrp_extract_run *R) {
    hipStream_t s = R->s;
    const int64_t n_reads = R->n_reads;
    const uint32_t *g_cig = (const uint32_t *) (R->d_in.p + R->o_cig);
    const ExRead *g_read = (const ExRead *) (R->d_in.p + R->o_read);
    const ExChunk *g_chunk = (const ExChunk *) (R->d_in.p + R->o_chunk);
    const ExVar *g_var = (const ExVar *) (R->d_in.p + R->o_var);
    const ExOpt eo{R->o.min_mapq, R->o.include_secondary, R->o.include_supplementary};
    EX_HIP(R->d_status.alloc((size_t) n_reads));
    EX_HIP(R->d_ops.alloc((size_t) R->n_ops));
    EX_HIP(R->d_state.alloc((size_t) n_reads));
    EX_HIP(R->d_count.alloc((size_t) n_reads));
    EX_HIP(R->d_eoff.alloc((size_t) n_reads + 1));
    EX_HIP(R->d_tot.alloc(1));
    EX_HIP(R->h_back.reserve(64));
    EX_HIP(hipEventRecord(R->ev[0], s));
    EX_HIP(hipMemsetAsync(R->d_tot.p, 0, sizeof(unsigned long long), s));
    if (n_reads > 0) {
        const int32_t *g_vorig = R->split ? (const int32_t *) (R->d_in.p + R->o_vorig) : nullptr;
        const auto scan = R->split ? ex_scan_kernel<2> : ex_scan_kernel<1>;
        const auto locate = R->split ? ex_locate_kernel<false, 2> : ex_locate_kernel<false, 1>;
        hipLaunchKernelGGL(scan, dim3((unsigned) n_reads), dim3(EX_WAVE), 0, s, g_read, g_cig, g_chunk, g_var, eo,
                           R->d_ops.p, R->d_state.p, R->d_status.p);
        EX_HIP(hipGetLastError());
        hipLaunchKernelGGL(locate, dim3((unsigned) n_reads), dim3(EX_WAVE), 0, s, g_read, R->d_status.p,
                           R->d_state.p, R->d_ops.p, g_chunk, g_var, g_vorig, R->d_count.p, R->d_tot.p, (const int64_t *) nullptr, (ExEntry *) nullptr);
        EX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ex_scan_i64, dim3(1), dim3(1024), 0, s, R->d_count.p, n_reads, R->d_eoff.p);
    EX_HIP(hipGetLastError());
    EX_HIP(hipEventRecord(R->ev[1], s));
    int64_t *hb = (int64_t *) R->h_back.p;
    EX_HIP(hipMemcpyAsync(hb, R->d_eoff.p + n_reads, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    EX_HIP(hipMemcpyAsync(hb + 1, R->d_tot.p, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    return MRP_OK;
}

/* beside the first half: the allele strings on the worker pool; then the total the second half is sized by */
int mrp_extract_run_totals(mrp_extract_run *R, int64_t *n_entries, int64_t *n_bases) {
    const int64_t n_chunks = R->n_chunks;
    const mrp_aligned_chunk *chunks = R->chunks;
    R->apool.resize((size_t) n_chunks);
    R->aoff.resize((size_t) n_chunks);
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) {
        const mrp_aligned_chunk &C = chunks[c];
        const std::vector<ExWindow> &win = R->win[(size_t) c];
        const int64_t na = C.n_variants ? C.allele_first[C.n_variants] : 0;
        std::vector<int64_t> &off = R->aoff[(size_t) c];
        off.assign((size_t) na + 1, 0);
        for (int64_t v = 0; v < C.n_variants; v++) {
            const ExWindow &w = win[(size_t) v];
            for (int64_t a = C.allele_first[v]; a < C.allele_first[v + 1]; a++) off[(size_t) a + 1] = w.pre_len + C.allele_len[a] + w.suf_len;
        }
        for (int64_t a = 0; a < na; a++) off[(size_t) a + 1] += off[(size_t) a];
        HostVec<uint8_t> &p = R->apool[(size_t) c];
        p.resize((size_t) off[(size_t) na]);
        for (int64_t v = 0; v < C.n_variants; v++) {
            const ExWindow &w = win[(size_t) v];
            for (int64_t a = C.allele_first[v]; a < C.allele_first[v + 1]; a++) {
                uint8_t *d = p.data() + off[(size_t) a];
                for (int64_t i = 0; i < w.pre_len; i++) *d++ = ex_symbol(C.reference[w.pre_at + i]);
                for (int32_t i = 0; i < C.allele_len[a]; i++) *d++ = ex_symbol(C.allele_chars[C.allele_off[a] + i]);
                for (int64_t i = 0; i < w.suf_len; i++) *d++ = ex_symbol(C.reference[w.suf_at + i]);
            }
        }
    });
    EX_HIP(hipStreamSynchronize(R->s));
    const int64_t *hb = (const int64_t *) R->h_back.p;
    R->n_ent = hb[0];
    R->n_bases = hb[1];
    if (R->n_ent >= (1ll << 31)) return mrp_set_error(MRP_ERR_UNSUPPORTED, "%s: more than 2^31 substrings in one call", R->who);
    if (n_entries) *n_entries = R->n_ent;
    if (n_bases) *n_bases = R->n_bases;
    return MRP_OK;
}

/* second half: write the substrings, sort them by entry, gather their bases -- into pool + base (a device pool of the caller's, with
 * room for the total's bases behind base), or with pool NULL into a pool of the run's own */
int mrp_extract_run_second_half(mrp_extract_run *R, uint8_t *pool, int64_t base) {
    hipStream_t s = R->s;
    const int64_t n_reads = R->n_reads, n_var = R->n_var, n_ent = R->n_ent;
    const ExRead *g_read = (const ExRead *) (R->d_in.p + R->o_read);
    const ExChunk *g_chunk = (const ExChunk *) (R->d_in.p + R->o_chunk);
    const ExVar *g_var = (const ExVar *) (R->d_in.p + R->o_var);
    const uint8_t *g_seq = R->d_in.p + R->o_seq;
    EX_HIP(R->d_entries.alloc((size_t) n_ent));
    EX_HIP(R->d_vcnt.alloc((size_t) n_var));
    EX_HIP(R->d_vfill.alloc((size_t) n_var));
    EX_HIP(R->d_vfirst.alloc((size_t) n_var + 1));
    EX_HIP(R->d_bucket.alloc((size_t) n_ent));
    EX_HIP(R->d_order.alloc((size_t) n_ent));
    EX_HIP(R->d_fread.alloc((size_t) n_ent));
    EX_HIP(R->d_flen.alloc((size_t) n_ent));
    EX_HIP(R->d_foff.alloc((size_t) n_ent + 1));
    if (!pool) {
        EX_HIP(R->d_pool.alloc((size_t) R->n_bases));
        pool = R->d_pool.p;
        base = 0;
    }
    R->g_pool = pool + base;
    EX_HIP(hipEventRecord(R->ev[2], s));
    if (n_var > 0) {
        EX_HIP(hipMemsetAsync(R->d_vcnt.p, 0, sizeof(int64_t) * (size_t) n_var, s));
        EX_HIP(hipMemsetAsync(R->d_vfill.p, 0, sizeof(int64_t) * (size_t) n_var, s));
    }
    if (n_ent > 0) {
        const int32_t *g_vorig = R->split ? (const int32_t *) (R->d_in.p + R->o_vorig) : nullptr;
        const auto locate = R->split ? ex_locate_kernel<true, 2> : ex_locate_kernel<true, 1>;
        hipLaunchKernelGGL(locate, dim3((unsigned) n_reads), dim3(EX_WAVE), 0, s, g_read, R->d_status.p,
                           R->d_state.p, R->d_ops.p, g_chunk, g_var, g_vorig, (int64_t *) nullptr, (unsigned long long *) nullptr, R->d_eoff.p, R->d_entries.p);
        EX_HIP(hipGetLastError());
        const unsigned blocks = (unsigned) ((n_ent + 255) / 256);
        hipLaunchKernelGGL(ex_var_count_kernel, dim3(blocks), dim3(256), 0, s, R->d_entries.p, n_ent, (unsigned long long *) R->d_vcnt.p);
        EX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ex_scan_i64, dim3(1), dim3(1024), 0, s, R->d_vcnt.p, n_var, R->d_vfirst.p);
    EX_HIP(hipGetLastError());
    if (n_ent > 0) {
        const unsigned blocks = (unsigned) ((n_ent + 255) / 256);
        hipLaunchKernelGGL(ex_bucket_kernel, dim3(blocks), dim3(256), 0, s, R->d_entries.p, n_ent, R->d_vfirst.p, (unsigned long long *) R->d_vfill.p, R->d_bucket.p);
        EX_HIP(hipGetLastError());
        hipLaunchKernelGGL(ex_rank_kernel, dim3((unsigned) std::min<int64_t>(n_var, 65536)), dim3(EX_WAVE), 0, s, R->d_vfirst.p, n_var, R->d_bucket.p, R->d_entries.p,
                           R->d_order.p, R->d_flen.p);
        EX_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(ex_scan_i64, dim3(1), dim3(1024), 0, s, R->d_flen.p, n_ent, R->d_foff.p);
    EX_HIP(hipGetLastError());
    if (n_ent > 0) {
        hipLaunchKernelGGL(ex_gather_kernel, dim3((unsigned) std::min<int64_t>(n_ent, 65536)), dim3(EX_WAVE), 0, s, R->d_order.p, n_ent, R->d_entries.p, R->d_foff.p,
                           g_seq, pool, base, R->d_fread.p);
        EX_HIP(hipGetLastError());
    }
    EX_HIP(hipEventRecord(R->ev[3], s));
    R->t_dev2 = R->t_end = ex_now_ms();
    return MRP_OK;
}

/* what the second half left on the device (valid until the run is destroyed) */
void mrp_extract_run_device(const mrp_extract_run *R, mrp_extract_device *D) {
    D->n_reads = R->n_reads;
    D->n_variants = R->n_var;
    D->n_entries = R->n_ent;
    D->n_bases = R->n_bases;
    D->read_status = R->d_status.p;
    D->entry_first = R->d_vfirst.p;
    D->entry_read = R->d_fread.p;
    D->entry_len = R->d_flen.p;
    D->entry_off = R->d_foff.p;
    D->symbols = R->g_pool;
    D->read_entry_first = R->d_eoff.p;
    static_assert(sizeof(ExState) % sizeof(int64_t) == 0 && offsetof(ExState, limit) % sizeof(int64_t) == 0, "the limit is read as a strided int64 array");
    D->read_limit = (const int64_t *) ((const uint8_t *) R->d_state.p + offsetof(ExState, limit));
    D->read_limit_stride = (int64_t) (sizeof(ExState) / sizeof(int64_t));
    D->read_first = R->rb.data();
    D->variant_first = R->vb.data();
}

int64_t mrp_extract_run_allele_bytes(const mrp_extract_run *R) {
    int64_t n = 0;
    for (const HostVec<uint8_t> &p : R->apool) n += (int64_t) p.size();
    return n;
}

/* every chunk's allele strings one after the other into dst (mrp_extract_run_allele_bytes), and per allele of the call, in chunk
 * then allele order, where its string lies in dst */
void mrp_extract_run_alleles(const mrp_extract_run *R, uint8_t *dst, int64_t *allele_off, int32_t *allele_len) {
    int64_t at = 0, ia = 0;
    for (int64_t c = 0; c < R->n_chunks; c++) {
        const std::vector<int64_t> &off = R->aoff[(size_t) c];
        const HostVec<uint8_t> &p = R->apool[(size_t) c];
        if (!p.empty()) memcpy(dst + at, p.data(), p.size());
        for (size_t a = 0; a + 1 < off.size(); a++, ia++) {
            allele_off[ia] = at + off[a];
            allele_len[ia] = (int32_t) (off[a + 1] - off[a]);
        }
        at += (int64_t) p.size();
    }
}

/* the events of the two halves and the counts; after the stream has drained.  total_ms ends where the second half was queued
 * (a run that stops there) or where the download ended */
int mrp_extract_run_stats(mrp_extract_run *R) {
    mrp_extract_stats *stats = R->stats;
    if (!stats) return MRP_OK;
    float a = 0.f, b = 0.f;
    EX_HIP(hipEventElapsedTime(&a, R->ev[0], R->ev[1]));
    EX_HIP(hipEventElapsedTime(&b, R->ev[2], R->ev[3]));
    stats->kernel_ms = (double) a + (double) b;
    stats->bytes_uploaded = (int64_t) R->in_bytes;
    stats->reads = R->n_reads;
    stats->cigar_ops = R->n_ops;
    for (int64_t c = 0; c < R->n_chunks; c++) stats->aligned_bases += R->aligned[(size_t) c];
    stats->entries = R->n_ent;
    return MRP_OK;
}

/* download and the per-chunk outputs */
int mrp_extract_run_download(mrp_extract_run *R, mrp_extracted_chunk **out) {
    const char *who = R->who;
    hipStream_t s = R->s;
    const int64_t n_chunks = R->n_chunks, n_reads = R->n_reads, n_var = R->n_var, n_ent = R->n_ent, n_bases = R->n_bases;
    const mrp_aligned_chunk *chunks = R->chunks;
    const std::vector<int64_t> &rb = R->rb, &vb = R->vb;
    /* back: per read status and count (the scan of the counts), per entry its variant CSR, read, length, pool offset, and the pool */
    const size_t b_status = 0, b_eoff = ex_align<int64_t>((size_t) n_reads), b_vfirst = b_eoff + 8 * ((size_t) n_reads + 1),
                 b_foff = b_vfirst + 8 * ((size_t) n_var + 1), b_flen = b_foff + 8 * ((size_t) n_ent + 1), b_fread = b_flen + 8 * (size_t) n_ent,
                 b_pool = b_fread + 4 * (size_t) n_ent, b_end = b_pool + (size_t) n_bases;
    EX_HIP(R->h_back.reserve(b_end));
    uint8_t *hk = (uint8_t *) R->h_back.p;
    if (n_reads) EX_HIP(hipMemcpyAsync(hk + b_status, R->d_status.p, (size_t) n_reads, hipMemcpyDeviceToHost, s));
    EX_HIP(hipMemcpyAsync(hk + b_eoff, R->d_eoff.p, 8 * ((size_t) n_reads + 1), hipMemcpyDeviceToHost, s));
    EX_HIP(hipMemcpyAsync(hk + b_vfirst, R->d_vfirst.p, 8 * ((size_t) n_var + 1), hipMemcpyDeviceToHost, s));
    EX_HIP(hipMemcpyAsync(hk + b_foff, R->d_foff.p, 8 * ((size_t) n_ent + 1), hipMemcpyDeviceToHost, s));
    if (n_ent) {
        EX_HIP(hipMemcpyAsync(hk + b_flen, R->d_flen.p, 8 * (size_t) n_ent, hipMemcpyDeviceToHost, s));
        EX_HIP(hipMemcpyAsync(hk + b_fread, R->d_fread.p, 4 * (size_t) n_ent, hipMemcpyDeviceToHost, s));
    }
    if (n_bases) EX_HIP(hipMemcpyAsync(hk + b_pool, R->g_pool, (size_t) n_bases, hipMemcpyDeviceToHost, s));
    EX_HIP(hipStreamSynchronize(s));
    R->t_dev2 = ex_now_ms();
    const uint8_t *k_status = hk + b_status;
    const int64_t *k_eoff = (const int64_t *) (hk + b_eoff), *k_vfirst = (const int64_t *) (hk + b_vfirst), *k_foff = (const int64_t *) (hk + b_foff),
                  *k_flen = (const int64_t *) (hk + b_flen);
    const int32_t *k_fread = (const int32_t *) (hk + b_fread);
    const uint8_t *k_pool = hk + b_pool;

    mrp_extracted_chunk *res = (mrp_extracted_chunk *) calloc((size_t) std::max<int64_t>(n_chunks, 1), sizeof(mrp_extracted_chunk));
    if (!res) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    std::atomic<bool> nomem{false};
    mrp_parallel_for(n_chunks, 1, [&](int64_t c) {
        const mrp_aligned_chunk &C = chunks[c];
        const std::vector<ExWindow> &win = R->win[(size_t) c];
        const std::vector<int64_t> &aoff = R->aoff[(size_t) c];
        mrp_extracted_chunk &X = res[c];
        const int64_t nv = C.n_variants, nr = C.n_reads, na = nv ? C.allele_first[nv] : 0;
        const int64_t e0 = k_vfirst[vb[(size_t) c]], e1 = k_vfirst[vb[(size_t) c + 1]], ne = e1 - e0;
        const int64_t abytes = aoff[(size_t) na], sbytes = k_foff[e1] - k_foff[e0];
        auto mk = [&](size_t bytes) { void *p = malloc(bytes ? bytes : 1); if (!p) nomem = true; return p; };
        X.n_variants = nv;
        X.n_reads = nr;
        X.ref_aln_start = (int64_t *) mk(8 * (size_t) nv);
        X.ref_aln_stop_incl = (int64_t *) mk(8 * (size_t) nv);
        X.allele_first = (int64_t *) mk(8 * ((size_t) nv + 1));
        X.allele_off = (int64_t *) mk(8 * (size_t) na);
        X.allele_len = (int32_t *) mk(4 * (size_t) na);
        X.read_status = (uint8_t *) mk((size_t) nr);
        X.read_n_substrings = (int32_t *) mk(4 * (size_t) nr);
        X.entry_first = (int64_t *) mk(8 * ((size_t) nv + 1));
        X.entry_read = (int32_t *) mk(4 * (size_t) ne);
        X.entry_off = (int64_t *) mk(8 * (size_t) ne);
        X.entry_len = (int32_t *) mk(4 * (size_t) ne);
        X.pool_bytes = abytes + sbytes;
        X.pool = (uint8_t *) mk((size_t) X.pool_bytes);
        if (nomem) return;
        for (int64_t v = 0; v < nv; v++) {
            X.ref_aln_start[v] = win[(size_t) v].start;
            X.ref_aln_stop_incl[v] = win[(size_t) v].stop;
            X.entry_first[v] = k_vfirst[vb[(size_t) c] + v] - e0;
        }
        X.entry_first[nv] = ne;
        if (nv) memcpy(X.allele_first, C.allele_first, 8 * ((size_t) nv + 1));
        else X.allele_first[0] = 0;
        for (int64_t a = 0; a < na; a++) {
            X.allele_off[a] = aoff[(size_t) a];
            X.allele_len[a] = (int32_t) (aoff[(size_t) a + 1] - aoff[(size_t) a]);
        }
        for (int64_t r = 0; r < nr; r++) {
            const int64_t g = rb[(size_t) c] + r;
            X.read_status[r] = k_status[g];
            X.read_n_substrings[r] = (int32_t) (k_eoff[g + 1] - k_eoff[g]);
        }
        for (int64_t e = 0; e < ne; e++) {
            X.entry_read[e] = (int32_t) (k_fread[e0 + e] - rb[(size_t) c]);
            X.entry_off[e] = abytes + k_foff[e0 + e] - k_foff[e0];
            X.entry_len[e] = (int32_t) k_flen[e0 + e];
        }
        if (abytes) memcpy(X.pool, R->apool[(size_t) c].data(), (size_t) abytes);
        if (sbytes) memcpy(X.pool + abytes, k_pool + k_foff[e0], (size_t) sbytes);
    });
    if (nomem) {
        ex_free_chunks(res, n_chunks);
        return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    }
    *out = res;
    return MRP_OK;
}

/* after the stream has drained: every device array back to the context's pool, at once reusable */
void mrp_extract_run_release(mrp_extract_run *R) {
    R->d_in.release(); R->d_status.release(); R->d_pool.release(); R->d_ops.release(); R->d_state.release(); R->d_count.release(); R->d_eoff.release();
    R->d_vcnt.release(); R->d_vfirst.release(); R->d_vfill.release(); R->d_flen.release(); R->d_foff.release(); R->d_tot.release(); R->d_entries.release();
    R->d_bucket.release(); R->d_order.release(); R->d_fread.release();
    R->g_pool = nullptr;
    if (R->ctx) R->ctx->pool.reclaim();
}

/* total_ms and host_ms of a run that has ended (t_end: now, or where the second half was queued) */
void mrp_extract_run_times(mrp_extract_run *R, bool to_now) {
    if (!R->stats) return;
    R->stats->total_ms = (to_now ? ex_now_ms() : R->t_end) - R->t_begin;
    R->stats->host_ms = R->stats->total_ms - (R->t_dev2 - R->t_dev0);
}

extern "C" {

/* vcf.c:173-185: an entry is structural if any of its alleles is longer than indelSizeForSVHandling, and none is at a threshold <= 0 */
int mrp_mark_structural_variants(const mrp_aligned_chunk *chunk, int64_t indel_size, uint8_t *is_sv_out) {
    static const char *who = "mrp_mark_structural_variants";
    if (!chunk || chunk->n_variants < 0 || (chunk->n_variants > 0 && (!is_sv_out || !chunk->allele_first || !chunk->allele_len)))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    for (int64_t v = 0; v < chunk->n_variants; v++) {
        if (chunk->allele_first[v] < 0 || chunk->allele_first[v + 1] < chunk->allele_first[v])
            return mrp_set_error(MRP_ERR_ARG, "%s: allele offsets not ascending at variant %lld", who, (long long) v);
        uint8_t sv = 0;
        for (int64_t a = chunk->allele_first[v]; a < chunk->allele_first[v + 1]; a++) sv |= indel_size > 0 && (int64_t) chunk->allele_len[a] > indel_size;
        is_sv_out[v] = sv;
    }
    return MRP_OK;
}

int mrp_extract_read_substrings(mrp_context *ctx, int64_t n_chunks, const mrp_aligned_chunk *chunks, const mrp_extract_options *options,
                                mrp_extracted_chunk **out, mrp_extract_stats *stats) {
    mrp_extract_run run("mrp_extract_read_substrings", n_chunks, chunks, options, stats);
    mrp_extract_run *R = &run;
    int rc = mrp_extract_run_check_args(R, out != nullptr);
    if (rc == MRP_OK) rc = mrp_extract_run_check_modes(R, ctx ? ctx->sv_split : 0); /* (a NULL context counts as off) */
    if (rc == MRP_OK) rc = mrp_extract_run_check_chunks(R);
    if (rc != MRP_OK) return rc;
    if (!ctx) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no context (the extraction has no CPU fallback)", R->who);
    *out = nullptr;
    mrp_extracted_chunk *res = nullptr;
    rc = mrp_extract_run_stage(R, ctx);
    if (rc == MRP_OK) rc = mrp_extract_run_first_half(R);
    if (rc == MRP_OK) rc = mrp_extract_run_totals(R, nullptr, nullptr);
    if (rc == MRP_OK) rc = mrp_extract_run_second_half(R, nullptr, 0);
    if (rc == MRP_OK) rc = mrp_extract_run_download(R, &res);
    if (rc == MRP_OK) rc = mrp_extract_run_stats(R);
    if (rc != MRP_OK) { /* (nothing is returned on error) */
        ex_free_chunks(res, n_chunks);
        return rc;
    }
    mrp_extract_run_release(R);
    *out = res;
    mrp_extract_run_times(R, true);
    return MRP_OK;
}

int mrp_string_chunk_from_extracted(const mrp_extracted_chunk *x, const uint8_t *keep, const char *const *read_names,
                                    const uint8_t *read_forward_strand, mrp_string_chunk *out, int64_t **bubble_variant) {
    static const char *who = "mrp_string_chunk_from_extracted";
    if (!x || !out || !bubble_variant || x->n_variants < 0 || x->n_reads < 0) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (x->n_reads > 0 && (!read_names || !read_forward_strand || !x->read_status)) return mrp_set_error(MRP_ERR_ARG, "%s: null read array", who);
    if (!x->allele_first || !x->entry_first || (x->n_variants > 0 && (!x->entry_read || !x->entry_off || !x->entry_len || !x->allele_off || !x->allele_len)))
        return mrp_set_error(MRP_ERR_ARG, "%s: null array", who);
    const int64_t nv = x->n_variants;
    auto use = [&](int64_t e) {
        const int32_t r = x->entry_read[e];
        return r >= 0 && r < x->n_reads && x->read_status[r] == MRP_READ_KEPT && (!keep || keep[r]);
    };
    for (int64_t e = 0; e < x->entry_first[nv]; e++)
        if (x->entry_read[e] < 0 || x->entry_read[e] >= x->n_reads) return mrp_set_error(MRP_ERR_ARG, "%s: entry %lld names read %d", who, (long long) e, x->entry_read[e]);
    int64_t nb = 0, na = 0, ns = 0;
    for (int64_t v = 0; v < nv; v++) {
        int64_t k = 0;
        for (int64_t e = x->entry_first[v]; e < x->entry_first[v + 1]; e++) k += use(e);
        if (!k) continue; /* :1366-1371 nothing to phase with */
        nb++;
        na += x->allele_first[v + 1] - x->allele_first[v];
        ns += k;
    }
    /* one block: allele_first, sub_first, bubble_variant (nb + 1 each), allele_off (na), sub_off (ns), then the int32 arrays */
    const size_t n64 = 3 * ((size_t) nb + 1) + (size_t) na + (size_t) ns, n32 = (size_t) na + 2 * (size_t) ns;
    uint8_t *blk = (uint8_t *) malloc(8 * n64 + 4 * n32 + 8);
    if (!blk) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    int64_t *a_first = (int64_t *) blk, *s_first = a_first + nb + 1, *bv = s_first + nb + 1, *a_off = bv + nb + 1, *s_off = a_off + na;
    int32_t *a_len = (int32_t *) (s_off + ns), *s_len = a_len + na, *s_read = s_len + ns;
    int64_t b = 0, ia = 0, is = 0;
    a_first[0] = s_first[0] = 0;
    for (int64_t v = 0; v < nv; v++) {
        int64_t k = 0;
        for (int64_t e = x->entry_first[v]; e < x->entry_first[v + 1]; e++) k += use(e);
        if (!k) continue;
        for (int64_t a = x->allele_first[v]; a < x->allele_first[v + 1]; a++, ia++) {
            a_off[ia] = x->allele_off[a];
            a_len[ia] = x->allele_len[a];
        }
        for (int64_t e = x->entry_first[v + 1] - 1; e >= x->entry_first[v]; e--) /* :1391-1393 b->reads[j] = stList_pop */
            if (use(e)) {
                s_off[is] = x->entry_off[e];
                s_len[is] = x->entry_len[e];
                s_read[is] = x->entry_read[e];
                is++;
            }
        bv[b] = v;
        b++;
        a_first[b] = ia;
        s_first[b] = is;
    }
    memset(out, 0, sizeof(*out));
    out->n_bubbles = nb;
    out->n_reads = x->n_reads;
    out->pool = x->pool;
    out->pool_bytes = x->pool_bytes;
    out->allele_first = a_first;
    out->allele_off = a_off;
    out->allele_len = a_len;
    out->sub_first = s_first;
    out->sub_off = s_off;
    out->sub_len = s_len;
    out->sub_read = s_read;
    out->read_names = read_names;
    out->read_forward_strand = read_forward_strand;
    *bubble_variant = bv;
    return MRP_OK;
}

int mrp_string_chunk_rest_from_extracted(const mrp_extracted_chunk *x, const uint8_t *keep, const uint8_t *read_forward_strand,
                                         const int64_t *bubble_variant, int64_t n_bubbles, const mrp_extracted_chunk *xf,
                                         const int64_t *fvariant_pos, const int32_t *gt, int64_t chunk_start, int64_t chunk_end,
                                         mrp_string_chunk_rest *out, int32_t **filtered_read, void **block) {
    static const char *who = "mrp_string_chunk_rest_from_extracted";
    if (!x || !xf || !out || !filtered_read || !block || x->n_variants < 0 || x->n_reads < 0 || xf->n_variants < 0 || n_bubbles < 0 || xf->pool_bytes < 0 ||
        x->pool_bytes < 0)
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    if (xf->n_reads != x->n_reads)
        return mrp_set_error(MRP_ERR_ARG, "%s: the two extractions are over %lld and %lld reads: not the same reads", who, (long long) x->n_reads, (long long) xf->n_reads);
    const int64_t nr = x->n_reads, nv = xf->n_variants;
    if (nr >= (1ll << 30)) return mrp_set_error(MRP_ERR_ARG, "%s: bad sizes", who);
    if (nr > 0 && (!read_forward_strand || !x->read_status || !xf->read_status)) return mrp_set_error(MRP_ERR_ARG, "%s: null read array", who);
    if (!x->entry_first || !xf->entry_first || !xf->allele_first || (n_bubbles > 0 && !bubble_variant) || (nv > 0 && (!fvariant_pos || !gt)))
        return mrp_set_error(MRP_ERR_ARG, "%s: null array", who);
    const int64_t ne = x->entry_first[x->n_variants], nef = xf->entry_first[nv], naf = xf->allele_first[nv];
    if ((ne > 0 && (!x->entry_read || !x->entry_off || !x->entry_len)) || (x->pool_bytes > 0 && !x->pool) || (nef > 0 && (!xf->entry_read || !xf->entry_off || !xf->entry_len)) ||
        (naf > 0 && (!xf->allele_off || !xf->allele_len)) || (xf->pool_bytes > 0 && !xf->pool))
        return mrp_set_error(MRP_ERR_ARG, "%s: null array", who);
    for (int64_t b = 0; b < n_bubbles; b++)
        if (bubble_variant[b] < 0 || bubble_variant[b] >= x->n_variants)
            return mrp_set_error(MRP_ERR_ARG, "%s: bubble %lld names variant %lld of %lld", who, (long long) b, (long long) bubble_variant[b], (long long) x->n_variants);
    for (int64_t e = 0; e < ne; e++)
        if (x->entry_read[e] < 0 || x->entry_read[e] >= nr || x->entry_len[e] < 0 || x->entry_off[e] < 0 || x->entry_off[e] + x->entry_len[e] > x->pool_bytes)
            return mrp_set_error(MRP_ERR_ARG, "%s: entry %lld names read %d or lies outside the pool", who, (long long) e, x->entry_read[e]);
    for (int64_t e = 0; e < nef; e++)
        if (xf->entry_read[e] < 0 || xf->entry_read[e] >= nr)
            return mrp_set_error(MRP_ERR_ARG, "%s: entry %lld at the filtered variants names read %d", who, (long long) e, xf->entry_read[e]);
    for (int64_t v = 0; v < nv; v++) {
        const int64_t k = xf->allele_first[v + 1] - xf->allele_first[v];
        for (int w = 0; w < 2; w++)
            if (gt[2 * v + w] < 0 || gt[2 * v + w] >= k)
                return mrp_set_error(MRP_ERR_ARG, "%s: filtered variant %lld: genotype %d outside its %lld alleles", who, (long long) v, gt[2 * v + w], (long long) k);
    }
    /* the filtered reads: (i) low mapq (htsIntegration.c:1824-1827), (ii) the downsampling's discards (phase.c:364-365,
     * htsIntegration.c:1204-1206), (iii) reads with a substring at a filtered variant only */
    auto primary = [&](int64_t r) { return x->read_status[r] == MRP_READ_KEPT && (!keep || keep[r]); };
    auto kind = [&](int64_t r) {
        if (x->read_status[r] == MRP_READ_FILTERED) return 0;
        if (x->read_status[r] == MRP_READ_KEPT) return primary(r) ? -1 : 1;
        return xf->read_status[r] == MRP_READ_KEPT ? 2 : -1;
    };
    int64_t n_kind[3] = {0, 0, 0};
    for (int64_t r = 0; r < nr; r++) {
        const int k = kind(r);
        if (k >= 0) n_kind[k]++;
    }
    const int64_t nf = n_kind[0] + n_kind[1] + n_kind[2];
    memset(out, 0, sizeof(*out));
    *filtered_read = nullptr;
    *block = nullptr;
    if (nf == 0 && nv == 0) return MRP_OK; /* the empty rest */
    /* sizes: the (i) / (ii) substrings at the bubbles, the kept reads' entries at the filtered variants inside the chunk (bubbleGraph.c:2179) */
    auto inside = [&](int64_t v) { return fvariant_pos[v] >= chunk_start && fvariant_pos[v] < chunk_end; };
    int64_t nfs = 0, nve = 0, fs_bytes = 0;
    for (int64_t b = 0; b < n_bubbles; b++)
        for (int64_t e = x->entry_first[bubble_variant[b]]; e < x->entry_first[bubble_variant[b] + 1]; e++) {
            const int k = kind(x->entry_read[e]);
            if (k == 0 || k == 1) { nfs++; fs_bytes += x->entry_len[e]; }
        }
    for (int64_t v = 0; v < nv; v++)
        if (inside(v))
            for (int64_t e = xf->entry_first[v]; e < xf->entry_first[v + 1]; e++) nve += xf->read_status[xf->entry_read[e]] == MRP_READ_KEPT;
    /* one block: int64 fsub_first (n_bubbles + 1), fsub_off (nfs), valle_first, ventry_first (nv + 1 each), valle_off (naf), ventry_off (nve);
     * int32 fsub_len, fsub_read (nfs each), valle_len (naf), gt (2 nv), ventry_read, ventry_len (nve each), filtered_read, the read -> filtered
     * index table (nr, scratch); then forward_strand (nf) and the pool */
    const size_t n64 = (size_t) n_bubbles + 1 + (size_t) nfs + 2 * ((size_t) nv + 1) + (size_t) naf + (size_t) nve;
    const size_t n32 = 2 * (size_t) nfs + (size_t) naf + 2 * (size_t) nv + 2 * (size_t) nve + (size_t) nf + (size_t) nr;
    const int64_t pool_bytes = xf->pool_bytes + fs_bytes;
    uint8_t *blk = (uint8_t *) malloc(8 * n64 + 4 * n32 + (size_t) nf + (size_t) pool_bytes + 8);
    if (!blk) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    int64_t *f_first = (int64_t *) blk, *f_off = f_first + n_bubbles + 1, *va_first = f_off + nfs, *ve_first = va_first + nv + 1, *va_off = ve_first + nv + 1,
            *ve_off = va_off + naf;
    int32_t *f_len = (int32_t *) (ve_off + nve), *f_read = f_len + nfs, *va_len = f_read + nfs, *g = va_len + naf, *ve_read = g + 2 * nv, *ve_len = ve_read + nve,
            *f_of = ve_len + nve, *findex = f_of + nf;
    uint8_t *strand = (uint8_t *) (findex + nr), *pool = strand + nf;
    {
        int64_t at[3] = {0, n_kind[0], n_kind[0] + n_kind[1]};
        for (int64_t r = 0; r < nr; r++) {
            const int k = kind(r);
            findex[r] = k < 0 ? -1 : (int32_t) at[k]++;
            if (k < 0) continue;
            f_of[findex[r]] = (int32_t) r;
            strand[findex[r]] = read_forward_strand[r] != 0;
        }
    }
    if (xf->pool_bytes) memcpy(pool, xf->pool, (size_t) xf->pool_bytes);
    /* per bubble the substrings of the (i) and (ii) reads in ascending filtered index: x lists a variant's entries in ascending read
     * order, and every (i) read comes before every (ii) read */
    int64_t is = 0, pat = xf->pool_bytes;
    f_first[0] = 0;
    for (int64_t b = 0; b < n_bubbles; b++) {
        const int64_t v = bubble_variant[b];
        for (int pass = 0; pass < 2; pass++)
            for (int64_t e = x->entry_first[v]; e < x->entry_first[v + 1]; e++) {
                const int32_t r = x->entry_read[e];
                if (kind(r) != pass) continue;
                f_off[is] = pat;
                f_len[is] = x->entry_len[e];
                f_read[is] = findex[r];
                if (x->entry_len[e]) memcpy(pool + pat, x->pool + x->entry_off[e], (size_t) x->entry_len[e]);
                pat += x->entry_len[e];
                is++;
            }
        f_first[b + 1] = is;
    }
    /* every variant of xf, index for index; one outside the chunk keeps its alleles and gt and lists no entry (bubbleGraph.c:2179); the others
     * list the entries of the reads xf kept, in its ascending read order (buildVcfEntryToReadSubstringsMap, bubbleGraph.c:1281-1323; the
     * low-mapq reads' entries, filteredReadsForFilteredVcfEntries of phase.c:354-357, are never read) */
    int64_t ie = 0;
    ve_first[0] = 0;
    for (int64_t v = 0; v <= nv; v++) va_first[v] = xf->allele_first[v];
    for (int64_t a = 0; a < naf; a++) { va_off[a] = xf->allele_off[a]; va_len[a] = xf->allele_len[a]; }
    for (int64_t v = 0; v < nv; v++) {
        g[2 * v] = gt[2 * v];
        g[2 * v + 1] = gt[2 * v + 1];
        if (inside(v))
            for (int64_t e = xf->entry_first[v]; e < xf->entry_first[v + 1]; e++) {
                const int32_t r = xf->entry_read[e];
                if (xf->read_status[r] != MRP_READ_KEPT) continue;
                ve_read[ie] = primary(r) ? r : (int32_t) (nr + findex[r]);
                ve_off[ie] = xf->entry_off[e];
                ve_len[ie] = xf->entry_len[e];
                ie++;
            }
        ve_first[v + 1] = ie;
    }
    out->n_filtered = nf;
    out->forward_strand = strand;
    out->pool = pool;
    out->pool_bytes = pool_bytes;
    out->fsub_first = f_first;
    out->fsub_off = f_off;
    out->fsub_len = f_len;
    out->fsub_read = f_read;
    out->n_variants = nv;
    out->valle_first = va_first;
    out->valle_off = va_off;
    out->valle_len = va_len;
    out->gt = g;
    out->ventry_first = ve_first;
    out->ventry_read = ve_read;
    out->ventry_off = ve_off;
    out->ventry_len = ve_len;
    *filtered_read = f_of;
    *block = blk;
    return MRP_OK;
}

int mrp_haptag_sites_from_extracted(int64_t n_chunks, const mrp_extracted_chunk *x, const int32_t *const *gt, mrp_haptag_sites *out, int64_t *read_first) {
    static const char *who = "mrp_haptag_sites_from_extracted";
    if (n_chunks < 0 || (n_chunks > 0 && (!x || !gt)) || !out || !read_first) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
    int64_t ns = 0, na = 0, ne = 0, nb = 0;
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_extracted_chunk &X = x[c];
        const int64_t nv = X.n_variants;
        if (nv < 0 || X.n_reads < 0 || X.pool_bytes < 0) return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: bad sizes", who, (long long) c);
        if (!X.allele_first || !X.entry_first || (X.n_reads > 0 && !X.read_status) || (X.pool_bytes > 0 && !X.pool) ||
            (nv > 0 && (!gt[c] || !X.allele_off || !X.allele_len || (X.entry_first[nv] > 0 && (!X.entry_read || !X.entry_off || !X.entry_len)))))
            return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: null array", who, (long long) c);
        for (int64_t v = 0; v < nv; v++) {
            const int64_t k = X.allele_first[v + 1] - X.allele_first[v];
            for (int w = 0; w < 2; w++)
                if (gt[c][2 * v + w] < 0 || gt[c][2 * v + w] >= k)
                    return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld, variant %lld: genotype %d outside its %lld alleles", who, (long long) c, (long long) v,
                                         gt[c][2 * v + w], (long long) k);
        }
        for (int64_t e = 0; e < X.entry_first[nv]; e++) {
            if (X.entry_read[e] < 0 || X.entry_read[e] >= X.n_reads)
                return mrp_set_error(MRP_ERR_ARG, "%s: chunk %lld: entry %lld names read %d", who, (long long) c, (long long) e, X.entry_read[e]);
            ne += X.read_status[X.entry_read[e]] == MRP_READ_KEPT;
        }
        ns += nv;
        na += X.allele_first[nv];
        nb += X.pool_bytes;
    }
    /* one block: allele_first, entry_first (ns + 1 each), allele_off (na), entry_read, entry_off (ne each), then the int32 arrays
     * allele_len (na), compare (2 ns), entry_len (ne), then the pool */
    const size_t n64 = 2 * ((size_t) ns + 1) + (size_t) na + 2 * (size_t) ne, n32 = (size_t) na + 2 * (size_t) ns + (size_t) ne;
    uint8_t *blk = (uint8_t *) malloc(8 * n64 + 4 * n32 + (size_t) nb + 8);
    if (!blk) return mrp_set_error(MRP_ERR_NOMEM, "%s: out of host memory", who);
    int64_t *a_first = (int64_t *) blk, *e_first = a_first + ns + 1, *a_off = e_first + ns + 1, *e_read = a_off + na, *e_off = e_read + ne;
    int32_t *a_len = (int32_t *) (e_off + ne), *cmp = a_len + na, *e_len = cmp + 2 * ns;
    uint8_t *pool = (uint8_t *) (e_len + ne);
    int64_t s = 0, ia = 0, ie = 0, base = 0;
    a_first[0] = e_first[0] = 0;
    read_first[0] = 0;
    for (int64_t c = 0; c < n_chunks; c++) {
        const mrp_extracted_chunk &X = x[c];
        for (int64_t v = 0; v < X.n_variants; v++, s++) { /* a variant without entries is a site too: the partition skips it itself */
            for (int64_t a = X.allele_first[v]; a < X.allele_first[v + 1]; a++, ia++) {
                a_off[ia] = base + X.allele_off[a];
                a_len[ia] = X.allele_len[a];
            }
            cmp[2 * s] = gt[c][2 * v];
            cmp[2 * s + 1] = gt[c][2 * v + 1];
            for (int64_t e = X.entry_first[v]; e < X.entry_first[v + 1]; e++) {
                if (X.read_status[X.entry_read[e]] != MRP_READ_KEPT) continue; /* filteredReads == NULL: low-mapq reads are skipped (htsIntegration.c:1825) */
                e_read[ie] = read_first[c] + X.entry_read[e];
                e_off[ie] = base + X.entry_off[e];
                e_len[ie] = X.entry_len[e];
                ie++;
            }
            a_first[s + 1] = ia;
            e_first[s + 1] = ie;
        }
        if (X.pool_bytes) memcpy(pool + base, X.pool, (size_t) X.pool_bytes);
        base += X.pool_bytes;
        read_first[c + 1] = read_first[c] + X.n_reads;
    }
    memset(out, 0, sizeof(*out));
    out->n_sites = ns;
    out->pool = pool;
    out->pool_bytes = nb;
    out->allele_first = a_first;
    out->allele_off = a_off;
    out->allele_len = a_len;
    out->compare = cmp;
    out->entry_first = e_first;
    out->entry_read = e_read;
    out->entry_off = e_off;
    out->entry_len = e_len;
    return MRP_OK;
}

}  // extern "C"
