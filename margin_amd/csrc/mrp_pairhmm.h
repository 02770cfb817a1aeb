/*
 * mrp_pairhmm.h -- what crosses the seams between the three units of the pair-HMM family: mrp_pairhmm.hip (the three kernels, the
 * launch scaffold, the small entries), mrp_string_chunks.hip (the string-chunk calls) and mrp_aligned.hip (the composites over the
 * extraction's result in HBM).  Internal; every unit that includes it is compiled with -ffp-contract=off.
 */
#ifndef MRP_PAIRHMM_H_
#define MRP_PAIRHMM_H_

#include <chrono>

#include "mrp_internal.h"

constexpr int PHM_WAVE = 64;
constexpr int PHM_WAVE_MAX_WIDTH = 2048; /* 3 diagonals * 2 048 cells * 3 states * 8 B = 144 KB */
constexpr int64_t PHM_WIDE_WORKSPACE_BYTES = (int64_t) 256 << 20; /* pair-per-workgroup kernel: what the slices of one launch may hold together */

struct PhmModelDev {
    double t[9];     /* order of mrp_pair_hmm */
    double em[25];   /* [cx * 5 + cy], N rows / columns hold log(0.25^2) as written in stateMachine.c:380 */
    double ex[5], ey[5];
    double start[3]; /* stateMachine3_startStateProb / raggedStartStateProb */
    double end[3];   /* stateMachine3_endStateProb / raggedEndStateProb */
};

/* The run-length emissions of one model (RleNucleotideEmissions, stateMachine.c:716-752) as the kernels read them:
 * rep[(cx * R + u) * R + o] = 2.3025 * logProbabilities[b(cx)][u][o], cx 0..4 the x symbol, b(cx) = strand ? cx : 3 - cx with N
 * mapped to A first (repeatSubMatrix.c:16-29), u the count of the x symbol (underlying), o that of the y symbol (observed) */
struct PhmRepeatDev {
    const double *rep;
    int32_t R;
};
/* The host half of a run-length batch: the counts (the caller's, parallel to the pool), every model's table back to back */
struct PhmRle {
    const uint8_t *counts = nullptr;
    HostVec<double> rep;
    std::vector<int64_t> rep_first; /* model i's table in rep */
    std::vector<int32_t> R;
    HostVec<double> rep_lane; /* [model][cx][u][o], u, o below the count bound of the pair-per-lane kernel: what that kernel stages in LDS */
};
/* (mrp_pairhmm.hip) every MRP_ERR_ARG of the two run-length entries; builds the tables.  The count check is what keeps every table
 * index of the kernels in range. */
struct PhmPairs;
int phm_rle_check_and_build(const char *who, const mrp_repeat_model *repeat, int32_t n_models, const uint8_t *counts, const PhmPairs &P,
                            PhmRle &out);
/* the device half: counts and tables uploaded on s; d_counts and d_models are what the run-length instantiations of the kernels are
 * handed (PhmRunLength::Args) */
struct PhmRleDev {
    DevBufGroup arrays;
    DevBuf<uint8_t> d_counts{arrays};
    DevBuf<double> d_rep{arrays};
    DevBuf<PhmRepeatDev> d_models{arrays};
    DevBuf<double> d_rep_lane{arrays}; /* phm_enqueue uploads it when the batch has lane pairs */
    hipError_t upload(DevPool *pool, const PhmRle &H, int64_t pool_bytes, hipStream_t s) {
        arrays.bind(pool);
        hipError_t e = d_counts.alloc((size_t) pool_bytes);
        if (e == hipSuccess && pool_bytes) e = hipMemcpyAsync(d_counts.p, H.counts, (size_t) pool_bytes, hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = d_rep.upload(H.rep, s);
        if (e != hipSuccess) return e;
        models.resize(H.R.size());
        for (size_t i = 0; i < H.R.size(); i++) models[i] = PhmRepeatDev{d_rep.p + H.rep_first[i], H.R[i]};
        return d_models.upload(models, s);
    }
    HostVec<PhmRepeatDev> models; /* the source of a queued copy: lives as long as the buffers */
};

struct PhmPair {
    int64_t x_off, y_off;
    int64_t band_off; /* first diagonal in the band array, -1: whole matrix */
    int32_t lx, ly, model, out;
};

struct PhmLanePair { /* pair-per-lane kernel: no band */
    int64_t x_off, y_off;
    int32_t lx, ly, model, out;
};

static inline int fail(int code, const char *msg) { return mrp_set_error(code, "%s", msg); }

#define PHM_HIP(expr)                                                                                                  \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess) return mrp_set_error(MRP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_));       \
    } while (0)

static inline double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

const int WAVE_CLASS_CAP[4] = {64, 256, 1024, PHM_WAVE_MAX_WIDTH};

/* (mrp_pairhmm.hip; kmer_anchors appends to out and returns the count) */
int band_closed_form(const int64_t *anchors, int64_t n_anchors, int64_t lx, int64_t ly, int64_t expansion, int32_t *L, int32_t *R,
                     int64_t *cells, int *max_width);
int64_t kmer_anchors(const uint8_t *sx, int64_t lx, const uint8_t *sy, int64_t ly, std::vector<int64_t> &out);
/* (mrp_pairhmm.hip) a model as the kernels read it: the N rows of the emissions, the start and end states of stateMachine.c:521-560 */
void model_to_device(const mrp_pair_hmm &m, int ragged_left, int ragged_right, PhmModelDev &d);

/* A batch's pairs as phm_classify reads them, in the order of the output: pair i aligns x (an allele) to y (a read substring), both
 * in one symbol pool, with model model[i] (NULL: model 0), inside the band of the anchors (x, y) anchors[2 * anchor_off[i]] up to
 * anchors[2 * anchor_off[i + 1]] (NULL: no pair is anchored).  The arrays are a PhmPairList's or a caller's. */
struct PhmPairs {
    int64_t n;
    const int64_t *x_off;
    const int32_t *x_len;
    const int64_t *y_off;
    const int32_t *y_len;
    const uint8_t *model;
    const int64_t *anchor_off, *anchors;
};

/* The pairs of a batch as the host makes them, one after the other (add) or side by side (resize, set, counts_to_offsets) */
struct PhmPairList {
    std::vector<int64_t> x_off, y_off, anchor_off{0}, anchors;
    std::vector<int32_t> x_len, y_len;
    std::vector<uint8_t> model;
    int64_t size() const { return (int64_t) x_off.size(); }
    /* pool: the symbols, for a pair that gets k-mer anchors; NULL for an unanchored one */
    void add(int64_t xo, int32_t xl, int64_t yo, int32_t yl, int mi, const uint8_t *pool) {
        x_off.push_back(xo); x_len.push_back(xl); y_off.push_back(yo); y_len.push_back(yl); model.push_back((uint8_t) mi);
        if (pool) kmer_anchors(pool + xo, xl, pool + yo, yl, anchors);
        anchor_off.push_back((int64_t) anchors.size() / 2);
    }
    void resize(int64_t n) {
        x_off.resize((size_t) n); x_len.resize((size_t) n); y_off.resize((size_t) n); y_len.resize((size_t) n); model.resize((size_t) n);
        anchor_off.assign((size_t) n + 1, 0);
    }
    /* n_anchors: a count for now; the caller appends the anchors themselves in pair order and calls counts_to_offsets() */
    void set(int64_t i, int64_t xo, int32_t xl, int64_t yo, int32_t yl, int mi, int64_t n_anchors) {
        x_off[(size_t) i] = xo; x_len[(size_t) i] = xl; y_off[(size_t) i] = yo; y_len[(size_t) i] = yl; model[(size_t) i] = (uint8_t) mi;
        anchor_off[(size_t) i + 1] = n_anchors;
    }
    void counts_to_offsets() {
        for (size_t i = 1; i < anchor_off.size(); i++) anchor_off[i] += anchor_off[i - 1];
    }
    void append(const PhmPairList &o) {
        x_off.insert(x_off.end(), o.x_off.begin(), o.x_off.end());
        x_len.insert(x_len.end(), o.x_len.begin(), o.x_len.end());
        y_off.insert(y_off.end(), o.y_off.begin(), o.y_off.end());
        y_len.insert(y_len.end(), o.y_len.begin(), o.y_len.end());
        model.insert(model.end(), o.model.begin(), o.model.end());
        for (size_t i = 1; i < o.anchor_off.size(); i++) anchor_off.push_back(anchor_off.back() + (o.anchor_off[i] - o.anchor_off[i - 1]));
        anchors.insert(anchors.end(), o.anchors.begin(), o.anchors.end());
    }
    PhmPairs view() const {
        const bool anchored = !anchors.empty();
        return PhmPairs{size(), x_off.data(), x_len.data(), y_off.data(), y_len.data(), model.data(), anchored ? anchor_off.data() : nullptr,
                        anchored ? anchors.data() : nullptr};
    }
};

/* A pair-HMM batch in two halves.  PhmLaunch, the host half (phm_classify): the pairs sorted into launch classes, the bands, the
 * models -- the sources of the uploads, so it outlives the device half.  PhmDev, the device half (phm_enqueue): the buffers of a
 * queued launch and where the log probabilities land (d_out, indexed by pair).  Its destructor drains the stream before the buffers
 * go back to their pool, so an early return never frees what a queued copy or kernel still reads. */
struct PhmLaunch {
    int64_t cells = 0;
    int n_models = 0, table_bytes = 0; /* phm_classify: what phm_enqueue sizes the launches by */
    bool has_switch = false;
    std::vector<PhmModelDev> hm;
    HostVec<PhmLanePair> lane_pairs[4];
    HostVec<PhmPair> wave_pairs[4];
    HostVec<PhmPair> wide_pairs; /* wide pairs on: the pairs beyond PHM_WAVE_MAX_WIDTH, for the pair-per-workgroup kernel */
    int wide_width = 0;          /* the widest diagonal among them: the cells of a workgroup's slice per diagonal and state */
    int64_t wide_cells = 0;      /* their share of cells */
    HostVec<int32_t> band;
    HostVec<uint32_t> key; /* phm_classify's sort keys (released with the launch, not between its two halves) */
    const PhmRle *rle = nullptr; /* set before phm_classify: run-length emissions */
    bool rle_lane = false;       /* set before phm_classify: a run-length batch's eligible pairs (unanchored, x within the cap, every count
                                  * below the kernel's bound) go to the pair-per-lane kernel; off: none does */
};
struct PhmDev {
    hipStream_t s = nullptr;
    DevBufGroup arrays; /* bound to the context's pool by phm_enqueue */
    DevBuf<PhmModelDev> d_models{arrays};
    DevBuf<uint8_t> d_pool{arrays};
    DevBuf<int32_t> d_band{arrays};
    DevBuf<double> d_out{arrays};
    DevBuf<PhmLanePair> d_lane[4]{DevBuf<PhmLanePair>{arrays}, DevBuf<PhmLanePair>{arrays}, DevBuf<PhmLanePair>{arrays}, DevBuf<PhmLanePair>{arrays}};
    DevBuf<PhmPair> d_wave[4]{DevBuf<PhmPair>{arrays}, DevBuf<PhmPair>{arrays}, DevBuf<PhmPair>{arrays}, DevBuf<PhmPair>{arrays}};
    DevBuf<PhmPair> d_wide{arrays};
    DevBuf<double> d_wide_ws{arrays}; /* [workgroup][diagonal being written, xay - 1, xay - 2][state][wide_width] */
    PhmRleDev rle;                    /* a run-length batch: counts and tables */
    ~PhmDev() {
        if (s) (void) hipStreamSynchronize(s);
    }
};

/* (mrp_pairhmm.hip) the x-length caps of the pair-per-lane kernel's four launch classes, -1 where no row fits; returns the tables' bytes */
int phm_lane_caps(int n_models, bool rle, int cap[4]);
/* wide_pairs: the caller's setting (mrp_context_set_wide_pairs / mrp_queue_set_wide_pairs); 0 is the refusal beyond PHM_WAVE_MAX_WIDTH */
int phm_classify(const char *who, const mrp_pair_hmm *models, int32_t n_models, int64_t pool_bytes, const PhmPairs &P, int64_t expansion,
                 int ragged_left, int ragged_right, int wide_pairs, PhmLaunch &L);
/* wide pairs on: MRP_OK, or the message of the cap a pair of this width and these cells exceeds (what: "pair 12", "chunk 3: a pair of bubble 7") */
int phm_wide_caps(const char *who, const char *what, int64_t width, int64_t cells);
int phm_enqueue(mrp_context *ctx, const uint8_t *pool, int64_t pool_bytes, int64_t n_pairs, const PhmLaunch &H, PhmDev &L, mrp_pairhmm_stats *stats,
                const uint8_t *device_pool = nullptr);

/* What the small entries share.  On ctx->stream: the pair-HMM kernels over P (classified first: every error of the batch is raised
 * on the host, before anything is launched) with ctx->ev[0] in front of them -- or, with no pairs, the event alone; then reduce(s, lp),
 * which uploads the entry's tables, launches its reduction over the log probabilities lp (indexed by pair; NULL with no pairs),
 * records ctx->ev[1] and queues its downloads.  Then the stream is drained, stats filled and the pool reclaimed.  reduce may keep its
 * device buffers as locals bound to ctx->pool: a block that went back to the pool is handed out again only after a reclaim().
 * The entry's tables are allocated and copied between the two events, so kernel_ms of the haplotagging entries covers those small
 * copies (and, on a cold pool, their hipMalloc) beside the kernels. */
template <class Reduce>
int phm_call(mrp_context *ctx, const char *who, const mrp_pair_hmm *models, int32_t n_models, const uint8_t *pool, int64_t pool_bytes,
             const PhmPairs &P, int64_t expansion, int ragged_left, int ragged_right, mrp_pairhmm_stats *stats, double t_begin, Reduce reduce,
             const PhmRle *rle = nullptr, bool rle_lane = false) {
    hipStream_t s = ctx->stream;
    {
        PhmLaunch H;
        H.rle = rle;
        H.rle_lane = rle_lane;
        PhmDev L;
        if (P.n > 0) { /* (the host's errors first, then the device: phm_enqueue makes it current) */
            int rc = phm_classify(who, models, n_models, pool_bytes, P, expansion, ragged_left, ragged_right, ctx->wide_pairs, H);
            if (rc == MRP_OK) rc = phm_enqueue(ctx, pool, pool_bytes, P.n, H, L, stats);
            if (rc != MRP_OK) return rc;
        } else {
            PHM_HIP(hipSetDevice(ctx->device));
            if (stats) PHM_HIP(hipStreamSynchronize(s));
            PHM_HIP(hipEventRecord(ctx->ev[0], s));
        }
        L.s = s; /* (whatever reduce has queued when it fails is drained as well) */
        const int rc = reduce(s, L.d_out.p);
        if (rc != MRP_OK) return rc;
        PHM_HIP(hipStreamSynchronize(s));
        if (stats) {
            float ms = 0.f;
            PHM_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1]));
            stats->kernel_ms = ms;
            stats->cells = H.cells;
        }
    }
    ctx->pool.reclaim();
    if (stats) stats->total_ms = now_ms() - t_begin;
    return MRP_OK;
}

void substring_owners(int64_t n_groups, const int64_t *first, const uint8_t *pool, const int64_t *off, const int32_t *len,
                      const uint8_t *may_own, bool last, std::vector<int64_t> &owner, const uint8_t *counts = nullptr);

/* stMath_logAddExact (sonLib), as mrp_kernels.hip and rphmm_frame.c state it */
static __device__ __forceinline__ double ht_log_add_exact(double x, double y) {
    if (x == -__builtin_inf()) return y;
    if (y == -__builtin_inf()) return x;
    return x > y ? x + log(1.0 + exp(y - x)) : y + log(1.0 + exp(x - y));
}

struct HtEntry { /* the two log probabilities (indices into the pair-HMM output) of one read at one site */
    int32_t a, b;
    int32_t hap1; /* phasing: the read is tagged haplotype 1 (else 2) */
    int32_t live; /* the back half in the string-chunk call (fs_* kernels): the record counts; the ht_* kernels do not read it */
};

/* One entry's share of a read's two totals, bubbleGraph.c:1881-1884: the supports are floats (:1869, :1881-1882) */
static __device__ __forceinline__ void ht_partition_term(const double *__restrict__ lp, const HtEntry &x, double &t1, double &t2) {
    const double s1 = (double) (float) lp[x.a], s2 = (double) (float) lp[x.b];
    t1 += s1 - ht_log_add_exact(s1, s2);
    t2 += s2 - ht_log_add_exact(s2, s1);
}
static __device__ __forceinline__ int32_t ht_hap(double t1, double t2) { return t1 > t2 ? 1 : (t2 > t1 ? 2 : 0); }

/* One tagged entry's share of a variant's two totals, bubbleGraph.c:2274-2298 (the supports stay doubles here).  Both contributions
 * come from the same two differences, so equal supports give equal totals (an exact tie). */
static __device__ __forceinline__ void ht_phase_term(const double *__restrict__ lp, const HtEntry &x, double &c, double &t) {
    const double sa = lp[x.a], sb = lp[x.b];
    const double l = ht_log_add_exact(sa, sb);
    const double da = sa - l, db = sb - l;
    c += x.hap1 ? da : db;
    t += x.hap1 ? db : da;
}
static __device__ __forceinline__ int32_t ht_state(bool visited, double c, double t) {
    return !visited ? MRP_VARIANT_NOT_VISITED : (c > t ? MRP_VARIANT_CIS : (t > c ? MRP_VARIANT_TRANS : MRP_VARIANT_TIE));
}

/* The reduce of mrp_partition_reads_by_haplotype on s (mrp_pairhmm.hip): the reads' entry lists go up, ht_partition_kernel walks them over
 * the log probabilities lp, ctx->ev[1] is recorded.  The caller owns the buffers and queues its downloads: d_hap, d_h = h1 | h2. */
struct HtPartitionDev {
    DevBufGroup arrays;
    DevBuf<int64_t> d_first{arrays};
    DevBuf<HtEntry> d_ent{arrays};
    DevBuf<int32_t> d_hap{arrays};
    DevBuf<double> d_h{arrays};
};
int ht_partition_enqueue(mrp_context *ctx, hipStream_t s, const HostVec<int64_t> &first, const HostVec<HtEntry> &ent, const double *lp, int64_t n_reads,
                         HtPartitionDev &B);

/* the pairs of the owning entries: (allele compare[0], entry) and (allele compare[1], entry) for every owner of an active
 * site; pair_of[k] = index of the first of the two (-1 for entries that own nothing) */
struct HtPairs {
    PhmPairList list;
    std::vector<int64_t> pair_of;
};

/* ---- the back half in the string-chunk call (mrp_phase_string_chunks_with_filtered) ------------------------------
 * A "site" is a primary bubble of a chunk with a rest (its entries: the bubble's primary substrings and the filtered reads') or a
 * filtered variant (its entries as listed).  The front groups a site's entries into classes of equal substrings and scores, for
 * every class and every strand that occurs in it, the pairs some outcome of the phasing could read: cbase[2 * class + reverse] is
 * the block of that (class, strand) in pidx, pidx[block + allele] (bubbles) / pidx[block + 0 / 1] (variants: gt1, gt2) the pair. */
struct FsEntry {
    int32_t cls;   /* class within the site */
    int32_t read;  /* the call's read index (primary reads of a chunk first, then its filtered reads) */
    int32_t key;   /* position in the site's listing order: the owner of a class is the max (bubbles) / min (variants) over its
                    * participating entries */
    int32_t flags; /* 1: reverse strand, 2: a filtered read */
};
struct FsSite {
    int64_t entry_first, cls_first;
    int32_t n_entries, n_classes;
    int32_t chunk, bubble; /* bubble < 0: a variant */
    int32_t n_alleles, visited; /* variants: gt1 != gt2 and entries (bubbleGraph.c:2174, :2186-2192) */
};

/* ---- the phased variant records behind the back half (mrp_phase_aligned_chunks_with_records) -------------------
 * A site is a variant of the call: the chunks' primary variants, then the rests'.  Its entries are the extraction's, read where the
 * extraction left them in HBM; its two lists go into its own slots of one array, hap1 from the front, hap2 from the back. */
struct RcSite {
    int64_t var;        /* the site's variant in the extraction's entry CSR */
    int64_t slot_first; /* its slots */
    int32_t n_slots;    /* one per entry of a primary read; 0 for a site that cannot be updated */
    int32_t chunk;
    int32_t bubble;     /* primary: its bubble, -1 without one or with a position outside [chunk_start, chunk_end); filtered: -1 */
    int32_t state;      /* filtered: where its state lies among the back half's variants; primary: -1 */
    int32_t gt1, gt2;   /* filtered: the rest's genotype */
    int32_t read_shift; /* entry_read - read_shift = the read among the call's primary reads (the rest's extraction numbers the same reads again) */
    int32_t read_base;  /* the chunk's first read among the call's primary reads */
};
struct RcOut {
    int32_t state, gt1, gt2, n_hap1, n_hap2;
};

/* the front of a string-chunk call: what mrp_string_front_create (or PaRun, over a device pool) makes and mrp_string_front_run reads */
struct mrp_string_front {
    int64_t n_chunks = 0, n_subs = 0, n_pairs = 0;
    const mrp_string_chunk *chunks = nullptr;          /* the caller's, alive until the run has returned */
    std::vector<int64_t> pool_base, sub_base;          /* n_chunks + 1: chunk c's symbols and substrings in the call's arrays */
    HostVec<uint8_t> gpool;                            /* every chunk's symbols: what the pair-HMM kernels read */
    const uint8_t *device_pool = nullptr;              /* set (mrp_phase_aligned_chunks): the symbols lie in HBM already, device_pool_bytes of */
    int64_t device_pool_bytes = 0;                     /* them, written by work queued on the run's stream; gpool is empty and not read */
    std::vector<int64_t> pair_first;                   /* per substring: the pair of its owner with the bubble's allele 0 */
    PhmLaunch L;                                       /* the pairs as phm_classify sorted them; the run adds the device half (PhmDev) */
    /* what only the front itself reads, kept until the front is destroyed: released between front and run, these ~100 bytes per
     * pair go back to the system and the run's own arrays fault fresh pages in (12 chunks of 2 000 sites: a call of 68-77 ms
     * instead of 56-61) */
    struct Scratch {
        std::vector<int64_t> g_sub_first, g_sub_off, owner;
        std::vector<int32_t> g_sub_len;
        PhmPairList pairs;                             /* the front's own, then the back half's speculative ones */
        std::vector<std::vector<int64_t>> chunk_anchors;
        /* a front over a device pool with a rest (mrp_phase_aligned_chunks_with_filtered): the host has no symbol, so the classes of equal
         * substrings come as ids (ec_classes_kernel: equal ids at a site = equal substrings) -- per substring of the call, per chunk per
         * fsub / ventry of its rest -- and the back half's pairs that want k-mer anchors are listed for the anchors kernel */
        bool classes_by_id = false;
        std::vector<int64_t> sub_cls;
        std::vector<std::vector<int64_t>> fsub_cls, ventry_cls;
        std::vector<int64_t> anchored_new;
    } scratch;
    double front_ms = 0;                               /* host wall time of the front (the one call adds its checks) */
    /* the back half (a call with rests): the static part of its sites, made with the pairs.  Sites: the bubbles of the chunks
     * with a rest, chunk by chunk, then the variants, chunk by chunk. */
    struct Filtered {
        bool on = false;
        const mrp_string_chunk_rest *rest = nullptr;   /* the caller's, as chunks */
        std::vector<int64_t> read_base, var_base;      /* n_chunks + 1: chunk c's reads (primary, then filtered) and variants in the call */
        int64_t n_bsites = 0, n_primary_pairs = 0;
        HostVec<FsEntry> entries;
        HostVec<FsSite> sites;
        HostVec<int32_t> cbase, pidx;
        HostVec<int64_t> cand_first;                   /* per read of the call: its entries at bubbles, in bubble order */
        HostVec<int32_t> cand;
    } fil;
    /* the records (a front over a device pool made for mrp_phase_aligned_chunks_with_records): the site table, the extraction's device
     * arrays the kernel reads (alive until the run has returned), and what the run brings back */
    struct Records {
        bool on = false;
        HostVec<RcSite> sites;
        std::vector<int64_t> read_first;               /* n_chunks + 1: chunk c's reads among the call's primary reads */
        int64_t n_slots = 0;
        const int64_t *entry_first = nullptr;          /* device: the entry CSR by variant of the call */
        const int32_t *entry_read = nullptr;           /* device: per entry its read of the call */
        const uint8_t *read_status = nullptr;          /* device: per read of the call MRP_READ_* */
        const uint8_t *take = nullptr;                 /* device: per read of the call the caller's mask (NULL: none) */
        std::vector<RcOut> out;                        /* filled by the run: per site */
        std::vector<int32_t> slots;                    /* the chunk's read index per slot that was written */
        float ms = 0.f;                                /* the kernel, HIP events */
    } rec;
};

int sc_filtered_front(mrp_string_front *F, const mrp_string_chunk_rest *rest, int64_t sv_threshold, const std::vector<int64_t> &rpool_base);

static inline void *sc_dup(const void *src, size_t bytes) { /* a result array the caller frees with mrp_free */
    void *p = malloc(bytes ? bytes : 1);
    if (p && bytes) memcpy(p, src, bytes);
    return p;
}

#endif /* MRP_PAIRHMM_H_ */
