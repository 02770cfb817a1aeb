/*
 * mrp_queue.cpp -- the host-side work queue that spreads genome chunks over the GPUs of one node.
 *
 * Reference: the chunk loop of phase.c.  The chunks are ordered by estimated depth, largest first (phase.c:257-263,
 * SCM_SIZE_DESC), and handed to the threads one at a time as they become free (phase.c:276-279,
 * "#pragma omp parallel for schedule(dynamic,1)"); chunks are independent until stitching, nothing is exchanged.
 * Here a "thread" is a device: one host thread and one context per device pull the next BATCH of chunks (a batch is
 * what one mrp_phase_reads_many call phases; its chunks share kernel launches), upload them, phase them and write the
 * results at the chunks' positions of the caller's array.  No collective, no device-to-device traffic.  The uploads of a
 * worker's next batch run on a second stream while the current batch is phased; every worker has its own host thread pool.
 * The same queue takes the chunks as read and allele strings (mrp_queue_phase_string_chunks): a batch is then what one
 * mrp_phase_string_chunks call phases, and what runs beside the current batch is the host front of the next one.
 * Aligned chunks come the same way, to be phased (mrp_queue_phase_aligned_chunks, with or without the filtered back half and the phased variant records) or haplotagged
 * from a phased VCF (mrp_queue_haplotag_aligned_chunks: the chunk loop of tools/tagFromPhasedVcf.c:227-309); beside a batch run the checks
 * and windows of the next one.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include <pthread.h>
#include <sched.h>
#include <cctype>

#include "mrp_internal.h"
#include "mrp_queue_lanes.h" /* the plan and the hand-out: plan_queue, active_lanes_of, run_lanes + LaneHooks */

int mrp_queue_threads_per_device(int n_devices);

extern "C" {

int mrp_queue_plan(int64_t n_chunks, const int64_t *cost, int64_t chunks_per_batch, int64_t *order_out, int64_t *batch_of_chunk_out) {
    if (n_chunks < 0 || (n_chunks > 0 && (!cost || !order_out))) return mrp_set_error(MRP_ERR_ARG, "mrp_queue_plan: bad arguments");
    const QueuePlan p = plan_queue(n_chunks, cost, chunks_per_batch);
    for (int64_t i = 0; i < n_chunks; i++) order_out[i] = p.order[(size_t) i];
    if (batch_of_chunk_out)
        for (size_t b = 0; b + 1 < p.batch_off.size(); b++)
            for (int64_t i = p.batch_off[b]; i < p.batch_off[b + 1]; i++) batch_of_chunk_out[p.order[(size_t) i]] = (int64_t) b;
    return MRP_OK;
}

int mrp_queue_dry_run(int32_t n_devices, int32_t lanes, int64_t n_chunks, const int64_t *cost, int64_t chunks_per_batch, double usec_per_cost,
                      int32_t *worker_of_chunk_out, int64_t *sequence_out) {
    if (n_devices < 1 || n_devices > MRP_MAX_QUEUE_DEVICES || lanes < 1 || lanes > 4 || n_chunks < 0 || (n_chunks > 0 && (!cost || !worker_of_chunk_out)))
        return mrp_set_error(MRP_ERR_ARG, "mrp_queue_dry_run: bad arguments");
    /* the plan and the hand-out of mrp_queue_phase_chunks for the same devices and lanes (worker = device * lanes + lane); the
     * stand-in for a call sleeps in proportion to the batch's cost, the stand-in for the upload of the next batch does nothing */
    const QueuePlan p = plan_queue(n_chunks, cost, chunks_per_batch, n_devices * lanes, n_devices);
    const int64_t n_batches = (int64_t) p.batch_off.size() - 1;
    std::atomic<int64_t> seq{0};
    LaneHooks hk;
    hk.phase = [&](int w, int64_t b) {
        int64_t c = 0;
        for (int64_t i = p.batch_off[(size_t) b]; i < p.batch_off[(size_t) b + 1]; i++) {
            const int64_t chunk = p.order[(size_t) i];
            worker_of_chunk_out[chunk] = w;
            if (sequence_out) sequence_out[chunk] = seq.fetch_add(1);
            c += cost[chunk];
        }
        if (usec_per_cost > 0) std::this_thread::sleep_for(std::chrono::microseconds((int64_t) (usec_per_cost * (double) c)));
        return (int) MRP_OK;
    };
    return run_lanes(n_devices, lanes, active_lanes_of(p, cost, n_devices, lanes), n_batches, hk, false, nullptr);
}

struct mrp_queue {
    std::vector<int32_t> devices;
    /* per lane (up to four per device): the context its batches are phased on, a second context on the same device whose
     * stream carries the uploads of the NEXT batch while the current one is phased, and its own host worker pool -- all
     * created by the worker on its first batch and kept between calls */
    std::vector<mrp_context *> ctx, stage_ctx; /* [device * lanes + lane] */
    std::vector<mrp_host_pool *> pools;        /* [device] */
    std::vector<mrp_chunk_block *> blocks;     /* [(device * lanes + lane) * 2 + parity] storage of a lane's current / next batch */
    int threads_per_device = 0;
    /* Calls of a device in flight at a time ("lanes", each a host thread with its own contexts); see plan_queue.  A short
     * queue uses one of them.  MRP_QUEUE_LANES=1..4 overrides. */
    int lanes = 4;
    int wide_pairs = 0; /* mrp_queue_set_wide_pairs: every lane's context gets it when the lane begins a call; the up-front checks read it */
    int sv_split = 0;   /* mrp_queue_set_sv_split: likewise */
    int64_t max_depth = 0; /* mrp_queue_set_downsampling: likewise */
    uint64_t downsampling_seed = 0;
};

int mrp_queue_create(const int32_t *devices, int32_t n_devices, mrp_queue **out) {
    if (!devices || !out || n_devices < 1 || n_devices > MRP_MAX_QUEUE_DEVICES) return mrp_set_error(MRP_ERR_ARG, "mrp_queue_create: bad arguments");
    *out = nullptr;
    const int visible = mrp_device_count();
    if (visible <= 0) return mrp_set_error(MRP_ERR_NO_DEVICE, "no HIP device visible: the stRPHmm sweep has no CPU fallback");
    for (int d = 0; d < n_devices; d++)
        if (devices[d] < 0 || devices[d] >= visible) return mrp_set_error(MRP_ERR_ARG, "device %d out of range (0..%d)", devices[d], visible - 1);
    mrp_queue *q = new (std::nothrow) mrp_queue();
    if (!q) return mrp_set_error(MRP_ERR_NOMEM, "out of host memory");
    q->devices.assign(devices, devices + n_devices);
    if (const char *le = getenv("MRP_QUEUE_LANES")) { const int v = atoi(le); if (v >= 1 && v <= 4) q->lanes = v; }
    q->ctx.assign((size_t) n_devices * (size_t) q->lanes, nullptr);
    q->stage_ctx.assign((size_t) n_devices * (size_t) q->lanes, nullptr);
    q->pools.assign((size_t) n_devices, nullptr);
    q->blocks.assign((size_t) n_devices * (size_t) q->lanes * 2, nullptr);
    q->threads_per_device = mrp_queue_threads_per_device(n_devices);
    *out = q;
    return MRP_OK;
}

void mrp_queue_destroy(mrp_queue *q) {
    if (!q) return;
    for (size_t i = 0; i < q->blocks.size(); i++)
        if (q->blocks[i]) { (void) hipSetDevice(q->devices[i / (2 * (size_t) q->lanes)]); delete q->blocks[i]; }
    for (auto *c : q->stage_ctx) mrp_context_destroy(c);
    for (auto *c : q->ctx) mrp_context_destroy(c);
    for (auto *p : q->pools) mrp_host_pool_destroy(p);
    delete q;
}

int mrp_queue_set_wide_pairs(mrp_queue *q, int on) {
    if (!q) return mrp_set_error(MRP_ERR_ARG, "mrp_queue_set_wide_pairs: queue is NULL");
    q->wide_pairs = on != 0;
    for (mrp_context *c : q->ctx)
        if (c) (void) mrp_context_set_wide_pairs(c, q->wide_pairs);
    return MRP_OK;
}

int mrp_queue_set_sv_split(mrp_queue *q, int on) {
    if (!q) return mrp_set_error(MRP_ERR_ARG, "mrp_queue_set_sv_split: queue is NULL");
    q->sv_split = on != 0;
    for (mrp_context *c : q->ctx)
        if (c) (void) mrp_context_set_sv_split(c, q->sv_split);
    return MRP_OK;
}

int mrp_queue_set_downsampling(mrp_queue *q, int64_t max_depth, uint64_t seed) {
    if (!q) return mrp_set_error(MRP_ERR_ARG, "mrp_queue_set_downsampling: queue is NULL");
    if (max_depth < 0) return mrp_set_error(MRP_ERR_ARG, "mrp_queue_set_downsampling: negative max_depth");
    q->max_depth = max_depth;
    q->downsampling_seed = seed;
    for (mrp_context *c : q->ctx)
        if (c) (void) mrp_context_set_downsampling(c, max_depth, seed);
    return MRP_OK;
}

int mrp_queue_wide_pair_count(mrp_queue *q, int64_t *pairs_out, int64_t *cells_out) {
    if (!q) return mrp_set_error(MRP_ERR_ARG, "mrp_queue_wide_pair_count: queue is NULL");
    int64_t pairs = 0, cells = 0;
    for (mrp_context *c : q->ctx) {
        int64_t p = 0, n = 0;
        if (c && mrp_context_wide_pair_count(c, &p, &n) == MRP_OK) { pairs += p; cells += n; }
    }
    if (pairs_out) *pairs_out = pairs;
    if (cells_out) *cells_out = cells;
    return MRP_OK;
}

}  /* extern "C" */

/* Host threads a worker gets: every device its own pool (phase.c:276-279 uses every core of the machine; one pool of sixteen
 * threads shared by eight devices would starve them).  mrp_set_host_threads() is the number PER DEVICE; by default the
 * machine's hardware threads are split evenly, at most 32 (16 through round 4) and at least 2 each. */
int mrp_queue_threads_per_device(int n_devices) {
    const int hw = (int) std::max(1u, std::thread::hardware_concurrency());
    const int asked = mrp_host_threads_setting();
    if (asked > 0) return asked;
    return std::max(2, std::min(32, hw / std::max(1, n_devices)));
}

/* The CPUs next to a device (Linux: /sys/bus/pci/devices/<bus id>/local_cpulist), for the worker of that device and every
 * thread it starts.  Only when a queue drives more than one device, and unless MRP_QUEUE_AFFINITY=0: a worker that reaches
 * across sockets for every staging copy and descriptor loses a third of its host bandwidth. */
static bool device_cpuset(int device, cpu_set_t *set) {
    char bus[64] = {0};
    if (hipDeviceGetPCIBusId(bus, (int) sizeof(bus) - 1, device) != hipSuccess) return false;
    for (char *c = bus; *c; c++) *c = (char) tolower((unsigned char) *c);
    const std::string path = std::string("/sys/bus/pci/devices/") + bus + "/local_cpulist";
    FILE *f = fopen(path.c_str(), "r");
    if (!f) return false;
    char line[4096] = {0};
    const bool got = fgets(line, sizeof(line), f) != nullptr;
    fclose(f);
    if (!got) return false;
    CPU_ZERO(set);
    int n = 0;
    for (char *tok = strtok(line, ",\n"); tok; tok = strtok(nullptr, ",\n")) {
        int lo = 0, hi = 0;
        if (sscanf(tok, "%d-%d", &lo, &hi) == 2) { for (int c = lo; c <= hi && c < CPU_SETSIZE; c++) { CPU_SET(c, set); n++; } }
        else if (sscanf(tok, "%d", &lo) == 1 && lo < CPU_SETSIZE) { CPU_SET(lo, set); n++; }
    }
    return n > 0;
}

/* What one call of the queue keeps beside its batches, whichever input they are made of (profile bytes: mrp_queue_phase_chunks,
 * strings: mrp_queue_phase_string_chunks): the lanes' contexts and pools, one error text per lane and ROLE (the call and the work
 * for the next batch run on two threads at a time), what each lane did. */
struct QueueCall {
    struct PerLane { int64_t chunks = 0, units = 0, fallback = 0; double busy_ms = 0; };
    mrp_queue *q;
    int64_t n_batches;
    int active_lanes;
    std::vector<std::string> errs, stage_errs;
    std::vector<PerLane> per;
    std::vector<void *> caller_pool; /* (lane 0 may run on the caller's thread: its pool comes back at the end) */
    std::mutex pool_mu;
    std::chrono::steady_clock::time_point t_call = std::chrono::steady_clock::now();
    const bool timing = getenv("MRP_TIMING") != nullptr;

    QueueCall(mrp_queue *queue, int64_t batches, int lanes_in_use)
        : q(queue), n_batches(batches), active_lanes(lanes_in_use), errs(queue->ctx.size()), stage_errs(queue->ctx.size()), per(queue->ctx.size()),
          caller_pool(queue->ctx.size(), nullptr) {}
    double since() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_call).count(); }

    /* the lane's context (and, for uploads beside the call, a second one on the same device) and its device's host pool, made
     * on first use and kept between calls */
    int lane_begin(int w, bool with_stage_ctx) {
        const int lanes = q->lanes, d = w / lanes; /* the device this lane works for */
        const int n_devices = (int) q->devices.size();
        int r = MRP_OK;
        if (!q->ctx[(size_t) w]) r = mrp_context_create(q->devices[(size_t) d], &q->ctx[(size_t) w]);
        if (r == MRP_OK && with_stage_ctx && !q->stage_ctx[(size_t) w]) r = mrp_context_create(q->devices[(size_t) d], &q->stage_ctx[(size_t) w]);
        if (r == MRP_OK) {
            std::lock_guard<std::mutex> lk(pool_mu);
            if (!q->pools[(size_t) d]) {
                q->pools[(size_t) d] = mrp_host_pool_create(q->threads_per_device);
                if (!q->pools[(size_t) d]) r = mrp_set_error(MRP_ERR_NOMEM, "out of host memory");
            }
        }
        if (r != MRP_OK) { errs[(size_t) w] = mrp_last_error(); return r; }
        if (lanes > 1) (void) mrp_context_set_grouped(q->ctx[(size_t) w], 1); /* the lanes of a device are concurrent batches of it */
        (void) mrp_context_set_wide_pairs(q->ctx[(size_t) w], q->wide_pairs);
        (void) mrp_context_set_sv_split(q->ctx[(size_t) w], q->sv_split);
        (void) mrp_context_set_downsampling(q->ctx[(size_t) w], q->max_depth, q->downsampling_seed);
        q->ctx[(size_t) w]->calls_sharing_device = n_batches > (int64_t) n_devices ? active_lanes : 1;
        caller_pool[(size_t) w] = mrp_pool_current();
        mrp_pool_adopt(q->pools[(size_t) d]);
        /* the lanes of a device share it: a call of a long queue runs 8 / lanes concurrent batches, the one call of a short
         * queue as many as its size asks for */
        (void) mrp_context_set_phase_groups(q->ctx[(size_t) w], n_batches > (int64_t) n_devices ? std::max(1, 8 / active_lanes) : 0);
        return (int) MRP_OK;
    }
    void lane_end(int w) { mrp_pool_adopt(caller_pool[(size_t) w]); }

    void fill(mrp_queue_stats *stats) const {
        if (!stats) return;
        for (size_t w = 0; w < per.size(); w++) {
            const size_t d = w / (size_t) q->lanes;
            stats->chunks_per_device[d] += per[w].chunks;
            stats->units_per_device[d] += per[w].units;
            stats->busy_ms_per_device[d] = std::max(stats->busy_ms_per_device[d], per[w].busy_ms);
            stats->fallback_chunks += per[w].fallback;
        }
    }
    int error(int rc) const { /* the first error text: the calls' before the staging threads' */
        for (auto &e : errs)
            if (!e.empty()) return mrp_set_error(rc, "%s", e.c_str());
        for (auto &e : stage_errs)
            if (!e.empty()) return mrp_set_error(rc, "%s", e.c_str());
        return mrp_set_error(rc, "work queue stopped");
    }
};

/* runs the lanes; when the queue drives more than one device, each on the CPUs next to its device */
static int run_call(QueueCall &call, const LaneHooks &hk) {
    mrp_queue *q = call.q;
    const int n_devices = (int) q->devices.size(), lanes = q->lanes;
    const char *aff_env = getenv("MRP_QUEUE_AFFINITY");
    const bool bind = n_devices > 1 && !(aff_env && aff_env[0] == '0');
    /* before the first thread of a worker is created (they inherit it): the CPUs next to its device */
    std::function<void(int)> on_start;
    if (bind) on_start = [q, lanes](int w) {
        cpu_set_t set;
        if (device_cpuset(q->devices[(size_t) (w / lanes)], &set)) (void) pthread_setaffinity_np(pthread_self(), sizeof(set), &set);
    };
    const int rc = run_lanes(n_devices, lanes, call.active_lanes, call.n_batches, hk, /* the caller's own affinity is left alone */ bind, on_start);
    if (call.timing) fprintf(stderr, "  [%7.1f] queue: workers joined\n", call.since());
    return rc;
}

/* What every chunk kind's batches share: the head of a staged batch, a lane's two of them -- the one it runs and the one its
 * prefetch makes beside it --, the one driver that takes a kind's batches through the lanes, and the create + call + destroy of the
 * *_on_devices forms. */
struct StagedBatch {
    std::atomic<int64_t> batch{-1}; /* (the call's thread looks its batch up while the stager fills the lane's OTHER slot) */
    int64_t first = 0, count = 0;   /* the batch is plan.order[first .. first + count) */
};
template <typename Staged>
struct LaneSlots {
    Staged st[2];
    int n_staged = 0;
    Staged *next(int *slot) { *slot = n_staged++ & 1; return &st[*slot]; } /* (the stager fills the slot the call's thread is not running) */
    Staged *find(int64_t b) { return st[0].batch.load() == b ? &st[0] : (st[1].batch.load() == b ? &st[1] : nullptr); }
};
static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}
/* (the three phasing kinds: a batch the resident path did not take went through the per-chunk path as a whole) */
static void count_fallback(QueueCall::PerLane &me, const mrp_phase_many_stats &ps, int64_t count) {
    me.fallback += ps.resident ? ps.fallback_chunks : count;
}

/* The queue for one chunk kind: the plan, the lanes, the two slots of each, the accounting and the MRP_TIMING lines; on an error
 * `clear_outputs()` and the first error text.  The preamble (the checks, zeroing the outputs, the costs) is the entry's.  A Body has
 *   Staged                   what it keeps of a staged batch, derived from StagedBatch;
 *   on_stage_ctx             the batch is made on, and lives on, a second context of the lane (uploads beside the call): the lane gets
 *                            one, and giving the batch back is device work that counts as the lane's busy time;
 *   staged_line, not_ready   the MRP_TIMING line of a prefetch; the error text of a batch that reaches its call unstaged;
 *   stage(w, slot, st, order)        gather the batch (chunks order[0 .. st.count)) and make its front or upload it: runs beside the
 *                                    lane's current call, from the second batch on on a thread of its own; MRP_OK: it can be run;
 *   run(w, st, order, me, &split_ms) the call, then the results to the caller's arrays at the positions order[i]; split_ms is what
 *                                    print_run wants beside the time of the whole;
 *   print_run(since, w, b, all_ms, split_ms)  the MRP_TIMING line of a call;
 *   drop(st)                         give back what the staged batch holds. */
template <typename Body, typename Clear>
static int run_queue(mrp_queue *q, int64_t n_chunks, const std::vector<int64_t> &cost, int64_t chunks_per_batch, mrp_queue_stats *stats, Body &body,
                     Clear clear_outputs) {
    using Staged = typename Body::Staged;
    const int n_devices = (int) q->devices.size(), lanes = q->lanes, n_workers = n_devices * lanes;
    const QueuePlan plan = plan_queue(n_chunks, cost.data(), chunks_per_batch, n_workers, n_devices);
    const int64_t n_batches = (int64_t) plan.batch_off.size() - 1;
    if (stats) stats->batches = n_batches;
    QueueCall call(q, n_batches, active_lanes_of(plan, cost.data(), n_devices, lanes));
    std::vector<LaneSlots<Staged>> lane_state((size_t) n_workers);
    auto staged_of = [&](int w, int64_t b) { return lane_state[(size_t) w].find(b); };
    auto drop = [&](int w, int64_t b) { if (Staged *st = staged_of(w, b)) { body.drop(*st); st->batch = -1; } };
    LaneHooks hk;
    hk.begin = [&](int w) { return call.lane_begin(w, Body::on_stage_ctx); };
    hk.prefetch = [&](int w, int64_t b) { /* (the first batch on the lane's thread, the later ones on a thread beside the call) */
        const auto t0 = std::chrono::steady_clock::now();
        mrp_pool_adopt(q->pools[(size_t) (w / lanes)]);
        int slot = 0;
        Staged *st = lane_state[(size_t) w].next(&slot);
        st->first = plan.batch_off[(size_t) b]; st->count = plan.batch_off[(size_t) b + 1] - st->first;
        st->batch.store(b);
        const int r = body.stage(w, slot, *st, plan.order.data() + st->first);
        if (r != MRP_OK) call.stage_errs[(size_t) w] = mrp_last_error();
        if (call.timing) fprintf(stderr, Body::staged_line, call.since(), w, (long long) b, (long long) st->count, ms_since(t0));
        return r;
    };
    hk.discard = drop;
    hk.phase = [&](int w, int64_t b) {
        Staged *cur = staged_of(w, b);
        if (!cur) { call.errs[(size_t) w] = Body::not_ready; return (int) MRP_ERR_ARG; }
        const auto t0 = std::chrono::steady_clock::now();
        const int64_t *order = plan.order.data() + cur->first;
        QueueCall::PerLane &me = call.per[(size_t) w];
        double split_ms = 0;
        const int r = body.run(w, *cur, order, me, &split_ms);
        if (r != MRP_OK) call.errs[(size_t) w] = mrp_last_error();
        else {
            for (int64_t i = 0; i < cur->count; i++) me.units += cost[(size_t) order[i]];
            me.chunks += cur->count;
        }
        const double all_ms = ms_since(t0);
        if (call.timing) body.print_run(call.since(), w, b, all_ms, split_ms);
        me.busy_ms += all_ms;
        return r;
    };
    /* (a batch on the lane's STAGING context, on which the stager thread makes the next batch while the call runs, goes after that
     * thread has ended: one host thread per context, include/margin_rphmm.h; a staged front holds arrays of the lane's context and
     * goes on the lane's thread with no other thread of the lane at work) */
    hk.retire = [&](int w, int64_t b) {
        const auto t0 = std::chrono::steady_clock::now();
        drop(w, b);
        if (Body::on_stage_ctx) call.per[(size_t) w].busy_ms += ms_since(t0);
    };
    hk.end = [&](int w) { call.lane_end(w); };
    const int rc = run_call(call, hk);
    call.fill(stats);
    if (rc == MRP_OK) return MRP_OK;
    clear_outputs();
    return call.error(rc);
}

/* the queue's own order of errors: a malformed call and a refused mode need no device; then mrp_queue_create's own error */
template <typename Check, typename Run>
static int checked_on_devices(const int32_t *devices, int32_t n_devices, Check check, Run run) {
    int rc = check();
    if (rc != MRP_OK) return rc;
    mrp_queue *q = nullptr;
    rc = mrp_queue_create(devices, n_devices, &q);
    if (rc == MRP_OK) rc = run(q);
    mrp_queue_destroy(q);
    return rc;
}

namespace {

/* chunks as profile bytes: a batch is what one mrp_phase_reads_many call phases; its chunks are on the device before the call (uploads
 * queued on the staging context's stream; the chunks carry the event that ends the upload, the first device work that reads one waits
 * for it) */
struct ProfileBody {
    struct Staged : StagedBatch { std::vector<mrp_chunk *> dch; };
    static constexpr bool on_stage_ctx = true;
    static constexpr const char *staged_line = "  [%7.1f] queue lane %d: batch %lld (%lld chunks) staged in %.1f ms\n";
    static constexpr const char *not_ready = "work queue: batch was not staged";
    mrp_queue *q;
    const mrp_chunk_desc *chunks;
    const mrp_params *params;
    mrp_phase_result **out;

    int stage(int w, int slot, Staged &st, const int64_t *order) {
        st.dch.assign((size_t) st.count, nullptr);
        mrp_context *sc = q->stage_ctx[(size_t) w];
        sc->pool.reclaim(); /* the block of the batch before last was emptied after its call returned */
        mrp_chunk_block *&blk = q->blocks[(size_t) w * 2 + (size_t) slot]; /* (the block of the slot: the other one's is in use) */
        if (!blk) blk = new (std::nothrow) mrp_chunk_block();
        if (!blk) return mrp_set_error(MRP_ERR_NOMEM, "out of host memory");
        std::vector<const mrp_chunk_desc *> dl((size_t) st.count);
        for (int64_t i = 0; i < st.count; i++) dl[(size_t) i] = &chunks[order[i]];
        /* (uploaded in the groups the call will deal the chunks to: its first batch starts on the device when an eighth of the bytes is there) */
        return mrp_chunk_block_create(sc, st.count, dl.data(), st.dch.data(), blk, mrp_phase_groups_for(q->ctx[(size_t) w], st.count));
    }
    int run(int w, Staged &st, const int64_t *order, QueueCall::PerLane &me, double *) {
        const size_t count = (size_t) st.count;
        std::vector<const mrp_chunk *> cch(st.dch.begin(), st.dch.end());
        std::vector<const mrp_read *> rd(count);
        std::vector<int64_t> nr(count);
        std::vector<mrp_phase_result *> res(count, nullptr);
        for (size_t i = 0; i < count; i++) { rd[i] = chunks[order[i]].reads; nr[i] = chunks[order[i]].n_reads; }
        mrp_phase_many_stats ps{};
        const int r = mrp_phase_reads_many(q->ctx[(size_t) w], st.count, cch.data(), rd.data(), nr.data(), params, res.data(), &ps);
        if (r != MRP_OK) return r;
        for (size_t i = 0; i < count; i++) out[order[i]] = res[i];
        count_fallback(me, ps, st.count);
        return r;
    }
    void print_run(double since, int w, int64_t b, double all_ms, double) const {
        fprintf(stderr, "  [%7.1f] queue lane %d: batch %lld phased in %.1f ms\n", since, w, (long long) b, all_ms);
    }
    void drop(Staged &st) { /* (a thousand chunks of a one-call queue: on the lane's pool, not one after the other) */
        mrp_parallel_for((int64_t) st.dch.size(), 8, [&](int64_t i) { if (st.dch[(size_t) i]) mrp_chunk_destroy(st.dch[(size_t) i]); });
        st.dch.clear();
    }
};

}  // namespace

extern "C" {

int mrp_queue_phase_chunks(mrp_queue *q, int64_t n_chunks, const mrp_chunk_desc *chunks, const mrp_params *params, int64_t chunks_per_batch,
                           mrp_phase_result **out, mrp_queue_stats *stats) {
    if (!q || n_chunks < 0 || !params || (n_chunks > 0 && (!chunks || !out))) return mrp_set_error(MRP_ERR_ARG, "mrp_queue_phase_chunks: bad arguments");
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_devices = (int) q->devices.size(); }
    for (int64_t i = 0; i < n_chunks; i++) out[i] = nullptr;
    if (n_chunks == 0) return MRP_OK;
    /* estimated cost of a chunk: its het-sites x reads (what the depth estimate of phase.c:259 stands for) */
    std::vector<int64_t> cost((size_t) n_chunks, 0);
    for (int64_t i = 0; i < n_chunks; i++) {
        const mrp_chunk_desc &c = chunks[i];
        if (c.n_sites < 0 || c.n_reads < 0 || (c.n_reads > 0 && !c.reads) || (c.n_sites > 0 && !c.allele_number))
            return mrp_set_error(MRP_ERR_ARG, "chunk %lld: bad description", (long long) i);
        for (int64_t r = 0; r < c.n_reads; r++) cost[(size_t) i] += c.reads[r].length;
    }
    ProfileBody body{q, chunks, params, out};
    return run_queue(q, n_chunks, cost, chunks_per_batch, stats, body, [&] {
        for (int64_t i = 0; i < n_chunks; i++) { mrp_phase_result_destroy(out[i]); out[i] = nullptr; }
    });
}

int mrp_phase_chunks_on_devices(const int32_t *devices, int32_t n_devices, int64_t n_chunks, const mrp_chunk_desc *chunks,
                                const mrp_params *params, int64_t chunks_per_batch, mrp_phase_result **out, mrp_queue_stats *stats) {
    /* (this form has no checks that come before the queue's own: mrp_queue_phase_chunks makes them) */
    return checked_on_devices(devices, n_devices, [] { return (int) MRP_OK; },
                              [&](mrp_queue *q) { return mrp_queue_phase_chunks(q, n_chunks, chunks, params, chunks_per_batch, out, stats); });
}

}  /* extern "C" */

namespace {

/* chunks as strings: a batch as one mrp_phase_string_chunks call sees it: its chunks side by side, and the host front made of them
 * (prefetch: beside the device work of the lane's current batch; the uploads follow on the lane's own stream when the batch is run) */
struct StringBody {
    struct Staged : StagedBatch {
        std::vector<mrp_string_chunk> sc;
        std::vector<mrp_string_chunk_rest> sr;
        mrp_string_front *front = nullptr;
    };
    static constexpr bool on_stage_ctx = false;
    static constexpr const char *staged_line = "  [%7.1f] queue lane %d: front of batch %lld (%lld chunks) in %.1f ms\n";
    static constexpr const char *not_ready = "work queue: batch has no front";
    mrp_queue *q;
    const mrp_string_chunk *chunks;
    const mrp_string_chunk_rest *rest; /* NULL: without the filtered half */
    const mrp_pair_hmm *forward_model, *reverse_model;
    int64_t expansion, sv_threshold;
    double het_substitution_probability;
    const mrp_params *params;
    int64_t min_phred;
    mrp_phase_result **out; int8_t *const *hap_out; double *const *phred_out; mrp_profile_out *profiles_out; mrp_filtered_out *filtered_out;

    int stage(int, int, Staged &st, const int64_t *order) {
        st.sc.resize((size_t) st.count);
        for (int64_t i = 0; i < st.count; i++) st.sc[(size_t) i] = chunks[order[i]];
        st.sr.resize(rest ? (size_t) st.count : 0);
        for (int64_t i = 0; rest && i < st.count; i++) st.sr[(size_t) i] = rest[order[i]];
        return mrp_string_front_create(st.count, st.sc.data(), rest ? st.sr.data() : nullptr, forward_model, reverse_model, expansion, sv_threshold,
                                       q->wide_pairs, &st.front);
    }
    int run(int w, Staged &st, const int64_t *order, QueueCall::PerLane &me, double *call_ms) {
        const size_t count = (size_t) st.count;
        std::vector<mrp_phase_result *> res(count, nullptr);
        std::vector<int8_t *> hap(count);
        std::vector<double *> phred(count);
        std::vector<mrp_profile_out> prof(profiles_out ? count : 0); /* (zeroed, as the next) */
        std::vector<mrp_filtered_out> fo(rest ? count : 0);
        for (size_t i = 0; i < count; i++) {
            hap[i] = hap_out[order[i]];
            if (phred_out) phred[i] = phred_out[order[i]];
        }
        mrp_string_chunks_stats ss{};
        const int r = mrp_string_front_run(q->ctx[(size_t) w], st.front, het_substitution_probability, params, min_phred, res.data(), hap.data(),
                                           phred_out ? phred.data() : nullptr, profiles_out ? prof.data() : nullptr, &ss, rest ? fo.data() : nullptr, nullptr);
        *call_ms = ss.total_ms;
        if (r != MRP_OK) return r;
        for (size_t i = 0; i < count; i++) {
            out[order[i]] = res[i];
            if (profiles_out) profiles_out[order[i]] = prof[i];
            if (rest) filtered_out[order[i]] = fo[i];
        }
        count_fallback(me, ss.phase, st.count);
        return r;
    }
    void print_run(double since, int w, int64_t b, double all_ms, double call_ms) const { /* (the call's own time counts its front) */
        fprintf(stderr, "  [%7.1f] queue lane %d: batch %lld run in %.1f ms, its front took %.1f ms\n", since, w, (long long) b, all_ms, call_ms - all_ms);
    }
    void drop(Staged &st) { mrp_string_front_destroy(st.front); st.front = nullptr; }
};

}  // namespace

/* mrp_queue_phase_string_chunks (rest == NULL) and mrp_queue_phase_string_chunks_with_filtered: the rest travels with its chunk */
static int queue_phase_string_chunks(mrp_queue *q, int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_string_chunk_rest *rest,
                                     const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold,
                                     double het_substitution_probability, const mrp_params *params, int64_t min_phred, int64_t chunks_per_batch,
                                     mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out,
                                     mrp_filtered_out *filtered_out, mrp_queue_stats *stats) {
    /* (messages carry the name of the one call a batch makes, as they did before the rest existed, or the entry's own) */
    const char *who = rest ? "mrp_queue_phase_string_chunks_with_filtered" : "mrp_phase_string_chunks";
    /* ---- every chunk's checks first, on the caller's thread and in the one call's order: no lane starts on a call that would be refused */
    int rc = mrp_string_chunks_check(n_chunks, chunks, forward_model, reverse_model, expansion, params, out, hap_out, phred_out, rest, who);
    if (rc != MRP_OK) return rc;
    if (!q) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no queue (the pair-HMM path has no CPU fallback)", rest ? who : "mrp_queue_phase_string_chunks");
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_devices = (int) q->devices.size(); }
    for (int64_t i = 0; i < n_chunks; i++) out[i] = nullptr;
    if (profiles_out) memset(profiles_out, 0, sizeof(*profiles_out) * (size_t) n_chunks);
    rc = mrp_string_chunks_check_pairs(n_chunks, chunks, expansion, sv_threshold, rest, who, q->wide_pairs);
    if (rc != MRP_OK) return rc;
    if (n_chunks == 0) return MRP_OK;
    /* phase.c:257-263 orders by estimated depth; here a chunk costs its (read, bubble) units, the unit the batches are cut by, and
     * with a rest that rest's (read, site) entries as well */
    std::vector<int64_t> cost((size_t) n_chunks, 0);
    for (int64_t i = 0; i < n_chunks; i++) {
        (void) mrp_string_chunk_units(&chunks[i], &cost[(size_t) i]);
        if (!rest) continue;
        if (rest[i].fsub_first && chunks[i].n_bubbles > 0) cost[(size_t) i] += rest[i].fsub_first[chunks[i].n_bubbles];
        if (rest[i].n_variants > 0) cost[(size_t) i] += rest[i].ventry_first[rest[i].n_variants];
    }
    StringBody body{q, chunks, rest, forward_model, reverse_model, expansion, sv_threshold, het_substitution_probability, params, min_phred,
                    out, hap_out, phred_out, profiles_out, filtered_out};
    return run_queue(q, n_chunks, cost, chunks_per_batch, stats, body, [&] {
        for (int64_t i = 0; i < n_chunks; i++) {
            mrp_phase_result_destroy(out[i]);
            out[i] = nullptr;
            if (profiles_out) mrp_profile_out_clear(&profiles_out[i]);
            if (rest) mrp_filtered_out_clear(&filtered_out[i]);
        }
    });
}

extern "C" {

int mrp_queue_phase_string_chunks(mrp_queue *q, int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_pair_hmm *forward_model,
                                  const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold, double het_substitution_probability,
                                  const mrp_params *params, int64_t min_phred, int64_t chunks_per_batch, mrp_phase_result **out, int8_t *const *hap_out,
                                  double *const *phred_out, mrp_profile_out *profiles_out, mrp_queue_stats *stats) {
    return queue_phase_string_chunks(q, n_chunks, chunks, nullptr, forward_model, reverse_model, expansion, sv_threshold, het_substitution_probability, params,
                                     min_phred, chunks_per_batch, out, hap_out, phred_out, profiles_out, nullptr, stats);
}

int mrp_queue_phase_string_chunks_with_filtered(mrp_queue *q, int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_string_chunk_rest *rest,
                                                const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
                                                int64_t sv_threshold, double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                                                int64_t chunks_per_batch, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out,
                                                mrp_profile_out *profiles_out, mrp_filtered_out *filtered_out, mrp_queue_stats *stats) {
    if (n_chunks > 0 && (!rest || !filtered_out)) return mrp_set_error(MRP_ERR_ARG, "mrp_queue_phase_string_chunks_with_filtered: null argument or bad sizes");
    if (filtered_out && n_chunks > 0) memset(filtered_out, 0, sizeof(*filtered_out) * (size_t) n_chunks);
    return queue_phase_string_chunks(q, n_chunks, chunks, rest, forward_model, reverse_model, expansion, sv_threshold, het_substitution_probability, params,
                                     min_phred, chunks_per_batch, out, hap_out, phred_out, profiles_out, filtered_out, stats);
}

int mrp_phase_string_chunks_with_filtered_on_devices(const int32_t *devices, int32_t n_devices, int64_t n_chunks, const mrp_string_chunk *chunks,
                                                     const mrp_string_chunk_rest *rest, const mrp_pair_hmm *forward_model,
                                                     const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold,
                                                     double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                                                     int64_t chunks_per_batch, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out,
                                                     mrp_profile_out *profiles_out, mrp_filtered_out *filtered_out, mrp_queue_stats *stats) {
    static const char *who = "mrp_phase_string_chunks_with_filtered_on_devices";
    return checked_on_devices(devices, n_devices, [&] {
        if (n_chunks > 0 && (!rest || !filtered_out)) return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", who);
        if (filtered_out && n_chunks > 0) memset(filtered_out, 0, sizeof(*filtered_out) * (size_t) n_chunks);
        return mrp_string_chunks_check(n_chunks, chunks, forward_model, reverse_model, expansion, params, out, hap_out, phred_out, rest, who);
    }, [&](mrp_queue *q) {
        return mrp_queue_phase_string_chunks_with_filtered(q, n_chunks, chunks, rest, forward_model, reverse_model, expansion, sv_threshold,
                                                           het_substitution_probability, params, min_phred, chunks_per_batch, out, hap_out, phred_out,
                                                           profiles_out, filtered_out, stats);
    });
}

int mrp_phase_string_chunks_on_devices(const int32_t *devices, int32_t n_devices, int64_t n_chunks, const mrp_string_chunk *chunks,
                                       const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold,
                                       double het_substitution_probability, const mrp_params *params, int64_t min_phred, int64_t chunks_per_batch,
                                       mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out,
                                       mrp_queue_stats *stats) {
    /* (the queue's own order of errors: a malformed call is MRP_ERR_ARG with or without a device) */
    return checked_on_devices(devices, n_devices, [&] {
        return mrp_string_chunks_check(n_chunks, chunks, forward_model, reverse_model, expansion, params, out, hap_out, phred_out, nullptr, "mrp_phase_string_chunks");
    }, [&](mrp_queue *q) {
        return mrp_queue_phase_string_chunks(q, n_chunks, chunks, forward_model, reverse_model, expansion, sv_threshold, het_substitution_probability, params,
                                             min_phred, chunks_per_batch, out, hap_out, phred_out, profiles_out, stats);
    });
}

}  /* extern "C" */

/* ---- aligned chunks: mrp_queue_phase_aligned_chunks (rest == NULL), mrp_queue_phase_aligned_chunks_with_filtered and
 * mrp_queue_phase_aligned_chunks_with_records (records_out beside filtered_out) -------------------------------------------------------- */
/* The (read, site) substrings uniform coverage gives a chunk: its bases x sites() / the length of its overlap, at most INT64_MAX
 * (B < 2^62 and the sites < 2^64: the product fits 128 bits).  The checks in the order of both entries: `negative_too` and
 * `no_genotypes` are what the entry's own second argument adds to them.  An error leaves *units_out alone. */
template <typename Sites>
static int aligned_units(const char *who, const mrp_aligned_chunk *chunk, int64_t *units_out, bool negative_too, bool no_genotypes, Sites sites) {
    if (!chunk || !units_out) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    const mrp_aligned_chunk &C = *chunk;
    if (C.n_reads < 0 || C.n_variants < 0 || negative_too) return mrp_set_error(MRP_ERR_ARG, "%s: negative count", who);
    if (C.overlap_end < C.overlap_start) return mrp_set_error(MRP_ERR_ARG, "%s: overlap_end before overlap_start", who);
    if (C.n_reads > 0 && !C.l_qseq) return mrp_set_error(MRP_ERR_ARG, "%s: null l_qseq", who);
    if (C.n_variants > 0 && no_genotypes) return mrp_set_error(MRP_ERR_ARG, "%s: null genotypes", who);
    unsigned __int128 bases = 0;
    for (int64_t r = 0; r < C.n_reads; r++) {
        if (C.l_qseq[r] < 0) return mrp_set_error(MRP_ERR_ARG, "%s: read %lld: negative l_qseq", who, (long long) r);
        bases += (unsigned __int128) C.l_qseq[r];
    }
    const unsigned __int128 length = (unsigned __int128) std::max<int64_t>(1, C.overlap_end - C.overlap_start);
    const unsigned __int128 units = bases * (unsigned __int128) sites(C) / length;
    *units_out = units > (unsigned __int128) INT64_MAX ? INT64_MAX : (int64_t) units;
    return MRP_OK;
}

extern "C" int mrp_aligned_chunk_units(const mrp_aligned_chunk *chunk, const mrp_aligned_chunk_rest *rest, int64_t *units_out) {
    return aligned_units("mrp_aligned_chunk_units", chunk, units_out, rest && rest->n_variants < 0, false, [&](const mrp_aligned_chunk &C) {
        return (unsigned __int128) C.n_variants + (unsigned __int128) (rest ? rest->n_variants : 0);
    });
}

namespace {

/* what a call of either entry carries beside the queue and the batch size */
struct AlignedQueueArgs {
    const char *who;
    mrp_aligned_args a;
    int64_t chunks_per_batch;
    mrp_queue_stats *stats;
    bool with_records = false;                     /* a.records_out is the caller's array: required, and travels with its chunk */
    mrp_queue_records_stats *records_stats = nullptr; /* may be NULL */
};

/* the entry's own null arguments, then every chunk's checks on the caller's thread and in the one call's order: MRP_ERR_ARG, then
 * MRP_ERR_UNSUPPORTED for the two refused extraction modes; no queue, no device */
int aligned_queue_check(const AlignedQueueArgs &A, bool with_rest) {
    const mrp_aligned_args &a = A.a;
    if (with_rest && (a.n_chunks < 0 || a.n_chunks >= (1ll << 30) || (a.n_chunks > 0 && (!a.chunks || !a.rest || !a.filtered_out || !a.filtered_read_out || (A.with_records && !a.records_out)))))
        return mrp_set_error(MRP_ERR_ARG, "%s: null argument or bad sizes", A.who);
    return mrp_aligned_chunks_check(A.who, &a);
}

/* (a batch's share of the records' stats to a lane's, the lanes' to the call's) */
template <typename Stats>
void add_records_stats(mrp_queue_records_stats &to, const Stats &b) {
    to.records_sites += b.records_sites;
    to.records_updated += b.records_updated;
    to.reads_listed += b.reads_listed;
    to.records_bytes_downloaded += b.records_bytes_downloaded;
    to.records_ms += b.records_ms;
}

/* aligned chunks to be phased: a batch as one mrp_phase_aligned_chunks(_with_filtered) call sees it: its chunks in plan order with what
 * travels with them, the call's outputs, and the front -- its host part (the extraction's records, the chunks' checks and windows) made
 * by the prefetch beside the lane's current batch, its device part staged on the lane's context when the batch is run */
struct AlignedBody {
    struct Staged : StagedBatch {
        std::vector<mrp_aligned_chunk> ch;
        std::vector<mrp_aligned_chunk_rest> rs;
        std::vector<const char *const *> names;
        std::vector<const uint8_t *> keep;
        std::vector<mrp_phase_result *> res;
        std::vector<int8_t *> hap;
        std::vector<double *> phred;
        std::vector<mrp_profile_out> prof;
        std::vector<int64_t *> bv;
        std::vector<mrp_filtered_out> fo;
        std::vector<int32_t *> fr;
        std::vector<mrp_variant_records> rec;                /* with records: the batch's records ... */
        std::vector<mrp_phase_aligned_records_stats> rst;    /* ... and, in one entry, its share of the records' stats */
        mrp_aligned_front *front = nullptr;
    };
    static constexpr bool on_stage_ctx = false;
    static constexpr const char *staged_line = "  [%7.1f] queue lane %d: checks and windows of batch %lld (%lld chunks) in %.1f ms\n";
    static constexpr const char *not_ready = "work queue: batch has no front";
    mrp_queue *q;
    const char *who;
    const mrp_aligned_args &a;
    const mrp_aligned_chunk_rest *rest; /* NULL: without the filtered half */
    bool records;
    std::vector<mrp_queue_records_stats> rec_per; /* [lane] what each lane's batches added to the records' stats */

    int stage(int, int, Staged &st, const int64_t *order) { /* host only: never the lane's context, its stream, its events or its pool */
        const double t_begin = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
        const size_t count = (size_t) st.count;
        const size_t n_rest = rest ? count : 0; /* (every array the call gets is as long as the batch or empty, its outputs zeroed) */
        st.ch.resize(count); st.names.resize(count); st.hap.resize(count); st.res.assign(count, nullptr);
        st.rs.resize(n_rest); st.fo.assign(n_rest, mrp_filtered_out{}); st.fr.assign(n_rest, nullptr);
        st.keep.resize(a.keep ? count : 0); st.phred.resize(a.phred_out ? count : 0);
        st.prof.assign(a.profiles_out ? count : 0, mrp_profile_out{}); st.bv.assign(a.bubble_variant_out ? count : 0, nullptr);
        st.rec.assign(records ? count : 0, mrp_variant_records{}); st.rst.assign(records ? 1 : 0, mrp_phase_aligned_records_stats{});
        for (size_t i = 0; i < count; i++) {
            const int64_t chunk = order[i];
            st.ch[i] = a.chunks[chunk];
            st.names[i] = a.read_names[chunk];
            st.hap[i] = a.hap_out[chunk];
            if (rest) st.rs[i] = rest[chunk];
            if (a.keep) st.keep[i] = a.keep[chunk];
            if (a.phred_out) st.phred[i] = a.phred_out[chunk];
        }
        mrp_aligned_args ba = a;
        ba.n_chunks = st.count;
        ba.chunks = st.ch.data();
        ba.rest = rest ? st.rs.data() : nullptr;
        ba.read_names = st.names.data();
        ba.keep = a.keep ? st.keep.data() : nullptr;
        ba.out = st.res.data();
        ba.hap_out = st.hap.data();
        ba.phred_out = a.phred_out ? st.phred.data() : nullptr;
        ba.profiles_out = a.profiles_out ? st.prof.data() : nullptr;
        ba.bubble_variant_out = a.bubble_variant_out ? st.bv.data() : nullptr;
        ba.filtered_out = rest ? st.fo.data() : nullptr;
        ba.filtered_read_out = rest ? st.fr.data() : nullptr;
        ba.records_out = records ? st.rec.data() : nullptr;
        ba.records_stats = records ? st.rst.data() : nullptr;
        return mrp_aligned_front_create(who, t_begin, &ba, nullptr, nullptr, &st.front);
    }
    int run(int w, Staged &st, const int64_t *order, QueueCall::PerLane &me, double *front_ms) {
        const auto t0 = std::chrono::steady_clock::now();
        mrp_string_chunks_stats ss{};
        int r = mrp_aligned_front_stage(q->ctx[(size_t) w], st.front);
        *front_ms = ms_since(t0);
        if (r == MRP_OK) r = mrp_aligned_front_run(st.front, &ss);
        if (r != MRP_OK) {
            for (mrp_variant_records &R : st.rec) mrp_variant_records_clear(&R); /* (a batch that failed behind its records hands none over) */
            return r;
        }
        if (records) add_records_stats(rec_per[(size_t) w], st.rst[0]);
        for (size_t i = 0; i < (size_t) st.count; i++) {
            const int64_t chunk = order[i];
            a.out[chunk] = st.res[i];
            if (records) { a.records_out[chunk] = st.rec[i]; memset(&st.rec[i], 0, sizeof(mrp_variant_records)); }
            if (a.profiles_out) a.profiles_out[chunk] = st.prof[i];
            if (a.bubble_variant_out) a.bubble_variant_out[chunk] = st.bv[i];
            if (rest) { a.filtered_out[chunk] = st.fo[i]; a.filtered_read_out[chunk] = st.fr[i]; }
        }
        count_fallback(me, ss.phase, st.count);
        return r;
    }
    void print_run(double since, int w, int64_t b, double all_ms, double front_ms) const {
        fprintf(stderr, "  [%7.1f] queue lane %d: batch %lld: device front in %.1f ms, run in %.1f ms\n", since, w, (long long) b, front_ms, all_ms - front_ms);
    }
    void drop(Staged &st) { mrp_aligned_front_destroy(st.front); st.front = nullptr; }
};

int queue_phase_aligned_chunks(mrp_queue *q, const AlignedQueueArgs &A, bool with_rest, bool checked = false) {
    const char *who = A.who;
    const mrp_aligned_args &a = A.a;
    const int64_t n_chunks = a.n_chunks;
    const mrp_aligned_chunk_rest *rest = with_rest ? a.rest : nullptr;
    mrp_queue_stats *stats = A.stats;
    const bool records = with_rest && A.with_records;
    int rc = checked ? (int) MRP_OK : aligned_queue_check(A, with_rest);
    if (rc != MRP_OK) return rc;
    if (!q) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no queue (the extraction and the pair-HMM have no CPU fallback)", who);
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_devices = (int) q->devices.size(); }
    for (int64_t i = 0; i < n_chunks; i++) {
        a.out[i] = nullptr;
        if (a.bubble_variant_out) a.bubble_variant_out[i] = nullptr;
        if (rest) a.filtered_read_out[i] = nullptr;
    }
    if (a.profiles_out && n_chunks > 0) memset(a.profiles_out, 0, sizeof(*a.profiles_out) * (size_t) n_chunks);
    if (rest && n_chunks > 0) memset(a.filtered_out, 0, sizeof(*a.filtered_out) * (size_t) n_chunks);
    if (records && n_chunks > 0) memset(a.records_out, 0, sizeof(*a.records_out) * (size_t) n_chunks);
    if (records && A.records_stats) memset(A.records_stats, 0, sizeof(*A.records_stats));
    if (n_chunks == 0) return MRP_OK;
    /* phase.c:257-263 orders by estimated depth; here by the (read, variant) substrings uniform coverage gives a chunk (a read the
     * extraction does not walk, l_qseq <= 0, passes its checks: such a chunk is ordered as if it cost nothing) */
    std::vector<int64_t> cost((size_t) n_chunks, 0);
    for (int64_t i = 0; i < n_chunks; i++)
        if (mrp_aligned_chunk_units(&a.chunks[i], rest ? &rest[i] : nullptr, &cost[(size_t) i]) != MRP_OK) cost[(size_t) i] = 0;
    AlignedBody body{q, who, a, rest, records, std::vector<mrp_queue_records_stats>(q->ctx.size(), mrp_queue_records_stats{})};
    rc = run_queue(q, n_chunks, cost, A.chunks_per_batch, stats, body, [&] {
        for (int64_t i = 0; i < n_chunks; i++) {
            mrp_phase_result_destroy(a.out[i]);
            a.out[i] = nullptr;
            if (a.profiles_out) mrp_profile_out_clear(&a.profiles_out[i]);
            if (a.bubble_variant_out) { free(a.bubble_variant_out[i]); a.bubble_variant_out[i] = nullptr; }
            if (rest) {
                mrp_filtered_out_clear(&a.filtered_out[i]);
                free(a.filtered_read_out[i]);
                a.filtered_read_out[i] = nullptr;
            }
            if (records) mrp_variant_records_clear(&a.records_out[i]);
        }
    });
    if (rc == MRP_OK && records && A.records_stats) /* in lane order: the sum of records_ms does not depend on which lane finished first */
        for (const mrp_queue_records_stats &b : body.rec_per) add_records_stats(*A.records_stats, b);
    return rc;
}

/* create + call + destroy, with the queue's own order of errors: a malformed call and a refused mode need no device */
int aligned_on_devices(const int32_t *devices, int32_t n_devices, const AlignedQueueArgs &A, bool with_rest) {
    return checked_on_devices(devices, n_devices, [&] { return aligned_queue_check(A, with_rest); },
                              [&](mrp_queue *q) { return queue_phase_aligned_chunks(q, A, with_rest, true); });
}

/* The arguments of the longest entry (with records); a shorter one passes NULL for what it has not.  q: the queue whose settings the
 * up-front checks read -- NULL (no queue, or none yet: *_on_devices) counts as all off, which is what a new queue has. */
AlignedQueueArgs aligned_queue_args(const char *who, const mrp_queue *q, int64_t n_chunks, const mrp_aligned_chunk *chunks, const mrp_aligned_chunk_rest *rest,
                                    const char *const *const *read_names, const uint8_t *const *keep, const mrp_extract_options *options,
                                    const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold,
                                    double het_substitution_probability, const mrp_params *params, int64_t min_phred, int64_t chunks_per_batch,
                                    mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out,
                                    int64_t **bubble_variant_out, mrp_filtered_out *filtered_out, int32_t **filtered_read_out, mrp_queue_stats *stats,
                                    bool with_records = false, mrp_variant_records *records_out = nullptr, mrp_queue_records_stats *records_stats = nullptr) {
    return {who,
            {n_chunks, chunks, rest, read_names, keep, options, forward_model, reverse_model, expansion, sv_threshold, het_substitution_probability, params,
             min_phred, out, hap_out, phred_out, profiles_out, bubble_variant_out, filtered_out, filtered_read_out, q ? q->sv_split : 0, records_out,
             /* records_stats: a batch's own */ nullptr, q ? q->max_depth : 0, q ? q->downsampling_seed : 0},
            chunks_per_batch, stats, with_records, records_stats};
}

}  // namespace

extern "C" {

int mrp_queue_phase_aligned_chunks(mrp_queue *q, int64_t n_chunks, const mrp_aligned_chunk *chunks, const char *const *const *read_names,
                                   const uint8_t *const *keep, const mrp_extract_options *options, const mrp_pair_hmm *forward_model,
                                   const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold, double het_substitution_probability,
                                   const mrp_params *params, int64_t min_phred, int64_t chunks_per_batch, mrp_phase_result **out, int8_t *const *hap_out,
                                   double *const *phred_out, mrp_profile_out *profiles_out, int64_t **bubble_variant_out, mrp_queue_stats *stats) {
    return queue_phase_aligned_chunks(q, aligned_queue_args("mrp_queue_phase_aligned_chunks", q, n_chunks, chunks, nullptr, read_names, keep, options, forward_model,
                                                            reverse_model, expansion, sv_threshold, het_substitution_probability, params, min_phred, chunks_per_batch,
                                                            out, hap_out, phred_out, profiles_out, bubble_variant_out, nullptr, nullptr, stats), false);
}

int mrp_queue_phase_aligned_chunks_with_filtered(mrp_queue *q, int64_t n_chunks, const mrp_aligned_chunk *chunks, const mrp_aligned_chunk_rest *rest,
                                                 const char *const *const *read_names, const uint8_t *const *keep, const mrp_extract_options *options,
                                                 const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
                                                 int64_t sv_threshold, double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                                                 int64_t chunks_per_batch, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out,
                                                 mrp_profile_out *profiles_out, int64_t **bubble_variant_out, mrp_filtered_out *filtered_out,
                                                 int32_t **filtered_read_out, mrp_queue_stats *stats) {
    return queue_phase_aligned_chunks(q, aligned_queue_args("mrp_queue_phase_aligned_chunks_with_filtered", q, n_chunks, chunks, rest, read_names, keep, options,
                                                            forward_model, reverse_model, expansion, sv_threshold, het_substitution_probability, params, min_phred,
                                                            chunks_per_batch, out, hap_out, phred_out, profiles_out, bubble_variant_out, filtered_out,
                                                            filtered_read_out, stats), true);
}

int mrp_queue_phase_aligned_chunks_with_records(mrp_queue *q, int64_t n_chunks, const mrp_aligned_chunk *chunks, const mrp_aligned_chunk_rest *rest,
                                                const char *const *const *read_names, const uint8_t *const *keep, const mrp_extract_options *options,
                                                const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
                                                int64_t sv_threshold, double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                                                int64_t chunks_per_batch, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out,
                                                mrp_profile_out *profiles_out, int64_t **bubble_variant_out, mrp_filtered_out *filtered_out,
                                                int32_t **filtered_read_out, mrp_variant_records *records_out, mrp_queue_stats *stats,
                                                mrp_queue_records_stats *records_stats) {
    return queue_phase_aligned_chunks(q, aligned_queue_args("mrp_queue_phase_aligned_chunks_with_records", q, n_chunks, chunks, rest, read_names, keep, options,
                                                            forward_model, reverse_model, expansion, sv_threshold, het_substitution_probability, params, min_phred,
                                                            chunks_per_batch, out, hap_out, phred_out, profiles_out, bubble_variant_out, filtered_out,
                                                            filtered_read_out, stats, true, records_out, records_stats), true);
}

int mrp_phase_aligned_chunks_with_records_on_devices(const int32_t *devices, int32_t n_devices, int64_t n_chunks, const mrp_aligned_chunk *chunks,
                                                     const mrp_aligned_chunk_rest *rest, const char *const *const *read_names, const uint8_t *const *keep,
                                                     const mrp_extract_options *options, const mrp_pair_hmm *forward_model,
                                                     const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold,
                                                     double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                                                     int64_t chunks_per_batch, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out,
                                                     mrp_profile_out *profiles_out, int64_t **bubble_variant_out, mrp_filtered_out *filtered_out,
                                                     int32_t **filtered_read_out, mrp_variant_records *records_out, mrp_queue_stats *stats,
                                                     mrp_queue_records_stats *records_stats) {
    return aligned_on_devices(devices, n_devices, aligned_queue_args("mrp_phase_aligned_chunks_with_records_on_devices", nullptr, n_chunks, chunks, rest, read_names,
                                                                     keep, options, forward_model, reverse_model, expansion, sv_threshold,
                                                                     het_substitution_probability, params, min_phred, chunks_per_batch, out, hap_out, phred_out,
                                                                     profiles_out, bubble_variant_out, filtered_out, filtered_read_out, stats, true, records_out,
                                                                     records_stats), true);
}

int mrp_phase_aligned_chunks_on_devices(const int32_t *devices, int32_t n_devices, int64_t n_chunks, const mrp_aligned_chunk *chunks,
                                        const char *const *const *read_names, const uint8_t *const *keep, const mrp_extract_options *options,
                                        const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold,
                                        double het_substitution_probability, const mrp_params *params, int64_t min_phred, int64_t chunks_per_batch,
                                        mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out,
                                        int64_t **bubble_variant_out, mrp_queue_stats *stats) {
    return aligned_on_devices(devices, n_devices, aligned_queue_args("mrp_phase_aligned_chunks_on_devices", nullptr, n_chunks, chunks, nullptr, read_names, keep, options,
                                                                     forward_model, reverse_model, expansion, sv_threshold, het_substitution_probability, params,
                                                                     min_phred, chunks_per_batch, out, hap_out, phred_out, profiles_out, bubble_variant_out, nullptr,
                                                                     nullptr, stats), false);
}

int mrp_phase_aligned_chunks_with_filtered_on_devices(const int32_t *devices, int32_t n_devices, int64_t n_chunks, const mrp_aligned_chunk *chunks,
                                                      const mrp_aligned_chunk_rest *rest, const char *const *const *read_names, const uint8_t *const *keep,
                                                      const mrp_extract_options *options, const mrp_pair_hmm *forward_model,
                                                      const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold,
                                                      double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                                                      int64_t chunks_per_batch, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out,
                                                      mrp_profile_out *profiles_out, int64_t **bubble_variant_out, mrp_filtered_out *filtered_out,
                                                      int32_t **filtered_read_out, mrp_queue_stats *stats) {
    return aligned_on_devices(devices, n_devices, aligned_queue_args("mrp_phase_aligned_chunks_with_filtered_on_devices", nullptr, n_chunks, chunks, rest, read_names,
                                                                     keep, options, forward_model, reverse_model, expansion, sv_threshold,
                                                                     het_substitution_probability, params, min_phred, chunks_per_batch, out, hap_out, phred_out,
                                                                     profiles_out, bubble_variant_out, filtered_out, filtered_read_out, stats), true);
}

}  /* extern "C" */

/* ---- haplotagging aligned chunks from a phased VCF: mrp_queue_haplotag_aligned_chunks ------------------------------------------------ */
extern "C" int mrp_haplotag_chunk_units(const mrp_aligned_chunk *chunk, const int32_t *gt, int64_t *units_out) {
    /* only a heterozygous variant is scored (bubbleGraph.c:1975): the chunk's pair-HMM work, not its variant count */
    return aligned_units("mrp_haplotag_chunk_units", chunk, units_out, false, !gt, [&](const mrp_aligned_chunk &C) {
        unsigned __int128 het = 0;
        for (int64_t v = 0; v < C.n_variants; v++) het += gt[2 * v] != gt[2 * v + 1];
        return het;
    });
}

namespace {

struct HaplotagQueueArgs {
    mrp_haplotag_args a;
    int64_t chunks_per_batch;
    mrp_queue_stats *stats;
};

/* aligned chunks to be haplotagged: a batch as one mrp_haplotag_aligned_chunks call sees it: its chunks in plan order with their
 * genotypes and output arrays, and the front -- its host part (the extraction's records, the checks, the windows) made by the prefetch
 * beside the lane's current batch, its device part staged on the lane's context when the batch is run */
struct HaplotagBody {
    struct Staged : StagedBatch {
        std::vector<mrp_aligned_chunk> ch;
        std::vector<const int32_t *> gt;
        std::vector<int8_t *> hap;
        std::vector<double *> h1, h2;
        mrp_haplotag_front *front = nullptr;
    };
    static constexpr bool on_stage_ctx = false;
    static constexpr const char *staged_line = "  [%7.1f] queue lane %d: checks and windows of batch %lld (%lld chunks) in %.1f ms\n";
    static constexpr const char *not_ready = "work queue: batch has no front";
    mrp_queue *q;
    const mrp_haplotag_args &a;

    int stage(int, int, Staged &st, const int64_t *order) { /* host only: never the lane's context, its stream, its events or its pool */
        const size_t count = (size_t) st.count;
        st.ch.resize(count); st.gt.resize(count); st.hap.resize(count);
        st.h1.resize(a.h1_out ? count : 0);
        st.h2.resize(a.h2_out ? count : 0);
        for (size_t i = 0; i < count; i++) {
            const int64_t chunk = order[i];
            st.ch[i] = a.chunks[chunk];
            st.gt[i] = a.gt[chunk];
            st.hap[i] = a.hap_out[chunk];
            if (a.h1_out) st.h1[i] = a.h1_out[chunk];
            if (a.h2_out) st.h2[i] = a.h2_out[chunk];
        }
        mrp_haplotag_args ba = a;
        ba.n_chunks = st.count;
        ba.chunks = st.ch.data();
        ba.gt = st.gt.data();
        ba.hap_out = st.hap.data();
        ba.h1_out = a.h1_out ? st.h1.data() : nullptr;
        ba.h2_out = a.h2_out ? st.h2.data() : nullptr;
        return mrp_haplotag_front_create(&ba, nullptr, &st.front);
    }
    int run(int w, Staged &st, const int64_t *, QueueCall::PerLane &, double *front_ms) { /* (no fallback to count: nothing is phased) */
        const auto t0 = std::chrono::steady_clock::now();
        int r = mrp_haplotag_front_stage(q->ctx[(size_t) w], st.front);
        *front_ms = ms_since(t0);
        if (r == MRP_OK) r = mrp_haplotag_front_run(st.front); /* (writes the batch's outputs at the chunks' own arrays) */
        return r;
    }
    void print_run(double since, int w, int64_t b, double all_ms, double front_ms) const {
        fprintf(stderr, "  [%7.1f] queue lane %d: batch %lld: extraction and owners in %.1f ms, pairs and scoring in %.1f ms\n", since, w, (long long) b,
                front_ms, all_ms - front_ms);
    }
    void drop(Staged &st) { mrp_haplotag_front_destroy(st.front); st.front = nullptr; }
};

int queue_haplotag_aligned_chunks(mrp_queue *q, const HaplotagQueueArgs &A, bool checked = false) {
    static const char *who = "mrp_queue_haplotag_aligned_chunks";
    const mrp_haplotag_args &a = A.a;
    const int64_t n_chunks = a.n_chunks;
    mrp_queue_stats *stats = A.stats;
    /* every chunk's checks on the caller's thread, in the one call's order and with its messages: MRP_ERR_ARG, then the refused modes */
    int rc = checked ? (int) MRP_OK : mrp_haplotag_chunks_check(&a);
    if (rc != MRP_OK) return rc;
    if (!q) return mrp_set_error(MRP_ERR_NO_DEVICE, "%s: no queue (the extraction and the pair-HMM have no CPU fallback)", who);
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_devices = (int) q->devices.size(); }
    if (n_chunks == 0) return MRP_OK;
    /* tools/tagFromPhasedVcf.c:208-225 orders the chunks largest first; here by the (read, het variant) substrings uniform coverage gives */
    std::vector<int64_t> cost((size_t) n_chunks, 0);
    for (int64_t i = 0; i < n_chunks; i++)
        if (mrp_haplotag_chunk_units(&a.chunks[i], a.gt[i], &cost[(size_t) i]) != MRP_OK) cost[(size_t) i] = 0;
    HaplotagBody body{q, a};
    return run_queue(q, n_chunks, cost, A.chunks_per_batch, stats, body, [] {}); /* (an error leaves the outputs unspecified) */
}

}  // namespace

extern "C" {

int mrp_queue_haplotag_aligned_chunks(mrp_queue *q, int64_t n_chunks, const mrp_aligned_chunk *chunks, const int32_t *const *gt,
                                      const mrp_extract_options *options, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model,
                                      int64_t expansion, int64_t chunks_per_batch, int8_t *const *hap_out, double *const *h1_out,
                                      double *const *h2_out, mrp_queue_stats *stats) {
    const HaplotagQueueArgs A{{n_chunks, chunks, gt, options, forward_model, reverse_model, expansion, hap_out, h1_out, h2_out, q ? q->sv_split : 0},
                              chunks_per_batch, stats};
    return queue_haplotag_aligned_chunks(q, A);
}

int mrp_haplotag_aligned_chunks_on_devices(const int32_t *devices, int32_t n_devices, int64_t n_chunks, const mrp_aligned_chunk *chunks,
                                           const int32_t *const *gt, const mrp_extract_options *options, const mrp_pair_hmm *forward_model,
                                           const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t chunks_per_batch, int8_t *const *hap_out,
                                           double *const *h1_out, double *const *h2_out, mrp_queue_stats *stats) {
    const HaplotagQueueArgs A{{n_chunks, chunks, gt, options, forward_model, reverse_model, expansion, hap_out, h1_out, h2_out}, chunks_per_batch, stats};
    return checked_on_devices(devices, n_devices, [&] { return mrp_haplotag_chunks_check(&A.a); },
                              [&](mrp_queue *q) { return queue_haplotag_aligned_chunks(q, A, true); });
}

}  /* extern "C" */
