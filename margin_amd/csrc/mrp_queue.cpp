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
#include <system_error>
#include <mutex>
#include <numeric>
#include <string>
#include <thread>
#include <vector>

#include <pthread.h>
#include <sched.h>
#include <cctype>

#include "mrp_internal.h"

int mrp_queue_threads_per_device(int n_devices);

namespace {

struct QueuePlan {
    std::vector<int64_t> order;     /* chunk indices, largest estimated cost first (ties: input order) */
    std::vector<int64_t> batch_off; /* batch b = order[batch_off[b] .. batch_off[b + 1]) */
};

/* phase.c:257-263: sort by estimated size, largest first; then cut into batches of consecutive chunks.
 * chunks_per_batch >= 1: batches of that many chunks.  0: the library's choice for n_workers pulling threads on n_devices
 * devices.  A batch is one mrp_phase_reads_many call; a call begins and ends with host work and walks its merge levels one
 * after the other, the top ones bound by per-column latency whatever the number of chunks.  A short queue (up to 1 280 chunks
 * of the 1 Mb kind per device -- 640 through round 3, when a device held twice as much per chunk; sizes are counted in units, below) is ONE batch per device: the call runs it as eight concurrent batches of its own (576 chunks: 170-182 ms).  A
 * longer one is handed out in batches of MRP_QUEUE_DEFAULT_BATCH chunks to the lanes of the devices (four per device, each
 * call two concurrent batches: the same eight in flight, but at different levels -- while one lane is in its host-bound
 * head or its latency-bound top levels the others stream; measured on 2 304 chunks: 153-160 ms per 576 against 174-177 for
 * one lane of 576-chunk calls), shrinking towards the end (several devices: "guided" schedule, remaining / workers, at least 96) so that the
 * devices finish within two percent of each other (tests/test_work_queue.py: 8 devices, 31 000 chunks) without the tail of
 * the queue dissolving into small, latency-bound calls. */
QueuePlan plan_queue(int64_t n, const int64_t *cost, int64_t chunks_per_batch, int n_workers = 1, int n_devices = 1) {
    QueuePlan p;
    p.order.resize((size_t) n);
    std::iota(p.order.begin(), p.order.end(), (int64_t) 0);
    std::stable_sort(p.order.begin(), p.order.end(), [&](int64_t a, int64_t b) { return cost[a] > cost[b]; });
    /* Sizes are counted in UNITS (a chunk's cost: its reads x the het sites they span), with the 1 Mb, 30x chunk of
     * BASELINE.json configs[1] (60 000 units) as the yardstick the policy was measured on: what a call costs the device and
     * what it keeps there grow with its units, not with its chunks -- 192 chunks of 130 sites would be a call of 9 ms. */
    const int64_t unit_chunk = MRP_QUEUE_UNITS_PER_CHUNK;
    const int64_t big = MRP_QUEUE_DEFAULT_BATCH * unit_chunk, short_queue = MRP_QUEUE_SHORT_CHUNKS * unit_chunk;
    auto units = [&](int64_t pos) { return std::max<int64_t>(1, cost[p.order[(size_t) pos]]); };
    int64_t total = 0;
    for (int64_t i = 0; i < n; i++) total += units(i);
    if (chunks_per_batch >= 1) {
        for (int64_t o = 0; o < n; o += chunks_per_batch) p.batch_off.push_back(o);
    } else if (total <= (int64_t) n_devices * short_queue) {
        /* up to MRP_QUEUE_SHORT_CHUNKS yardstick chunks per device ONE call per device is the fastest */
        const int64_t parts = std::min<int64_t>(n, n_devices);
        /* these batches all start at once: deal the chunks out in stripes (batch b takes the b-th, (b + parts)-th, ... of the
         * cost order), so that every batch gets its share of the expensive ones -- consecutive runs of a largest-first order
         * would make the first batch the slowest by a third */
        std::vector<int64_t> striped;
        striped.reserve((size_t) n);
        for (int64_t b = 0; b < parts; b++) {
            p.batch_off.push_back((int64_t) striped.size());
            for (int64_t i = b; i < n; i += parts) striped.push_back(p.order[(size_t) i]);
        }
        p.order.swap(striped);
    } else {
        int64_t left = total;
        /* one device: its lanes share it, so there is nothing to even out between them towards the end -- but they should all be
         * busy to the end: as many equal batches as fill whole rounds of the lanes (1 152 chunks on four lanes: 8 batches of 144
         * rather than 6 of 192, of which the last two would run on half the lanes) */
        const int64_t lanes_of_device = std::max(1, n_workers / std::max(1, n_devices));
        const int64_t rounds = (total + lanes_of_device * big - 1) / (lanes_of_device * big);
        const int64_t even = (total + rounds * lanes_of_device - 1) / (rounds * lanes_of_device);
        for (int64_t o = 0; o < n;) { /* several devices: full batches while every lane can still get two, then shrinking, at least a quarter batch */
            p.batch_off.push_back(o);
            /* (a lane holds two batches, the one it phases and the one it took ahead: what is left is shared out as if there were
             * twice the lanes; the floor of a quarter batch keeps the tail from dissolving into latency-bound calls) */
            const int64_t target = n_devices > 1 ? std::max<int64_t>(big / 4, std::min<int64_t>(big, left / (2 * (int64_t) std::max(1, n_workers)))) : even;
            int64_t got = 0;
            do { got += units(o); o++; } while (o < n && got + units(o) / 2 < target);
            if (left - got < target / 2) /* (what would be left is no batch of its own) */
                while (o < n) { got += units(o); o++; }
            left -= got;
        }
    }
    p.batch_off.push_back(n);
    return p;
}

/* How many calls of a device run at a time: a device holds what its calls in flight need (some 170 MB per 1 Mb chunk = 60 000 units,
 * DevPool): four lanes for batches of up to 288 such chunks, two up to 576, one beyond; a queue of no more batches than
 * devices needs one lane each. */
int active_lanes_of(const QueuePlan &plan, const int64_t *cost, int n_devices, int lanes) {
    const int64_t n_batches = (int64_t) plan.batch_off.size() - 1;
    int64_t max_batch = 0;
    for (int64_t b = 0; b < n_batches; b++) {
        int64_t u = 0;
        for (int64_t i = plan.batch_off[(size_t) b]; i < plan.batch_off[(size_t) b + 1]; i++) u += cost[(size_t) plan.order[(size_t) i]];
        max_batch = std::max(max_batch, u);
    }
    const int64_t yard = MRP_QUEUE_UNITS_PER_CHUNK;
    return n_batches <= (int64_t) n_devices ? 1 : (max_batch <= 288 * yard ? lanes : (max_batch <= 576 * yard ? std::min(lanes, 2) : 1));
}

/* The hand-out of the queue, shared by the real workers and the dry run: lane w = device w / lanes; a lane that is active takes
 * its first batch (fixed, below), then -- schedule(dynamic,1), one batch ahead -- takes its NEXT batch when it starts on the current one
 * (`prefetch(w, next batch)` runs beside `phase(w, current batch)`: the real worker uploads there) and goes on until the shared
 * counter runs out.  A lane without a first batch does nothing (no contexts, no streams).  begin(w) / end(w) bracket a lane that
 * got work; any non-zero status stops the queue.  Every lane is a host thread; lane 0 runs on the caller's thread unless
 * `own_thread_for_lane0`. */
struct LaneHooks {
    std::function<int(int)> begin;                     /* lane */
    std::function<int(int, int64_t)> prefetch;         /* lane, batch: may run on another thread than phase */
    std::function<int(int, int64_t)> phase;            /* lane, batch */
    std::function<void(int, int64_t)> retire;          /* lane, batch: after phase AND after the prefetch that ran beside it has ended */
    std::function<void(int, int64_t)> discard;         /* lane, batch: a prefetched batch that will not be phased */
    std::function<void(int)> end;
};
int run_lanes(int n_devices, int lanes, int active_lanes, int64_t n_batches, const LaneHooks &hk, bool own_thread_for_lane0,
              const std::function<void(int)> &on_thread_start) {
    const int n_workers = n_devices * lanes;
    /* The FIRST batch of a lane is fixed: batch (lane of device) * n_devices + device, so the largest batches start on different
     * devices and no lane that starts early can take (and, one ahead, reserve) the work of a device whose thread is not up yet --
     * with as many batches as devices every device gets exactly one.  From there on the hand-out is dynamic. */
    std::atomic<int64_t> next{std::min<int64_t>(n_batches, (int64_t) n_devices * active_lanes)};
    std::atomic<int> status{MRP_OK};
    auto fail = [&](int rc) { int expect = MRP_OK; status.compare_exchange_strong(expect, rc); };
    auto work = [&](int w) {
        if (on_thread_start) on_thread_start(w);
        if (w % lanes >= active_lanes) return; /* (large caller-chosen batches: fewer calls of a device in flight) */
        const int64_t first = (int64_t) (w % lanes) * n_devices + w / lanes;
        if (first >= n_batches) return;
        int rc = hk.begin ? hk.begin(w) : MRP_OK;
        if (rc != MRP_OK) { fail(rc); return; }
        rc = hk.prefetch ? hk.prefetch(w, first) : MRP_OK;
        int64_t cur = first;
        while (cur >= 0) {
            if (rc != MRP_OK) { fail(rc); if (hk.discard) hk.discard(w, cur); break; }
            if (status.load() != MRP_OK) { if (hk.discard) hk.discard(w, cur); break; }
            const int64_t nb = next.fetch_add(1);
            int prc = MRP_OK;
            std::thread stager;
            bool inline_stage = false;
            if (nb < n_batches && hk.prefetch) {
                try { stager = std::thread([&, nb] { prc = hk.prefetch(w, nb); }); }
                catch (const std::system_error &) { inline_stage = true; } /* no thread to be had: stage after the call instead */
            }
            rc = hk.phase(w, cur);
            if (stager.joinable()) stager.join();
            if (hk.retire) hk.retire(w, cur); /* (what the batch held goes back with no other thread of the lane at work) */
            if (inline_stage) prc = hk.prefetch(w, nb);
            if (rc != MRP_OK) { fail(rc); if (nb < n_batches && hk.discard) hk.discard(w, nb); break; }
            cur = nb < n_batches ? nb : -1;
            rc = prc;
        }
        if (hk.end) hk.end(w);
    };
    std::vector<std::thread> th;
    std::vector<int> inline_lanes; /* lanes whose thread could not be created run on the caller's thread, after lane 0 */
    for (int w = 1; w < n_workers; w++) {
        try { th.emplace_back(work, w); }
        catch (const std::system_error &) { inline_lanes.push_back(w); }
    }
    if (own_thread_for_lane0) {
        bool started = false;
        try { std::thread t0(work, 0); started = true; t0.join(); }
        catch (const std::system_error &) { if (!started) work(0); }
    } else work(0);
    for (int w : inline_lanes) work(w);
    for (auto &t : th) t.join();
    return status.load();
}

}  // namespace

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

    /* runs the lanes; when the queue drives more than one device, each on the CPUs next to its device */
    int run(const LaneHooks &hk) {
        const int n_devices = (int) q->devices.size(), lanes = q->lanes;
        const char *aff_env = getenv("MRP_QUEUE_AFFINITY");
        const bool bind = n_devices > 1 && !(aff_env && aff_env[0] == '0');
        /* before the first thread of a worker is created (they inherit it): the CPUs next to its device */
        std::function<void(int)> on_start;
        if (bind) on_start = [this, lanes](int w) {
            cpu_set_t set;
            if (device_cpuset(q->devices[(size_t) (w / lanes)], &set)) (void) pthread_setaffinity_np(pthread_self(), sizeof(set), &set);
        };
        const int rc = run_lanes(n_devices, lanes, active_lanes, n_batches, hk, /* the caller's own affinity is left alone */ bind, on_start);
        if (timing) fprintf(stderr, "  [%7.1f] queue: workers joined\n", since());
        return rc;
    }
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

/* What the bodies whose prefetch makes a host front share (string chunks, aligned chunks phased and haplotagged): a lane's two staged batches -- the one it runs and the one its
 * prefetch makes beside it -- and the create + call + destroy of the *_on_devices forms. */
template <typename Staged>
struct LaneSlots {
    Staged st[2];
    int n_staged = 0;
    Staged *next() { return &st[n_staged++ & 1]; } /* (the stager fills the slot the call's thread is not running) */
    Staged *find(int64_t b) { return st[0].batch.load() == b ? &st[0] : (st[1].batch.load() == b ? &st[1] : nullptr); }
};
static double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
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

extern "C" {

int mrp_queue_phase_chunks(mrp_queue *q, int64_t n_chunks, const mrp_chunk_desc *chunks, const mrp_params *params, int64_t chunks_per_batch,
                           mrp_phase_result **out, mrp_queue_stats *stats) {
    if (!q || n_chunks < 0 || !params || (n_chunks > 0 && (!chunks || !out))) return mrp_set_error(MRP_ERR_ARG, "mrp_queue_phase_chunks: bad arguments");
    const int n_devices = (int) q->devices.size();
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_devices = n_devices; }
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
    const int lanes = q->lanes, n_workers = n_devices * lanes;
    const QueuePlan plan = plan_queue(n_chunks, cost.data(), chunks_per_batch, n_workers, n_devices);
    const int64_t n_batches = (int64_t) plan.batch_off.size() - 1;
    if (stats) stats->batches = n_batches;

    QueueCall call(q, n_batches, active_lanes_of(plan, cost.data(), n_devices, lanes));
    std::vector<std::string> &errs = call.errs, &stage_errs = call.stage_errs;
    std::vector<QueueCall::PerLane> &per = call.per;

    /* the chunks of one batch on the device (uploads queued on the staging context's stream; the chunks carry the event that
     * ends the upload, the first device work that reads one waits for it) */
    struct Staged {
        std::atomic<int64_t> batch{-1}; /* (the call's thread looks its batch up while the stager fills the lane's OTHER slot) */
        int64_t first = 0, count = 0;
        std::vector<mrp_chunk *> dch;
    };
    struct Lane { Staged st[2]; int n_staged = 0; };
    std::vector<Lane> lane_state((size_t) n_workers);
    const bool timing = call.timing;
    auto since = [&]() { return call.since(); };
    auto drop = [&](Staged *st) { /* (a thousand chunks of a one-call queue: on the lane's pool, not one after the other) */
        mrp_parallel_for((int64_t) st->dch.size(), 8, [&](int64_t i) { if (st->dch[(size_t) i]) mrp_chunk_destroy(st->dch[(size_t) i]); });
        st->dch.clear();
        st->batch = -1;
    };
    auto staged_of = [&](int w, int64_t b) -> Staged * {
        Lane &L = lane_state[(size_t) w];
        return L.st[0].batch.load() == b ? &L.st[0] : (L.st[1].batch.load() == b ? &L.st[1] : nullptr);
    };
    LaneHooks hk;
    hk.begin = [&](int w) { return call.lane_begin(w, true); };
    hk.prefetch = [&](int w, int64_t b) { /* (the first batch on the lane's thread, the later ones on a thread beside the call) */
        const auto ts0 = std::chrono::steady_clock::now();
        const int d = w / lanes;
        mrp_pool_adopt(q->pools[(size_t) d]);
        Lane &L = lane_state[(size_t) w];
        const int parity = L.n_staged++ & 1;
        Staged *st = &L.st[parity];
        st->first = plan.batch_off[(size_t) b]; st->count = plan.batch_off[(size_t) b + 1] - st->first;
        st->dch.assign((size_t) st->count, nullptr);
        st->batch.store(b);
        mrp_context *sc = q->stage_ctx[(size_t) w];
        sc->pool.reclaim(); /* the block of the batch before last was emptied after its call returned */
        mrp_chunk_block *&blk = q->blocks[(size_t) w * 2 + (size_t) parity];
        if (!blk) blk = new (std::nothrow) mrp_chunk_block();
        std::vector<const mrp_chunk_desc *> dl((size_t) st->count);
        for (int64_t i = 0; i < st->count; i++) dl[(size_t) i] = &chunks[plan.order[(size_t) (st->first + i)]];
        /* (uploaded in the groups the call will deal the chunks to: its first batch starts on the device when an eighth of the bytes is there) */
        const int rc = blk ? mrp_chunk_block_create(sc, st->count, dl.data(), st->dch.data(), blk, mrp_phase_groups_for(q->ctx[(size_t) w], st->count))
                           : mrp_set_error(MRP_ERR_NOMEM, "out of host memory");
        if (rc != MRP_OK) stage_errs[(size_t) w] = mrp_last_error();
        if (timing) fprintf(stderr, "  [%7.1f] queue lane %d: batch %lld (%lld chunks) staged in %.1f ms\n", since(), w, (long long) b, (long long) st->count,
                            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - ts0).count());
        return rc;
    };
    hk.discard = [&](int w, int64_t b) { if (Staged *st = staged_of(w, b)) drop(st); };
    hk.phase = [&](int w, int64_t b) {
        Staged *cur = staged_of(w, b);
        if (!cur) { errs[(size_t) w] = "work queue: batch was not staged"; return (int) MRP_ERR_ARG; }
        auto t0 = std::chrono::steady_clock::now();
        const int64_t count = cur->count;
        std::vector<const mrp_chunk *> cch((size_t) count);
        std::vector<const mrp_read *> rd((size_t) count);
        std::vector<int64_t> nr((size_t) count);
        std::vector<mrp_phase_result *> res((size_t) count, nullptr);
        for (int64_t i = 0; i < count; i++) {
            const mrp_chunk_desc &c = chunks[plan.order[(size_t) (cur->first + i)]];
            cch[(size_t) i] = cur->dch[(size_t) i]; rd[(size_t) i] = c.reads; nr[(size_t) i] = c.n_reads;
        }
        mrp_phase_many_stats ps{};
        const int r = mrp_phase_reads_many(q->ctx[(size_t) w], count, cch.data(), rd.data(), nr.data(), params, res.data(), &ps);
        if (r != MRP_OK) errs[(size_t) w] = mrp_last_error();
        for (int64_t i = 0; i < count; i++) {
            const int64_t chunk = plan.order[(size_t) (cur->first + i)];
            if (r == MRP_OK) { out[chunk] = res[(size_t) i]; per[(size_t) w].units += cost[(size_t) chunk]; }
        }
        if (r == MRP_OK) { per[(size_t) w].chunks += count; per[(size_t) w].fallback += ps.resident ? ps.fallback_chunks : count; }
        if (timing) fprintf(stderr, "  [%7.1f] queue lane %d: batch %lld phased in %.1f ms\n", since(), w, (long long) b,
                            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
        per[(size_t) w].busy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        return r;
    };
    /* the batch's chunks live on the lane's STAGING context, on which the stager thread makes the next batch's block while the call
     * runs: they are destroyed after that thread has ended (one host thread per context, include/margin_rphmm.h) */
    hk.retire = [&](int w, int64_t b) {
        const auto t0 = std::chrono::steady_clock::now();
        if (Staged *st = staged_of(w, b)) drop(st);
        per[(size_t) w].busy_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    hk.end = [&](int w) { call.lane_end(w); };
    const int rc = call.run(hk);
    call.fill(stats);
    if (rc != MRP_OK) {
        for (int64_t i = 0; i < n_chunks; i++) { mrp_phase_result_destroy(out[i]); out[i] = nullptr; }
        return call.error(rc);
    }
    return MRP_OK;
}

int mrp_phase_chunks_on_devices(const int32_t *devices, int32_t n_devices, int64_t n_chunks, const mrp_chunk_desc *chunks,
                                const mrp_params *params, int64_t chunks_per_batch, mrp_phase_result **out, mrp_queue_stats *stats) {
    mrp_queue *q = nullptr;
    int rc = mrp_queue_create(devices, n_devices, &q);
    if (rc == MRP_OK) rc = mrp_queue_phase_chunks(q, n_chunks, chunks, params, chunks_per_batch, out, stats);
    mrp_queue_destroy(q);
    return rc;
}

}  /* extern "C" */

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
    const int n_devices = (int) q->devices.size();
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_devices = n_devices; }
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
    const int lanes = q->lanes, n_workers = n_devices * lanes;
    const QueuePlan plan = plan_queue(n_chunks, cost.data(), chunks_per_batch, n_workers, n_devices);
    const int64_t n_batches = (int64_t) plan.batch_off.size() - 1;
    if (stats) stats->batches = n_batches;
    QueueCall call(q, n_batches, active_lanes_of(plan, cost.data(), n_devices, lanes));

    /* a batch as one mrp_phase_string_chunks call sees it: its chunks side by side, and the host front made of them (prefetch:
     * beside the device work of the lane's current batch; the uploads follow on the lane's own stream when the batch is run) */
    struct Staged {
        std::atomic<int64_t> batch{-1}; /* (the call's thread looks its batch up while the stager fills the lane's OTHER slot) */
        int64_t first = 0, count = 0;
        std::vector<mrp_string_chunk> sc;
        std::vector<mrp_string_chunk_rest> sr;
        mrp_string_front *front = nullptr;
    };
    std::vector<LaneSlots<Staged>> lane_state((size_t) n_workers);
    auto staged_of = [&](int w, int64_t b) { return lane_state[(size_t) w].find(b); };
    auto drop = [&](Staged *st) { mrp_string_front_destroy(st->front); st->front = nullptr; st->batch = -1; };
    LaneHooks hk;
    hk.begin = [&](int w) { return call.lane_begin(w, false); };
    hk.prefetch = [&](int w, int64_t b) {
        const auto t0 = std::chrono::steady_clock::now();
        mrp_pool_adopt(q->pools[(size_t) (w / lanes)]);
        Staged *st = lane_state[(size_t) w].next();
        st->first = plan.batch_off[(size_t) b]; st->count = plan.batch_off[(size_t) b + 1] - st->first;
        st->sc.resize((size_t) st->count);
        for (int64_t i = 0; i < st->count; i++) st->sc[(size_t) i] = chunks[plan.order[(size_t) (st->first + i)]];
        st->sr.resize(rest ? (size_t) st->count : 0);
        for (int64_t i = 0; rest && i < st->count; i++) st->sr[(size_t) i] = rest[plan.order[(size_t) (st->first + i)]];
        st->batch.store(b);
        const int r = mrp_string_front_create(st->count, st->sc.data(), rest ? st->sr.data() : nullptr, forward_model, reverse_model, expansion, sv_threshold,
                                              q->wide_pairs, &st->front);
        if (r != MRP_OK) call.stage_errs[(size_t) w] = mrp_last_error();
        if (call.timing) fprintf(stderr, "  [%7.1f] queue lane %d: front of batch %lld (%lld chunks) in %.1f ms\n", call.since(), w, (long long) b, (long long) st->count, ms_since(t0));
        return r;
    };
    hk.discard = [&](int w, int64_t b) { if (Staged *st = staged_of(w, b)) drop(st); };
    hk.phase = [&](int w, int64_t b) {
        Staged *cur = staged_of(w, b);
        if (!cur || !cur->front) { call.errs[(size_t) w] = "work queue: batch has no front"; return (int) MRP_ERR_ARG; }
        const auto t0 = std::chrono::steady_clock::now();
        const int64_t count = cur->count;
        std::vector<mrp_phase_result *> res((size_t) count, nullptr);
        std::vector<int8_t *> hap((size_t) count);
        std::vector<double *> phred((size_t) count);
        std::vector<mrp_profile_out> prof(profiles_out ? (size_t) count : 0);
        if (profiles_out) memset(prof.data(), 0, sizeof(mrp_profile_out) * prof.size());
        for (int64_t i = 0; i < count; i++) {
            const int64_t chunk = plan.order[(size_t) (cur->first + i)];
            hap[(size_t) i] = hap_out[chunk];
            if (phred_out) phred[(size_t) i] = phred_out[chunk];
        }
        std::vector<mrp_filtered_out> fo(rest ? (size_t) count : 0);
        if (rest) memset(fo.data(), 0, sizeof(mrp_filtered_out) * fo.size());
        mrp_string_chunks_stats ss;
        memset(&ss, 0, sizeof(ss));
        const int r = mrp_string_front_run(q->ctx[(size_t) w], cur->front, het_substitution_probability, params, min_phred, res.data(), hap.data(),
                                           phred_out ? phred.data() : nullptr, profiles_out ? prof.data() : nullptr, &ss, rest ? fo.data() : nullptr, nullptr);
        QueueCall::PerLane &me = call.per[(size_t) w];
        if (r != MRP_OK) call.errs[(size_t) w] = mrp_last_error();
        else {
            for (int64_t i = 0; i < count; i++) {
                const int64_t chunk = plan.order[(size_t) (cur->first + i)];
                out[chunk] = res[(size_t) i];
                if (profiles_out) profiles_out[chunk] = prof[(size_t) i];
                if (rest) filtered_out[chunk] = fo[(size_t) i];
                me.units += cost[(size_t) chunk];
            }
            me.chunks += count;
            me.fallback += ss.phase.resident ? ss.phase.fallback_chunks : count;
        }
        const double run_ms = ms_since(t0);
        if (call.timing) fprintf(stderr, "  [%7.1f] queue lane %d: batch %lld run in %.1f ms, its front took %.1f ms\n", call.since(), w, (long long) b, run_ms,
                                 ss.total_ms - run_ms);
        me.busy_ms += run_ms;
        return r;
    };
    hk.retire = [&](int w, int64_t b) { if (Staged *st = staged_of(w, b)) drop(st); };
    hk.end = [&](int w) { call.lane_end(w); };
    rc = call.run(hk);
    call.fill(stats);
    if (rc != MRP_OK) {
        for (int64_t i = 0; i < n_chunks; i++) {
            mrp_phase_result_destroy(out[i]);
            out[i] = nullptr;
            if (profiles_out) mrp_profile_out_clear(&profiles_out[i]);
            if (rest) mrp_filtered_out_clear(&filtered_out[i]);
        }
        return call.error(rc);
    }
    return MRP_OK;
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
    if (n_chunks > 0 && (!rest || !filtered_out)) return mrp_set_error(MRP_ERR_ARG, "mrp_phase_string_chunks_with_filtered_on_devices: null argument or bad sizes");
    if (filtered_out && n_chunks > 0) memset(filtered_out, 0, sizeof(*filtered_out) * (size_t) n_chunks);
    int rc = mrp_string_chunks_check(n_chunks, chunks, forward_model, reverse_model, expansion, params, out, hap_out, phred_out, rest, "mrp_phase_string_chunks_with_filtered_on_devices");
    if (rc != MRP_OK) return rc;
    mrp_queue *q = nullptr;
    rc = mrp_queue_create(devices, n_devices, &q);
    if (rc == MRP_OK)
        rc = mrp_queue_phase_string_chunks_with_filtered(q, n_chunks, chunks, rest, forward_model, reverse_model, expansion, sv_threshold,
                                                         het_substitution_probability, params, min_phred, chunks_per_batch, out, hap_out, phred_out, profiles_out,
                                                         filtered_out, stats);
    mrp_queue_destroy(q);
    return rc;
}

int mrp_phase_string_chunks_on_devices(const int32_t *devices, int32_t n_devices, int64_t n_chunks, const mrp_string_chunk *chunks,
                                       const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold,
                                       double het_substitution_probability, const mrp_params *params, int64_t min_phred, int64_t chunks_per_batch,
                                       mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out,
                                       mrp_queue_stats *stats) {
    /* (the queue's own order of errors: a malformed call is MRP_ERR_ARG with or without a device) */
    int rc = mrp_string_chunks_check(n_chunks, chunks, forward_model, reverse_model, expansion, params, out, hap_out, phred_out, nullptr, "mrp_phase_string_chunks");
    if (rc != MRP_OK) return rc;
    mrp_queue *q = nullptr;
    rc = mrp_queue_create(devices, n_devices, &q);
    if (rc == MRP_OK)
        rc = mrp_queue_phase_string_chunks(q, n_chunks, chunks, forward_model, reverse_model, expansion, sv_threshold, het_substitution_probability, params,
                                           min_phred, chunks_per_batch, out, hap_out, phred_out, profiles_out, stats);
    mrp_queue_destroy(q);
    return rc;
}

}  /* extern "C" */

/* ---- aligned chunks: mrp_queue_phase_aligned_chunks (rest == NULL), mrp_queue_phase_aligned_chunks_with_filtered and
 * mrp_queue_phase_aligned_chunks_with_records (records_out beside filtered_out) -------------------------------------------------------- */
extern "C" int mrp_aligned_chunk_units(const mrp_aligned_chunk *chunk, const mrp_aligned_chunk_rest *rest, int64_t *units_out) {
    static const char *who = "mrp_aligned_chunk_units";
    if (!chunk || !units_out) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    const mrp_aligned_chunk &C = *chunk;
    if (C.n_reads < 0 || C.n_variants < 0 || (rest && rest->n_variants < 0)) return mrp_set_error(MRP_ERR_ARG, "%s: negative count", who);
    if (C.overlap_end < C.overlap_start) return mrp_set_error(MRP_ERR_ARG, "%s: overlap_end before overlap_start", who);
    if (C.n_reads > 0 && !C.l_qseq) return mrp_set_error(MRP_ERR_ARG, "%s: null l_qseq", who);
    unsigned __int128 bases = 0;
    for (int64_t r = 0; r < C.n_reads; r++) {
        if (C.l_qseq[r] < 0) return mrp_set_error(MRP_ERR_ARG, "%s: read %lld: negative l_qseq", who, (long long) r);
        bases += (unsigned __int128) C.l_qseq[r];
    }
    /* (B < 2^62 and V < 2^64: the product fits 128 bits) */
    const unsigned __int128 variants = (unsigned __int128) C.n_variants + (unsigned __int128) (rest ? rest->n_variants : 0);
    const unsigned __int128 length = (unsigned __int128) std::max<int64_t>(1, C.overlap_end - C.overlap_start);
    const unsigned __int128 units = bases * variants / length;
    *units_out = units > (unsigned __int128) INT64_MAX ? INT64_MAX : (int64_t) units;
    return MRP_OK;
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
    const int n_devices = (int) q->devices.size();
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_devices = n_devices; }
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
    const int lanes = q->lanes, n_workers = n_devices * lanes;
    const QueuePlan plan = plan_queue(n_chunks, cost.data(), A.chunks_per_batch, n_workers, n_devices);
    const int64_t n_batches = (int64_t) plan.batch_off.size() - 1;
    if (stats) stats->batches = n_batches;
    QueueCall call(q, n_batches, active_lanes_of(plan, cost.data(), n_devices, lanes));

    /* a batch as one mrp_phase_aligned_chunks(_with_filtered) call sees it: its chunks in plan order with what travels with them, the
     * call's outputs, and the front -- its host part (the extraction's records, the chunks' checks and windows) made by the prefetch
     * beside the lane's current batch, its device part staged on the lane's context when the batch is run */
    struct Staged {
        std::atomic<int64_t> batch{-1}; /* (the call's thread looks its batch up while the stager fills the lane's OTHER slot) */
        int64_t first = 0, count = 0;
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
    std::vector<LaneSlots<Staged>> lane_state((size_t) n_workers);
    std::vector<mrp_queue_records_stats> rec_per((size_t) n_workers); /* what each lane's batches added to the records' stats */
    memset(rec_per.data(), 0, sizeof(mrp_queue_records_stats) * rec_per.size());
    auto staged_of = [&](int w, int64_t b) { return lane_state[(size_t) w].find(b); };
    /* (a staged front holds arrays of the lane's context: it goes with no other thread of the lane at work, on the lane's thread) */
    auto drop = [&](Staged *st) { mrp_aligned_front_destroy(st->front); st->front = nullptr; st->batch = -1; };
    LaneHooks hk;
    hk.begin = [&](int w) { return call.lane_begin(w, false); };
    hk.prefetch = [&](int w, int64_t b) { /* host only: never the lane's context, its stream, its events or its pool */
        const auto t0 = std::chrono::steady_clock::now();
        mrp_pool_adopt(q->pools[(size_t) (w / lanes)]);
        Staged *st = lane_state[(size_t) w].next();
        st->first = plan.batch_off[(size_t) b]; st->count = plan.batch_off[(size_t) b + 1] - st->first;
        const size_t count = (size_t) st->count;
        st->ch.resize(count); st->names.resize(count); st->hap.resize(count);
        st->rs.resize(rest ? count : 0);
        st->keep.resize(a.keep ? count : 0);
        st->phred.resize(a.phred_out ? count : 0);
        st->res.assign(count, nullptr);
        st->bv.assign(a.bubble_variant_out ? count : 0, nullptr);
        st->fr.assign(rest ? count : 0, nullptr);
        st->prof.resize(a.profiles_out ? count : 0);
        st->fo.resize(rest ? count : 0);
        if (a.profiles_out) memset(st->prof.data(), 0, sizeof(mrp_profile_out) * count);
        if (rest) memset(st->fo.data(), 0, sizeof(mrp_filtered_out) * count);
        st->rec.resize(records ? count : 0);
        st->rst.resize(records ? 1 : 0);
        if (records) {
            memset(st->rec.data(), 0, sizeof(mrp_variant_records) * count);
            memset(st->rst.data(), 0, sizeof(mrp_phase_aligned_records_stats));
        }
        for (size_t i = 0; i < count; i++) {
            const int64_t chunk = plan.order[(size_t) st->first + i];
            st->ch[i] = a.chunks[chunk];
            st->names[i] = a.read_names[chunk];
            st->hap[i] = a.hap_out[chunk];
            if (rest) st->rs[i] = rest[chunk];
            if (a.keep) st->keep[i] = a.keep[chunk];
            if (a.phred_out) st->phred[i] = a.phred_out[chunk];
        }
        st->batch.store(b);
        mrp_aligned_args ba = a;
        ba.n_chunks = st->count;
        ba.chunks = st->ch.data();
        ba.rest = rest ? st->rs.data() : nullptr;
        ba.read_names = st->names.data();
        ba.keep = a.keep ? st->keep.data() : nullptr;
        ba.out = st->res.data();
        ba.hap_out = st->hap.data();
        ba.phred_out = a.phred_out ? st->phred.data() : nullptr;
        ba.profiles_out = a.profiles_out ? st->prof.data() : nullptr;
        ba.bubble_variant_out = a.bubble_variant_out ? st->bv.data() : nullptr;
        ba.filtered_out = rest ? st->fo.data() : nullptr;
        ba.filtered_read_out = rest ? st->fr.data() : nullptr;
        ba.records_out = records ? st->rec.data() : nullptr;
        ba.records_stats = records ? st->rst.data() : nullptr;
        const double t_begin = std::chrono::duration<double, std::milli>(t0.time_since_epoch()).count();
        const int r = mrp_aligned_front_create(who, t_begin, &ba, nullptr, nullptr, &st->front);
        if (r != MRP_OK) call.stage_errs[(size_t) w] = mrp_last_error();
        if (call.timing) fprintf(stderr, "  [%7.1f] queue lane %d: checks and windows of batch %lld (%lld chunks) in %.1f ms\n", call.since(), w, (long long) b,
                                 (long long) st->count, ms_since(t0));
        return r;
    };
    hk.discard = [&](int w, int64_t b) { if (Staged *st = staged_of(w, b)) drop(st); };
    hk.phase = [&](int w, int64_t b) {
        Staged *cur = staged_of(w, b);
        if (!cur || !cur->front) { call.errs[(size_t) w] = "work queue: batch has no front"; return (int) MRP_ERR_ARG; }
        const auto t0 = std::chrono::steady_clock::now();
        const int64_t count = cur->count;
        mrp_string_chunks_stats ss;
        memset(&ss, 0, sizeof(ss));
        int r = mrp_aligned_front_stage(q->ctx[(size_t) w], cur->front);
        const double front_ms = ms_since(t0);
        if (r == MRP_OK) r = mrp_aligned_front_run(cur->front, &ss);
        QueueCall::PerLane &me = call.per[(size_t) w];
        if (r != MRP_OK) {
            call.errs[(size_t) w] = mrp_last_error();
            for (mrp_variant_records &R : cur->rec) mrp_variant_records_clear(&R); /* (a batch that failed behind its records hands none over) */
        } else {
            if (records) {
                mrp_queue_records_stats &mine = rec_per[(size_t) w];
                const mrp_phase_aligned_records_stats &b = cur->rst[0];
                mine.records_sites += b.records_sites;
                mine.records_updated += b.records_updated;
                mine.reads_listed += b.reads_listed;
                mine.records_bytes_downloaded += b.records_bytes_downloaded;
                mine.records_ms += b.records_ms;
            }
            for (int64_t i = 0; i < count; i++) {
                const int64_t chunk = plan.order[(size_t) (cur->first + i)];
                a.out[chunk] = cur->res[(size_t) i];
                if (records) { a.records_out[chunk] = cur->rec[(size_t) i]; memset(&cur->rec[(size_t) i], 0, sizeof(mrp_variant_records)); }
                if (a.profiles_out) a.profiles_out[chunk] = cur->prof[(size_t) i];
                if (a.bubble_variant_out) a.bubble_variant_out[chunk] = cur->bv[(size_t) i];
                if (rest) { a.filtered_out[chunk] = cur->fo[(size_t) i]; a.filtered_read_out[chunk] = cur->fr[(size_t) i]; }
                me.units += cost[(size_t) chunk];
            }
            me.chunks += count;
            me.fallback += ss.phase.resident ? ss.phase.fallback_chunks : count;
        }
        const double all_ms = ms_since(t0);
        if (call.timing) fprintf(stderr, "  [%7.1f] queue lane %d: batch %lld: device front in %.1f ms, run in %.1f ms\n", call.since(), w, (long long) b, front_ms,
                                 all_ms - front_ms);
        me.busy_ms += all_ms;
        return r;
    };
    hk.retire = [&](int w, int64_t b) { if (Staged *st = staged_of(w, b)) drop(st); };
    hk.end = [&](int w) { call.lane_end(w); };
    rc = call.run(hk);
    call.fill(stats);
    if (rc != MRP_OK) {
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
        return call.error(rc);
    }
    if (records && A.records_stats)
        for (const mrp_queue_records_stats &b : rec_per) { /* in lane order: the sum of records_ms does not depend on which lane finished first */
            A.records_stats->records_sites += b.records_sites;
            A.records_stats->records_updated += b.records_updated;
            A.records_stats->reads_listed += b.reads_listed;
            A.records_stats->records_bytes_downloaded += b.records_bytes_downloaded;
            A.records_stats->records_ms += b.records_ms;
        }
    return MRP_OK;
}

/* create + call + destroy, with the queue's own order of errors: a malformed call and a refused mode need no device */
int aligned_on_devices(const int32_t *devices, int32_t n_devices, const AlignedQueueArgs &A, bool with_rest) {
    return checked_on_devices(devices, n_devices, [&] { return aligned_queue_check(A, with_rest); },
                              [&](mrp_queue *q) { return queue_phase_aligned_chunks(q, A, with_rest, true); });
}

}  // namespace

extern "C" {

int mrp_queue_phase_aligned_chunks(mrp_queue *q, int64_t n_chunks, const mrp_aligned_chunk *chunks, const char *const *const *read_names,
                                   const uint8_t *const *keep, const mrp_extract_options *options, const mrp_pair_hmm *forward_model,
                                   const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold, double het_substitution_probability,
                                   const mrp_params *params, int64_t min_phred, int64_t chunks_per_batch, mrp_phase_result **out, int8_t *const *hap_out,
                                   double *const *phred_out, mrp_profile_out *profiles_out, int64_t **bubble_variant_out, mrp_queue_stats *stats) {
    const AlignedQueueArgs A{"mrp_queue_phase_aligned_chunks",
                             {n_chunks, chunks, nullptr, read_names, keep, options, forward_model, reverse_model, expansion, sv_threshold,
                              het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, bubble_variant_out, nullptr, nullptr,
                              q ? q->sv_split : 0, nullptr, nullptr, q ? q->max_depth : 0, q ? q->downsampling_seed : 0}, /* (a NULL queue counts as off) */
                             chunks_per_batch, stats};
    return queue_phase_aligned_chunks(q, A, false);
}

int mrp_queue_phase_aligned_chunks_with_filtered(mrp_queue *q, int64_t n_chunks, const mrp_aligned_chunk *chunks, const mrp_aligned_chunk_rest *rest,
                                                 const char *const *const *read_names, const uint8_t *const *keep, const mrp_extract_options *options,
                                                 const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
                                                 int64_t sv_threshold, double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                                                 int64_t chunks_per_batch, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out,
                                                 mrp_profile_out *profiles_out, int64_t **bubble_variant_out, mrp_filtered_out *filtered_out,
                                                 int32_t **filtered_read_out, mrp_queue_stats *stats) {
    const AlignedQueueArgs A{"mrp_queue_phase_aligned_chunks_with_filtered",
                             {n_chunks, chunks, rest, read_names, keep, options, forward_model, reverse_model, expansion, sv_threshold,
                              het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, bubble_variant_out, filtered_out,
                              filtered_read_out, q ? q->sv_split : 0, nullptr, nullptr, q ? q->max_depth : 0, q ? q->downsampling_seed : 0},
                             chunks_per_batch, stats};
    return queue_phase_aligned_chunks(q, A, true);
}

int mrp_queue_phase_aligned_chunks_with_records(mrp_queue *q, int64_t n_chunks, const mrp_aligned_chunk *chunks, const mrp_aligned_chunk_rest *rest,
                                                const char *const *const *read_names, const uint8_t *const *keep, const mrp_extract_options *options,
                                                const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion,
                                                int64_t sv_threshold, double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                                                int64_t chunks_per_batch, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out,
                                                mrp_profile_out *profiles_out, int64_t **bubble_variant_out, mrp_filtered_out *filtered_out,
                                                int32_t **filtered_read_out, mrp_variant_records *records_out, mrp_queue_stats *stats,
                                                mrp_queue_records_stats *records_stats) {
    const AlignedQueueArgs A{"mrp_queue_phase_aligned_chunks_with_records",
                             {n_chunks, chunks, rest, read_names, keep, options, forward_model, reverse_model, expansion, sv_threshold,
                              het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, bubble_variant_out, filtered_out,
                              filtered_read_out, q ? q->sv_split : 0, records_out, nullptr, q ? q->max_depth : 0, q ? q->downsampling_seed : 0},
                             chunks_per_batch, stats, true, records_stats};
    return queue_phase_aligned_chunks(q, A, true);
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
    const AlignedQueueArgs A{"mrp_phase_aligned_chunks_with_records_on_devices",
                             {n_chunks, chunks, rest, read_names, keep, options, forward_model, reverse_model, expansion, sv_threshold,
                              het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, bubble_variant_out, filtered_out,
                              filtered_read_out, 0, records_out},
                             chunks_per_batch, stats, true, records_stats};
    return aligned_on_devices(devices, n_devices, A, true);
}

int mrp_phase_aligned_chunks_on_devices(const int32_t *devices, int32_t n_devices, int64_t n_chunks, const mrp_aligned_chunk *chunks,
                                        const char *const *const *read_names, const uint8_t *const *keep, const mrp_extract_options *options,
                                        const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold,
                                        double het_substitution_probability, const mrp_params *params, int64_t min_phred, int64_t chunks_per_batch,
                                        mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out,
                                        int64_t **bubble_variant_out, mrp_queue_stats *stats) {
    const AlignedQueueArgs A{"mrp_phase_aligned_chunks_on_devices",
                             {n_chunks, chunks, nullptr, read_names, keep, options, forward_model, reverse_model, expansion, sv_threshold,
                              het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, bubble_variant_out, nullptr, nullptr},
                             chunks_per_batch, stats};
    return aligned_on_devices(devices, n_devices, A, false);
}

int mrp_phase_aligned_chunks_with_filtered_on_devices(const int32_t *devices, int32_t n_devices, int64_t n_chunks, const mrp_aligned_chunk *chunks,
                                                      const mrp_aligned_chunk_rest *rest, const char *const *const *read_names, const uint8_t *const *keep,
                                                      const mrp_extract_options *options, const mrp_pair_hmm *forward_model,
                                                      const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold,
                                                      double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                                                      int64_t chunks_per_batch, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out,
                                                      mrp_profile_out *profiles_out, int64_t **bubble_variant_out, mrp_filtered_out *filtered_out,
                                                      int32_t **filtered_read_out, mrp_queue_stats *stats) {
    const AlignedQueueArgs A{"mrp_phase_aligned_chunks_with_filtered_on_devices",
                             {n_chunks, chunks, rest, read_names, keep, options, forward_model, reverse_model, expansion, sv_threshold,
                              het_substitution_probability, params, min_phred, out, hap_out, phred_out, profiles_out, bubble_variant_out, filtered_out,
                              filtered_read_out},
                             chunks_per_batch, stats};
    return aligned_on_devices(devices, n_devices, A, true);
}

}  /* extern "C" */

/* ---- haplotagging aligned chunks from a phased VCF: mrp_queue_haplotag_aligned_chunks ------------------------------------------------ */
extern "C" int mrp_haplotag_chunk_units(const mrp_aligned_chunk *chunk, const int32_t *gt, int64_t *units_out) {
    static const char *who = "mrp_haplotag_chunk_units";
    if (!chunk || !units_out) return mrp_set_error(MRP_ERR_ARG, "%s: null argument", who);
    const mrp_aligned_chunk &C = *chunk;
    if (C.n_reads < 0 || C.n_variants < 0) return mrp_set_error(MRP_ERR_ARG, "%s: negative count", who);
    if (C.overlap_end < C.overlap_start) return mrp_set_error(MRP_ERR_ARG, "%s: overlap_end before overlap_start", who);
    if (C.n_reads > 0 && !C.l_qseq) return mrp_set_error(MRP_ERR_ARG, "%s: null l_qseq", who);
    if (C.n_variants > 0 && !gt) return mrp_set_error(MRP_ERR_ARG, "%s: null genotypes", who);
    unsigned __int128 bases = 0;
    for (int64_t r = 0; r < C.n_reads; r++) {
        if (C.l_qseq[r] < 0) return mrp_set_error(MRP_ERR_ARG, "%s: read %lld: negative l_qseq", who, (long long) r);
        bases += (unsigned __int128) C.l_qseq[r];
    }
    /* only a heterozygous variant is scored (bubbleGraph.c:1975): the chunk's pair-HMM work, not its variant count */
    unsigned __int128 het = 0;
    for (int64_t v = 0; v < C.n_variants; v++) het += gt[2 * v] != gt[2 * v + 1];
    /* (B < 2^62 and H < 2^63: the product fits 128 bits) */
    const unsigned __int128 length = (unsigned __int128) std::max<int64_t>(1, C.overlap_end - C.overlap_start);
    const unsigned __int128 units = bases * het / length;
    *units_out = units > (unsigned __int128) INT64_MAX ? INT64_MAX : (int64_t) units;
    return MRP_OK;
}

namespace {

struct HaplotagQueueArgs {
    mrp_haplotag_args a;
    int64_t chunks_per_batch;
    mrp_queue_stats *stats;
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
    const int n_devices = (int) q->devices.size();
    if (stats) { memset(stats, 0, sizeof(*stats)); stats->n_devices = n_devices; }
    if (n_chunks == 0) return MRP_OK;
    /* tools/tagFromPhasedVcf.c:208-225 orders the chunks largest first; here by the (read, het variant) substrings uniform coverage gives */
    std::vector<int64_t> cost((size_t) n_chunks, 0);
    for (int64_t i = 0; i < n_chunks; i++)
        if (mrp_haplotag_chunk_units(&a.chunks[i], a.gt[i], &cost[(size_t) i]) != MRP_OK) cost[(size_t) i] = 0;
    const int lanes = q->lanes, n_workers = n_devices * lanes;
    const QueuePlan plan = plan_queue(n_chunks, cost.data(), A.chunks_per_batch, n_workers, n_devices);
    const int64_t n_batches = (int64_t) plan.batch_off.size() - 1;
    if (stats) stats->batches = n_batches;
    QueueCall call(q, n_batches, active_lanes_of(plan, cost.data(), n_devices, lanes));

    /* a batch as one mrp_haplotag_aligned_chunks call sees it: its chunks in plan order with their genotypes and output arrays, and the
     * front -- its host part (the extraction's records, the checks, the windows) made by the prefetch beside the lane's current batch,
     * its device part staged on the lane's context when the batch is run */
    struct Staged {
        std::atomic<int64_t> batch{-1}; /* (the call's thread looks its batch up while the stager fills the lane's OTHER slot) */
        int64_t first = 0, count = 0;
        std::vector<mrp_aligned_chunk> ch;
        std::vector<const int32_t *> gt;
        std::vector<int8_t *> hap;
        std::vector<double *> h1, h2;
        mrp_haplotag_front *front = nullptr;
    };
    std::vector<LaneSlots<Staged>> lane_state((size_t) n_workers);
    auto staged_of = [&](int w, int64_t b) { return lane_state[(size_t) w].find(b); };
    /* (a staged front holds arrays of the lane's context: it goes with no other thread of the lane at work, on the lane's thread) */
    auto drop = [&](Staged *st) { mrp_haplotag_front_destroy(st->front); st->front = nullptr; st->batch = -1; };
    LaneHooks hk;
    hk.begin = [&](int w) { return call.lane_begin(w, false); };
    hk.prefetch = [&](int w, int64_t b) { /* host only: never the lane's context, its stream, its events or its pool */
        const auto t0 = std::chrono::steady_clock::now();
        mrp_pool_adopt(q->pools[(size_t) (w / lanes)]);
        Staged *st = lane_state[(size_t) w].next();
        st->first = plan.batch_off[(size_t) b]; st->count = plan.batch_off[(size_t) b + 1] - st->first;
        const size_t count = (size_t) st->count;
        st->ch.resize(count); st->gt.resize(count); st->hap.resize(count);
        st->h1.resize(a.h1_out ? count : 0);
        st->h2.resize(a.h2_out ? count : 0);
        for (size_t i = 0; i < count; i++) {
            const int64_t chunk = plan.order[(size_t) st->first + i];
            st->ch[i] = a.chunks[chunk];
            st->gt[i] = a.gt[chunk];
            st->hap[i] = a.hap_out[chunk];
            if (a.h1_out) st->h1[i] = a.h1_out[chunk];
            if (a.h2_out) st->h2[i] = a.h2_out[chunk];
        }
        st->batch.store(b);
        mrp_haplotag_args ba = a;
        ba.n_chunks = st->count;
        ba.chunks = st->ch.data();
        ba.gt = st->gt.data();
        ba.hap_out = st->hap.data();
        ba.h1_out = a.h1_out ? st->h1.data() : nullptr;
        ba.h2_out = a.h2_out ? st->h2.data() : nullptr;
        const int r = mrp_haplotag_front_create(&ba, nullptr, &st->front);
        if (r != MRP_OK) call.stage_errs[(size_t) w] = mrp_last_error();
        if (call.timing) fprintf(stderr, "  [%7.1f] queue lane %d: checks and windows of batch %lld (%lld chunks) in %.1f ms\n", call.since(), w, (long long) b,
                                 (long long) st->count, ms_since(t0));
        return r;
    };
    hk.discard = [&](int w, int64_t b) { if (Staged *st = staged_of(w, b)) drop(st); };
    hk.phase = [&](int w, int64_t b) {
        Staged *cur = staged_of(w, b);
        if (!cur || !cur->front) { call.errs[(size_t) w] = "work queue: batch has no front"; return (int) MRP_ERR_ARG; }
        const auto t0 = std::chrono::steady_clock::now();
        int r = mrp_haplotag_front_stage(q->ctx[(size_t) w], cur->front);
        const double front_ms = ms_since(t0);
        if (r == MRP_OK) r = mrp_haplotag_front_run(cur->front); /* (writes the batch's outputs at the chunks' own arrays) */
        QueueCall::PerLane &me = call.per[(size_t) w];
        if (r != MRP_OK) call.errs[(size_t) w] = mrp_last_error();
        else {
            for (int64_t i = 0; i < cur->count; i++) me.units += cost[(size_t) plan.order[(size_t) (cur->first + i)]];
            me.chunks += cur->count;
        }
        const double all_ms = ms_since(t0);
        if (call.timing) fprintf(stderr, "  [%7.1f] queue lane %d: batch %lld: extraction and owners in %.1f ms, pairs and scoring in %.1f ms\n", call.since(), w,
                                 (long long) b, front_ms, all_ms - front_ms);
        me.busy_ms += all_ms;
        return r;
    };
    hk.retire = [&](int w, int64_t b) { if (Staged *st = staged_of(w, b)) drop(st); };
    hk.end = [&](int w) { call.lane_end(w); };
    rc = call.run(hk);
    call.fill(stats);
    return rc != MRP_OK ? call.error(rc) : (int) MRP_OK;
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
