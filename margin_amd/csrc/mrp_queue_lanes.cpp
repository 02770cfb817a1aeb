/* mrp_queue_lanes.cpp -- the plan and the hand-out of the work queue (mrp_queue.cpp): chunks ordered by cost and cut into batches
 * (phase.c:257-263), batches handed to the lanes of the devices as they become free (phase.c:276-279).  Plain C++, no HIP. */
#include "mrp_queue_lanes.h"

#include <algorithm>
#include <atomic>
#include <numeric>
#include <system_error>
#include <thread>

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
QueuePlan plan_queue(int64_t n, const int64_t *cost, int64_t chunks_per_batch, int n_workers, int n_devices) {
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
