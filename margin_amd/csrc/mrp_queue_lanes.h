/* mrp_queue_lanes.h -- the plan and the hand-out of the work queue (mrp_queue_lanes.cpp): which chunks make a batch, which lane
 * takes which batch and when.  Plain C++: no HIP, no context, no error text; mrp_queue.cpp hangs the real work on the hooks,
 * mrp_queue_dry_run a simulated clock, tests/queue_lanes_check.cpp fakes that fail. */
#ifndef MRP_QUEUE_LANES_H_
#define MRP_QUEUE_LANES_H_

#include <cstdint>
#include <functional>
#include <vector>

#include "../../include/margin_rphmm.h" /* MRP_QUEUE_*, MRP_OK */

#pragma GCC visibility push(hidden) /* (the library's own: not part of its C-ABI) */

struct QueuePlan {
    std::vector<int64_t> order;     /* chunk indices, largest estimated cost first (ties: input order) */
    std::vector<int64_t> batch_off; /* batch b = order[batch_off[b] .. batch_off[b + 1]) */
};
QueuePlan plan_queue(int64_t n, const int64_t *cost, int64_t chunks_per_batch, int n_workers = 1, int n_devices = 1);
int active_lanes_of(const QueuePlan &plan, const int64_t *cost, int n_devices, int lanes);

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
              const std::function<void(int)> &on_thread_start);

#pragma GCC visibility pop

#endif
