/*
 * mrp_host_pool.cpp -- the persistent host worker pool behind the library's parallel loops, and mrp_host_threads /
 * mrp_set_host_threads.  Locks, atomics and threads only: no HIP, so tests/host_pool_check.cpp runs it under the sanitizers.
 *
 * mrp_pool_run(n, grain, fn, arg) calls fn(i, arg) for every i in [0, n) on the calling thread and the pool's workers and
 * returns when all are done.  The resident pipeline issues ~50 short parallel loops per call; creating and joining 15
 * threads for each of them cost more than many of the loops.  Several callers may be inside at once (the concurrent
 * batches of mrp_phase_reads_many): jobs queue up, a worker serves the job of the most urgent caller that still has indices
 * to hand out (mrp_pool_set_priority: batch 0 before batch 1 ...: the batches then leave their host-only phases one after
 * the other instead of all together, and the device has work while the later ones are still being prepared), the oldest
 * among equals. */
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <ctime>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "mrp_host_pool.h"

std::atomic<long long> g_pool_task_cpu_ns{0};
std::atomic<long long> g_pool_tag_cpu_ns[16];
static thread_local long long t_pool_task_cpu_ns = 0; /* pool tasks executed by the calling thread itself */
extern "C" long long mrp_pool_task_cpu_ns(void) { return g_pool_task_cpu_ns.load(); }
extern "C" long long mrp_pool_task_cpu_ns_this_thread(void) { return t_pool_task_cpu_ns; }
extern "C" long long mrp_pool_tag_cpu_ns(int tag) { return g_pool_tag_cpu_ns[tag & 15].load(); }
namespace {
thread_local int t_pool_priority = 0;
thread_local int t_pool_tag = 0;
thread_local int t_pool_weight_ns = 0; /* mrp_pool_set_weight: what one index of the calling thread's next loops costs, roughly; 0: unknown */
/* The indices of a loop are dealt out from MRP_POOL_RANGES contiguous ranges, and a thread starts with the range of its own
 * number before it helps with the others: the loops of a batch's levels run over the same chunks in the same order, so the
 * thread that built a chunk's hmms at one level mostly meets them again at the next (their blocks are in its cache, or its
 * neighbours') instead of wherever a single shared counter sends it. */
#define MRP_POOL_RANGES 16 /* (1, 8 or 32 ranges: the same CPU time per loop family) */
struct alignas(64) PoolRange { std::atomic<int64_t> next{0}; int64_t end = 0; };
struct PoolJob {
    void (*fn)(int64_t, void *);
    void *arg;
    int64_t n, grain;
    int prio = 0, tag = 0;
    PoolRange range[MRP_POOL_RANGES];
    std::atomic<int64_t> done{0};
    std::atomic<int> exhausted{0}; /* ranges that have nothing left to hand out */
    int active = 0; /* workers currently holding the pointer (under Pool::mu) */
    std::condition_variable cv; /* the posting thread waits here: woken by the last worker to let go of the job, not by every worker of every job */
    bool has_work() const { return exhausted.load(std::memory_order_relaxed) < MRP_POOL_RANGES; }
};
thread_local int t_pool_slot = -1; /* the calling thread's number in its pool: workers 0 .. threads - 2, a posting thread threads - 1 */
}  // namespace
/* One pool serves the process by default (mrp_set_host_threads); a work queue gives every device its own (mrp_queue.cpp:
 * the reference's axis is "every core works", phase.c:276-279 -- eight devices on one shared pool of sixteen threads would
 * starve each other), optionally bound to the CPUs next to the device.  A thread posts its loops to the pool it has adopted
 * (mrp_pool_adopt; the batch threads of mrp_phase_reads_many inherit their caller's).
 * Wake-ups are counted: a loop wakes as many sleeping workers as it has grains to give away (a call posts some four hundred loops,
 * half of them over a few hundred indices: waking every worker for each of them, and every posting thread whenever any worker
 * finished, was a seventh of the call's host CPU time in futex calls and on the pool's mutex). */
struct mrp_host_pool {
    std::mutex mu;
    std::condition_variable cv_work;
    std::vector<PoolJob *> jobs;
    std::vector<std::thread> workers;
    int idle = 0; /* workers asleep in cv_work (under mu) */
    bool stop = false;
    int fixed_threads = 0; /* 0: the process-wide pool, sized by mrp_host_threads() */
    static void run_chunks(PoolJob *j) {
        struct Acc { /* MRP_TIMING: thread CPU spent inside pool tasks */
            timespec a;
            int tag;
            Acc(int t) : tag(t) { clock_gettime(CLOCK_THREAD_CPUTIME_ID, &a); }
            ~Acc() { timespec b; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &b); const long long d = (b.tv_sec - a.tv_sec) * 1000000000ll + (b.tv_nsec - a.tv_nsec);
                     g_pool_task_cpu_ns.fetch_add(d); g_pool_tag_cpu_ns[tag & 15].fetch_add(d); t_pool_task_cpu_ns += d; }
        } acc(j->tag);
        const int home = (t_pool_slot >= 0 ? t_pool_slot : 0) % MRP_POOL_RANGES;
        int64_t mine = 0; /* booked once: the counter is one cache line shared by every thread of the loop */
        for (int k = 0; k < MRP_POOL_RANGES; k++) {
            PoolRange &r = j->range[(home + k) % MRP_POOL_RANGES];
            for (;;) {
                if (r.next.load(std::memory_order_relaxed) >= r.end) break;
                const int64_t lo = r.next.fetch_add(j->grain);
                if (lo >= r.end) break;
                const int64_t hi = std::min(r.end, lo + j->grain);
                if (lo + j->grain >= r.end) j->exhausted.fetch_add(1); /* (took the range's last grain: exactly one thread does) */
                for (int64_t i = lo; i < hi; i++) j->fn(i, j->arg);
                mine += hi - lo;
            }
        }
        if (mine) j->done.fetch_add(mine);
    }
    void worker() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            PoolJob *j = nullptr;
            for (PoolJob *q : jobs)
                if (q->has_work() && (!j || q->prio < j->prio)) j = q;
            if (!j) {
                if (stop) return;
                idle++;
                cv_work.wait(lk);
                idle--;
                continue;
            }
            j->active++;
            lk.unlock();
            run_chunks(j);
            lk.lock();
            if (--j->active == 0 && j->done.load() >= j->n) j->cv.notify_one();
        }
    }
    void ensure(int n_workers) {
        std::lock_guard<std::mutex> lk(mu);
        while ((int) workers.size() < n_workers) { const int slot = (int) workers.size(); workers.emplace_back([this, slot] { t_pool_slot = slot; worker(); }); }
    }
    ~mrp_host_pool() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv_work.notify_all();
        for (auto &t : workers) t.join();
    }
};
namespace {
typedef mrp_host_pool Pool;
thread_local Pool *t_pool_current = nullptr;
Pool &pool() {
    static Pool *p = new Pool(); /* never destroyed: worker threads must not be joined from a static destructor at exit */
    return *p;
}
}  // namespace

extern "C" void mrp_pool_run(int64_t n, int64_t grain, void (*fn)(int64_t, void *), void *arg) {
    if (n <= 0) return;
    if (grain < 1) grain = 1;
    Pool &P = t_pool_current ? *t_pool_current : pool();
    const int threads = P.fixed_threads > 0 ? P.fixed_threads : mrp_host_threads();
    const int nt = (int) std::min<int64_t>(threads, (n + grain - 1) / grain);
    if (nt <= 1) {
        for (int64_t i = 0; i < n; i++) fn(i, arg);
        return;
    }
    /* a loop whose whole work is a few dozen microseconds is run here: posting it costs the poster and every woken worker a futex
     * call and a turn on the pool's mutex each (the levels of a call of small chunks post hundreds of such loops) */
    const int64_t est_ns = t_pool_weight_ns > 0 ? n * (int64_t) t_pool_weight_ns : -1;
    if (est_ns >= 0 && est_ns < 60000) {
        for (int64_t i = 0; i < n; i++) fn(i, arg);
        return;
    }
    P.ensure(threads - 1);
    PoolJob j;
    j.fn = fn; j.arg = arg; j.n = n; j.grain = grain; j.prio = t_pool_priority; j.tag = t_pool_tag;
    {   /* ranges of whole grains; the empty ones (a short loop) count as exhausted from the start */
        const int64_t grains = (n + grain - 1) / grain;
        int empty = 0;
        for (int r = 0; r < MRP_POOL_RANGES; r++) {
            const int64_t lo = std::min(n, grains * r / MRP_POOL_RANGES * grain), hi = std::min(n, grains * (r + 1) / MRP_POOL_RANGES * grain);
            j.range[r].next.store(lo); j.range[r].end = hi;
            if (lo >= hi) empty++;
        }
        j.exhausted.store(empty);
    }
    if (t_pool_slot < 0) t_pool_slot = threads - 1;
    int wake;
    {
        std::lock_guard<std::mutex> lk(P.mu);
        P.jobs.push_back(&j);
        /* one sleeper per grain beyond the poster's own (a worker that is busy looks at the job list when it is done: nothing is lost) */
        wake = (int) std::min<int64_t>(P.idle, std::min<int64_t>(threads - 1, (n + grain - 1) / grain - 1));
        if (est_ns >= 0) wake = (int) std::min<int64_t>(wake, est_ns / 100000); /* ... that has some 100 us of work to find */
    }
    for (int k = 0; k < wake; k++) P.cv_work.notify_one();
    Pool::run_chunks(&j);
    std::unique_lock<std::mutex> lk(P.mu);
    j.cv.wait(lk, [&] { return j.done.load() >= j.n && j.active == 0; });
    P.jobs.erase(std::find(P.jobs.begin(), P.jobs.end(), &j));
}

/* a pool of its own with `threads` threads (the posting thread counts as one); its workers are created by the first loop
 * posted to it and inherit the CPU affinity of the thread that posts it */
mrp_host_pool *mrp_host_pool_create(int threads) {
    mrp_host_pool *p = new (std::nothrow) mrp_host_pool();
    if (p) p->fixed_threads = threads < 1 ? 1 : threads;
    return p;
}
void mrp_host_pool_destroy(mrp_host_pool *p) { delete p; }
extern "C" void *mrp_pool_current(void) { return t_pool_current; }
extern "C" void mrp_pool_adopt(void *p) { t_pool_current = static_cast<mrp_host_pool *>(p); }

extern "C" void mrp_pool_set_priority(int p) { t_pool_priority = p; }
extern "C" void mrp_pool_set_weight(int ns_per_index) { t_pool_weight_ns = ns_per_index; }
extern "C" void mrp_pool_set_tag(int t) { t_pool_tag = t; } /* MRP_TIMING: which loop the CPU time of the pool tasks is booked to */

static std::atomic<int> g_host_threads{0};
static std::atomic<bool> g_host_threads_set{false};
int mrp_host_threads(void) {
    int n = g_host_threads.load();
    if (n <= 0) {
        n = (int) std::min<unsigned>(16u, std::max(1u, std::thread::hardware_concurrency()));
        g_host_threads.store(n);
    }
    return n;
}
int mrp_host_threads_setting(void) { return g_host_threads_set.load() ? g_host_threads.load() : 0; } /* 0: never set */
int mrp_set_host_threads(int n) {
    if (n < 1 || n > 256) return mrp_set_error(MRP_ERR_ARG, "mrp_set_host_threads: %d outside 1..256", n);
    g_host_threads.store(n);
    g_host_threads_set.store(true);
    return MRP_OK;
}
