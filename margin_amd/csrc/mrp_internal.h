/*
 * mrp_internal.h -- host-side objects behind the opaque handles of include/margin_rphmm.h, shared by mrp_context.cpp,
 * mrp_chunk.cpp, mrp_batch.cpp (forward/backward seam) and mrp_engine.cpp (device-resident merge levels).
 */
#ifndef MRP_INTERNAL_H_
#define MRP_INTERNAL_H_

#include <hip/hip_runtime.h>
#include <cstring>
#include <cstdlib>

#include <time.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <functional>
#include <iterator>
#include <map>
#include <memory>
#include <new>
#include <type_traits>
#include <mutex>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/margin_rphmm.h"
#include "mrp_census.h"
#include "mrp_device.h"
#include "mrp_host_pool.h"
#include "mrp_kernels.h"
#include "rphmm_host.h"

#define HIP_TRY(expr)                                                                                          \
    do {                                                                                                       \
        hipError_t e_ = (expr);                                                                                \
        if (e_ != hipSuccess) return mrp_set_error(MRP_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)
/* Declared after the host staging vectors and scratch buffers of a function that queues work on s: whatever way the function
 * is left, the stream is drained before they go. */
struct Drain { hipStream_t s; ~Drain() { (void) hipStreamSynchronize(s); } };

/* A kernel attribute (the opt-in to more than 64 KB of dynamic LDS) belongs to the function ON A DEVICE: set once per device,
 * by whichever context of that device launches first (the C-ABI lets one process hold contexts on several devices). */
struct PerDeviceOnce {
    std::mutex mu;
    bool done[64] = {false};
    template <class F> hipError_t run(F f) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev < 0 || dev >= 64) return f();
        std::lock_guard<std::mutex> lock(mu);
        if (done[dev]) return hipSuccess;
        e = f();
        if (e == hipSuccess) done[dev] = true;
        return e;
    }
};

/* std::vector whose resize() leaves trivially constructible elements uninitialised: the descriptor arrays of a level
 * are tens of megabytes that the filling threads overwrite entirely; zero-filling them first is a serial pass. */
template <class T>
struct DefaultInitAllocator : std::allocator<T> {
    template <class U> struct rebind { using other = DefaultInitAllocator<U>; };
    using std::allocator<T>::allocator;
    template <class U> void construct(U *p) noexcept(std::is_nothrow_default_constructible<U>::value) { ::new (static_cast<void *>(p)) U; }
    template <class U, class... Args> void construct(U *p, Args &&...args) { ::new (static_cast<void *>(p)) U(std::forward<Args>(args)...); }
};
template <class T> using HostVec = std::vector<T, DefaultInitAllocator<T>>;

/* Caching device allocator of a context.  hipMalloc / hipFree of multi-GB arrays cost hundreds of
 * milliseconds and hipFree synchronizes the device, so blocks are kept and handed out again by size
 * class (1/8-octave rounding).  A released block becomes reusable only at the next reclaim(), which the
 * owners call right after they synchronized the context's stream: nothing in flight can still touch it. */
struct DevPool;
/* Every pool of the process, by device: what the pools of a device hold together (live and cached) is kept below the
 * device's memory less a head room (the runtime allocates scratch and queue memory of its own and ABORTS when it cannot),
 * and a pool the driver refuses a block gives back what idles in all of them, whoever owns them (the halves of one call,
 * a work queue's lanes, a caller's other contexts). */
struct DevPoolRegistry {
    static constexpr int MAX_DEVICES = 64;
    std::mutex mu;
    std::vector<DevPool *> pools;
    std::atomic<size_t> held[MAX_DEVICES];   /* bytes the pools of a device got from hipMalloc and have not given back */
    std::atomic<size_t> budget[MAX_DEVICES]; /* 0: not asked yet */
    DevPoolRegistry() { for (int d = 0; d < MAX_DEVICES; d++) { held[d].store(0); budget[d].store(0); oom_events[d].store(0); inject_oom[d].store(0); } }
    static DevPoolRegistry &get() { static DevPoolRegistry r; return r; }
    std::atomic<int> inject_oom[MAX_DEVICES];      /* test hook (mrp_context_set_test_hooks bit 2): refuse the next large allocation */
    std::atomic<uint64_t> oom_events[MAX_DEVICES]; /* allocations the driver refused for good (after every cache was given back) */
    /* What the pools of a device may hold together: the memory that is FREE when the first pool of the process asks (another
     * process, or allocations of the caller's own, are not ours to count on) less a head room of a sixteenth of the device,
     * and never more than the device less an eighth.  MRP_POOL_BUDGET_MB overrides. */
    size_t budget_of(int device) {
        size_t b = budget[device].load(std::memory_order_relaxed);
        if (b == 0) {
            size_t total = 0, free_now = 0, tot2 = 0; /* (by ordinal: the calling thread's current device may be another one) */
            b = hipDeviceTotalMem(&total, device) == hipSuccess && total > 0 ? total - total / 8 : ~(size_t) 0;
            int cur = -1;
            if (total > 0 && hipGetDevice(&cur) == hipSuccess && hipSetDevice(device) == hipSuccess) {
                if (hipMemGetInfo(&free_now, &tot2) == hipSuccess && free_now > 0) {
                    const size_t ours = held[device].load(std::memory_order_relaxed), room = total / 16;
                    const size_t avail = free_now + ours > room ? free_now + ours - room : free_now + ours;
                    if (avail < b) b = avail;
                }
                (void) hipSetDevice(cur);
            }
            (void) hipGetLastError();
            if (const char *e = getenv("MRP_POOL_BUDGET_MB")) { const long long v = atoll(e); if (v > 0) b = (size_t) v << 20; }
            budget[device].store(b, std::memory_order_relaxed);
        }
        return b;
    }
    /* the budget is asked for again at its next use (mrp_context_trim: the caches have just been given back, so what is free now
     * is what another tenant's transient pressure -- the reason a budget was shrunk -- has left or given back) */
    void forget_budget(int device) { if (device >= 0 && device < MAX_DEVICES) budget[device].store(0, std::memory_order_relaxed); }
    /* after the driver refused an allocation although nothing idles in any pool: what we hold now is what there is */
    void shrink_budget(int device) {
        const size_t ours = held[device].load(std::memory_order_relaxed);
        size_t b = budget[device].load(std::memory_order_relaxed);
        if (ours > ((size_t) 1 << 30) && (b == 0 || ours < b)) budget[device].store(ours, std::memory_order_relaxed);
    }
    inline void trim_device(int device, DevPool *but);
};

struct DevPool {
    std::mutex mu;
    std::multimap<size_t, void *> free_blocks;
    std::vector<std::pair<size_t, void *>> pending;
    size_t cached_bytes = 0;                 /* bytes in free_blocks */
    size_t cache_limit = (size_t) 64 << 30;  /* beyond this the largest cached blocks go back to the driver; what really bounds the
                                              * caches is the device's budget (registry): a batch of a call keeps some 170 MB
                                              * per 1 Mb chunk of its widest level for reuse (576 chunks in eight batches: 107 GB
                                              * held, 96 of them idle between calls); a limit of 24 GB per pool made every call
                                              * with more than ~100 chunks per batch give back and re-allocate (4x slower) */
    int device = -1;                         /* attach(): the device whose registry entry this pool is */
    std::atomic<uint64_t> oom_local{0};      /* allocations the driver refused THIS pool for good: a call looks at the pools of its own contexts,
                                              * not at the device-wide count (another lane's refusal is not this call's) */
    void attach(int dev) {
        device = dev >= 0 && dev < DevPoolRegistry::MAX_DEVICES ? dev : -1;
        if (device < 0) return;
        DevPoolRegistry &r = DevPoolRegistry::get();
        std::lock_guard<std::mutex> lock(r.mu);
        r.pools.push_back(this);
    }
    void detach() {
        if (device < 0) return;
        DevPoolRegistry &r = DevPoolRegistry::get();
        std::lock_guard<std::mutex> lock(r.mu);
        for (size_t i = 0; i < r.pools.size(); i++)
            if (r.pools[i] == this) { r.pools.erase(r.pools.begin() + (long) i); break; }
        device = -1;
    }
    void held_add(size_t b) { if (device >= 0) DevPoolRegistry::get().held[device].fetch_add(b, std::memory_order_relaxed); }
    void held_sub(size_t b) { if (device >= 0) DevPoolRegistry::get().held[device].fetch_sub(b, std::memory_order_relaxed); }
    bool over_budget() const {
        if (device < 0) return false;
        DevPoolRegistry &r = DevPoolRegistry::get();
        return r.held[device].load(std::memory_order_relaxed) > r.budget_of(device);
    }
    static size_t size_class(size_t bytes) {
        if (bytes < 256) bytes = 256;
        const int lg = 63 - __builtin_clzll((unsigned long long) bytes);
        const size_t step = (size_t) 1 << (lg > 3 ? lg - 3 : 0);
        return (bytes + step - 1) & ~(step - 1);
    }
    hipError_t alloc(void **p, size_t bytes, size_t *cls_out) {
        const size_t cls = size_class(bytes);
        *cls_out = cls;
        {
            std::lock_guard<std::mutex> lock(mu);
            /* best fit: the smallest idle block of this class or up to half as large again (the batches of a work queue differ
             * by some per cent from call to call: exact classes alone would miss, and every miss is a hipMalloc of a gigabyte) */
            auto it = free_blocks.lower_bound(cls);
            if (it != free_blocks.end() && it->first <= cls + cls / 2) {
                *p = it->second;
                *cls_out = it->first;
                cached_bytes -= it->first;
                free_blocks.erase(it);
                return hipSuccess;
            }
        }
        if (device >= 0 && DevPoolRegistry::get().held[device].load(std::memory_order_relaxed) + cls > DevPoolRegistry::get().budget_of(device)) {
            trim(); /* the device's budget: first what idles here, then what idles in the other pools */
            if (DevPoolRegistry::get().held[device].load(std::memory_order_relaxed) + cls > DevPoolRegistry::get().budget_of(device))
                DevPoolRegistry::get().trim_device(device, this);
        }
        if (device >= 0 && cls >= ((size_t) 1 << 20) && DevPoolRegistry::get().inject_oom[device].load(std::memory_order_relaxed) > 0 &&
            DevPoolRegistry::get().inject_oom[device].exchange(0) > 0) { /* fault injection of the test suite */
            DevPoolRegistry::get().oom_events[device].fetch_add(1, std::memory_order_relaxed);
            oom_local.fetch_add(1, std::memory_order_relaxed);
            return hipErrorOutOfMemory;
        }
        hipError_t e = hipMalloc(p, cls);
        if (e != hipSuccess) { /* give the cache back and try once more */
            (void) hipGetLastError();
            trim();
            e = hipMalloc(p, cls);
        }
        if (e != hipSuccess && device >= 0) { /* ... and what idles in the other contexts of this device */
            (void) hipGetLastError();
            DevPoolRegistry::get().trim_device(device, this);
            e = hipMalloc(p, cls);
        }
        if (e == hipSuccess) held_add(cls);
        else if (e == hipErrorOutOfMemory && device >= 0) { /* callers that can re-slice their work look at this count */
            DevPoolRegistry::get().oom_events[device].fetch_add(1, std::memory_order_relaxed);
            oom_local.fetch_add(1, std::memory_order_relaxed);
            DevPoolRegistry::get().shrink_budget(device);
        }
        return e;
    }
    void release(void *p, size_t cls) {
        std::lock_guard<std::mutex> lock(mu);
        pending.emplace_back(cls, p);
    }
    /* Only when nothing queued can still touch a pending block.  Either the context's streams were synchronized, or -- the resident
     * engine's level_retire(complete = true), with later levels in flight -- every pending block belongs to a level whose `done`
     * event has completed: a level's arrays are empty when it is staged and no array of a level in flight is ever allocated
     * again, so a level in flight releases nothing. */
    void reclaim() {
        std::lock_guard<std::mutex> lock(mu);
        for (auto &b : pending) {
            free_blocks.emplace(b.first, b.second);
            cached_bytes += b.first;
        }
        pending.clear();
        while ((cached_bytes > cache_limit || over_budget()) && !free_blocks.empty()) {
            auto it = std::prev(free_blocks.end());
            (void) hipFree(it->second);
            held_sub(it->first);
            cached_bytes -= it->first;
            free_blocks.erase(it);
        }
    }
    void trim() { /* frees the reusable blocks */
        std::lock_guard<std::mutex> lock(mu);
        for (auto &b : free_blocks) { (void) hipFree(b.second); held_sub(b.first); }
        free_blocks.clear();
        cached_bytes = 0;
    }
    void destroy() { /* context teardown: everything, after a device synchronize */
        reclaim();
        trim();
        detach();
    }
};

inline void DevPoolRegistry::trim_device(int device, DevPool *but) {
    std::lock_guard<std::mutex> lock(mu);
    for (DevPool *q : pools)
        if (q != but && q->device == device) q->trim();
}

/* The device arrays of one owner (a batch, a level of the resident engine): an array declared with the group -- DevBuf<T> a{arrays}; --
 * is bound to a pool and released with all the others, so a new array is one declaration.  The entries point at the owner's members:
 * owners are heap objects that are never copied or moved. */
struct DevBufGroup {
    struct Member { void *buf; void (*release)(void *); void (*bind)(void *, DevPool *); };
    std::vector<Member> members;
    DevBufGroup() = default;
    DevBufGroup(const DevBufGroup &) = delete;
    DevBufGroup &operator=(const DevBufGroup &) = delete;
    void bind(DevPool *pl) { for (Member &m : members) m.bind(m.buf, pl); }
    void release() { for (Member &m : members) m.release(m.buf); }
};

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t n = 0;
    DevPool *pool = nullptr; /* NULL: plain hipMalloc / hipFree */
    size_t cls = 0;
    DevBuf() = default;
    explicit DevBuf(DevBufGroup &g) {
        g.members.push_back({this, [](void *b) { static_cast<DevBuf *>(b)->release(); }, [](void *b, DevPool *pl) { static_cast<DevBuf *>(b)->pool = pl; }});
    }
    ~DevBuf() { release(); }
    void release() {
        if (p) {
            if (pool) pool->release(p, cls);
            else (void) hipFree(p);
        }
        p = nullptr;
        n = 0;
    }
    hipError_t alloc(size_t count) {
        release();
        n = count;
        const size_t bytes = std::max<size_t>(count, 1) * sizeof(T) + 64;
        hipError_t e = pool ? pool->alloc((void **) &p, bytes, &cls) : hipMalloc((void **) &p, bytes);
#ifdef MRP_POISON_ALLOC /* debugging aid: every buffer starts as garbage, so a read of a never-written element shows */
        if (e == hipSuccess) {
            (void) hipDeviceSynchronize();
            e = hipMemset(p, 0xA5, bytes);
            (void) hipDeviceSynchronize();
        }
#endif
        return e;
    }
    template <class A>
    hipError_t upload(const std::vector<T, A> &h, hipStream_t s) {
        hipError_t e = alloc(h.size());
        if (e != hipSuccess || h.empty()) return e;
        return hipMemcpyAsync(p, h.data(), h.size() * sizeof(T), hipMemcpyHostToDevice, s);
    }
};

struct mrp_context {
    int device = 0;
    hipStream_t stream = nullptr;
    /* Streams beyond the main one are made when first asked for: the device's hardware queues (GPU_MAX_HW_QUEUES, as the
     * environment sets it) are dealt to streams in creation order, and every stream more than that shares a queue with another --
     * whose kernels it then waits for.  A context that is one of several concurrent batches (`grouped`: the siblings of
     * mrp_phase_reads_many, a work queue's contexts) runs its size classes on its main stream (2 streams a batch, 16 for the
     * eight batches of a call); a context on its own runs them side by side on two more. */
    hipStream_t aux[2] = {nullptr, nullptr};
    bool grouped = false;
    int concurrent_batches = 1; /* how many batches of a mrp_phase_reads_many call run side by side on the device (this context's is one of them) */
    int calls_sharing_device = 1; /* a work queue's lanes: this many calls run on the device at a time (set on the lane's context) */
    hipError_t side_streams(hipStream_t *a0, hipStream_t *a1) {
        if (grouped) { *a0 = *a1 = stream; return hipSuccess; }
        for (int i = 0; i < 2; i++)
            if (!aux[i]) { const hipError_t e = hipStreamCreateWithFlags(&aux[i], hipStreamNonBlocking); if (e != hipSuccess) return e; }
        *a0 = aux[0]; *a1 = aux[1];
        return hipSuccess;
    }
    hipError_t copy_stream(hipStream_t *cs) { /* uploads of a staged level of the resident engine, beside the kernels of the level before */
        if (!pre) { const hipError_t e = hipStreamCreateWithFlags(&pre, hipStreamNonBlocking); if (e != hipSuccess) return e; }
        *cs = pre;
        return hipSuccess;
    }
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    hipStream_t pre = nullptr; /* copy_stream() */
    hipEvent_t last_emission = nullptr; /* end of the emission kernel of the most recent launch on this context (owned by its batch) */
    hipEvent_t fork = nullptr, join[2] = {nullptr, nullptr};
    /* Waiting for a stream without burning a core: hipStreamSynchronize polls (a batch thread of mrp_phase_reads_many spent
     * 85 % of a call spinning in it); an event created with hipEventBlockingSync makes the waiter sleep until the
     * interrupt.  One event per context: a context is driven by one host thread at a time. */
    hipEvent_t block_ev = nullptr;
    double wait_cpu_ms = 0, wait_wall_ms = 0; /* MRP_TIMING: thread CPU / wall time spent inside wait_stream */
    hipError_t wait_stream(hipStream_t s) {
        timespec c0, c1, w0, w1;
        clock_gettime(CLOCK_THREAD_CPUTIME_ID, &c0); clock_gettime(CLOCK_MONOTONIC, &w0);
        const hipError_t e = wait_stream_impl(s);
        clock_gettime(CLOCK_THREAD_CPUTIME_ID, &c1); clock_gettime(CLOCK_MONOTONIC, &w1);
        wait_cpu_ms += 1e3 * (c1.tv_sec - c0.tv_sec) + 1e-6 * (c1.tv_nsec - c0.tv_nsec);
        wait_wall_ms += 1e3 * (w1.tv_sec - w0.tv_sec) + 1e-6 * (w1.tv_nsec - w0.tv_nsec);
        return e;
    }
    hipError_t wait_stream_impl(hipStream_t s) {
        if (!block_ev) {
            hipError_t e = hipEventCreateWithFlags(&block_ev, hipEventDisableTiming);
            if (e != hipSuccess) { block_ev = nullptr; return hipStreamSynchronize(s); }
        }
        hipError_t e = hipEventRecord(block_ev, s);
        if (e != hipSuccess) return e;
        /* hipEventSynchronize spins on this runtime even for an event created with hipEventBlockingSync (measured: 68 ms of
         * wall = 68 ms of thread CPU per batch thread and call): query and sleep instead -- a level waits milliseconds, 30 us
         * of extra latency per wait is nothing */
        for (;;) {
            e = hipEventQuery(block_ev);
            if (e != hipErrorNotReady) return e;
            timespec ts{0, 30000};
            nanosleep(&ts, nullptr);
        }
    }
    DevPool pool;
    int test_hooks = 0;   /* mrp_context_set_test_hooks (test suite only) */
    LaunchCensus census;  /* launches of the resident path by class, this context's own (mrp_context_launch_census sums the siblings') */
    int wide_pairs = 0;   /* mrp_context_set_wide_pairs: pairs beyond the pair-per-wave kernel's 2 048 cells go to the pair-per-workgroup kernel */
    int sv_split = 0;     /* mrp_context_set_sv_split: indel_size_for_sv_handling > 0 splits the extraction's walk by class of variant */
    int64_t max_depth = 0;   /* mrp_context_set_downsampling: > 0 makes the aligned composites' mask on the device (0: off) */
    uint64_t downsampling_seed = 0;
    mrp_downsampling_stats last_downsampling{}; /* mrp_context_last_downsampling */
    int64_t posterior_workspace = 0; /* mrp_context_set_posterior_workspace: bytes of forward diagonals a group of mrp_posterior_aligned_pairs keeps (0: the default) */
    mrp_posterior_stats last_posterior{}; /* mrp_context_last_posterior */
    int64_t wide_pair_count = 0, wide_cell_count = 0; /* what that kernel has taken on this context (mrp_context_wide_pair_count) */
    int phase_groups = 0; /* concurrent batches of mrp_phase_reads_many (mrp_context_set_phase_groups); 0: chosen by batch size */
    std::vector<mrp_context *> siblings; /* further contexts on the same device (concurrent batches of mrp_phase_reads_many) */
    std::mutex sibling_mu;
    /* the emptied batch objects of the last resident engine on this context (their host arrays keep their capacity and their mapped
     * pages from one mrp_phase_reads_many call to the next) and its level objects (page-locked staging blocks, events): allocating
     * page-locked memory takes milliseconds and synchronizes the device (owned here, managed by mrp_engine.cpp) */
    std::vector<struct mrp_engine_level_state *> spare_levels;
    std::vector<struct mrp_batch *> spare_batches;
    int posterior_wide_pairs = 0; /* mrp_context_set_posterior_wide_pairs: the posterior entries run pairs beyond 2 048 cells on their pair-per-workgroup kernels */
    int64_t posterior_wide_count = 0, posterior_wide_cells = 0; /* what those kernels have taken on this context (mrp_context_posterior_wide_count) */
    int rle_lane_pairs = 0; /* mrp_context_set_rle_lane_pairs: mrp_forward_probabilities_rle runs its eligible pairs on the pair-per-lane kernel */
};

struct mrp_chunk {
    mrp_context *ctx = nullptr;
    int64_t n_sites = 0, pool_bytes = 0;
    std::vector<uint32_t> allele_number, allele_offset, sub_offset;
    std::vector<int32_t> same_until; /* [n_sites] first site after i whose allele count differs from site i's (n_sites if none) */
    std::vector<uint16_t> sub, prior; /* host copies for the structural code (rphmm_*.c) */
    std::vector<uint8_t> pool;
    const uint8_t *pool_host = nullptr; /* the profile bytes on the host: pool.data(), or the copy in the page-locked block of a work queue's batch */
    uint32_t max_sub = 0, max_prior = 0, max_alleles = 1;
    DevBufGroup arrays; /* mrp_chunk_create: the chunk's own device arrays (a chunk of a block has none) */
    DevBuf<uint32_t> d_allele_number{arrays}, d_allele_offset{arrays}, d_sub_offset{arrays};
    DevBuf<int32_t> d_same_until{arrays};
    DevBuf<uint16_t> d_sub{arrays}, d_prior{arrays};
    DevBuf<uint8_t> d_pool{arrays};
    DevChunk dev{};
    /* a chunk whose uploads were queued but not waited for (a work queue uploads its next batch beside the current one): the
     * event ends them.  Device work that reads the chunk waits for it on its stream (mrp_engine.cpp) or on the host
     * (host_wait: the paths that upload on the default path). */
    mutable hipEvent_t ready = nullptr;
    bool owns_ready = true; /* false: the event belongs to the block the chunk was uploaded with (mrp_chunk_block) */
    mutable std::atomic<bool> ready_pending{false};
    /* a chunk whose profile bytes were written on the device (mrp_phase_string_chunks): pool_host is filled by a download still in
     * flight, which this event (not owned) ends; mrp_chunk_host_view waits for it before the host code reads a byte */
    hipEvent_t pool_host_ready = nullptr;
    mutable std::atomic<bool> pool_host_pending{false};
    hipError_t host_wait() const {
        if (!ready_pending.load()) return hipSuccess;
        const hipError_t e = hipEventSynchronize(ready);
        if (e == hipSuccess) ready_pending.store(false);
        return e;
    }
    ~mrp_chunk() {
        if (ready && owns_ready) { (void) hipEventSynchronize(ready); (void) hipEventDestroy(ready); }
    }
};

/* page-locked, grow-only host buffer: source of asynchronous uploads */
struct PinnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    ~PinnedBuf() { if (p) (void) hipHostFree(p); }
    hipError_t reserve(size_t want) {
        if (want <= bytes) return hipSuccess;
        if (p) (void) hipHostFree(p);
        p = nullptr; bytes = 0;
        const size_t sz = std::max<size_t>(want + want / 4, (size_t) 1 << 20);
        hipError_t e = hipHostMalloc(&p, sz, hipHostMallocDefault);
        if (e == hipSuccess) bytes = sz;
        return e;
    }
};

/* device + staging storage of the chunks of one batch of a work queue (mrp_chunk_block_create); outlives its chunks and
 * is reused for the batch after next */
struct mrp_chunk_block {
    PinnedBuf host;
    DevBuf<uint8_t> dev;
    hipEvent_t ready = nullptr;              /* end of the whole upload */
    std::vector<hipEvent_t> group_ready;     /* end of the upload of every group of chunks (the chunks of a group are contiguous in the block) */
    ~mrp_chunk_block() {
        if (ready) { (void) hipEventSynchronize(ready); (void) hipEventDestroy(ready); }
        for (hipEvent_t e : group_ready) if (e) (void) hipEventDestroy(e);
    }
};

struct JobOut {
    double *cell_f, *cell_b, *merge_f, *merge_b, *col_total, *hmm_f, *hmm_b;
    int64_t cell0, n_cells, mcell0, n_merge, col0, n_cols;
    bool int_path = false; /* swept by the max-plus int32 kernel (decided in mrp_batch_upload) */
};

struct mrp_batch {
    mrp_context *ctx = nullptr;
    std::mutex mu; /* mrp_batch_add may be called from several host threads (recording) */
    std::vector<const mrp_chunk *> chunks;
    HostVec<DevHmm> hmms;
    HostVec<DevCol> cols;
    HostVec<int64_t> read_byte_off;
    HostVec<uint64_t> partition;
    HostVec<SweepCol> scols;
    HostVec<PlaneCol> pcols;
    HostVec<uint32_t> cell_next, cell_prev, cell_np;
    HostVec<EmitTile> tiles;
    int64_t n_fast_tiles = 0;
    int64_t n_tiles_dev = 0;   /* tiles on the device (a resident batch's are written there from d_tilecols: tiles stays empty) */
    /* resident merge levels: launched between the byte packing and the recursion kernels, in place of the emission kernel
     * (cross product + emission in one pass, mrp_launch_cross_emit) */
    std::function<hipError_t(hipStream_t)> pre_sweep;
    DevBufGroup arrays; /* every device array of the batch */
    DevBuf<TileCol> d_tilecols{arrays};
    bool need_wide = false;
    std::vector<JobOut> outs;
    int64_t n_merge = 0, n_slots = 0;
    int64_t n_cells_total = 0; /* cells incl. alignment padding */
    bool resident = false;     /* cell arrays are produced on the device */
    mrp_launch_stats stats{};
    /* launch plan */
    std::vector<int32_t> order_wide, order_mid, order_narrow, order_f64, order_lse, order_lse_big, order_gen; /* order_f64 = order_lse + order_lse_big + order_gen */
    int max_merge_wide = 1, max_merge_mid = 1, max_merge_narrow = 1, max_merge_lse = 1, max_merge_lse_big = 1;
    /* device */
    bool uploaded = false, launched = false;
    /* events of the most recent launches: [0] planes start, [1] planes end, [2] sweeps end, [3] emission end, [4] emission start */
    static constexpr int EV_RING = 32;
    std::vector<std::array<hipEvent_t, 5>> ev_ring;
    int64_t n_launches = 0, stats_mark = 0; /* stats_mark: launches already reported by an earlier mrp_batch_stats */
    DevBuf<DevHmm> d_hmms{arrays};
    DevBuf<DevCol> d_cols{arrays};
    DevBuf<DevChunk> d_chunks{arrays};
    DevBuf<int64_t> d_read_byte_off{arrays};
    DevBuf<uint64_t> d_partition{arrays}, d_planes{arrays};
    DevBuf<SweepCol> d_scols{arrays};
    DevBuf<PlaneCol> d_pcols{arrays};
    DevBuf<uint32_t> d_next{arrays}, d_prev{arrays}, d_np{arrays}, d_slot_total{arrays}, d_slot_bytes{arrays}, d_cost{arrays};
    DevBuf<double> d_f{arrays}, d_b{arrays}, d_mf{arrays}, d_mb{arrays}, d_total{arrays}, d_hmm_fb{arrays};
    DevBuf<int32_t> d_f32{arrays}, d_b32{arrays}, d_mf32{arrays}, d_mb32{arrays};
    DevBuf<int32_t> d_order_wide{arrays}, d_order_mid{arrays}, d_order_narrow{arrays}, d_order_f64{arrays}, d_order_lse{arrays}, d_order_lse_big{arrays},
        d_pack_list{arrays}, d_plane_list{arrays};
    DevBuf<EmitTile> d_tiles{arrays};
    MrpBatchDev dev{};
    /* back to the empty state, keeping the capacity of the host arrays (the resident engine reuses one batch object for
     * all levels of a run: their descriptor arrays are tens of megabytes).  Only after the stream was synchronized. */
    void recycle() {
        arrays.release();
        chunks.clear(); hmms.clear(); cols.clear(); read_byte_off.clear(); partition.clear(); scols.clear(); pcols.clear();
        cell_next.clear(); cell_prev.clear(); cell_np.clear(); tiles.clear(); outs.clear();
        order_wide.clear(); order_mid.clear(); order_narrow.clear(); order_f64.clear(); order_lse.clear(); order_lse_big.clear(); order_gen.clear();
        n_fast_tiles = 0; n_tiles_dev = 0; need_wide = false; n_merge = 0; n_slots = 0; n_cells_total = 0; resident = false;
        stats = mrp_launch_stats{};
        max_merge_wide = max_merge_mid = max_merge_narrow = max_merge_lse = max_merge_lse_big = 1;
        uploaded = launched = false;
        n_launches = 0; stats_mark = 0; /* (the events stay: every launch of the emptied batch has been waited for) */
        dev = MrpBatchDev{};
    }
    void bind_pool(DevPool *pl) { arrays.bind(pl); }
    /* The device view of the batch: every pointer from its DevBuf (NULL for an array that was never allocated or was released) and
     * the counts the batch knows.  The resident engine overrides what is its own (launch_size_batch). */
    MrpBatchDev view() const {
        MrpBatchDev d{};
        d.hmms = d_hmms.p; d.cols = d_cols.p; d.scols = d_scols.p; d.pcols = d_pcols.p; d.chunks = d_chunks.p; d.read_byte_off = d_read_byte_off.p;
        d.pack_list = d_pack_list.p; d.plane_list = d_plane_list.p; d.n_pack_list = (int64_t) d_pack_list.n; d.n_plane_list = (int64_t) d_plane_list.n;
        d.partition = d_partition.p; d.cell_np = d_np.p; d.cell_next = d_next.p; d.cell_prev = d_prev.p;
        d.planes = d_planes.p; d.slot_total = d_slot_total.p; d.slot_bytes = d_slot_bytes.p; d.cell_cost = d_cost.p;
        d.cell_f32 = d_f32.p; d.cell_b32 = d_b32.p; d.merge_f32 = d_mf32.p; d.merge_b32 = d_mb32.p;
        d.cell_f = d_f.p; d.cell_b = d_b.p; d.merge_f = d_mf.p; d.merge_b = d_mb.p; d.col_total = d_total.p; d.hmm_fb = d_hmm_fb.p;
        d.n_hmms = (int64_t) hmms.size(); d.n_cols = (int64_t) cols.size(); d.n_cells = n_cells_total; d.n_merge = n_merge; d.n_slots = n_slots;
        return d;
    }
};

/* releases what mrp_engine.cpp parked in the context (mrp_context_destroy) */
void mrp_engine_release_context_cache(mrp_context *ctx);
/* groups > 1: chunk i belongs to group i % groups (the concurrent batches mrp_phase_reads_many will deal the chunks to); the block is
 * laid out and uploaded group by group, and a chunk is ready when its group's copy has ended -- the first batch's kernels need not wait
 * for the last batch's bytes */
/* device_pools (optional): the profile bytes of chunk i are already on the device at device_pools[i] (followed by
 * MRP_POOL_TAIL_PAD bytes of the allocation) and descs[i]->profile_pool is the caller's host copy of them; only the site tables are staged */
int mrp_chunk_block_create(mrp_context *ctx, int64_t n, const mrp_chunk_desc *const *descs, mrp_chunk **out, mrp_chunk_block *blk, int groups = 1,
                           const uint8_t *const *device_pools = nullptr);
/* mrp_phase_string_chunks in three steps (mrp_string_chunks.hip), so that a work queue can check every chunk before its first lane
 * starts and a lane can make the front of its next batch while the current one is on the device:
 *   check        MRP_ERR_ARG for malformed arguments (host only, the one call's own checks);
 *   check_pairs  MRP_ERR_UNSUPPORTED for a pair whose diagonal exceeds the pair-per-wave kernel's limit (host only);
 *   front        symbol pool, substring owners, pair list, anchors, launch classes (host only, no context; any thread);
 *   run          uploads, kernels, phasing, HP tags, results -- on the thread of ctx; a front is run once.
 * The front keeps pointers into chunks[]: the array lives until the run has returned. */
struct mrp_string_front;
/* rest (NULL, or one mrp_string_chunk_rest per chunk): the back half of mrp_phase_string_chunks_with_filtered travels with its chunk
 * through the same three steps; filtered_out (zeroed by the caller) and filtered_stats (added to) are filled when the front was made
 * with a rest.  who: the entry the caller called, the prefix of every message. */
int mrp_string_chunks_check(int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_pair_hmm *forward_model, const mrp_pair_hmm *reverse_model,
                            int64_t expansion, const mrp_params *params, mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out,
                            const mrp_string_chunk_rest *rest, const char *who);
/* wide_pairs: the caller's setting (a context's or a queue's): check_pairs and the front then refuse only beyond the wide kernel's caps */
int mrp_string_chunks_check_pairs(int64_t n_chunks, const mrp_string_chunk *chunks, int64_t expansion, int64_t sv_threshold, const mrp_string_chunk_rest *rest,
                                  const char *who, int wide_pairs);
int mrp_string_front_create(int64_t n_chunks, const mrp_string_chunk *chunks, const mrp_string_chunk_rest *rest, const mrp_pair_hmm *forward_model,
                            const mrp_pair_hmm *reverse_model, int64_t expansion, int64_t sv_threshold, int wide_pairs, mrp_string_front **front_out);
void mrp_string_front_destroy(mrp_string_front *front);
int mrp_string_front_run(mrp_context *ctx, mrp_string_front *front, double het_substitution_probability, const mrp_params *params, int64_t min_phred,
                         mrp_phase_result **out, int8_t *const *hap_out, double *const *phred_out, mrp_profile_out *profiles_out,
                         mrp_string_chunks_stats *stats, mrp_filtered_out *filtered_out, mrp_string_filtered_stats *filtered_stats);
/* frees every array of a result the string-chunk calls filled (mrp_free is free) and zeroes the struct */
static inline void mrp_profile_out_clear(mrp_profile_out *P) {
    free(P->seqs); free(P->read_of_seq); free(P->pool); free(P->allele_number); free(P->substitution); free(P->prior);
    memset(P, 0, sizeof(*P));
}
static inline void mrp_filtered_out_clear(mrp_filtered_out *O) {
    free(O->read_hap); free(O->h1); free(O->h2); free(O->variant_state); free(O->cis); free(O->trans);
    memset(O, 0, sizeof(*O));
}
static inline void mrp_variant_records_clear(mrp_variant_records *R) {
    free(R->state); free(R->gt); free(R->genotype_log_prob); free(R->hap1_log_prob); free(R->hap2_log_prob); free(R->read_first); free(R->n_hap1);
    free(R->n_hap2); free(R->reads);
    memset(R, 0, sizeof(*R));
}
/* mrp_extract_read_substrings as one run taken through steps (mrp_extract.hip), so that a composite (mrp_haplotag_aligned_chunks,
 * mrp_aligned.hip) can stop before the download and read the result where it lies in HBM:
 *   check_args / check_modes / check_chunks   MRP_ERR_ARG for malformed arguments, MRP_ERR_UNSUPPORTED for the two refused modes, the
 *                  chunks' own checks and the windows (host only; the entry decides their order);
 *   stage          the call's reads, ops, bases and variants in one staging block, and its upload on ctx->stream;
 *   first_half     scan, count; the one total starts on its way back;
 *   totals         the allele strings on the worker pool beside the first half, then the wait for the total;
 *   second_half    locate, sort by variant, gather: the symbols go to pool + base (a device pool of the caller's with room for
 *                  n_bases behind base) or, with pool NULL, to a pool of the run's own;
 *   download       everything back and the per-chunk outputs (mrp_extract_read_substrings only);
 *   stats / times  the events and counts (after the stream has drained), then total_ms and host_ms;
 *   release        every device array back to ctx's pool, which is reclaimed (after the stream has drained).
 * The run keeps pointers into chunks[] and writes stats (zeroed by create; may be NULL). */
struct mrp_extract_run;
struct mrp_extract_device { /* what the second half leaves in HBM; read indices are global to the call */
    int64_t n_reads, n_variants, n_entries, n_bases;
    const uint8_t *read_status;  /* n_reads: MRP_READ_* */
    const int64_t *entry_first;  /* n_variants + 1: the entry CSR by variant, entries in ascending read order */
    const int32_t *entry_read;   /* per entry */
    const int64_t *entry_len;
    const int64_t *entry_off;    /* n_entries + 1: the scan of entry_len, from 0 */
    const uint8_t *symbols;      /* entry e's symbols: symbols[entry_off[e] .. + entry_len[e]) (= pool + base) */
    /* per read, as the first half left them (what the downsampling reads, mrp_downsample.hip): read r saved
     * read_entry_first[r + 1] - read_entry_first[r] substrings (n_reads + 1, from 0), and the walk bound alnReadLength + 1 of a read that
     * is not MRP_READ_DROPPED is read_limit[r * read_limit_stride] (never written for a dropped read) */
    const int64_t *read_entry_first, *read_limit;
    int64_t read_limit_stride;
    const int64_t *read_first, *variant_first; /* host, n_chunks + 1: chunk c's share of the call's reads / variants */
};
mrp_extract_run *mrp_extract_run_create(const char *who, int64_t n_chunks, const mrp_aligned_chunk *chunks, const mrp_extract_options *options,
                                        mrp_extract_stats *stats);
void mrp_extract_run_destroy(mrp_extract_run *run);
int mrp_extract_run_check_args(mrp_extract_run *run, bool have_out);
/* sv_split: the caller's setting (a context's or a queue's; 0 for none): indel_size_for_sv_handling > 0 then runs the walk per class
 * of variant instead of being refused */
int mrp_extract_run_check_modes(mrp_extract_run *run, int sv_split);
int mrp_extract_run_check_chunks(mrp_extract_run *run);
int mrp_extract_run_stage(mrp_extract_run *run, mrp_context *ctx);
int mrp_extract_run_first_half(mrp_extract_run *run);
int mrp_extract_run_totals(mrp_extract_run *run, int64_t *n_entries, int64_t *n_bases);
int mrp_extract_run_second_half(mrp_extract_run *run, uint8_t *pool, int64_t base);
int mrp_extract_run_download(mrp_extract_run *run, mrp_extracted_chunk **out);
int mrp_extract_run_stats(mrp_extract_run *run);
void mrp_extract_run_times(mrp_extract_run *run, bool to_now);
void mrp_extract_run_release(mrp_extract_run *run);
void mrp_extract_run_device(const mrp_extract_run *run, mrp_extract_device *view);
/* every chunk's allele strings (prefix + allele + suffix, symbols) one after the other: their bytes; the strings into dst and, per allele
 * of the call in chunk then allele order, where each lies in dst */
int64_t mrp_extract_run_allele_bytes(const mrp_extract_run *run);
void mrp_extract_run_alleles(const mrp_extract_run *run, uint8_t *dst, int64_t *allele_off, int32_t *allele_len);
/* getKmerAlignmentAnchors on the device (mrp_anchors.hip) for n_pairs pairs (host arrays) over a symbol pool that is already in HBM,
 * written by work queued on ctx->stream before this call: anchor_off[n_pairs + 1] from 0 and the anchors (x, y) in pair order.  Runs on
 * ctx->stream and returns with the stream drained; its device arrays go back to ctx's pool, which the caller reclaims.  The anchors
 * come back as diagonal runs (x, y, length) and are expanded here.  kernel_ms (HIP events around the kernels), bytes_downloaded (4 B
 * per pair, 12 B per run) and n_runs_out may be NULL. */
int mrp_kmer_anchors_on_device(mrp_context *ctx, const char *who, const uint8_t *device_pool, int64_t n_pairs, const int64_t *x_off,
                               const int32_t *x_len, const int64_t *y_off, const int32_t *y_len, int64_t *anchor_off, std::vector<int64_t> &anchors,
                               double *kernel_ms, int64_t *bytes_downloaded, int64_t *n_runs_out);
/* mrp_phase_aligned_chunks and mrp_phase_aligned_chunks_with_filtered in steps (mrp_aligned.hip), so that a work queue can check every
 * chunk before its first lane starts and a lane can make the host part of its next batch's front beside the current batch:
 *   check    every MRP_ERR_ARG of the call, then MRP_ERR_UNSUPPORTED for the two refused extraction modes, over all chunks and in the
 *            one call's order (host only, no context; messages name the chunks as the one call does);
 *   create   the same checks, and the front they leave: the extraction's records and run with the windows (host only; any thread);
 *   stage    on ctx, on its thread: the extraction, the classes, the owners, the pair list, the rests, the anchors, the launch
 *            classes -- MRP_ERR_NO_DEVICE for a NULL ctx, MRP_ERR_UNSUPPORTED for a diagonal beyond 2 048 cells;
 *   run      the string run over the staged front and the per-chunk lists; a front is staged and run once, on one thread;
 *   destroy  on the thread of ctx once the front was staged (it drains the stream and gives the device arrays back).
 * rest, filtered_out and filtered_read_out are NULL for the plain call.  The front keeps every pointer of args: the arrays live until it
 * is destroyed.  stats / filtered_stats (zeroed by the caller) may be NULL; chunk_stats of run: where the string run's stats go when
 * the front has no stats. */
struct mrp_aligned_front;
struct mrp_aligned_args {
    int64_t n_chunks;
    const mrp_aligned_chunk *chunks;
    const mrp_aligned_chunk_rest *rest;
    const char *const *const *read_names;
    const uint8_t *const *keep;
    const mrp_extract_options *options;
    const mrp_pair_hmm *forward_model, *reverse_model;
    int64_t expansion, sv_threshold;
    double het_substitution_probability;
    const mrp_params *params;
    int64_t min_phred;
    mrp_phase_result **out;
    int8_t *const *hap_out;
    double *const *phred_out;
    mrp_profile_out *profiles_out;
    int64_t **bubble_variant_out;
    mrp_filtered_out *filtered_out;
    int32_t **filtered_read_out;
    int sv_split; /* the context's or the queue's setting at the call (mrp_context_set_sv_split); the checks need no context */
    /* mrp_phase_aligned_chunks_with_records only (NULL otherwise): the records and their share of the stats */
    mrp_variant_records *records_out;
    mrp_phase_aligned_records_stats *records_stats;
    /* the context's or the queue's setting at the call (mrp_context_set_downsampling; 0: off): the checks need no context */
    int64_t max_depth;
    uint64_t downsampling_seed;
};
int mrp_aligned_chunks_check(const char *who, const mrp_aligned_args *args);
int mrp_aligned_front_create(const char *who, double t_begin_ms, const mrp_aligned_args *args, mrp_phase_aligned_stats *stats,
                             mrp_phase_aligned_filtered_stats *filtered_stats, mrp_aligned_front **front_out);
int mrp_aligned_front_stage(mrp_context *ctx, mrp_aligned_front *front);
int mrp_aligned_front_run(mrp_aligned_front *front, mrp_string_chunks_stats *chunk_stats);
void mrp_aligned_front_destroy(mrp_aligned_front *front);

/* mrp_haplotag_aligned_chunks in the same steps (mrp_aligned.hip):
 *   check    create + destroy over all chunks: every MRP_ERR_ARG of the call, then the two refused modes (host only, no context);
 *   create   HaRun::check and the front it leaves: the extraction's run with the windows (host only; any thread);
 *   stage    on ctx, on its thread: the extraction and the owners -- MRP_ERR_NO_DEVICE for a NULL ctx;
 *   run      the pair list, the pair-HMM and the scoring, the outputs -- MRP_ERR_UNSUPPORTED for a diagonal beyond 2 048 cells, raised
 *            before any pair-HMM kernel; a front is staged and run once, on one thread;
 *   destroy  on the thread of ctx once the front was staged.
 * The front keeps every pointer of args: the arrays live until it is destroyed.  stats (zeroed by the caller) may be NULL. */
struct mrp_haplotag_front;
struct mrp_haplotag_args {
    int64_t n_chunks;
    const mrp_aligned_chunk *chunks;
    const int32_t *const *gt;
    const mrp_extract_options *options;
    const mrp_pair_hmm *forward_model, *reverse_model;
    int64_t expansion;
    int8_t *const *hap_out;
    double *const *h1_out, *const *h2_out;
    int sv_split; /* the context's or the queue's setting at the call (mrp_context_set_sv_split); the checks need no context */
};
int mrp_haplotag_chunks_check(const mrp_haplotag_args *args);
int mrp_haplotag_front_create(const mrp_haplotag_args *args, mrp_haplotag_aligned_stats *stats, mrp_haplotag_front **front_out);
int mrp_haplotag_front_stage(mrp_context *ctx, mrp_haplotag_front *front);
int mrp_haplotag_front_run(mrp_haplotag_front *front);
void mrp_haplotag_front_destroy(mrp_haplotag_front *front);
/* The downsampling to maxDepth on the device (mrp_downsample.hip): one workgroup per chunk over device arrays,
 * queued on s.  A chunk owns reads [first, first + n_reads) of the call; the per-read inputs are either the seam's (l, h) or the
 * extraction's own (entry_first, limit: mrp_extract_device's read_entry_first / read_limit).  d_keep gets a byte per read of the chunks,
 * d_prob (may be NULL) its probability, d_downsampled per chunk whether it was not shallow. */
struct MrpDsChunk { int64_t first, n_reads, V, overlap_start, overlap_end; };
struct MrpDsIn {
    const int32_t *l, *h;                    /* NULL: read the extraction's */
    const int64_t *entry_first, *limit;
    int64_t limit_stride;
};
hipError_t mrp_downsample_launch(hipStream_t s, int64_t n_chunks, const MrpDsChunk *d_chunks, const MrpDsIn &in, const uint8_t *d_status, int64_t max_depth,
                                 uint64_t seed, double *d_prob, uint8_t *d_keep, int32_t *d_downsampled);
extern "C" void mrp_batch_last_launch_ms(struct mrp_batch *b, float *pack, float *emission, float *recursion);

/* development: MRP_DUP=<letters> launches the named kernel families of a resident level TWICE (they are idempotent) -- the slow-down of a
 * step is that family's marginal cost in situ: p packing, x cross product + emission, s recursion, r prune, c compaction, l layout,
 * m the one-wave kernel of the small hmms, t the structure kernel, b the trace back */
static inline bool mrp_dup(char c) { const char *e = getenv("MRP_DUP"); return e && strchr(e, c) != nullptr; }
#endif
