/*
 * host_pool_check.cpp -- the persistent host thread pool (margin_amd/csrc/mrp_host_pool.cpp) on its own: every index of every
 * loop runs exactly once, whatever the loop's length and grain, the number of threads, who posts it and to which pool.
 * Built together with the pool and run by tests/test_host_pool.py, once with the thread sanitizer and once with the address and
 * undefined-behaviour sanitizers; prints "host pool ok".
 */
#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <thread>
#include <vector>

#include "../margin_amd/csrc/mrp_host_pool.h"

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

/* stands in for the library's error slot (mrp_context.cpp) */
static thread_local char g_err[256] = "";
extern "C" int mrp_set_error(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

struct Hits {
    int64_t n;
    std::unique_ptr<std::atomic<int>[]> count;
    explicit Hits(int64_t n_) : n(n_), count(new std::atomic<int>[(size_t) n_ + 1]) { for (int64_t i = 0; i <= n; i++) count[(size_t) i].store(0); }
    static void hit(int64_t i, void *arg) {
        Hits *h = static_cast<Hits *>(arg);
        CHECK(i >= 0 && i < h->n);
        h->count[(size_t) i].fetch_add(1, std::memory_order_relaxed);
    }
    void check_once() const { for (int64_t i = 0; i < n; i++) CHECK(count[(size_t) i].load() == 1); CHECK(count[(size_t) n].load() == 0); }
};

static void run_once(int64_t n, int64_t grain) {
    Hits h(n);
    mrp_pool_run(n, grain, Hits::hit, &h);
    h.check_once();
}

/* lengths and grains on both sides of the thread count and of the pool's 16 index ranges, and the range split itself */
static void check_shapes() {
    for (int64_t n : {0, 1, 15, 16, 17, 4097})
        for (int64_t grain : {(int64_t) 1, (int64_t) 3, n, n + 1}) run_once(n, grain);
    for (int64_t grain : {1, 2, 3, 7, 64})
        for (int64_t n : {16 * grain - 1, 16 * grain, 16 * grain + 1}) run_once(n, grain);
}

/* four threads post 50 loops each at the same time, each with its own priority */
static void check_concurrent_posters() {
    std::vector<std::thread> th;
    for (int p = 0; p < 4; p++)
        th.emplace_back([p] {
            mrp_pool_set_priority(p);
            for (int r = 0; r < 50; r++) run_once(1 + (r * 37 + p * 11) % 600, 1 + r % 4);
        });
    for (auto &t : th) t.join();
}

/* a loop posted from inside a loop body (by the poster or by a worker, whoever runs the index) */
static void check_nested() {
    struct Outer { Hits outer{12}; std::vector<std::unique_ptr<Hits>> inner; } o;
    for (int i = 0; i < 12; i++) o.inner.emplace_back(new Hits(40 + i));
    mrp_pool_run(12, 1, [](int64_t i, void *arg) {
        Outer *q = static_cast<Outer *>(arg);
        Hits::hit(i, &q->outer);
        mrp_pool_run(q->inner[(size_t) i]->n, 2, Hits::hit, q->inner[(size_t) i].get());
    }, &o);
    o.outer.check_once();
    for (auto &h : o.inner) h->check_once();
}

/* mrp_pool_set_weight: a loop announced as a few microseconds runs on the calling thread; a long one wakes a capped number of workers */
static void check_weights() {
    mrp_pool_set_weight(1);
    struct Here { std::thread::id me; Hits h{300}; } q;
    q.me = std::this_thread::get_id();
    mrp_pool_run(300, 1, [](int64_t i, void *arg) {
        Here *p = static_cast<Here *>(arg);
        CHECK(std::this_thread::get_id() == p->me);
        Hits::hit(i, &p->h);
    }, &q);
    q.h.check_once();
    for (int64_t n : {1, 17, 4097}) run_once(n, 1);
    mrp_pool_set_weight(1000);
    run_once(4097, 1);
    run_once(4097, 3);
    mrp_pool_set_weight(0);
}

/* a pool of its own: adopted by two threads at once, given back, destroyed while the process pool lives on */
static void check_private_pool() {
    mrp_host_pool *p = mrp_host_pool_create(3);
    CHECK(p != nullptr);
    std::vector<std::thread> th;
    for (int t = 0; t < 2; t++)
        th.emplace_back([p, t] {
            CHECK(mrp_pool_current() == nullptr);
            mrp_pool_adopt(p);
            CHECK(mrp_pool_current() == p);
            for (int r = 0; r < 30; r++) run_once(1 + (r * 53 + t * 7) % 900, 1 + r % 5);
            mrp_pool_adopt(nullptr);
            CHECK(mrp_pool_current() == nullptr);
            run_once(333, 2); /* the process pool again */
        });
    for (auto &t : th) t.join();
    mrp_host_pool_destroy(p);
    run_once(4097, 1);
}

int main() {
    CHECK(mrp_set_host_threads(0) == MRP_ERR_ARG && strstr(g_err, "outside 1..256"));
    CHECK(mrp_set_host_threads(257) == MRP_ERR_ARG);
    CHECK(mrp_host_threads_setting() == 0);
    for (int threads : {1, 8}) { /* 1: every loop runs inline */
        CHECK(mrp_set_host_threads(threads) == MRP_OK);
        CHECK(mrp_host_threads() == threads && mrp_host_threads_setting() == threads);
        check_shapes();
        check_concurrent_posters();
        check_nested();
        check_weights();
        check_private_pool();
    }
    printf("host pool ok\n");
    return 0;
}
