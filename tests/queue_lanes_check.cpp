/*
 * queue_lanes_check.cpp -- the hand-out of the work queue (margin_amd/csrc/mrp_queue_lanes.cpp) on its own, against the contract
 * written above LaneHooks: fake hooks record every call under a mutex and fail where they are told to; the record is then held to
 * what run_lanes promises, with and without a failure.  Built together with mrp_queue_lanes.cpp and run by tests/test_queue_lanes.py,
 * once with the thread sanitizer and once with the address and undefined-behaviour sanitizers; prints "queue lanes ok".
 */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <set>
#include <thread>
#include <vector>

#include "../margin_amd/csrc/mrp_queue_lanes.h"

#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) { fprintf(stderr, "%s:%d: %s [%s]\n", __FILE__, __LINE__, #cond, g_case); exit(1); } \
    } while (0)
static char g_case[160] = "";

enum Kind { START, BEGIN, PREFETCH, PREFETCHED, PHASE, RETIRE, DISCARD, END };
struct Event { Kind kind; int w; int64_t b; int rc; };

/* where a run fails: in begin of lane `w`, or in the prefetch / the phase of batch `b` (a batch is prefetched and phased at most once,
 * and a lane's first batch is fixed, so a batch names its place: first of a lane, taken later, the last one) */
struct Inject { Kind kind; int w; int64_t b; int code; };

struct Run {
    int n_devices, lanes, active;
    int64_t n_batches;
    std::vector<Inject> inject;
    std::mutex mu;
    std::vector<Event> ev;
    std::vector<int> staging;  /* [lane] prefetches of the lane that have not returned */
    int overlaps = 0;          /* phases that began while a prefetch of their lane was running */

    Run(int d, int l, int a, int64_t n) : n_devices(d), lanes(l), active(a), n_batches(n), staging((size_t) (d * l), 0) {}

    int failure(Kind kind, int w, int64_t b) const {
        for (const Inject &i : inject)
            if (i.kind == kind && (kind == BEGIN ? i.w == w : i.b == b)) return i.code;
        return MRP_OK;
    }
    int note(Kind kind, int w, int64_t b) {
        const int rc = failure(kind, w, b);
        {
            std::lock_guard<std::mutex> lk(mu);
            CHECK(w >= 0 && w < n_devices * lanes);
            CHECK(kind == START || kind == BEGIN || kind == END || (b >= 0 && b < n_batches));
            if (kind == PREFETCH) staging[(size_t) w]++;
            if (kind == PHASE && staging[(size_t) w] > 0) overlaps++;
            /* retire(w, cur): the prefetch that ran beside phase(w, cur) has returned; no lane stages two batches at a time */
            if (kind == RETIRE) CHECK(staging[(size_t) w] == 0);
            if (kind == PREFETCH) CHECK(staging[(size_t) w] == 1);
            ev.push_back({kind, w, b, rc});
        }
        std::this_thread::yield(); /* (lets the lanes interleave) */
        if (kind == PREFETCH) {
            std::lock_guard<std::mutex> lk(mu);
            staging[(size_t) w]--;
            ev.push_back({PREFETCHED, w, b, rc});
        }
        return rc;
    }

    int go(bool own_thread_for_lane0, bool with_start) {
        LaneHooks hk;
        hk.begin = [this](int w) { return note(BEGIN, w, -1); };
        hk.prefetch = [this](int w, int64_t b) { return note(PREFETCH, w, b); };
        hk.phase = [this](int w, int64_t b) { return note(PHASE, w, b); };
        hk.retire = [this](int w, int64_t b) { (void) note(RETIRE, w, b); };
        hk.discard = [this](int w, int64_t b) { (void) note(DISCARD, w, b); };
        hk.end = [this](int w) { (void) note(END, w, -1); };
        std::function<void(int)> on_start;
        if (with_start) on_start = [this](int w) { (void) note(START, w, -1); };
        const int rc = run_lanes(n_devices, lanes, active, n_batches, hk, own_thread_for_lane0, on_start);
        size_t n_events;
        { std::lock_guard<std::mutex> lk(mu); n_events = ev.size(); }
        std::this_thread::yield();
        std::lock_guard<std::mutex> lk(mu);
        CHECK(ev.size() == n_events); /* no hook is called after run_lanes has returned */
        for (int s : staging) CHECK(s == 0);
        return rc;
    }

    /* positions in the record of the calls of one kind for batch b (any lane) */
    std::vector<size_t> where(Kind kind, int64_t b) const {
        std::vector<size_t> at;
        for (size_t i = 0; i < ev.size(); i++)
            if (ev[i].kind == kind && ev[i].b == b) at.push_back(i);
        return at;
    }

    /* what holds with and without a failure */
    void check_always(bool with_start) const {
        const int n_workers = n_devices * lanes;
        for (int w = 0; w < n_workers; w++) {
            std::vector<Event> mine;
            for (const Event &e : ev)
                if (e.w == w) mine.push_back(e);
            /* on_thread_start: once per worker, before any other hook of that worker */
            if (with_start) { CHECK(!mine.empty() && mine[0].kind == START); mine.erase(mine.begin()); }
            for (const Event &e : mine) CHECK(e.kind != START);
            const int64_t first = (int64_t) (w % lanes) * n_devices + w / lanes;
            if (w % lanes >= active || first >= n_batches) { CHECK(mine.empty()); continue; } /* a lane without work calls no hook */
            /* begin first; end last, and if and only if begin returned MRP_OK; neither twice */
            CHECK(!mine.empty() && mine[0].kind == BEGIN);
            const bool began = mine[0].rc == MRP_OK;
            if (!began) { CHECK(mine.size() == 1); continue; }
            CHECK(mine.size() >= 3 && mine.back().kind == END);
            for (size_t i = 1; i + 1 < mine.size(); i++) CHECK(mine[i].kind != BEGIN && mine[i].kind != END);
            CHECK(mine[1].kind == PREFETCH && mine[1].b == first); /* the lane's first batch is fixed */
        }
        for (int64_t b = 0; b < n_batches; b++) {
            const std::vector<size_t> pre = where(PREFETCH, b), done = where(PREFETCHED, b), ph = where(PHASE, b), re = where(RETIRE, b), di = where(DISCARD, b);
            CHECK(pre.size() <= 1 && ph.size() <= 1); /* no batch is staged or phased twice */
            if (pre.empty()) { CHECK(ph.empty() && re.empty() && di.empty()); continue; }
            /* every batch whose prefetch was called ends in exactly one of retire and discard, on its lane, after the prefetch returned */
            CHECK(re.size() + di.size() == 1);
            const size_t last = re.empty() ? di[0] : re[0];
            const int w = ev[pre[0]].w;
            CHECK(done.size() == 1 && done[0] < last && ev[last].w == w);
            /* phased: after a prefetch that returned MRP_OK, then retired; not phased: discarded */
            CHECK(ph.empty() == re.empty());
            if (!ph.empty()) CHECK(ev[pre[0]].rc == MRP_OK && done[0] < ph[0] && ph[0] < re[0] && ev[ph[0]].w == w);
        }
    }
    void check_all_done() const { /* without a failure: every batch prefetched, phased and retired once; nothing discarded */
        for (int64_t b = 0; b < n_batches; b++) CHECK(where(PREFETCH, b).size() == 1 && where(PHASE, b).size() == 1 && where(RETIRE, b).size() == 1);
        for (const Event &e : ev) CHECK(e.kind != DISCARD && e.rc == MRP_OK);
    }
};

static int g_overlaps = 0;

static void no_failure(int n_devices, int lanes, int active, int64_t n_batches, bool own_thread, bool with_start) {
    snprintf(g_case, sizeof(g_case), "%d x %d lanes, %d active, %lld batches, own thread %d, start hook %d", n_devices, lanes, active,
             (long long) n_batches, (int) own_thread, (int) with_start);
    Run r(n_devices, lanes, active, n_batches);
    CHECK(r.go(own_thread, with_start) == MRP_OK);
    r.check_always(with_start);
    r.check_all_done();
    g_overlaps += r.overlaps;
}

static void with_failures(const char *what, std::vector<Inject> inject, bool own_thread) {
    snprintf(g_case, sizeof(g_case), "2 x 4 lanes, 23 batches, failing in %s, own thread %d", what, (int) own_thread);
    Run r(2, 4, 4, 23);
    r.inject = inject;
    const int rc = r.go(own_thread, true);
    std::set<int> codes, raised;
    for (const Inject &i : inject) codes.insert(i.code);
    for (const Event &e : r.ev)
        if (e.rc != MRP_OK && e.kind != PREFETCHED) raised.insert(e.rc);
    CHECK(rc != MRP_OK && codes.count(rc) == 1 && raised.count(rc) == 1); /* one of the injected codes, and one that was returned to it */
    r.check_always(true);
    /* the batch that failed: a failed prefetch is discarded unphased, a failed phase is retired; what its lane had taken ahead is discarded */
    for (const Inject &i : inject) {
        if (i.kind == PREFETCH && !r.where(PREFETCH, i.b).empty()) CHECK(r.where(PHASE, i.b).empty() && r.where(DISCARD, i.b).size() == 1);
        if (i.kind == PHASE && !r.where(PHASE, i.b).empty()) CHECK(r.where(RETIRE, i.b).size() == 1);
    }
    if (inject.size() == 1 && inject[0].kind != BEGIN) CHECK(!r.where(inject[0].kind, inject[0].b).empty()); /* (a lone failure is reached) */
}

int main() {
    const int shapes[4][2] = {{1, 1}, {2, 1}, {2, 4}, {3, 4}};
    for (const auto &s : shapes) {
        const int n_devices = s[0], lanes = s[1];
        const int64_t counts[6] = {0, 1, n_devices, (int64_t) n_devices * lanes - 1, (int64_t) n_devices * lanes, 23};
        for (int64_t n_batches : counts)
            for (int active : std::set<int>{1, std::min(2, lanes), lanes})
                for (int own_thread = 0; own_thread < 2; own_thread++) {
                    no_failure(n_devices, lanes, active, n_batches, own_thread != 0, true);
                    no_failure(n_devices, lanes, active, n_batches, own_thread != 0, false);
                }
    }
    /* 2 devices x 4 lanes: lane w starts on batch (w % 4) * 2 + w / 4 -- batch 3 is the first of lane 5, batch 2 of lane 1; batches 8..22
     * are taken as lanes become free */
    for (int own_thread = 0; own_thread < 2; own_thread++) {
        with_failures("begin", {{BEGIN, 3, -1, 41}}, own_thread != 0);
        with_failures("the first prefetch of a lane", {{PREFETCH, -1, 3, 42}}, own_thread != 0);
        with_failures("a later prefetch", {{PREFETCH, -1, 15, 43}}, own_thread != 0);
        with_failures("the phase of a lane's first batch", {{PHASE, -1, 2, 44}}, own_thread != 0);
        with_failures("the phase of a middle batch", {{PHASE, -1, 12, 45}}, own_thread != 0);
        with_failures("the phase of the last batch", {{PHASE, -1, 22, 46}}, own_thread != 0);
        with_failures("two lanes", {{PHASE, -1, 2, 47}, {PHASE, -1, 5, 48}}, own_thread != 0);
        with_failures("a begin and a phase", {{BEGIN, 6, -1, 49}, {PHASE, -1, 9, 50}}, own_thread != 0);
    }
    /* the plan the lanes are handed: every chunk once, largest first inside the caller's batches */
    const int64_t cost[7] = {5, 9, 1, 9, 0, 7, 3};
    const QueuePlan p = plan_queue(7, cost, 3, 8, 2);
    CHECK(p.batch_off == (std::vector<int64_t>{0, 3, 6, 7}) && p.order == (std::vector<int64_t>{1, 3, 5, 0, 6, 2, 4}));
    CHECK(active_lanes_of(p, cost, 2, 4) == 4 && active_lanes_of(p, cost, 3, 4) == 1);
    fprintf(stderr, "%d phases began beside a prefetch of their lane\n", g_overlaps); /* (allowed, not promised) */
    printf("queue lanes ok\n");
    return 0;
}
