// Stand-alone check of pairec_amd/csrc/coalescer_policy.hpp (built and run by test_coalescer_policy_cpu.py; host only).  The time
// points are made by hand; the expected values are written out from the rules as the coalescer's workers stated them before they
// moved into the header.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "coalescer_policy.hpp"

using namespace pg::policy;

static int g_failed = 0;
#define CHECK(cond)                                                       \
    do {                                                                  \
        if (!(cond)) {                                                    \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                   \
        }                                                                 \
    } while (0)

// microsecond `us` of the test's time line (well away from the clock's epoch, which means "no hold")
static Time at(long us) { return Time(std::chrono::seconds(1000)) + std::chrono::microseconds(us); }
static bool near(double a, double b) { return std::fabs(a - b) <= 1e-12; }

enum { RECALL = 0, RECOMMEND = 1, DPP = 2, RANK = 3, NQ = 4 };       // a small set of queues: two recall-based, two per-item
constexpr uint32_t kWait = 100;

struct World {
    QueueView q[NQ];
    QueuePolicy p[NQ];
    World() { q[DPP].per_item = q[RANK].per_item = true; }
    void put(int f, size_t len, long head_us, bool full = false) {
        q[f].len = len;
        q[f].head_arrived = at(head_us);
        q[f].full = full;
    }
    Choice go(bool idle, long now_us, bool slot_free = true) const { return choose(q, p, NQ, idle, at(now_us), kWait, slot_free); }
};
static bool none_until(const Choice& c, long us) { return c.queue == -1 && c.timed && c.wake == at(us); }
static bool none_signal(const Choice& c) { return c.queue == -1 && !c.timed; }

static void arrivals() {
    QueuePolicy p;
    CHECK(!p.seen_arrival && p.gap_ewma_us == 0.0);
    p.on_arrival(at(0));                                  // the first arrival seeds 0
    CHECK(p.seen_arrival && p.gap_ewma_us == 0.0 && p.last_arrival == at(0));
    p.on_arrival(at(400));                                // 0.75 * 0 + 0.25 * 400
    CHECK(p.gap_ewma_us == 100.0);
    p.on_arrival(at(600));                                // 75 + 50
    CHECK(p.gap_ewma_us == 125.0);
    p.on_arrival(at(600 + 1000000));                      // a second's gap enters as 1e5 us: 93.75 + 25000
    CHECK(p.gap_ewma_us == 25093.75);
    p.on_arrival(at(500));                                // a negative gap enters as 0 — and is the last arrival all the same
    CHECK(p.gap_ewma_us == 18820.3125 && p.last_arrival == at(500));
    p.on_arrival(at(900));                                // 14115.234375 + 100
    CHECK(p.gap_ewma_us == 14215.234375);
    // the wait: none above max_wait_us, max_wait_us at it and below
    CHECK(p.wait_us(kWait) == 0);
    p.gap_ewma_us = 100.0;
    CHECK(p.wait_us(kWait) == kWait);
    p.gap_ewma_us = 100.0000001;
    CHECK(p.wait_us(kWait) == 0);
}

static void lone_caller() {
    World w;
    w.put(RECALL, 1, 1000);
    w.p[RECALL].gap_ewma_us = 150.0;                      // company is unlikely: at once
    CHECK(w.go(true, 1000).queue == RECALL);
    w.p[RECALL].gap_ewma_us = 50.0;                       // company is likely: max_wait_us
    CHECK(none_until(w.go(true, 1000), 1100));
    CHECK(none_until(w.go(true, 1099), 1100));
    CHECK(w.go(true, 1100).queue == RECALL);
    World empty;                                          // nothing waits: a signal
    CHECK(none_signal(empty.go(true, 1000)));
}

static void busy_and_idle() {
    World w;
    w.put(RECALL, 4, 1000, true);                         // full: ready while the device is busy
    CHECK(w.go(false, 1000).queue == RECALL);
    w.put(RECALL, 3, 1000, false);                        // partial: not while busy, however long it has waited — and no timer helps
    CHECK(none_signal(w.go(false, 5000)));
    CHECK(w.go(true, 5000).queue == RECALL);              // only when idle
    for (int f : {RANK, DPP}) {                           // per-item queues: a partial batch goes at its deadline while busy
        World v;
        v.put(f, 2, 1000);
        CHECK(none_until(v.go(false, 1050), 1100));
        CHECK(v.go(false, 1100).queue == f);
    }
}

static void oldest_head_wins() {
    World w;
    w.put(RECALL, 1, 300);
    w.put(RECOMMEND, 1, 100);
    w.put(RANK, 1, 200);
    CHECK(w.go(true, 1000).queue == RECOMMEND);
    w.put(RECOMMEND, 1, 950);                             // (not ready yet: deadline 1050)
    CHECK(w.go(true, 1000).queue == RANK);
    w.put(RECALL, 4, 990, true);                          // a full queue with a younger head does not overtake a ready older one
    CHECK(w.go(true, 1000).queue == RANK);
    w.put(RANK, 0, 0);
    CHECK(w.go(true, 1000).queue == RECALL);
    w.put(RECOMMEND, 4, 990, true);                       // equal heads: the first queue stays
    CHECK(w.go(true, 1000).queue == RECALL);
}

static void wake_time() {
    World w;
    w.put(RECALL, 1, 100);                                // deadline 200 — not eligible while busy
    w.put(RANK, 1, 320);                                  // 420
    w.put(DPP, 1, 300);                                   // 400
    CHECK(none_until(w.go(false, 250), 400));
    CHECK(none_until(w.go(true, 150), 200));              // idle: the recall's deadline counts, and is the earliest
    // no slot free: a signal, whatever is ready or due
    CHECK(none_signal(w.go(true, 150, false)));
    CHECK(none_signal(w.go(true, 1000, false)));
    w.put(RECALL, 4, 100, true);
    CHECK(none_signal(w.go(false, 150, false)));
}

static void rejoin_hold() {
    World w;
    QueuePolicy& p = w.p[RECALL];
    CHECK(p.rejoin_score == 1.0);                         // optimistic
    p.on_completion(at(1000), 32, 5, 2.0);                // 32 answered, 5 waiting: back at 37, window 50 + 2 * 32
    CHECK(p.rejoin_n == 32 && p.rejoin_target == 37 && p.rejoin_until == at(1114));
    w.put(RECALL, 36, 0);                                 // (head's own deadline long past)
    CHECK(none_until(w.go(true, 1010), 1114));            // not before the window closes
    CHECK(none_until(w.go(true, 1113), 1114));
    CHECK(w.go(true, 1114).queue == RECALL);              // closed
    w.put(RECALL, 37, 1005);                              // target reached: at once, whatever the head's deadline (1105)
    CHECK(w.go(true, 1010).queue == RECALL);
    w.put(RECALL, 1, 1100);                               // a head whose deadline lies behind the window keeps it
    CHECK(none_until(w.go(true, 1110), 1200));
    CHECK(none_until(w.go(true, 1150), 1200));
    // the hold does not make a busy device's partial recall batch ready
    w.put(RECALL, 37, 1005);
    CHECK(none_signal(w.go(false, 1010)));
    QueuePolicy v;                                        // the window is 50 + us_per_caller * n, truncated
    v.on_completion(at(0), 3, 0, 2.5);
    CHECK(v.rejoin_until == at(57) && v.rejoin_target == 3);
}

static void rejoin_score() {
    QueuePolicy p;
    p.on_dispatch(100);                                   // no hold to score
    CHECK(p.rejoin_score == 1.0 && p.rejoin_n == 0);
    p.on_completion(at(1000), 32, 5, 2.0);
    p.on_dispatch(5);                                     // nobody came back
    CHECK(near(p.rejoin_score, 0.8) && p.rejoin_n == 0 && p.rejoin_until == Time());
    p.on_completion(at(2000), 32, 5, 2.0);
    p.on_dispatch(3);                                     // (fewer than waited then: still nobody)
    CHECK(near(p.rejoin_score, 0.8 * 0.8));
    p.on_completion(at(3000), 32, 5, 2.0);
    p.on_dispatch(5 + 16);                                // half of them
    CHECK(near(p.rejoin_score, 0.8 * (0.8 * 0.8) + 0.2 * 0.5));
    const double s = p.rejoin_score;
    p.on_completion(at(4000), 32, 5, 2.0);
    p.on_dispatch(37);                                    // all of them
    CHECK(near(p.rejoin_score, 0.8 * s + 0.2));
    p.on_completion(at(5000), 32, 5, 2.0);
    p.on_dispatch(64);                                    // more than all counts as all
    CHECK(near(p.rejoin_score, 0.8 * (0.8 * s + 0.2) + 0.2));
}

static void probe() {
    QueuePolicy p;
    p.rejoin_score = 0.5;                                 // at one half the hold is still on
    p.on_completion(at(0), 4, 0, 2.0);
    CHECK(p.rejoin_n == 4 && p.rejoin_probe == 0);
    p = QueuePolicy();
    p.rejoin_score = 0.4;                                 // below: off, tried again at every sixteenth completion
    for (int i = 1; i <= 15; ++i) {
        p.on_completion(at(100 * i), 4, 0, 2.0);
        CHECK(p.rejoin_n == 0 && p.rejoin_until == Time() && p.rejoin_probe == (uint32_t)i);
    }
    p.on_completion(at(1600), 4, 2, 2.0);
    CHECK(p.rejoin_n == 4 && p.rejoin_target == 6 && p.rejoin_until == at(1658) && p.rejoin_probe == 16);
    p.on_dispatch(2);                                     // nobody: 0.32
    CHECK(near(p.rejoin_score, 0.32) && p.rejoin_n == 0);
    for (int i = 17; i <= 31; ++i) {
        p.on_completion(at(100 * i), 4, 0, 2.0);
        CHECK(p.rejoin_n == 0);
    }
    p.on_completion(at(3200), 4, 0, 2.0);
    CHECK(p.rejoin_n == 4 && p.rejoin_probe == 32);
}

static void full_rules() {
    CHECK(!recall_queue_full(3, 4) && recall_queue_full(4, 4) && recall_queue_full(5, 4) && recall_queue_full(1, 1));
    // rank: max_rank_reqs requests, or max_batch * k candidates
    CHECK(!rank_queue_full(16383, 31, 16384, 4, 8));
    CHECK(rank_queue_full(16384, 0, 16384, 4, 8));
    CHECK(rank_queue_full(1, 32, 16384, 4, 8));
    CHECK(!rank_queue_full(1, 0xFFFFFFFFull, 16384, 65536, 65536));      // (the product is taken in 64 bits)
    // dpp: item_cap / n, 2^27 / n^2, max_requests — whichever is smallest, and at least 1
    CHECK(dpp_batch_limit(131072, 1, 256) == 256);        // n = 1: the cap on requests
    CHECK(dpp_batch_limit(131072, 512, 256) == 256);      // 256 = item_cap / n, 512 from n^2
    CHECK(dpp_batch_limit(131072, 600, 256) == 218);      // item_cap / n binds (n^2: 372)
    CHECK(dpp_batch_limit(131072, 1024, 256) == 128);     // both 128
    CHECK(dpp_batch_limit(1u << 20, 2048, 256) == 32);    // n^2 binds (item_cap / n: 512)
    CHECK(dpp_batch_limit(131072, 20000, 256) == 1);      // n^2 gives 0: one request all the same
    CHECK(dpp_batch_limit(131072, 1, 8) == 8);
    CHECK(!dpp_queue_full(127, 131072, 1024, 256) && dpp_queue_full(128, 131072, 1024, 256));
    CHECK(!dpp_queue_full(255, 131072, 1, 256) && dpp_queue_full(256, 131072, 1, 256));
}

int main() {
    arrivals();
    lone_caller();
    busy_and_idle();
    oldest_head_wins();
    wake_time();
    rejoin_hold();
    rejoin_score();
    probe();
    full_rules();
    if (g_failed) {
        std::printf("coalescer_policy: %d check(s) failed\n", g_failed);
        return 1;
    }
    std::printf("coalescer_policy OK\n");
    return 0;
}
