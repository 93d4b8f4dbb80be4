// coalescer_policy.hpp — when the request coalescer (coalescer.hip) closes a batch.  No HIP, no threads, no clock reads: time
// comes in as an argument, so every rule can be checked with hand-made time points (tests/coalescer_policy_check.cpp).
//
// Invariant: a QueuePolicy is read and written only under pg_coalescer::mu.
//
// The rules, once:
// * Arrivals.  Every queue keeps an EWMA of its inter-arrival gap: the first arrival seeds 0 (nothing is known yet: it waits),
//   every later gap is clamped to [0, 1e5] us and enters as ewma = 0.75 ewma + 0.25 gap.  A request that arrives at an idle
//   device only waits for company when company is likely: its batch's deadline is the head's arrival + max_wait_us while the
//   EWMA is at most max_wait_us, and the head's arrival itself (a lone caller is dispatched at once) above it.
// * Full.  A recall-based queue (recall, recommend, and the L2 / exclusion recalls) is full at its batch limit; a rank queue
//   at max_rank_reqs requests or max_batch * k candidates; the DPP / SSD queue at dpp_batch_limit of its head's shape.
// * Ready.  A full batch is ready.  A partial one is ready at its deadline — for the recall-based queues only while nothing
//   is in flight (a table pass costs the same for 1 query as for 256: dispatching early could not start it any sooner), for the
//   per-item queues (rank, DPP: a launch costs what its items cost) also while the device is busy.  Among ready queues the one
//   with the oldest head goes; it goes when a slot is free.
// * Waking.  With a slot free and nothing ready the dispatcher sleeps until the earliest deadline that time alone will make
//   ready; otherwise (no slot free, or nothing that time will change) it waits for a signal.
// * Rejoin hold (recall-based queues).  Callers are closed loops (a goroutine blocked in Recall.GetCandidateItems /
//   IAlgorithm.Run issues its next request when this one returns), so the n callers of a batch that just completed are back
//   within some tens of microseconds — and a partial batch dispatched the moment the device falls idle splits them from the
//   requests that waited meanwhile into two cohorts that alternate for ever (32 callers: two batches of ~16, every request
//   waits for the other cohort's pass: p50 3.2 ms where one batch of 32 takes 1.8).  When a batch of n completes and leaves
//   the device idle, the waiting partial batch is therefore held until those n are back (queue length >= the length then + n:
//   it goes at once), at most for the window of 50 + us_per_caller * n microseconds (not before the window closes otherwise).
//   The score tracks how many came back in time (open-loop arrivals do not): at dispatch, with f the fraction of the n that
//   are in the queue, score = 0.8 score + 0.2 f, and the hold is cleared.  It starts at 1 (optimistic); below 0.5 the hold is
//   off, and tried again at every sixteenth completion.
#pragma once

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdint>

namespace pg {
namespace policy {

using Time = std::chrono::steady_clock::time_point;

struct QueuePolicy {
    Time last_arrival;
    double gap_ewma_us = 0.0;
    bool seen_arrival = false;
    Time rejoin_until;               // the hold's window closes (epoch: no hold)
    size_t rejoin_target = 0;        // queue length at which everyone the last batch answered is back
    uint32_t rejoin_n = 0;           // callers of that batch (0: no hold to score)
    double rejoin_score = 1.0;       // (optimistic: callers are closed loops until they show otherwise)
    uint32_t rejoin_probe = 0;       // completions seen with the hold off

    void on_arrival(Time t) {
        if (seen_arrival) {
            double gap = std::chrono::duration<double, std::micro>(t - last_arrival).count();
            gap = gap < 0.0 ? 0.0 : (gap > 1e5 ? 1e5 : gap);
            gap_ewma_us = 0.75 * gap_ewma_us + 0.25 * gap;
        } else {
            seen_arrival = true;
            gap_ewma_us = 0.0;
        }
        last_arrival = t;
    }

    // how long a partial batch's head waits for company
    uint32_t wait_us(uint32_t max_wait_us) const { return gap_ewma_us > (double)max_wait_us ? 0u : max_wait_us; }

    // a batch is taken from the queue, which holds `have` requests: how much of the last batch's callers made it into this one
    void on_dispatch(size_t have) {
        if (!rejoin_n) return;
        const size_t base = rejoin_target - rejoin_n;
        const double frac = have <= base ? 0.0 : (have - base >= rejoin_n ? 1.0 : (double)(have - base) / rejoin_n);
        rejoin_score = 0.8 * rejoin_score + 0.2 * frac;
        rejoin_n = 0;
        rejoin_until = Time();
    }

    // a batch of n_req requests of this queue completed and left the device idle; `waiting` requests are in the queue
    void on_completion(Time now, uint32_t n_req, size_t waiting, double us_per_caller) {
        const bool on = rejoin_score >= 0.5 || (++rejoin_probe & 15u) == 0;
        if (!on) return;
        rejoin_n = n_req;
        rejoin_target = waiting + n_req;
        rejoin_until = now + std::chrono::microseconds(50 + (int)(us_per_caller * n_req));
    }
};

// ---- the "full" rules ----
inline bool recall_queue_full(size_t reqs, uint32_t batch_limit) { return reqs >= batch_limit; }
inline bool rank_queue_full(size_t reqs, uint64_t items, uint32_t max_rank_reqs, uint32_t max_batch, uint32_t k) {
    return reqs >= max_rank_reqs || items >= (uint64_t)max_batch * k;
}
// how many DPP requests of `n` candidates one batch takes: bounded by the staging buffers (item_cap candidates), by the kernel
// matrices (n^2 doubles per request in the context's scratch: at most 1 GiB of them per batch) and by max_requests
inline uint32_t dpp_batch_limit(uint32_t item_cap, uint32_t n, uint32_t max_requests) {
    uint64_t b = item_cap / std::max(n, 1u);
    b = std::min<uint64_t>(b, (1ull << 27) / ((uint64_t)n * n));
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(b, max_requests));
}
inline bool dpp_queue_full(size_t reqs, uint32_t item_cap, uint32_t head_n, uint32_t max_requests) {
    return reqs >= dpp_batch_limit(item_cap, head_n, max_requests);
}

// ---- the dispatcher's choice ----
struct QueueView {
    size_t len = 0;                  // requests waiting (0: the queue takes no part)
    Time head_arrived;               // arrival of the oldest
    bool full = false;
    bool per_item = false;           // rank / DPP: a partial batch goes out at its deadline while the device is busy
};

struct Choice {
    int queue = -1;                  // the queue to dispatch now (-1: none)
    bool timed = false;              // none: wake at `wake`; false: wait for a signal
    Time wake;
};

inline Choice choose(const QueueView* q, const QueuePolicy* p, int n_queues, bool idle, Time now, uint32_t max_wait_us, bool slot_free) {
    int kind = -1;
    bool any = false;
    Time earliest = Time::max();
    for (int f = 0; f < n_queues; ++f) {
        if (q[f].len == 0) continue;
        any = true;
        Time deadline = q[f].head_arrived + std::chrono::microseconds(p[f].wait_us(max_wait_us));
        // (rejoin hold: everyone the last batch answered is back -> go at once; else not before the window closes)
        const bool holding = now < p[f].rejoin_until;
        const bool rejoined = holding && q[f].len >= p[f].rejoin_target;
        if (rejoined) deadline = now;
        else if (holding && p[f].rejoin_until > deadline) deadline = p[f].rejoin_until;
        const bool timely = idle || q[f].per_item;
        if (timely && deadline < earliest) earliest = deadline;      // (a deadline that time alone will make ready)
        if ((q[f].full || (timely && now >= deadline)) && (kind < 0 || q[f].head_arrived < q[kind].head_arrived)) kind = f;
    }
    Choice c;
    if (kind >= 0 && slot_free) {
        c.queue = kind;
    } else if (any && kind < 0 && slot_free && earliest != Time::max()) {
        // nothing ready: an idle device (or a per-item queue) additionally wakes at the oldest request's deadline
        c.timed = true;
        c.wake = earliest;
    }
    return c;
}

}  // namespace policy
}  // namespace pg
