// traffic_host.hpp — what a TrafficControlSort macro-control answer IS (include/pairec_gpu.h "TrafficControlSort"),
// free of HIP: the four tables (built once, here and nowhere else, with the host's libm), goint and the wrapping int64 arithmetic
// behind it, the table look-ups, a target's per-request numbers, one entry's delta / control id / new position, and the host
// statement.  traffic.hip includes it for both sides: the kernels and pg_traffic_sort_host run the same functions on the same
// table values, so the two differ in nothing but who adds the chains.  The step numbers are the header's.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/pairec_gpu.h"

#ifdef __HIPCC__
#define PG_TRAFFIC_HD __host__ __device__ __forceinline__
#else
#define PG_TRAFFIC_HD inline
#endif

namespace pg {

constexpr uint32_t kTrafficMaxTargets = 8;
constexpr uint32_t kTrafficPosN = 500, kTrafficExpN = 1000, kTrafficTanhN = 3000, kTrafficSigN = 10000;
constexpr uint32_t kTrafficPosAt = 0, kTrafficExpAt = kTrafficPosAt + kTrafficPosN, kTrafficTanhAt = kTrafficExpAt + kTrafficExpN,
                   kTrafficSigAt = kTrafficTanhAt + kTrafficTanhN, kTrafficTableN = kTrafficSigAt + kTrafficSigN;
constexpr double kTrafficPosTail = 0.006737946999;                     // posWeight beyond 500 (:241)
constexpr double kTrafficE = 2.71828182845904523536028747135266249775724709369995957496696763;      // math.E
constexpr unsigned long long kTrafficNanBits = 0x7FF8000000000000ull;  // new_pos of an element that is no entry
static_assert(kTrafficMaxTargets == PG_TRAFFIC_MAX_TARGETS && kTrafficMaxTargets <= 8, "a member mask is one byte");

// 3. the tables, one array: positionWeight | expTable | tanhTable | sigmoidTable (:45-66)
inline const double* traffic_tables() {
    static const std::vector<double> tab = [] {
        std::vector<double> t(kTrafficTableN);
        for (uint32_t i = 0; i < kTrafficPosN; ++i) t[kTrafficPosAt + i] = std::exp(-0.01 * (double)i);
        for (uint32_t i = 0; i < kTrafficExpN; ++i) t[kTrafficExpAt + i] = std::exp((double)i / 1000.0);
        for (uint32_t i = 0; i < kTrafficTanhN; ++i) t[kTrafficTanhAt + i] = std::tanh((double)i / 1000.0);
        for (uint32_t i = 0; i < kTrafficSigN; ++i) {
            const double x = (double)i / 1000.0 + 5.0;
            t[kTrafficSigAt + i] = 1.0 / (1.0 + std::exp(10.0 - x));
        }
        return t;
    }();
    return tab.data();
}

// 2. Go's float64 -> int on amd64 (CVTTSD2SQ): no cast ever sees a value outside the range
PG_TRAFFIC_HD long long traffic_goint(double x) {
    return x > -9223372036854775808.0 && x < 9223372036854775808.0 ? (long long)x : (long long)(-9223372036854775807LL - 1);
}
PG_TRAFFIC_HD long long traffic_wrap_add(long long a, long long b) { return (long long)((unsigned long long)a + (unsigned long long)b); }
PG_TRAFFIC_HD double traffic_nan() {
    const unsigned long long b = kTrafficNanBits;
    double d;
    memcpy(&d, &b, 8);
    return d;
}
PG_TRAFFIC_HD double traffic_tanh_tab(const double* tab, double x) {                 // :942-950
    long long idx = traffic_goint(x * 1000.0);
    if (idx < 0) idx = 0;
    else if (idx >= (long long)kTrafficTanhN) idx = kTrafficTanhN - 1;
    return tab[kTrafficTanhAt + idx];
}
PG_TRAFFIC_HD double traffic_sigmoid_tab(const double* tab, double x, double rho) {  // :952-960
    long long idx = traffic_wrap_add(traffic_goint(rho * x * 1000.0), -5000);
    if (idx < 0) idx = 0;
    else if (idx >= (long long)kTrafficSigN) return 1.0;
    return tab[kTrafficSigAt + idx];
}
PG_TRAFFIC_HD double traffic_pos_weight(const double* tab, uint32_t i) { return i < kTrafficPosN ? tab[kTrafficPosAt + i] : kTrafficPosTail; }
// 4. s_i and itemScore_i
PG_TRAFFIC_HD double traffic_s(double score) { return score == 0.0 ? 1e-8 : score; }
PG_TRAFFIC_HD double traffic_item_score(const double* tab, uint32_t i, double s, double max_score) {
    if (i == 0) return kTrafficE;
    long long idx = traffic_goint(s / max_score * 1000.0);
    if (idx < 0) idx = 0;
    if (idx >= (long long)kTrafficExpN) idx = kTrafficExpN - 1;
    return tab[kTrafficExpAt + idx];
}

// a target's numbers for one request, behind the sums
struct TrafficTarget {
    double alpha;           // as step 5 left it
    double weight;          // weight_t
    double rho;             // the pull-down's rho (read when alpha < 0)
    long long start;        // the uplift's distinctStartPos
};
struct TrafficScalars {
    uint32_t ctx_size, page_no;
    double gamma, beta, eta;
};
// steps 4 (the division), 5 and the per-target part of 6; hit: the target received at least one addition
PG_TRAFFIC_HD TrafficTarget traffic_target(const double* tab, const TrafficScalars& sc, double alpha, double sum, double total, bool hit) {
    TrafficTarget t;
    t.weight = hit ? sum / total : 0.0;
    if (alpha > 0) {
        const double th = traffic_tanh_tab(tab, sc.beta * t.weight);
        const double g = sc.gamma * th;
        const double rho = 1.0 + g;
        alpha = alpha * rho;
    }
    t.alpha = alpha;
    const double one_minus = 1.0 - traffic_tanh_tab(tab, t.weight);
    t.rho = sc.eta * one_minus;
    t.start = (long long)sc.ctx_size;
    if (sc.page_no > 1) {
        const double multiple = (t.weight - 0.3) * 10.0;
        t.start = traffic_wrap_add(t.start, traffic_goint(multiple * (double)sc.ctx_size));
    }
    return t;
}
// steps 6 and 7 for entry i; types / ids: the compiled set's
PG_TRAFFIC_HD void traffic_entry(const double* tab, const TrafficTarget* tg, const int32_t* control_type, const int32_t* target_id, uint32_t T,
                                 uint32_t i, double item_score, uint32_t member, int32_t* control_id, double* new_pos) {
    const int32_t origin = (int32_t)(i + 1);
    int32_t cid = origin;
    double fin = 0.0;
    for (uint32_t t = 0; t < T; ++t) {
        const double alpha = tg[t].alpha;
        if (!((member >> t) & 1u) || alpha == 0) continue;
        double delta;
        if (alpha < 0.0) {
            delta = alpha * traffic_sigmoid_tab(tab, (double)i, tg[t].rho);
        } else {
            delta = alpha * item_score;
            if ((long long)i > tg[t].start && delta >= 1.0) {
                if (control_type[t] == PG_TRAFFIC_PERCENT) cid = -target_id[t];
                else if (cid > 0) cid = 0;
            }
        }
        fin = fin + delta;
    }
    double pos = (double)origin;
    if (fin != 0.0) {
        if (cid == 0 && fin < 1.0) cid = origin;
        pos = (double)origin - fin;
        if (pos != pos) pos = traffic_nan();               // (7.: IEEE 754 leaves a NaN's sign and payload to the hardware; the answer does not)
    }
    *new_pos = pos;
    *control_id = cid;
}
// step 8's "a sorts before b" for list positions a < b or a > b
inline bool traffic_before(double pa, uint32_t a, double pb, uint32_t b) {
    const bool na = pa != pa, nb = pb != pb;
    if (na || nb) return na == nb ? a < b : nb;
    if (pa != pb) return pa < pb;
    return a < b;
}

// the host statement for one request: list entry j is element elem(j) of score / member / the two optional outputs (all of the
// request, `cap` elements); every element of out (cap), *out_count, control_id and new_pos (cap, where given) is written once
inline void traffic_host_request(const TrafficScalars& sc, const int32_t* control_type, const int32_t* target_id, uint32_t T, uint32_t n,
                                 uint32_t cap, const double* score, const uint8_t* member, const uint32_t* order, const double* alpha_in,
                                 uint32_t* out, uint32_t* out_count, int32_t* control_id, double* new_pos) {
    const double* tab = traffic_tables();
    auto elem = [&](uint32_t j) { return order ? order[j] : j; };
    double total = 0.0, sum[kTrafficMaxTargets] = {0}, max_score = 0.0;
    bool hit[kTrafficMaxTargets] = {false};
    for (uint32_t i = 0; i < n && T; ++i) {                              // (without targets nothing is read: score and member may be NULL)
        const double s = traffic_s(score[elem(i)]);
        if (i == 0) max_score = s;
        const double w = s * traffic_pos_weight(tab, i);
        total = total + w;
        for (uint32_t t = 0; t < T; ++t)
            if (alpha_in[t] != 0 && ((member[elem(i)] >> t) & 1u)) {
                sum[t] = sum[t] + w;
                hit[t] = true;
            }
    }
    TrafficTarget tg[kTrafficMaxTargets];
    for (uint32_t t = 0; t < T; ++t) tg[t] = traffic_target(tab, sc, alpha_in[t], sum[t], total, hit[t]);
    std::vector<double> pos(n);
    std::vector<uint32_t> idx(n);
    if (control_id) std::fill(control_id, control_id + cap, 0);
    if (new_pos) std::fill(new_pos, new_pos + cap, traffic_nan());
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t e = elem(i);
        int32_t cid = (int32_t)(i + 1);
        pos[i] = (double)(i + 1);
        if (T) traffic_entry(tab, tg, control_type, target_id, T, i, traffic_item_score(tab, i, traffic_s(score[e]), max_score), member[e], &cid, &pos[i]);
        if (control_id) control_id[e] = cid;
        if (new_pos) new_pos[e] = pos[i];
        idx[i] = i;
    }
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) { return traffic_before(pos[a], a, pos[b], b); });
    for (uint32_t k = 0; k < cap; ++k) out[k] = k < n ? elem(idx[k]) : 0xFFFFFFFFu;
    *out_count = n;
}

}  // namespace pg
