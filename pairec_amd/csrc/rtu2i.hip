// rtu2i.hip — RealTimeU2IRecall's trigger stage: a compiled UserTriggerDaoConf and the kernel that turns each
// request's latest behaviour events into weighted trigger items.
//
// RealtimeUser2ItemHologresDao.GetTriggerInfos (module/realtime_user2item_hologres_dao.go:213-333) reads the user's last `Limit`
// events, drops an event whose play time does not exceed its event's threshold, weighs the rest with
// EventWeight[event] * WeightExpression(currentTime, eventTime), combines the weights per item (sum, or max), sorts descending
// and keeps TriggerCount items; ListItemsByUser (:98-211) expands them through the item-to-item table (cf.hip: pg_rtu2i_expand).
// The config strings are parsed as NewRealtimeUser2ItemBaseDao does (module/realtime_user2item_dao.go:96-120), the expression by
// expr.hip's govaluate front end with the DAO's own function table (exp alone).
//
// One workgroup of 1024 threads per request, one lane per event.  Items are keyed in an LDS open-addressed table (cf.hip's
// hash); the table tells every event whether its item has other events.  Only those lanes look for the item's NEXT event, and
// the lane of an item's first event walks that chain: the combination follows event order whatever the lane and hash order,
// with plain fp64 operations of one lane.  The order of the at most 1024 distinct items is one bitonic network in LDS over
// (order-mapped weight bits, first index).
#include "cf_shared.hpp"
#include "cond_eval.hpp"
#include "expr_prog.hpp"

#include <cerrno>
#include <cmath>
#include <unordered_map>

namespace pg {
namespace {

constexpr uint32_t kRtThreads = 1024;            // = the most events of one request: one lane per event
constexpr uint32_t kRtMaxEvents = 1024;
constexpr uint32_t kRtSlots = 2048;              // load factor <= 0.5
constexpr uint32_t kRtMaxOps = 64, kRtMaxDepth = 8;
constexpr uint32_t kRtMaxEventNames = 65536;     // event codes are uint16
constexpr uint32_t kRtNone = 0xFFFFFFFFu;
constexpr uint32_t kVarNow = 0, kVarEvent = 1;   // Instr.arg of currentTime / eventTime

}  // namespace

struct RtProg {
    Instr prog[kRtMaxOps];
    uint32_t n;
    uint32_t pad;
};

}  // namespace pg

struct pg_rtu2i {
    std::string source;
    pg::RtProg prog;
    std::vector<double> tab;                      // [n_events][2]: the event's weight (1 where it has none), its play-time threshold (NaN where it has none: no play time is <= NaN)
    uint32_t n_events = 0;
    bool max_mode = false;
    uint32_t T = 0;                               // the effective trigger count
    pg::SetTable table;                           // tab on the device
};

namespace pg {
namespace {

// the weight expression on one event; the stack's top is st[0] (cond.hip's discipline: the values stay in registers)
__host__ __device__ __forceinline__ double rt_eval(const RtProg& p, double now, double et) {
    double st[kRtMaxDepth];
#pragma unroll
    for (uint32_t j = 0; j < kRtMaxDepth; ++j) st[j] = 0.0;
    for (uint32_t pc = 0; pc < p.n; ++pc) {
        const Instr in = p.prog[pc];
        if (in.op == OP_CONST || in.op == OP_VAR) {
            const double v = in.op == OP_CONST ? in.val : in.arg == kVarNow ? now : et;
#pragma unroll
            for (uint32_t j = kRtMaxDepth - 1; j > 0; --j) st[j] = st[j - 1];
            st[0] = v;
        } else if (in.op == OP_NEG) {
            st[0] = -st[0];
        } else if (in.op == OP_EXP) {
            st[0] = go_exp(st[0]);
        } else {
            double v;
            expr_binop(in.op, st[1], st[0], &v);            // (the govaluate front end emits no operator that panics)
            st[0] = v;
#pragma unroll
            for (uint32_t j = 1; j + 1 < kRtMaxDepth; ++j) st[j] = st[j + 1];
        }
    }
    return st[0];
}

// one event: false = dropped (an item the engine does not hold; a play time at or under its event's threshold)
__host__ __device__ __forceinline__ bool rt_event(const RtProg& p, const double* tab, uint32_t n_events, uint32_t rows, uint32_t row, uint32_t code,
                                                  double play_time, long long now, long long et, double* weight) {
    if (row >= rows) return false;
    double w = 1.0;
    if (code < n_events) {
        if (play_time <= tab[2 * code + 1]) return false;
        w = tab[2 * code];
    }
    *weight = w * rt_eval(p, (double)now, (double)et);
    return true;
}

// sort records as cf.hip's: ascending (x, y) is weight descending (-0.0 ranks as 0.0), then first index ascending
__host__ __device__ __forceinline__ void rt_record(double w, uint32_t first, uint32_t row, unsigned long long* x, unsigned long long* y) {
    unsigned long long b;
    memcpy(&b, &w, 8);
    const unsigned long long negzero = b == 0x8000000000000000ull ? 1ull : 0ull;
    if (negzero) b = 0;
    const unsigned long long asc = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
    *x = ~asc;
    *y = ((unsigned long long)first << 33) | ((unsigned long long)row << 1) | negzero;
}
__host__ __device__ __forceinline__ void rt_unrecord(unsigned long long x, unsigned long long y, uint32_t* row, double* w) {
    const unsigned long long asc = ~x;
    unsigned long long b = (asc >> 63) ? (asc & 0x7FFFFFFFFFFFFFFFull) : ~asc;
    if (y & 1ull) b = 0x8000000000000000ull;
    memcpy(w, &b, 8);
    *row = (uint32_t)(y >> 1);
}
__host__ __device__ __forceinline__ bool rt_finite(double w) { return w == w && fabs(w) != __builtin_inf(); }

struct RtArgs {
    RtProg p;
    const double* tab;
    uint32_t n_events, rows, max_mode, T;
    const uint32_t* ev_rows;
    const uint16_t* ev_code;
    const double* ev_pt;           // NULL: every play time is 0
    const long long* ev_time;
    const uint32_t* ev_off;        // [nq + 1]
    const long long* now;          // [nq]
    uint32_t* out_rows;            // [nq][T]
    double* out_weight;
    uint32_t* out_count;           // [nq]
};

// Request q = blockIdx.x, event e0 + tid on lane tid.
__global__ __launch_bounds__(kRtThreads) void rt_trigger_kernel(RtArgs a) {
    __shared__ uint32_t keys[kRtSlots];           // the item's row
    __shared__ uint32_t first[kRtSlots];          // its first surviving event
    __shared__ uint32_t cnt[kRtSlots];            // its surviving events
    __shared__ uint32_t ev_slot[kRtMaxEvents];    // the event's item (kRtNone: dropped)
    __shared__ uint32_t ev_next[kRtMaxEvents];    // the item's next event (kRtNone: the last)
    __shared__ double ev_w[kRtMaxEvents];
    __shared__ ulonglong2 rec[kRtMaxEvents];
    __shared__ uint32_t n_valid;
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const uint32_t e0 = a.ev_off[q];
    const uint32_t n = min(a.ev_off[q + 1] - e0, kRtMaxEvents);
    if (n == 0) {                                 // (uniform: no barrier is skipped by a part of the workgroup)
        if (tid == 0) a.out_count[q] = 0;
        if (tid < a.T) {
            a.out_rows[(size_t)q * a.T + tid] = kRtNone;
            a.out_weight[(size_t)q * a.T + tid] = -__builtin_inf();
        }
        return;
    }
    for (uint32_t i = tid; i < kRtSlots; i += kRtThreads) {
        keys[i] = kCfEmpty;
        first[i] = kRtNone;
        cnt[i] = 0;
    }
    if (tid == 0) n_valid = 0;
    bool live = false;
    double w = 0.0;
    uint32_t row = kRtNone;
    if (tid < n) {
        row = a.ev_rows[e0 + tid];
        const uint32_t code = a.ev_code[e0 + tid];
        const double pt = a.ev_pt ? a.ev_pt[e0 + tid] : 0.0;
        live = rt_event(a.p, a.tab, a.n_events, a.rows, row, code, pt, a.now[q], a.ev_time[e0 + tid], &w);
    }
    __syncthreads();
    uint32_t h = kRtNone;
    if (live) {
        for (h = cf_slot(row, kRtSlots);; h = h + 1 == kRtSlots ? 0 : h + 1) {
            uint32_t cur = __hip_atomic_load(&keys[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            if (cur == kCfEmpty) {
                cur = atomicCAS(&keys[h], kCfEmpty, row);
                if (cur == kCfEmpty) break;
            }
            if (cur == row) break;
        }
        atomicAdd(&cnt[h], 1u);
        atomicMin(&first[h], tid);
    }
    ev_slot[tid] = h;
    ev_w[tid] = w;
    __syncthreads();
    // an event whose item has others finds the next one behind it
    uint32_t nx = kRtNone;
    if (live && cnt[h] > 1)
        for (uint32_t j = tid + 1; j < n; ++j)
            if (ev_slot[j] == h) {
                nx = j;
                break;
            }
    ev_next[tid] = nx;
    __syncthreads();
    // the lane of an item's first event combines the item's weights in event order
    ulonglong2 r = make_ulonglong2(~0ull, ~0ull);
    if (live && first[h] == tid) {
        double acc = w;
        for (uint32_t j = nx; j != kRtNone; j = ev_next[j]) {
            const double x = ev_w[j];
            if (!a.max_mode) acc = acc + x;
            else if (x > acc) acc = x;
        }
        if (rt_finite(acc)) {
            unsigned long long x, y;
            rt_record(acc, tid, row, &x, &y);
            r = make_ulonglong2(x, y);
            atomicAdd(&n_valid, 1u);
        }
    }
    rec[tid] = r;
    uint32_t np2 = 1;
    while (np2 < n) np2 <<= 1;
    __syncthreads();
    for (uint32_t k = 2; k <= np2; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            if (tid < (np2 >> 1)) {
                const uint32_t i = ((tid & ~(j - 1)) << 1) | (tid & (j - 1)), l = i | j;
                const bool up = (i & k) == 0;
                const ulonglong2 x = rec[i], y = rec[l];
                const bool less = y.x < x.x || (y.x == x.x && y.y < x.y);
                if (less == up) {
                    rec[i] = y;
                    rec[l] = x;
                }
            }
            __syncthreads();
        }
    }
    const uint32_t kept = min(n_valid, a.T);
    if (tid < a.T) {
        uint32_t orow = kRtNone;
        double ow = -__builtin_inf();
        if (tid < kept) rt_unrecord(rec[tid].x, rec[tid].y, &orow, &ow);
        a.out_rows[(size_t)q * a.T + tid] = orow;
        a.out_weight[(size_t)q * a.T + tid] = ow;
    }
    if (tid == 0) a.out_count[q] = kept;
}

// ---- the config strings (module/realtime_user2item_dao.go:96-120) ------------------------------------------------------------------
bool ieq(const std::string& a, const char* b) {
    if (a.size() != strlen(b)) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if ((a[i] | 0x20) != b[i]) return false;
    return true;
}
// strconv.ParseFloat(s, 64): 1 = a number, 0 = Go reports an error (the piece is skipped), -1 = a form Go reads that this front
// end does not (hexadecimal, digit-separating underscores)
int rt_parse_float(const std::string& t, double* v) {
    size_t i = 0;
    const size_t n = t.size();
    bool neg = false, sign = false;
    if (i < n && (t[i] == '+' || t[i] == '-')) {
        neg = t[i] == '-';
        sign = true;
        ++i;
    }
    const std::string rest = t.substr(i);
    if (ieq(rest, "inf") || ieq(rest, "infinity")) {
        *v = neg ? -__builtin_inf() : __builtin_inf();
        return 1;
    }
    if (!sign && ieq(rest, "nan")) {
        *v = __builtin_nan("");
        return 1;
    }
    if (t.find('_') != std::string::npos) return -1;
    if (rest.size() >= 2 && rest[0] == '0' && (rest[1] | 0x20) == 'x') return -1;
    size_t digits = 0;
    while (i < n && t[i] >= '0' && t[i] <= '9') { ++i; ++digits; }
    if (i < n && t[i] == '.') {
        ++i;
        while (i < n && t[i] >= '0' && t[i] <= '9') { ++i; ++digits; }
    }
    if (digits == 0) return 0;
    if (i < n && (t[i] | 0x20) == 'e') {
        ++i;
        if (i < n && (t[i] == '+' || t[i] == '-')) ++i;
        size_t ne = 0;
        while (i < n && t[i] >= '0' && t[i] <= '9') { ++i; ++ne; }
        if (ne == 0) return 0;
    }
    if (i != n) return 0;
    const double d = strtod(t.c_str(), nullptr);
    if (std::isinf(d)) return 0;                  // ErrRange
    *v = d;
    return 1;
}
std::vector<std::string> split(const std::string& s, char sep) {           // strings.Split: n separators, n + 1 parts
    std::vector<std::string> out;
    size_t b = 0;
    for (;;) {
        const size_t e = s.find(sep, b);
        out.push_back(s.substr(b, e == std::string::npos ? std::string::npos : e - b));
        if (e == std::string::npos) return out;
        b = e + 1;
    }
}
// the valid "name:number" pieces of `s` in order (a later piece of a name overwrites an earlier one: the reference's map)
int rt_parse_pairs(const char* field, const std::string& s, std::vector<std::pair<std::string, double>>* out) {
    for (const std::string& piece : split(s, ';')) {
        const std::vector<std::string> parts = split(piece, ':');
        if (parts.size() != 2) continue;
        double v;
        const int r = rt_parse_float(parts[1], &v);
        if (r < 0) {
            set_error("pg_rtu2i_compile: %s: the number \"%.60s\" (hexadecimal, or with '_' between digits) is read by strconv.ParseFloat "
                      "but not by this front end", field, parts[1].c_str());
            return PG_ERR_UNSUPPORTED;
        }
        if (r == 0) continue;
        out->emplace_back(parts[0], v);
    }
    return PG_OK;
}

// pg_rtu2i_triggers_host's body; what the kernel computes, one request after the other
void rt_triggers_host(const pg_rtu2i* c, uint32_t rows, const uint32_t* ev_rows, const uint16_t* ev_code, const double* ev_pt, const int64_t* ev_time,
                      const uint32_t* off, const int64_t* now, uint32_t nq, uint32_t* out_rows, double* out_w, uint32_t* out_count) {
    const uint32_t T = c->T;
    struct Item { uint32_t row, first; double w; };
    for (uint32_t q = 0; q < nq; ++q) {
        std::vector<Item> items;
        std::unordered_map<uint32_t, size_t> at;
        for (uint32_t e = off[q]; e < off[q + 1]; ++e) {
            double w;
            if (!rt_event(c->prog, c->tab.data(), c->n_events, rows, ev_rows[e], ev_code[e], ev_pt ? ev_pt[e] : 0.0, now[q], ev_time[e], &w)) continue;
            const auto it = at.find(ev_rows[e]);
            if (it == at.end()) {
                at.emplace(ev_rows[e], items.size());
                items.push_back({ev_rows[e], e - off[q], w});
            } else {
                double& acc = items[it->second].w;
                if (!c->max_mode) acc = acc + w;
                else if (w > acc) acc = w;
            }
        }
        std::vector<std::pair<unsigned long long, unsigned long long>> recs;
        for (const Item& it : items) {
            if (!rt_finite(it.w)) continue;
            unsigned long long x, y;
            rt_record(it.w, it.first, it.row, &x, &y);
            recs.emplace_back(x, y);
        }
        std::sort(recs.begin(), recs.end());
        const uint32_t kept = (uint32_t)std::min<size_t>(recs.size(), T);
        for (uint32_t j = 0; j < T; ++j) {
            uint32_t row = kRtNone;
            double w = -__builtin_inf();
            if (j < kept) rt_unrecord(recs[j].first, recs[j].second, &row, &w);
            out_rows[(size_t)q * T + j] = row;
            out_w[(size_t)q * T + j] = w;
        }
        out_count[q] = kept;
    }
}

}  // namespace

int rt_check(const char* who, const pg_rtu2i* c, uint64_t rows, const void* ev_rows, const void* ev_code, const void* ev_time,
             const uint32_t* ev_off, const int64_t* now, uint32_t nq) {
    PG_REQUIRE(c && ev_off && now, "%s: NULL argument", who);
    PG_REQUIRE(nq >= 1 && nq <= (uint32_t)kMaxQueries, "%s: nq=%u must be in [1,%d]", who, nq, kMaxQueries);
    PG_REQUIRE(rows >= 1 && rows <= 0xFFFFFFFFull, "%s: an item table of %llu rows (1 .. 2^32 - 1)", who, (unsigned long long)rows);
    for (uint32_t q = 0; q < nq; ++q) {
        PG_REQUIRE(ev_off[q + 1] >= ev_off[q], "%s: event_offsets[%u] = %u is below event_offsets[%u] = %u", who, q + 1, ev_off[q + 1], q, ev_off[q]);
        if (ev_off[q + 1] - ev_off[q] > kRtMaxEvents) {
            set_error("%s: request %u has %u events (at most %u per request: the reference's Limit cuts them)", who, q, ev_off[q + 1] - ev_off[q],
                      kRtMaxEvents);
            return PG_ERR_UNSUPPORTED;
        }
    }
    PG_REQUIRE((ev_rows && ev_code && ev_time) || ev_off[nq] == ev_off[0], "%s: NULL argument", who);
    return PG_OK;
}

int rt_triggers_enqueue_locked(const char* who, pg_ctx* ctx, pg_rtu2i* c, uint32_t rows, const uint32_t* d_ev_rows, const uint16_t* d_ev_code,
                               const double* d_ev_play_time, const int64_t* d_ev_time, const uint32_t* ev_off, const int64_t* now, uint32_t nq,
                               uint32_t* d_out_rows, double* d_out_weight, uint32_t* d_out_count, CfTrigDev* out) {
    int rc;
    const bool own = !d_out_rows;
    uint32_t* d_off; long long* d_now;
    if ((rc = scratch_carve(ctx, kSlotRtU2I, [&](Carve& cv) {
            d_off = cv.take<uint32_t>((size_t)nq + 1);
            d_now = cv.take<long long>(nq);
            if (own) {
                d_out_rows = cv.take<uint32_t>((size_t)nq * c->T);
                d_out_weight = cv.take<double>((size_t)nq * c->T);
                d_out_count = cv.take<uint32_t>(nq);
            }
        }))) return rc;
    if ((rc = c->table.ensure(ctx, who, {{c->tab.data(), c->tab.size() * 8}}))) return rc;
    PG_HIP(hipMemcpyAsync(d_off, ev_off, ((size_t)nq + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    PG_HIP(hipMemcpyAsync(d_now, now, (size_t)nq * 8, hipMemcpyHostToDevice, ctx->stream));
    RtArgs a;
    a.p = c->prog;
    a.tab = c->table.part<double>(0);
    a.n_events = c->n_events;
    a.rows = rows;
    a.max_mode = c->max_mode ? 1u : 0u;
    a.T = c->T;
    a.ev_rows = d_ev_rows;
    a.ev_code = d_ev_code;
    a.ev_pt = d_ev_play_time;
    a.ev_time = (const long long*)d_ev_time;
    a.ev_off = d_off;
    a.now = d_now;
    a.out_rows = d_out_rows;
    a.out_weight = d_out_weight;
    a.out_count = d_out_count;
    rt_trigger_kernel<<<nq, kRtThreads, 0, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    out->d_rows = d_out_rows;
    out->d_weight = d_out_weight;
    out->d_count = d_out_count;
    out->stride = c->T;
    return PG_OK;
}

}  // namespace pg

extern "C" {

int pg_rtu2i_compile(const pg_rtu2i_conf* conf, pg_rtu2i** out) {
    PG_REQUIRE(conf && out && conf->weight_expression, "pg_rtu2i_compile: NULL argument");
    PG_REQUIRE(conf->n_events == 0 || conf->event_names, "pg_rtu2i_compile: event_names is NULL");
    PG_REQUIRE(conf->n_events <= pg::kRtMaxEventNames, "pg_rtu2i_compile: %u event names (codes are uint16: at most %u)", conf->n_events,
               pg::kRtMaxEventNames);
    for (uint32_t i = 0; i < conf->n_events; ++i) PG_REQUIRE(conf->event_names[i], "pg_rtu2i_compile: event_names[%u] is NULL", i);
    const std::string mode = conf->weight_mode ? conf->weight_mode : "";
    PG_REQUIRE(mode.empty() || mode == "sum" || mode == "max",
               "pg_rtu2i_compile: weight_mode \"%.40s\" (\"sum\", \"max\" or \"\" = sum; the reference sums under any name but \"max\")", mode.c_str());
    const uint32_t T = conf->trigger_count ? conf->trigger_count : conf->limit;
    if (T < 1 || T > pg::kCfMaxTriggers) {
        pg::set_error("pg_rtu2i_compile: an effective trigger count of %u (trigger_count, or limit where that is 0) is unsupported (1..%u)", T,
                      pg::kCfMaxTriggers);
        return PG_ERR_UNSUPPORTED;
    }
    std::vector<std::pair<std::string, double>> weights, thresholds;
    int rc;
    const std::string ew = conf->event_weight ? conf->event_weight : "", ep = conf->event_play_time ? conf->event_play_time : "";
    if ((rc = pg::rt_parse_pairs("event_play_time", ep, &thresholds))) return rc;
    if ((rc = pg::rt_parse_pairs("event_weight", ew, &weights))) return rc;
    PG_REQUIRE(ew.empty() || !weights.empty(), "pg_rtu2i_compile: event_weight \"%.100s\" holds no valid name:number pair (the reference panics: "
               "\"UserTriggerDaoConf.EventWeight is empty\")", ew.c_str());
    PG_REQUIRE(conf->weight_expression[0], "pg_rtu2i_compile: weight_expression is empty (in the reference no evaluation yields a number: every "
               "weight would be 0)");
    pg_expr e;
    if ((rc = pg::gv_compile("pg_rtu2i_compile", conf->weight_expression, pg::kGvExp, &e))) return rc;
    if (e.prog.size() > pg::kRtMaxOps || (uint32_t)e.max_depth > pg::kRtMaxDepth) {
        pg::set_error("pg_rtu2i_compile: weight_expression too large (%zu operations, depth %d; at most %u, %u)", e.prog.size(), e.max_depth,
                      pg::kRtMaxOps, pg::kRtMaxDepth);
        return PG_ERR_UNSUPPORTED;
    }
    uint32_t var_of[pg::kMaxProg];
    for (size_t v = 0; v < e.vars.size(); ++v) {
        if (e.vars[v] == "currentTime") var_of[v] = pg::kVarNow;
        else if (e.vars[v] == "eventTime") var_of[v] = pg::kVarEvent;
        else {
            pg::set_error("pg_rtu2i_compile: variable \"%.100s\" of the weight_expression: the DAO binds only currentTime and eventTime (in the "
                          "reference every evaluation fails and every weight is 0)", e.vars[v].c_str());
            return PG_ERR_INVALID;
        }
    }
    pg_rtu2i* c = new pg_rtu2i();
    c->source = conf->weight_expression;
    memset(&c->prog, 0, sizeof c->prog);
    c->prog.n = (uint32_t)e.prog.size();
    for (size_t i = 0; i < e.prog.size(); ++i) {
        c->prog.prog[i] = e.prog[i];
        if (e.prog[i].op == pg::OP_VAR) c->prog.prog[i].arg = var_of[e.prog[i].arg];
    }
    c->n_events = conf->n_events;
    c->max_mode = mode == "max";
    c->T = T;
    c->tab.assign((size_t)conf->n_events * 2, 1.0);
    for (uint32_t i = 0; i < conf->n_events; ++i) c->tab[2 * (size_t)i + 1] = __builtin_nan("");
    // a name that is not in the dictionary can never match an event: ignored
    for (uint32_t i = 0; i < conf->n_events; ++i) {
        for (const auto& p : weights)
            if (p.first == conf->event_names[i]) c->tab[2 * (size_t)i] = p.second;
        for (const auto& p : thresholds)
            if (p.first == conf->event_names[i]) c->tab[2 * (size_t)i + 1] = p.second;
    }
    *out = c;
    return PG_OK;
}

int pg_rtu2i_free(pg_rtu2i* c) {
    if (!c) return PG_OK;
    c->table.release();
    delete c;
    return PG_OK;
}

int pg_rtu2i_trigger_count(const pg_rtu2i* c) { return c ? (int)c->T : 0; }

int pg_rtu2i_triggers_host(const pg_rtu2i* c, uint64_t rows, const uint32_t* event_rows, const uint16_t* event_code, const double* event_play_time,
                           const int64_t* event_time, const uint32_t* event_offsets, const int64_t* now, uint32_t nq, uint32_t* out_rows,
                           double* out_weight, uint32_t* out_count) {
    int rc;
    if ((rc = pg::rt_check("pg_rtu2i_triggers_host", c, rows, event_rows, event_code, event_time, event_offsets, now, nq))) return rc;
    PG_REQUIRE(out_rows && out_weight && out_count, "pg_rtu2i_triggers_host: NULL argument");
    pg::rt_triggers_host(c, (uint32_t)rows, event_rows, event_code, event_play_time, event_time, event_offsets, now, nq, out_rows, out_weight, out_count);
    return PG_OK;
}

int pg_rtu2i_triggers_dev(pg_ctx* ctx, pg_rtu2i* c, uint64_t rows, const uint32_t* d_event_rows, const uint16_t* d_event_code,
                          const double* d_event_play_time, const int64_t* d_event_time, const uint32_t* event_offsets, const int64_t* now,
                          uint32_t nq, uint32_t* d_out_rows, double* d_out_weight, uint32_t* d_out_count) {
    int rc;
    PG_REQUIRE(ctx, "pg_rtu2i_triggers_dev: NULL argument");
    if ((rc = pg::rt_check("pg_rtu2i_triggers_dev", c, rows, d_event_rows, d_event_code, d_event_time, event_offsets, now, nq))) return rc;
    PG_REQUIRE(d_out_rows && d_out_weight && d_out_count, "pg_rtu2i_triggers_dev: NULL argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    pg::CfTrigDev td;
    if ((rc = pg::rt_triggers_enqueue_locked("pg_rtu2i_triggers_dev", ctx, c, (uint32_t)rows, d_event_rows, d_event_code, d_event_play_time,
                                             d_event_time, event_offsets, now, nq, d_out_rows, d_out_weight, d_out_count, &td)))
        return rc;
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

int pg_rtu2i_triggers(pg_ctx* ctx, pg_rtu2i* c, uint64_t rows, const uint32_t* event_rows, const uint16_t* event_code, const double* event_play_time,
                      const int64_t* event_time, const uint32_t* event_offsets, const int64_t* now, uint32_t nq, uint32_t* out_rows,
                      double* out_weight, uint32_t* out_count) {
    int rc;
    PG_REQUIRE(ctx, "pg_rtu2i_triggers: NULL argument");
    if ((rc = pg::rt_check("pg_rtu2i_triggers", c, rows, event_rows, event_code, event_time, event_offsets, now, nq))) return rc;
    PG_REQUIRE(out_rows && out_weight && out_count, "pg_rtu2i_triggers: NULL argument");
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    const uint32_t total = event_offsets[nq] - event_offsets[0], T = c->T;
    uint32_t *d_er, *d_or, *d_oc; uint16_t* d_ec; double *d_ep, *d_ow; int64_t* d_et;
    if ((rc = pg::scratch_carve(ctx, pg::kSlotStaging, [&](pg::Carve& cv) {
            d_er = cv.take<uint32_t>(total);
            d_ec = cv.take<uint16_t>(total);
            d_ep = cv.take<double>(event_play_time ? total : 0);
            d_et = cv.take<int64_t>(total);
            d_or = cv.take<uint32_t>((size_t)nq * T);
            d_ow = cv.take<double>((size_t)nq * T);
            d_oc = cv.take<uint32_t>(nq);
        }))) return rc;
    uint32_t h_off[pg::kMaxQueries + 1];
    for (uint32_t q = 0; q <= nq; ++q) h_off[q] = event_offsets[q] - event_offsets[0];
    if (total) {
        PG_HIP(hipMemcpyAsync(d_er, event_rows + event_offsets[0], (size_t)total * 4, hipMemcpyHostToDevice, ctx->stream));
        PG_HIP(hipMemcpyAsync(d_ec, event_code + event_offsets[0], (size_t)total * 2, hipMemcpyHostToDevice, ctx->stream));
        if (event_play_time) PG_HIP(hipMemcpyAsync(d_ep, event_play_time + event_offsets[0], (size_t)total * 8, hipMemcpyHostToDevice, ctx->stream));
        PG_HIP(hipMemcpyAsync(d_et, event_time + event_offsets[0], (size_t)total * 8, hipMemcpyHostToDevice, ctx->stream));
    }
    pg::CfTrigDev td;
    if ((rc = pg::rt_triggers_enqueue_locked("pg_rtu2i_triggers", ctx, c, (uint32_t)rows, d_er, d_ec, event_play_time ? d_ep : nullptr, d_et, h_off, now,
                                             nq, d_or, d_ow, d_oc, &td)))
        return rc;
    PG_HIP(hipMemcpyAsync(out_rows, d_or, (size_t)nq * T * 4, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipMemcpyAsync(out_weight, d_ow, (size_t)nq * T * 8, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipMemcpyAsync(out_count, d_oc, (size_t)nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    PG_HIP(hipStreamSynchronize(ctx->stream));
    return PG_OK;
}

}  // extern "C"
