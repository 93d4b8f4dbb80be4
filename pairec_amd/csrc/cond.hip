// cond.hip — module.FilterParam as a compiled object with one device evaluator, and the two stages that are nothing but it
// (DESIGN.md 4.1p): ItemStateFilter (filter/item_state_filter.go:47-57, module/item_state_filter_hologres_dao.go:86-357: keep, in
// order, the candidates whose state columns pass one FilterParam) and BoostScoreSort (sort/boost_score_sort.go:73-104: the first
// BoostScoreCondition whose FilterParam matches rewrites Item.Score by a govaluate expression; with
// BoostScoreConditionsFilterAll every matching one does, in sequence).
//
// A FilterParam (module/filter_op.go:453-540) is a list of `name OP value` operators, all ANDed by EvaluateByDomain (:507-540).
// Here a rule is that list compiled against declared columns; the reference's "property missing from the map" branch is taken
// for a candidate whose row lies outside the feature store (item properties) and for a user slot whose presence bit is clear
// (user properties).  What every operator answers, transcribed operator by operator from the form EvaluateByDomain dispatches to
// (DomainEvaluate for all but is_null / is_not_null, which only have Evaluate):
//   left missing        not_equal → true (:231-234); is_null → true (:1588-1596); every other operator → false
//                       (:85-88, :356-359, :597-600, :771, :945, :1119, :1492-1495, :1621-1626)
//   type not listed     equal / not_equal with float → false (:167-169, :310-312); in / not_in with int64 or float → false
//                       (:420, :1562: their switches list "string" and "int" only); left present or not
//   `user.x` missing    equal → false (:98-101), not_equal → true (:244-247), the four ordered comparisons → false (:610-613 …)
//   `item.x` missing    equal → false (:106-109), not_equal → true (:252-255); ordered comparisons: true for float
//                       (:618-621, :792-795, :966-969, :1140-1143) and false for int / int64 (:643-646, :667-670 …).  With one
//                       store per rule set this is reached by user-domain terms only: an item-domain term of such a candidate
//                       has already answered for its missing left side.
//   values              int / int64 compare as int64 (utils.ToInt / ToInt64 of an integer column; Go's int is 64-bit); float
//                       compares float64(value) (utils.ToFloat); string compares dictionary ids the caller encoded
//   bool                one level (:1679-1756): Type "" / "or" → any child (no children: false), anything else → every child
//                       (no children: true); its own domain is always item (:1758-1760)
//   no operators        true (:539)
// in lists are sorted at compile time and searched.  Everything the evaluator does not state exactly is refused by name at
// compile (pg_cond_compile in include/pairec_gpu.h lists it).
//
// Kernels: one lane per candidate.  The lane loads its row, then every referenced column's value (raw bits, <= 16 loads issued
// before the first use), then walks the terms, which travel as a by-value kernel argument; in lists and expression programs lie
// in a small device table uploaded once per compiled set and are read with wave-uniform addresses.  The expression walk keeps
// an 8-deep stack in registers (constant indices only: the top is always slot 0).  The candidate's loads, the pick of a column's
// value and its reading as float64 are cond_eval.hpp's, shared with classcut.hip; the compiled object, its terms and rules
// (CondProgram, cond_term, cond_rule) and their bind to a store are stated there too, shared with mixsort.hip.
//   item_state_filter_kernel   one workgroup per request walks cap in chunks of 1 024 (block_rank.hpp's chunk_rank: one barrier
//                              per chunk); kept entries move to the front with everything carried.
//   boost_scores_kernel        256 lanes per workgroup, grid (cap / 256, nq).
//   distinct_ids_kernel        the same grid: DistinctIdSort (sort/distinct_id_sort.go:52-72) — the id of the
//                              first rule that matches, else the entry's position + 1.
#include "pipeline.hpp"
#include "cond_eval.hpp"
#include "block_rank.hpp"
#include "expr_prog.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstring>
#include <memory>

namespace pg {
namespace {

constexpr uint32_t kCondChunk = 1024, kCondWaves = kCondChunk / kWave;
constexpr uint32_t kVarScore = 0xFFFFu;           // Instr.arg of the variable `score`

// rule r's expression on the candidate (boost_score_sort.go:81-94): false = govaluate errors (a column of a candidate outside the
// store: "No parameter found"), the score stays.  The stack's top is st[0]; a push moves everything down one slot.
__host__ __device__ __forceinline__ bool cond_expr(const CondProgram& p, uint32_t r, const CondItem& it, double score, double* out) {
    double st[kCondMaxExprDepth];
#pragma unroll
    for (uint32_t j = 0; j < kCondMaxExprDepth; ++j) st[j] = 0.0;
    bool ok = true;
    const Instr* prog = p.progs + p.rules[r].prog_off;
    const uint32_t n = p.rules[r].prog_n;
    for (uint32_t pc = 0; pc < n; ++pc) {
        const Instr in = prog[pc];
        if (in.op == OP_CONST || in.op == OP_VAR) {
            double v = in.val;
            if (in.op == OP_VAR) {
                if (in.arg == kVarScore) v = score;
                else if (it.item_in) v = cond_col_f64(p, it, in.arg);
                else ok = false;
            }
#pragma unroll
            for (uint32_t j = kCondMaxExprDepth - 1; j > 0; --j) st[j] = st[j - 1];
            st[0] = v;
        } else if (in.op == OP_NEG) {
            st[0] = -st[0];
        } else if (in.op == OP_ROUND) {
            st[0] = round(st[0]);
        } else {
            double v;
            expr_binop(in.op, st[1], st[0], &v);            // (the govaluate front end emits no operator that panics)
            st[0] = v;
#pragma unroll
            for (uint32_t j = 1; j + 1 < kCondMaxExprDepth; ++j) st[j] = st[j + 1];
        }
    }
    *out = st[0];
    return ok;
}

// BoostScoreSort.doSort's inner loop for one item (:79-99): returns the last rule that matched (0xFF: none)
__host__ __device__ __forceinline__ uint32_t cond_boost(const CondProgram& p, bool filter_all, const CondItem& it, const CondUser& u, double* score) {
    uint32_t last = 0xFFu;
    for (uint32_t r = 0; r < p.n_rules; ++r) {
        if (!cond_rule(p, r, it, u)) continue;
        double v;
        if (cond_expr(p, r, it, *score, &v)) *score = v;
        last = r;
        if (!filter_all) break;                          // (outside the else: an expression that errors still ends the walk)
    }
    return last;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
struct FilterArgs {
    CandIn in;
    CandOut out;                                 // (out_cap = cap: the kept entries move to the front of their own list)
    const unsigned long long* user_vals;         // [nq][kCondMaxSlots] or NULL
    const uint32_t* user_present;                // [nq] or NULL
};

// Request q = blockIdx.x.
__global__ __launch_bounds__(kCondChunk) void item_state_filter_kernel(CondProgram p, FilterArgs a) {
    __shared__ uint32_t wcnt[2 * kCondWaves];
    const uint32_t q = blockIdx.x, tid = threadIdx.x;
    const size_t q0 = (size_t)q * a.in.cap;
    const uint32_t n_valid = cand_n_valid(a.in, q);
    CondUser u;
    u.vals = a.user_vals ? a.user_vals + (size_t)q * kCondMaxSlots : nullptr;
    u.present = a.user_present ? a.user_present[q] : 0u;
    uint32_t run = 0;                                                // the entries kept so far: every lane counts along
    for (uint32_t c0 = 0, it = 0; c0 < n_valid; c0 += kCondChunk, ++it) {
        const uint32_t pos = c0 + tid;
        bool keep = false;
        if (pos < n_valid) {
            const unsigned long long row = a.in.rows[q0 + pos];
            if (row != kCandPad) {
                CondItem item;
                cond_load(p, row, &item);
                keep = cond_rule(p, 0, item, u);
            }
        }
        uint32_t r, total;
        chunk_rank<kCondWaves>(keep, wcnt, it, &r, &total);
        if (keep) cand_carry(a.in, a.out, q0 + pos, q0 + run + r, true);                   // (run + r <= pos < cap)
        run += total;
    }
    cand_pad(a.in, a.out, q, run + tid, kCondChunk, kCandNan);          // padding behind the count
    if (tid == 0) a.out.count[q] = run;
}

constexpr uint32_t kBoostThreads = 256;
// Request q = blockIdx.y, positions blockIdx.x * 256 ...
__global__ __launch_bounds__(kBoostThreads) void boost_scores_kernel(CondProgram p, const uint64_t* __restrict__ rows,
                                                                     const unsigned long long* score, const uint32_t* __restrict__ count,
                                                                     const unsigned long long* __restrict__ user_vals,
                                                                     const uint32_t* __restrict__ user_present, uint32_t cap, uint32_t filter_all,
                                                                     unsigned long long* out_score, uint8_t* __restrict__ out_rule) {      // (out_score may be score: a lane reads its entry, then writes it)
    const uint32_t q = blockIdx.y, pos = blockIdx.x * kBoostThreads + threadIdx.x;
    if (pos >= cap) return;
    const size_t i = (size_t)q * cap + pos;
    const uint32_t n_valid = count ? min(count[q], cap) : cap;      // (a score rewrite in place: no lists move, no CandIn)
    unsigned long long bits = score[i];
    uint32_t last = 0xFFu;
    const unsigned long long row = rows[i];
    if (pos < n_valid && row != kCandPad) {
        CondUser u;
        u.vals = user_vals ? user_vals + (size_t)q * kCondMaxSlots : nullptr;
        u.present = user_present ? user_present[q] : 0u;
        CondItem item;
        cond_load(p, row, &item);
        double s = cand_bits_f64(bits);
        last = cond_boost(p, filter_all != 0, item, u, &s);
        memcpy(&bits, &s, 8);                                            // (moves only: an untouched score keeps its bits)
    }
    out_score[i] = bits;                                                 // padding entries keep their score bits
    if (out_rule) out_rule[i] = (uint8_t)last;
}

// DistinctIdSort.doSort's inner loop for one item at position pos (distinct_id_sort.go:57-67, every condition under one name):
// the id of the first rule that matches, else pos + 1 (an evaluation error is cond_rule's false, and :60's err != nil a non-match)
struct DistinctIds { long long id[kCondMaxRules]; };
__host__ __device__ __forceinline__ long long cond_distinct_id(const CondProgram& p, const DistinctIds& ids, const CondItem& it, const CondUser& u, uint32_t pos) {
    for (uint32_t r = 0; r < p.n_rules; ++r)
        if (cond_rule(p, r, it, u)) return ids.id[r];
    return (long long)pos + 1;
}

// Request q = blockIdx.y, positions blockIdx.x * 256 ...
__global__ __launch_bounds__(kBoostThreads) void distinct_ids_kernel(CondProgram p, DistinctIds ids, const uint64_t* __restrict__ rows,
                                                                     const uint32_t* __restrict__ count,
                                                                     const unsigned long long* __restrict__ user_vals,
                                                                     const uint32_t* __restrict__ user_present, uint32_t cap,
                                                                     long long* __restrict__ out_id) {
    const uint32_t q = blockIdx.y, pos = blockIdx.x * kBoostThreads + threadIdx.x;
    if (pos >= cap) return;
    const size_t i = (size_t)q * cap + pos;
    const uint32_t n_valid = count ? min(count[q], cap) : cap;
    const unsigned long long row = rows[i];
    long long id = 0;                                                    // padding entries get 0
    if (pos < n_valid && row != kCandPad) {
        CondUser u;
        u.vals = user_vals ? user_vals + (size_t)q * kCondMaxSlots : nullptr;
        u.present = user_present ? user_present[q] : 0u;
        CondItem item;
        cond_load(p, row, &item);
        id = cond_distinct_id(p, ids, item, u, pos);
    }
    out_id[i] = id;
}

}  // namespace
}  // namespace pg

namespace pg {
namespace {

const char* const kCondOpNames[] = {"equal", "not_equal", "greater", "greaterThan", "less", "lessThan", "in", "not_in",
                                    "is_null", "is_not_null", "bool", "contains", "not_contains", "expression"};

struct CondCompiler {
    pg_cond* c;
    const pg_cond_col* cols;
    uint32_t n_cols;
    int refuse(int code, const char* fmt, ...) __attribute__((format(printf, 3, 4))) {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        set_error("pg_cond_compile: %s", buf);
        return code;
    }
    // a column by name → its index among the referenced ones; need_int: the value is read as an integer
    int column(const char* name, bool need_int, uint32_t rule, const char* what, uint8_t* out) {
        uint32_t d = 0;
        for (; d < n_cols; ++d)
            if (!strcmp(cols[d].name, name)) break;
        if (d == n_cols) return refuse(PG_ERR_INVALID, "rule %u: %s \"%s\" is not among the declared columns", rule, what, name);
        if (need_int && cols[d].dtype != PG_F_I32 && cols[d].dtype != PG_F_I64)
            return refuse(PG_ERR_UNSUPPORTED, "rule %u: %s \"%s\" is a float column read by an int / int64 / string term (utils.ToInt has no "
                          "float32 case and truncates float64): not served", rule, what, name);
        size_t k = 0;
        for (; k < c->used.size(); ++k)
            if (c->used[k] == (int)d) break;
        if (k == c->used.size()) {
            if (k == kCondMaxCols) return refuse(PG_ERR_UNSUPPORTED, "more than %u referenced columns (\"%s\")", kCondMaxCols, name);
            c->used.push_back((int)d);
        }
        *out = (uint8_t)k;
        return PG_OK;
    }
    // kind: 0 read as an integer, 1 read as a float, 2 only its presence is read
    int slot(const char* name, uint8_t kind, uint32_t rule, uint8_t* out) {
        size_t k = 0;
        for (; k < c->slot_names.size(); ++k)
            if (c->slot_names[k] == name) break;
        if (k == c->slot_names.size()) {
            if (k == kCondMaxSlots) return refuse(PG_ERR_UNSUPPORTED, "more than %u user slots (\"%s\")", kCondMaxSlots, name);
            c->slot_names.push_back(name);
            c->slot_float.push_back(kind);
        } else if (c->slot_float[k] == 2) {
            c->slot_float[k] = kind;
        } else if (kind != 2 && c->slot_float[k] != kind) {
            return refuse(PG_ERR_INVALID, "rule %u: user property \"%s\" is read both as a float and as an integer: a slot holds one 8-byte value", rule, name);
        }
        *out = (uint8_t)k;
        return PG_OK;
    }
    int term(const pg_cond_term& s, uint32_t rule, uint32_t idx, bool in_bool) {
        int rc;
        if (s.op < 0 || s.op > PG_COND_EXPRESSION) return refuse(PG_ERR_INVALID, "rule %u term %u: unknown operator %d", rule, idx, s.op);
        const char* opn = kCondOpNames[s.op];
        if (s.op == PG_COND_CONTAINS || s.op == PG_COND_NOT_CONTAINS)
            return refuse(PG_ERR_UNSUPPORTED, "rule %u term %u: operator \"%s\" (list-valued properties) is not served", rule, idx, opn);
        if (s.op == PG_COND_EXPRESSION)
            return refuse(PG_ERR_UNSUPPORTED, "rule %u term %u: operator \"expression\" (expr-lang) is not served", rule, idx);
        if (s.depth > 1 || (s.depth == 1 && s.op == PG_COND_BOOL))
            return refuse(PG_ERR_UNSUPPORTED, "rule %u term %u: operator \"%s\" nested deeper than one bool is not served", rule, idx, opn);
        if (s.depth == 1 && !in_bool) return refuse(PG_ERR_INVALID, "rule %u term %u: a child term (\"%s\") without a bool in front", rule, idx, opn);
        CondTerm t{};
        t.op = (uint8_t)s.op;
        t.depth = (uint8_t)s.depth;
        if (s.op == PG_COND_BOOL) {
            t.is_and = s.bool_and ? 1 : 0;
            c->terms.push_back(t);
            return PG_OK;
        }
        const char* dom = s.domain && s.domain[0] ? s.domain : "item";
        if (strcmp(dom, "item") && strcmp(dom, "user"))
            return refuse(PG_ERR_UNSUPPORTED, "rule %u term %u: domain \"%s\" (EvaluateByDomain serves item and user, filter_op.go:533-535)", rule, idx, dom);
        if (!s.name || !s.name[0]) return refuse(PG_ERR_INVALID, "rule %u term %u: operator \"%s\" without a property name", rule, idx, opn);
        t.user_left = !strcmp(dom, "user");
        const bool nullish = s.op == PG_COND_IS_NULL || s.op == PG_COND_IS_NOT_NULL;
        if (!nullish && (s.type < 0 || s.type > PG_COND_STRING)) return refuse(PG_ERR_INVALID, "rule %u term %u (\"%s\"): unknown type %d", rule, idx, s.name, s.type);
        t.type = nullish ? (uint8_t)PG_COND_INT : (uint8_t)s.type;
        const bool ordered = s.op >= PG_COND_GREATER && s.op <= PG_COND_LESS_THAN;
        const bool listed = s.op == PG_COND_IN || s.op == PG_COND_NOT_IN;
        if (ordered && s.type == PG_COND_STRING)
            return refuse(PG_ERR_UNSUPPORTED, "rule %u term %u: \"%s\" on the string property \"%s\": ordered comparisons of strings are not served", rule, idx, opn, s.name);
        // does this term ever read a value?  (equal / not_equal with float and in / not_in with int64 / float answer from the
        // presence alone: their switches do not list the type)
        const bool reads = !nullish && !((s.op <= PG_COND_NOT_EQUAL && s.type == PG_COND_FLOAT) || (listed && (s.type == PG_COND_FLOAT || s.type == PG_COND_INT64)));
        const bool as_float = s.type == PG_COND_FLOAT;
        if (c->boost && !t.user_left && !strcmp(s.name, "score"))
            return refuse(PG_ERR_UNSUPPORTED, "rule %u term %u: an item term named \"score\" in a boost rule set (the reference's clone gains a "
                          "score key in the middle of the walk, boost_score_sort.go:81)", rule, idx);
        if (t.user_left) {
            if ((rc = slot(s.name, !reads ? 2 : as_float ? 1 : 0, rule, &t.left))) return rc;
        } else if (reads) {
            if ((rc = column(s.name, !as_float, rule, "property", &t.left))) return rc;
        } else {
            uint8_t dummy;                                     // named, never read: it must still exist
            if ((rc = column(s.name, false, rule, "property", &dummy))) return rc;
            t.left = dummy;
        }
        if (nullish) {
            c->terms.push_back(t);
            return PG_OK;
        }
        if (listed) {
            if (s.rhs != PG_COND_RHS_CONST)
                return refuse(PG_ERR_UNSUPPORTED, "rule %u term %u: \"%s\" on \"%s\" against the list-valued property %s%s is not served", rule, idx, opn,
                              s.name, s.rhs == PG_COND_RHS_ITEM ? "item." : "user.", s.rhs_name ? s.rhs_name : "");
            if (s.n_list > kCondMaxList) return refuse(PG_ERR_UNSUPPORTED, "rule %u term %u: \"%s\" on \"%s\" with %u values (at most %u)", rule, idx, opn, s.name, s.n_list, kCondMaxList);
            if (s.n_list && !s.list) return refuse(PG_ERR_INVALID, "rule %u term %u: \"%s\" on \"%s\": NULL list", rule, idx, opn, s.name);
            t.list_off = (uint16_t)c->lists.size();
            t.list_n = (uint16_t)s.n_list;
            c->lists.insert(c->lists.end(), s.list, s.list + s.n_list);
            std::sort(c->lists.begin() + t.list_off, c->lists.end());
            c->terms.push_back(t);
            return PG_OK;
        }
        if (s.rhs == PG_COND_RHS_USER_LIST)
            return refuse(PG_ERR_UNSUPPORTED, "rule %u term %u: the list-valued right-hand side user.%s is not served", rule, idx, s.rhs_name ? s.rhs_name : "");
        if (s.rhs < 0 || s.rhs > PG_COND_RHS_ITEM) return refuse(PG_ERR_INVALID, "rule %u term %u (\"%s\"): unknown right-hand side kind %d", rule, idx, s.name, s.rhs);
        t.rhs = (uint8_t)s.rhs;
        if (s.rhs == PG_COND_RHS_CONST) {
            if (as_float) t.c.f = s.f; else t.c.i = s.i;
        } else {
            if (!s.rhs_name || !s.rhs_name[0]) return refuse(PG_ERR_INVALID, "rule %u term %u (\"%s\"): the right-hand side has no name", rule, idx, s.name);
            if (s.rhs == PG_COND_RHS_USER) {
                if ((rc = slot(s.rhs_name, !reads ? 2 : as_float ? 1 : 0, rule, &t.rhs_idx))) return rc;
            } else {
                if (c->boost && !strcmp(s.rhs_name, "score"))
                    return refuse(PG_ERR_UNSUPPORTED, "rule %u term %u: item.score in a boost rule set (the reference's clone gains a score key in "
                                  "the middle of the walk, boost_score_sort.go:81)", rule, idx);
                if (reads) {
                    if ((rc = column(s.rhs_name, !as_float, rule, "right-hand side item.", &t.rhs_idx))) return rc;
                } else {
                    uint8_t dummy;
                    if ((rc = column(s.rhs_name, false, rule, "right-hand side item.", &dummy))) return rc;
                    t.rhs_idx = dummy;
                }
            }
        }
        c->terms.push_back(t);
        return PG_OK;
    }
};

int cond_compile(const pg_cond_rule* rules, uint32_t n_rules, const pg_cond_col* cols, uint32_t n_cols, uint32_t boost, pg_cond* c) {
    CondCompiler cc{c, cols, n_cols};
    if (!rules || n_rules < 1) return cc.refuse(PG_ERR_INVALID, "no rules");
    if (n_rules > kCondMaxRules) return cc.refuse(PG_ERR_UNSUPPORTED, "%u rules (at most %u)", n_rules, kCondMaxRules);
    if (n_cols && !cols) return cc.refuse(PG_ERR_INVALID, "NULL column declarations");
    for (uint32_t d = 0; d < n_cols; ++d) {
        if (!cols[d].name || !cols[d].name[0]) return cc.refuse(PG_ERR_INVALID, "declared column %u has no name", d);
        if (cols[d].dtype < PG_F_I32 || cols[d].dtype > PG_F_F64) return cc.refuse(PG_ERR_INVALID, "declared column \"%s\" has unknown dtype %d", cols[d].name, cols[d].dtype);
        for (uint32_t e = 0; e < d; ++e)
            if (!strcmp(cols[e].name, cols[d].name)) return cc.refuse(PG_ERR_INVALID, "column \"%s\" is declared twice", cols[d].name);
        c->col_names.push_back(cols[d].name);
        c->col_dtypes.push_back(cols[d].dtype);
    }
    c->boost = boost != 0;
    int rc;
    for (uint32_t r = 0; r < n_rules; ++r) {
        const pg_cond_rule& ru = rules[r];
        if (ru.n_terms > kCondMaxTerms) return cc.refuse(PG_ERR_UNSUPPORTED, "rule %u has %u operators, a bool's children counted (at most %u)", r, ru.n_terms, kCondMaxTerms);
        if (ru.n_terms && !ru.terms) return cc.refuse(PG_ERR_INVALID, "rule %u: NULL terms", r);
        CondRule out{};
        out.term_off = (uint8_t)c->terms.size();
        out.n_terms = (uint8_t)ru.n_terms;
        bool in_bool = false;
        for (uint32_t i = 0; i < ru.n_terms; ++i) {
            if (ru.terms[i].depth == 0) in_bool = false;
            if ((rc = cc.term(ru.terms[i], r, i, in_bool))) return rc;
            if (ru.terms[i].op == PG_COND_BOOL) in_bool = true;
        }
        if (c->boost) {
            // an empty Expression leaves evaluableExpression nil and a matching condition dereferences it (boost_score_sort.go:22-29,82)
            if (!ru.expression || !ru.expression[0]) return cc.refuse(PG_ERR_INVALID, "rule %u: a boost rule without an expression (the reference dereferences nil when its condition matches)", r);
            pg_expr* e = nullptr;
            if ((rc = pg_expr_compile_govaluate(ru.expression, &e))) return rc;
            std::unique_ptr<pg_expr> hold(e);
            if (e->prog.size() > kCondMaxExprOps || (uint32_t)e->max_depth > kCondMaxExprDepth)
                return cc.refuse(PG_ERR_UNSUPPORTED, "rule %u: expression '%.200s' has %zu operations at depth %d (at most %u at depth %u)", r, ru.expression,
                                 e->prog.size(), e->max_depth, kCondMaxExprOps, kCondMaxExprDepth);
            out.prog_off = (uint16_t)c->progs.size();
            out.prog_n = (uint16_t)e->prog.size();
            for (Instr in : e->prog) {
                if (in.op == OP_VAR) {
                    const std::string& name = e->vars[in.arg];
                    if (name == "score") {
                        in.arg = kVarScore;
                    } else {
                        uint8_t k;
                        if ((rc = cc.column(name.c_str(), false, r, "expression variable", &k))) return rc;
                        in.arg = k;
                    }
                }
                c->progs.push_back(in);
            }
        } else if (ru.expression && ru.expression[0]) {
            return cc.refuse(PG_ERR_INVALID, "rule %u carries an expression but the set is not a boost rule set", r);
        }
        c->rules.push_back(out);
    }
    return PG_OK;
}

int item_state_filter_locked(pg_ctx* ctx, pg_cond* c, const pg_features* fs, const CandIn& in, const CandOut& out, const uint64_t* d_user_vals,
                             const uint32_t* d_user_present) {
    CondProgram p;
    int rc;
    if ((rc = cond_bind_locked(ctx, c, fs, "pg_item_state_filter_dev", &p))) return rc;
    FilterArgs a{};
    a.in = in;
    a.out = out;
    a.user_vals = reinterpret_cast<const unsigned long long*>(d_user_vals);
    a.user_present = d_user_present;
    item_state_filter_kernel<<<in.nq, kCondChunk, 0, ctx->stream>>>(p, a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int boost_scores_locked(pg_ctx* ctx, pg_cond* c, const pg_features* fs, uint32_t filter_all, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                        const double* d_score, const uint32_t* d_count, const uint64_t* d_user_vals, const uint32_t* d_user_present,
                        double* d_out_score, uint8_t* d_out_rule) {
    CondProgram p;
    int rc;
    if ((rc = cond_bind_locked(ctx, c, fs, "pg_boost_scores_dev", &p))) return rc;
    boost_scores_kernel<<<dim3((cap + kBoostThreads - 1) / kBoostThreads, nq), kBoostThreads, 0, ctx->stream>>>(
        p, d_rows, reinterpret_cast<const unsigned long long*>(d_score), d_count, reinterpret_cast<const unsigned long long*>(d_user_vals),
        d_user_present, cap, filter_all, reinterpret_cast<unsigned long long*>(d_out_score), d_out_rule);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

int distinct_ids_locked(pg_ctx* ctx, pg_cond* c, const pg_features* fs, const int64_t* ids, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                        const uint32_t* d_count, const uint64_t* d_user_vals, const uint32_t* d_user_present, int64_t* d_out_id, const char* who) {
    CondProgram p;
    int rc;
    if ((rc = cond_bind_locked(ctx, c, fs, who, &p))) return rc;
    DistinctIds di{};
    for (size_t r = 0; r < c->rules.size(); ++r) di.id[r] = ids[r];
    distinct_ids_kernel<<<dim3((cap + kBoostThreads - 1) / kBoostThreads, nq), kBoostThreads, 0, ctx->stream>>>(
        p, di, d_rows, d_count, reinterpret_cast<const unsigned long long*>(d_user_vals), d_user_present, cap, reinterpret_cast<long long*>(d_out_id));
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// The one-request entries over the candidates' own values (pg_boost_scores, pg_distinct_ids): the values become a store of n
// rows in scratch, candidate i reads row i, one outside the store row n.  rows_of: the row ids to stage; stage_cols appends
// the referenced columns to the staging list (a column of up to 8-byte values each), store_of makes the store over them once
// staged_run has placed them (it never owns: the columns point into scratch).
void cond_own_rows(uint32_t n, const uint8_t* item_in, std::vector<uint64_t>* rows) {
    rows->resize(n);
    for (uint32_t i = 0; i < n; ++i) (*rows)[i] = !item_in || item_in[i] ? i : n;
}
void cond_stage_cols(const pg_cond* c, uint32_t n, const void* const* cols, std::vector<Staged>* st) {
    for (size_t k = 0; k < c->used.size(); ++k) {
        const int dt = c->col_dtypes[(size_t)c->used[k]];
        st->push_back({cols[c->used[k]], (size_t)n * (dt == PG_F_I32 || dt == PG_F_F32 ? 4 : 8), Staged::kIn, (size_t)n * 8});
    }
}
void cond_own_store(const pg_cond* c, uint32_t n, const Staged* staged_cols, pg_features* tmp) {
    tmp->rows = n;
    for (size_t k = 0; k < c->used.size(); ++k) {
        const int d = c->used[k];
        pg_features::Column col;
        col.name = c->col_names[(size_t)d];
        col.dtype = c->col_dtypes[(size_t)d];
        col.d = staged_cols[k].dev;
        tmp->cols.push_back(col);
    }
}

}  // namespace
}  // namespace pg

extern "C" {

int pg_cond_compile(const pg_cond_rule* rules, uint32_t n_rules, const pg_cond_col* cols, uint32_t n_cols, uint32_t boost, pg_cond** out) {
    PG_REQUIRE(out, "pg_cond_compile: NULL argument");
    if (n_cols > 256) {
        pg::set_error("pg_cond_compile: %u declared columns (at most 256)", n_cols);
        return PG_ERR_UNSUPPORTED;
    }
    std::unique_ptr<pg_cond> c(new pg_cond());
    const int rc = pg::cond_compile(rules, n_rules, cols, n_cols, boost, c.get());
    if (rc) return rc;
    *out = c.release();
    return PG_OK;
}

int pg_cond_free(pg_cond* c) {
    if (!c) return PG_OK;
    c->table.release();
    delete c;
    return PG_OK;
}

int pg_cond_num_rules(const pg_cond* c) { return c ? (int)c->rules.size() : 0; }
int pg_cond_num_user_slots(const pg_cond* c) { return c ? (int)c->slot_names.size() : 0; }
const char* pg_cond_user_slot_name(const pg_cond* c, int i) { return c && i >= 0 && i < (int)c->slot_names.size() ? c->slot_names[(size_t)i].c_str() : ""; }
int pg_cond_user_slot_is_float(const pg_cond* c, int i) { return c && i >= 0 && i < (int)c->slot_float.size() && c->slot_float[(size_t)i] == 1 ? 1 : 0; }

int pg_cond_match_host(const pg_cond* c, uint32_t rule, uint32_t n, const uint8_t* item_in, const void* const* cols, const uint64_t* user_vals,
                       uint32_t user_present, uint8_t* out_match) {
    PG_REQUIRE(c && (n == 0 || out_match), "pg_cond_match_host: NULL argument");
    PG_REQUIRE(rule < c->rules.size(), "pg_cond_match_host: rule %u of %zu", rule, c->rules.size());
    int rc;
    if (n && (rc = pg::cond_host_check(c, cols, user_vals, "pg_cond_match_host"))) return rc;
    pg::CondProgram p;
    std::vector<const void*> none(c->col_names.size(), nullptr);
    pg::cond_program(c, none.data(), c->lists.data(), c->progs.data(), 0, &p);
    const pg::CondUser u{reinterpret_cast<const unsigned long long*>(user_vals), user_present};
    for (uint32_t i = 0; i < n; ++i) {
        pg::CondItem it;
        pg::cond_host_item(c->used, c->col_dtypes, cols, item_in, i, &it);
        out_match[i] = pg::cond_rule(p, rule, it, u) ? 1 : 0;
    }
    return PG_OK;
}

int pg_boost_scores_host(const pg_cond* c, uint32_t filter_all, uint32_t n, const uint8_t* item_in, const void* const* cols,
                         const uint64_t* user_vals, uint32_t user_present, const double* score, double* out_score, uint8_t* out_rule) {
    PG_REQUIRE(c && (n == 0 || (score && out_score)), "pg_boost_scores_host: NULL argument");
    PG_REQUIRE(c->boost, "pg_boost_scores_host: the set was not compiled as a boost rule set");
    int rc;
    if (n && (rc = pg::cond_host_check(c, cols, user_vals, "pg_boost_scores_host"))) return rc;
    pg::CondProgram p;
    std::vector<const void*> none(c->col_names.size(), nullptr);
    pg::cond_program(c, none.data(), c->lists.data(), c->progs.data(), 0, &p);
    const pg::CondUser u{reinterpret_cast<const unsigned long long*>(user_vals), user_present};
    for (uint32_t i = 0; i < n; ++i) {
        pg::CondItem it;
        pg::cond_host_item(c->used, c->col_dtypes, cols, item_in, i, &it);
        double s = score[i];
        const uint32_t last = pg::cond_boost(p, filter_all != 0, it, u, &s);
        memcpy(&out_score[i], &s, 8);                    // (moves only: an untouched score keeps its bits)
        if (out_rule) out_rule[i] = (uint8_t)last;
    }
    return PG_OK;
}

int pg_item_state_filter_dev(pg_ctx* ctx, pg_cond* c, const pg_features* fs, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                             const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64,
                             uint32_t n_f64, const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32,
                             const uint64_t* d_user_vals, const uint32_t* d_user_present, uint64_t* d_out_rows, double* d_out_score,
                             uint8_t* d_out_source, double* d_out_planes_f64, uint32_t* d_out_source_mask, float* d_out_planes_f32,
                             uint32_t* d_out_count) {
    const char* who = "pg_item_state_filter_dev";
    const pg::CandCall l{d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count};
    int rc;
    if ((rc = pg::cand_call_required(l, ctx && c && fs, who))) return rc;
    PG_REQUIRE(!c->boost, "%s: the set was compiled as a boost rule set", who);
    if ((rc = pg::cond_check_shape(nq, cap, who))) return rc;
    PG_REQUIRE(c->slot_names.empty() || (d_user_vals && d_user_present), "%s: the set reads user properties: d_user_vals and d_user_present are needed", who);
    if ((rc = pg::cand_lists_check(l, pg::kCandMaxPlanes, who)) || (rc = pg::cand_call_apart(l, nq, cap, cap, who))) return rc;
    pg::CandIn in;
    pg::CandOut out;
    pg::cand_lists_bind(l, nq, cap, cap, &in, &out);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::item_state_filter_locked(ctx, c, fs, in, out, d_user_vals, d_user_present);
}

int pg_boost_scores_dev(pg_ctx* ctx, pg_cond* c, const pg_features* fs, uint32_t filter_all, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                        const double* d_score, const uint32_t* d_count, const uint64_t* d_user_vals, const uint32_t* d_user_present,
                        double* d_out_score, uint8_t* d_out_rule) {
    PG_REQUIRE(ctx && c && fs && d_rows && d_score && d_out_score, "pg_boost_scores_dev: NULL argument");
    PG_REQUIRE(c->boost, "pg_boost_scores_dev: the set was not compiled as a boost rule set");
    int rc;
    if ((rc = pg::cond_check_shape(nq, cap, "pg_boost_scores_dev"))) return rc;
    PG_REQUIRE(c->slot_names.empty() || (d_user_vals && d_user_present), "pg_boost_scores_dev: the set reads user properties: d_user_vals and d_user_present are needed");
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::boost_scores_locked(ctx, c, fs, filter_all, nq, cap, d_rows, d_score, d_count, d_user_vals, d_user_present, d_out_score, d_out_rule);
}

// ---- one request on host arrays (staged_run, cand_lists.hpp) ---------------------------------------------------------------------
int pg_item_state_filter(pg_ctx* ctx, pg_cond* c, const pg_features* fs, uint32_t n, const uint64_t* rows, const double* score, const uint8_t* source,
                         const uint64_t* user_vals, uint32_t user_present, uint64_t* out_rows, double* out_score, uint8_t* out_source,
                         uint32_t* out_count) {
    PG_REQUIRE(ctx && c && fs && out_count && (n == 0 || (rows && score && out_rows && out_score)), "pg_item_state_filter: NULL argument");
    PG_REQUIRE(!c->boost, "pg_item_state_filter: the set was compiled as a boost rule set");
    PG_REQUIRE(!source == !out_source, "pg_item_state_filter: source and out_source come in pairs");
    PG_REQUIRE(c->slot_names.empty() || user_vals, "pg_item_state_filter: the set reads user properties: user_vals is needed");
    int rc;
    if (n == 0) {                                    // an empty request: an empty answer
        *out_count = 0;
        return PG_OK;
    }
    if ((rc = pg::cond_check_shape(1, n, "pg_item_state_filter"))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    uint64_t uv[pg::kCondMaxSlots] = {0};
    if (user_vals) memcpy(uv, user_vals, c->slot_names.size() * 8);
    using pg::Staged;
    enum { kRows, kScore, kOutRows, kOutScore, kSource, kOutSource, kUserVals, kUserPresent, kCount };
    Staged st[] = {{rows, (size_t)n * 8, Staged::kIn},      {score, (size_t)n * 8, Staged::kIn},   {out_rows, (size_t)n * 8, Staged::kOut},
                   {out_score, (size_t)n * 8, Staged::kOut}, {source, n, Staged::in_if(source)},    {out_source, n, Staged::out_if(source)},
                   {uv, sizeof uv, Staged::kIn},             {&user_present, 4, Staged::kIn},       {out_count, 4, Staged::kOut}};
    return pg::staged_run(ctx, pg::kSlotCond, st, sizeof st / sizeof *st, true /* uv and user_present are this frame's */, [&] {
        pg::CandIn in{};
        in.rows = st[kRows].at<uint64_t>();
        in.score = st[kScore].at<unsigned long long>();
        in.source = source ? st[kSource].at<uint8_t>() : nullptr;
        in.nq = 1;
        in.cap = n;
        pg::CandOut out{};
        out.rows = st[kOutRows].at<uint64_t>();
        out.score = st[kOutScore].at<unsigned long long>();
        out.source = source ? st[kOutSource].at<uint8_t>() : nullptr;
        out.count = st[kCount].at<uint32_t>();
        out.out_cap = n;
        return pg::item_state_filter_locked(ctx, c, fs, in, out, st[kUserVals].at<uint64_t>(), st[kUserPresent].at<uint32_t>());
    });
}

int pg_boost_scores(pg_ctx* ctx, pg_cond* c, uint32_t filter_all, uint32_t n, const uint8_t* item_in, const void* const* cols,
                    const uint64_t* user_vals, uint32_t user_present, const double* score, double* out_score, uint8_t* out_rule) {
    PG_REQUIRE(ctx && c && (n == 0 || (score && out_score)), "pg_boost_scores: NULL argument");
    PG_REQUIRE(c->boost, "pg_boost_scores: the set was not compiled as a boost rule set");
    int rc;
    if (n == 0) return PG_OK;                        // an empty request: nothing to rewrite
    if ((rc = pg::cond_check_shape(1, n, "pg_boost_scores"))) return rc;
    if ((rc = pg::cond_host_check(c, cols, user_vals, "pg_boost_scores"))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    std::vector<uint64_t> rows;
    pg::cond_own_rows(n, item_in, &rows);
    uint64_t uv[pg::kCondMaxSlots] = {0};
    if (user_vals) memcpy(uv, user_vals, c->slot_names.size() * 8);
    using pg::Staged;
    enum { kRows, kScore, kOutScore, kOutRule, kUserVals, kUserPresent, kCols };
    std::vector<Staged> st = {{rows.data(), (size_t)n * 8, Staged::kIn},      {score, (size_t)n * 8, Staged::kIn},
                              {out_score, (size_t)n * 8, Staged::kOut},       {out_rule, n, Staged::out_if(out_rule)},
                              {uv, sizeof uv, Staged::kIn},                   {&user_present, 4, Staged::kIn}};
    pg::cond_stage_cols(c, n, cols, &st);
    return pg::staged_run(ctx, pg::kSlotCond, st.data(), st.size(), true /* rows, uv and user_present are this frame's */, [&] {
        pg_features tmp;
        pg::cond_own_store(c, n, st.data() + kCols, &tmp);
        return pg::boost_scores_locked(ctx, c, &tmp, filter_all, 1, n, st[kRows].at<uint64_t>(), st[kScore].at<double>(), nullptr,
                                       st[kUserVals].at<uint64_t>(), st[kUserPresent].at<uint32_t>(), st[kOutScore].at<double>(),
                                       st[kOutRule].at<uint8_t>());
    });
}

// ---- DistinctIdSort ------------------------------------------------------------------------------------------------------------------
int pg_distinct_ids_host(const pg_cond* c, const int64_t* ids, uint32_t n, const uint8_t* item_in, const void* const* cols,
                         const uint64_t* user_vals, uint32_t user_present, int64_t* out_id) {
    PG_REQUIRE(c && ids && (n == 0 || out_id), "pg_distinct_ids_host: NULL argument");
    PG_REQUIRE(!c->boost, "pg_distinct_ids_host: the set was compiled as a boost rule set");
    int rc;
    if (n && (rc = pg::cond_host_check(c, cols, user_vals, "pg_distinct_ids_host"))) return rc;
    pg::CondProgram p;
    std::vector<const void*> none(c->col_names.size(), nullptr);
    pg::cond_program(c, none.data(), c->lists.data(), c->progs.data(), 0, &p);
    const pg::CondUser u{reinterpret_cast<const unsigned long long*>(user_vals), user_present};
    pg::DistinctIds di{};
    for (size_t r = 0; r < c->rules.size(); ++r) di.id[r] = ids[r];
    for (uint32_t i = 0; i < n; ++i) {
        pg::CondItem it;
        pg::cond_host_item(c->used, c->col_dtypes, cols, item_in, i, &it);
        out_id[i] = pg::cond_distinct_id(p, di, it, u, i);
    }
    return PG_OK;
}

int pg_distinct_ids_dev(pg_ctx* ctx, pg_cond* c, const pg_features* fs, const int64_t* ids, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                        const uint32_t* d_count, const uint64_t* d_user_vals, const uint32_t* d_user_present, int64_t* d_out_id) {
    const char* who = "pg_distinct_ids_dev";
    PG_REQUIRE(ctx && c && fs && ids && d_rows && d_out_id, "%s: NULL argument", who);
    PG_REQUIRE(!c->boost, "%s: the set was compiled as a boost rule set", who);
    int rc;
    if ((rc = pg::cond_check_shape(nq, cap, who))) return rc;
    PG_REQUIRE(c->slot_names.empty() || (d_user_vals && d_user_present), "%s: the set reads user properties: d_user_vals and d_user_present are needed", who);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::distinct_ids_locked(ctx, c, fs, ids, nq, cap, d_rows, d_count, d_user_vals, d_user_present, d_out_id, who);
}

int pg_distinct_ids(pg_ctx* ctx, pg_cond* c, const int64_t* ids, uint32_t n, const uint8_t* item_in, const void* const* cols,
                    const uint64_t* user_vals, uint32_t user_present, int64_t* out_id) {
    const char* who = "pg_distinct_ids";
    PG_REQUIRE(ctx && c && ids && (n == 0 || out_id), "%s: NULL argument", who);
    PG_REQUIRE(!c->boost, "%s: the set was compiled as a boost rule set", who);
    int rc;
    if (n == 0) return PG_OK;                        // an empty request: nothing to tag
    if ((rc = pg::cond_check_shape(1, n, who))) return rc;
    if ((rc = pg::cond_host_check(c, cols, user_vals, who))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    std::vector<uint64_t> rows;
    pg::cond_own_rows(n, item_in, &rows);
    uint64_t uv[pg::kCondMaxSlots] = {0};
    if (user_vals) memcpy(uv, user_vals, c->slot_names.size() * 8);
    using pg::Staged;
    enum { kRows, kOutId, kUserVals, kUserPresent, kCols };
    std::vector<Staged> st = {{rows.data(), (size_t)n * 8, Staged::kIn}, {out_id, (size_t)n * 8, Staged::kOut}, {uv, sizeof uv, Staged::kIn},
                              {&user_present, 4, Staged::kIn}};
    pg::cond_stage_cols(c, n, cols, &st);
    return pg::staged_run(ctx, pg::kSlotCond, st.data(), st.size(), true /* rows, uv and user_present are this frame's */, [&] {
        pg_features tmp;
        pg::cond_own_store(c, n, st.data() + kCols, &tmp);
        return pg::distinct_ids_locked(ctx, c, &tmp, ids, 1, n, st[kRows].at<uint64_t>(), nullptr, st[kUserVals].at<uint64_t>(),
                                       st[kUserPresent].at<uint32_t>(), st[kOutId].at<int64_t>(), who);
    });
}

}  // extern "C"
