// classcut.hip — DiversityAdjustCountFilter on the device: quotas per expression class.
//
// The reference (filter/diversity_adjust_count_filter.go:75-143) sorts a request's merged candidates by Item.Score, evaluates
// every config's govaluate expression on every item's feature map (:92-103: an evaluation error or a result that is not `true`
// means "not in this class") and walks the configs in order (:115-140): class c offers its first limit_c members in score order
// — count_c for "fix", count_c - accumulator for "accumulator" — and keeps those no earlier class kept; an already kept member
// still uses up a place (`i < count` indexes the class's list).  Classes may overlap, which is what the trim's kernel cannot
// serve: its classes are disjoint sources.
//
// Three parts:
//   front end     a statically typed boolean subset of govaluate compiled to the postfix program of expr_prog.hpp: numbers as
//                 pg_expr_compile_govaluate reads them, comparators, `in` over constants, && || !, declared item columns,
//                 recall_score and recall_name.  Everything else is refused by name, never evaluated differently.
//   mask kernel   one lane per candidate: its row, every referenced column's raw value (all loads issued before the first use),
//                 then each class's program on an 8-deep register stack with one error bit beside every slot (the technique of
//                 cond.hip's cond_expr; the shared pieces are cond_eval.hpp) → one byte per candidate, bit c = member of class c.
//   cut kernel    one workgroup of 1 024 lanes per request over the trim's score order.  Classes run one after another (limit_c
//                 needs the picks of the classes before it); inside a class the order is walked 1 024 positions at a time: a
//                 member's rank = the running count + the members in the waves before it (per-wave counts in LDS) + those in the
//                 lanes before it (block_rank.hpp's wave_rank); it is in the window iff rank < limit_c and picked iff its bit in a 2 KB LDS
//                 bitmap of input positions is clear; picks get base + their prefix count and set their bit.  The walk of a
//                 class ends with the chunk in which the rank reaches the limit.  Whatever steers the walk is the same in every
//                 lane: it comes out of LDS behind a barrier.
// pg_classcut_masks_host / pg_candidates_classcut_host state the same answer on host arrays with plain containers.
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

constexpr uint32_t kCcMaxClasses = 8, kCcMaxOps = 64, kCcMaxDepth = 8, kCcMaxList = 64, kCcMaxRecalls = 32, kCcMaxListTotal = 4096;
constexpr uint32_t kCcChunk = 1024, kCcWaves = kCcChunk / kWave, kCcMaskThreads = 256;
static_assert(kCcMaxClasses == PG_CLASSCUT_MAX_CLASSES && kCcMaxOps == PG_COND_MAX_EXPR_OPS && kCcMaxDepth == PG_COND_MAX_EXPR_DEPTH &&
                  kCcMaxList == PG_COND_MAX_LIST && kCcMaxRecalls == PG_CLASSCUT_MAX_RECALLS && kCcChunk == PG_TRIM_CHUNK,
              "include/pairec_gpu.h repeats these");
static_assert(kCcMaxClasses <= 8, "a candidate's classes travel as one byte");
constexpr uint32_t kCcVarScore = 0xFFFFu;         // Instr.arg of the variable recall_score

struct CcRule { uint16_t prog_off, prog_n; };
struct CcProgram {                                // what the mask kernel and the host statements walk
    CondCol cols[kCondMaxCols];                   // the referenced columns (host statements: unused, the values come by CondItem)
    CcRule rules[kCcMaxClasses];
    const double* lists;
    const Instr* progs;
    uint32_t n_used, n_classes;
    uint64_t store_rows;
};

// class c's expression on one candidate (diversity_adjust_count_filter.go:94-101): true iff it evaluates, without an error, to
// true.  The stack's top is st[0]; bit j of err: slot j holds govaluate's error ("No parameter found": a declared column of a
// candidate outside the store), which every operator hands on except && and ||, whose left side may decide alone.
__host__ __device__ __forceinline__ bool cc_member(const CcProgram& p, uint32_t c, const CondItem& it, double score, uint32_t source) {
    double st[kCcMaxDepth];
#pragma unroll
    for (uint32_t j = 0; j < kCcMaxDepth; ++j) st[j] = 0.0;
    uint32_t err = 0;
    const Instr* prog = p.progs + p.rules[c].prog_off;
    const uint32_t n = p.rules[c].prog_n;
    for (uint32_t pc = 0; pc < n; ++pc) {
        const Instr in = prog[pc];
        if (in.op == OP_CONST || in.op == OP_VAR || in.op == OP_SRC) {
            double v = in.val;
            uint32_t e = 0;
            if (in.op == OP_VAR) {
                if (in.arg == kCcVarScore) v = score;
                else if (it.item_in) v = cond_col_f64(p, it, in.arg);
                else e = 1;
            } else if (in.op == OP_SRC) {
                v = source < 32u && ((in.arg >> source) & 1u) ? 1.0 : 0.0;
            }
#pragma unroll
            for (uint32_t j = kCcMaxDepth - 1; j > 0; --j) st[j] = st[j - 1];
            st[0] = v;
            err = (err << 1) | e;
        } else if (in.op == OP_NEG) {
            st[0] = -st[0];
        } else if (in.op == OP_ROUND) {
            st[0] = round(st[0]);
        } else if (in.op == OP_NOT) {
            st[0] = st[0] != 0.0 ? 0.0 : 1.0;
        } else if (in.op == OP_IN) {
            const double* list = p.lists + (in.arg & 0xFFFFu);
            const uint32_t ln = in.arg >> 16;
            bool found = false;
            for (uint32_t j = 0; j < ln; ++j) found = found || list[j] == st[0];       // (== as the comparator: NaN is in no list)
            st[0] = found ? 1.0 : 0.0;
        } else {
            const double l = st[1], r = st[0];
            const uint32_t el = (err >> 1) & 1u, er = err & 1u;
            double v = 0.0;
            uint32_t e = el | er;
            switch (in.op) {
                case OP_EQ: v = l == r ? 1.0 : 0.0; break;
                case OP_NE: v = l != r ? 1.0 : 0.0; break;
                case OP_GT: v = l > r ? 1.0 : 0.0; break;
                case OP_GE: v = l >= r ? 1.0 : 0.0; break;
                case OP_LT: v = l < r ? 1.0 : 0.0; break;
                case OP_LE: v = l <= r ? 1.0 : 0.0; break;
                case OP_AND:                                              // a && b: a's error; false if a is; else b
                    v = l != 0.0 ? r : 0.0;
                    e = el | (l != 0.0 ? er : 0u);
                    break;
                case OP_OR:                                               // a || b: a's error; true if a is; else b
                    v = l != 0.0 ? 1.0 : r;
                    e = el | (l != 0.0 ? 0u : er);
                    break;
                default: expr_binop(in.op, l, r, &v); break;              // (this front end emits no operator that panics)
            }
            st[0] = v;
#pragma unroll
            for (uint32_t j = 1; j + 1 < kCcMaxDepth; ++j) st[j] = st[j + 1];
            err = ((err >> 2) << 1) | e;
        }
    }
    return !(err & 1u) && st[0] != 0.0;
}

// every class of one candidate → its mask byte
__host__ __device__ __forceinline__ uint32_t cc_classes(const CcProgram& p, const CondItem& it, double score, uint32_t source) {
    uint32_t m = 0;
    for (uint32_t c = 0; c < p.n_classes; ++c) m |= cc_member(p, c, it, score, source) ? 1u << c : 0u;
    return m;
}

// ---- kernels ---------------------------------------------------------------------------------------------------------------
// Request q = blockIdx.y, positions blockIdx.x * 256 ...: every byte of out [nq][cap] is written, padding gets 0.
__global__ __launch_bounds__(kCcMaskThreads) void classcut_masks_kernel(CcProgram p, const uint64_t* __restrict__ rows,
                                                                        const unsigned long long* __restrict__ score,
                                                                        const uint8_t* __restrict__ source, const uint32_t* __restrict__ count,
                                                                        uint32_t cap, uint8_t* __restrict__ out) {
    const uint32_t q = blockIdx.y, pos = blockIdx.x * kCcMaskThreads + threadIdx.x;
    if (pos >= cap) return;
    const size_t i = (size_t)q * cap + pos;
    const uint32_t n_valid = count ? min(count[q], cap) : cap;
    uint32_t m = 0;
    const unsigned long long row = rows[i];
    if (pos < n_valid && row != kCandPad) {
        CondItem item;
        cond_load(p, row, &item);
        m = cc_classes(p, item, cand_bits_f64(score[i]), source ? (uint32_t)source[i] : 0xFFu);
    }
    out[i] = (uint8_t)m;
}

struct CutArgs {
    CandIn in;
    CandOut out;
    const uint32_t* order;                       // [nq][cap]: each request's positions in score order
    const uint8_t* masks;                        // [nq][cap]: bit c = the entry is a member of class c (padding: 0)
    uint32_t n_classes;
    uint32_t r_count[kCcMaxClasses];
    uint8_t r_type[kCcMaxClasses];
};

// Request q = blockIdx.x.
__global__ __launch_bounds__(kCcChunk) void candidates_classcut_kernel(CutArgs a) {
    __shared__ uint32_t taken[kCandMaxCap / 32];                     // one bit per input position: an earlier pick
    __shared__ uint32_t wmem[kCcWaves], wpick[kCcWaves];             // this chunk's members / picks per wave
    const uint32_t q = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid & (kWave - 1);
    const uint32_t cap = a.in.cap, out_cap = a.out.out_cap;
    const size_t in0 = (size_t)q * cap, out0 = (size_t)q * out_cap;
    for (uint32_t w = tid; w < kCandMaxCap / 32; w += kCcChunk) taken[w] = 0u;
    __syncthreads();
    uint32_t acc = 0, base = 0;                                      // the accumulator and the picks so far: every lane counts along
    for (uint32_t c = 0; c < a.n_classes; ++c) {
        const uint32_t cnt = a.r_count[c];
        const uint32_t limit = a.r_type[c] == PG_TRIM_FIX ? cnt : (cnt > acc ? cnt - acc : 0u);
        uint32_t rank_run = 0, picks = 0;                            // class c's members met and picks made in the chunks before
        for (uint32_t c0 = 0; c0 < cap && rank_run < limit; c0 += kCcChunk) {
            const uint32_t i = c0 + tid;
            uint32_t pos = 0;
            bool member = false;
            if (i < cap) {
                pos = a.order[in0 + i];
                if (pos < cap) member = ((a.masks[in0 + pos] >> c) & 1u) != 0;
            }
            uint32_t n_mem;
            const uint32_t mbefore = wave_rank(member, &n_mem);
            if (lane == 0) wmem[wave] = n_mem;
            __syncthreads();                                          // (also: the picks' bits of the chunk before are set)
            uint32_t mbelow = 0, mtotal = 0;
#pragma unroll
            for (uint32_t w = 0; w < kCcWaves; ++w) {
                const uint32_t n = wmem[w];
                mbelow += w < wave ? n : 0u;
                mtotal += n;
            }
            // the window: the class's first `limit` members; a place an earlier pick holds is used up all the same
            const bool pick = member && rank_run + mbelow + mbefore < limit && !((taken[pos >> 5] >> (pos & 31u)) & 1u);
            uint32_t n_pick;
            const uint32_t pbefore = wave_rank(pick, &n_pick);
            if (lane == 0) wpick[wave] = n_pick;
            __syncthreads();                                          // (every lane has read wmem and its bit of taken)
            uint32_t pbelow = 0, ptotal = 0;
#pragma unroll
            for (uint32_t w = 0; w < kCcWaves; ++w) {
                const uint32_t n = wpick[w];
                pbelow += w < wave ? n : 0u;
                ptotal += n;
            }
            if (pick) {
                const uint32_t dst = base + picks + pbelow + pbefore;
                if (dst < out_cap) cand_carry(a.in, a.out, in0 + pos, out0 + dst, true);      // (always: pg_classcut_out_cap's bound)
                atomicOr(&taken[pos >> 5], 1u << (pos & 31u));        // (the order is a permutation: no other lane reads this bit now)
            }
            rank_run += mtotal;
            picks += ptotal;
            // (wmem is next written behind this chunk's second barrier, wpick behind the next chunk's first: both after every read)
        }
        if (a.r_type[c] != PG_TRIM_FIX) acc += picks;
        base += picks;
    }
    const uint32_t total = min(base, out_cap);
    cand_pad(a.in, a.out, q, total + tid, kCcChunk, kCandNegInf);
    if (tid == 0) a.out.count[q] = total;
}

}  // namespace
}  // namespace pg

// ---- the compiled object ------------------------------------------------------------------------------------------------------
struct pg_classcut {
    std::vector<std::string> col_names;           // as declared
    std::vector<int> col_dtypes;
    std::vector<int> used;                        // referenced columns → declared index (<= kCondMaxCols)
    std::vector<std::string> recall_names;
    std::vector<pg::CcRule> rules;
    std::vector<uint8_t> types;                   // PG_TRIM_FIX / PG_TRIM_ACCUMULATE
    std::vector<uint32_t> counts;
    std::vector<double> lists;
    std::vector<pg::Instr> progs;
    bool reads_source = false;                    // an expression reads recall_name
    pg::SetTable table;                           // lists | programs
};

namespace pg {
namespace {

// ---- the front end: govaluate's boolean subset, statically typed ------------------------------------------------------------
// Precedence, loosest first (govaluate's planner): ||  <  &&  <  == != > >= < <= in  <  + -  <  * / %  <  **  <  prefix - !  <
// value; && and || and the arithmetic levels are left-associative; -a ** 2 is (-a) ** 2 (as pg_expr_compile_govaluate).  A
// subexpression is a number, a bool, the name recall_name or a string literal; the last two are legal only as the two sides of
// == / != or as recall_name in ('a', 'b').  (A parser of its own rather than a mode of expr.hip's GvParser: every production
// here returns and checks a type, and that one must keep refusing what this one accepts.)
enum CcType { T_FAIL = 0, T_NUM, T_BOOL, T_NAME, T_STR };

struct CcParser {
    const std::string& s;
    pg_classcut* set;
    const pg_cond_col* cols;
    uint32_t n_cols;
    size_t i = 0;
    size_t prog0;                                 // where this expression's program starts in set->progs
    int depth = 0, max_depth = 0, nest = 0;
    int code = PG_ERR_UNSUPPORTED;
    std::string err, str_lit;
    CcParser(const std::string& src, pg_classcut* out, const pg_cond_col* c, uint32_t n) : s(src), set(out), cols(c), n_cols(n), prog0(out->progs.size()) {}

    void ws() { while (i < s.size() && (s[i] == ' ' || s[i] == '\t' || s[i] == '\n' || s[i] == '\r')) ++i; }
    CcType fail(const std::string& m) { if (err.empty()) err = m; return T_FAIL; }
    bool at(const char* t) { ws(); return s.compare(i, strlen(t), t) == 0; }
    static bool is_alpha(char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; }
    static bool is_digit(char c) { return c >= '0' && c <= '9'; }
    bool at_word(const char* w) {                 // the keyword w, not the head of a longer name
        ws();
        const size_t n = strlen(w);
        return s.compare(i, n, w) == 0 && !(i + n < s.size() && (is_alpha(s[i + n]) || is_digit(s[i + n]) || s[i + n] == '.'));
    }
    void push(uint32_t op, uint32_t arg, double val) {
        set->progs.push_back({op, arg, val});
        if (op == OP_CONST || op == OP_VAR || op == OP_SRC) max_depth = std::max(max_depth, ++depth);
        else if (op != OP_NEG && op != OP_ROUND && op != OP_NOT && op != OP_IN) --depth;
    }
    bool num(CcType t, const char* where) {       // t must be a number
        if (t == T_FAIL) return false;
        if (t == T_NUM) return true;
        if (t == T_BOOL) fail(std::string("a bool where a number is needed (") + where + ")");
        else if (t == T_NAME) fail(std::string("recall_name is legal only as recall_name == 'x', != 'x' and in ('x', 'y'): ordered comparisons on it and arithmetic with it are not in the served subset (") + where + ")");
        else fail(std::string("a string literal other than against recall_name is not in the served subset (") + where + ")");
        return false;
    }
    bool boolean(CcType t, const char* where) {   // t must be a bool
        if (t == T_FAIL) return false;
        if (t == T_BOOL) return true;
        if (t == T_NUM) fail(std::string("a number where a bool is needed (") + where + ")");
        else if (t == T_NAME) fail(std::string("recall_name where a bool is needed (") + where + ")");
        else fail(std::string("a string literal other than against recall_name is not in the served subset (") + where + ")");
        return false;
    }
    // names what stands at the cursor: an operator of the language outside the subset, or the character
    CcType unexpected(const std::string& what) {
        ws();
        if (i >= s.size()) return fail(what + ": end of the expression");
        static const char* const ops[] = {"??", "=~", "!~", "<<", ">>", "?", ":", "~", "&", "|", "^"};
        static const char* const names[] = {"the operator '\?\?'", "the regex comparator '=~'", "the regex comparator '!~'", "the bitwise operator '<<'",
                                            "the bitwise operator '>>'", "the ternary '?'", "the ternary ':'", "the bitwise operator '~'",
                                            "the bitwise operator '&'", "the bitwise operator '|'", "the bitwise operator '^'"};
        for (size_t k = 0; k < sizeof ops / sizeof ops[0]; ++k)
            if (s.compare(i, strlen(ops[k]), ops[k]) == 0) return fail(std::string(names[k]) + " is not in the served subset");
        if (is_alpha(s[i])) {
            size_t j = i;
            while (j < s.size() && (is_alpha(s[j]) || is_digit(s[j]))) ++j;
            return fail(what + " \"" + s.substr(i, j - i) + "\"");
        }
        return fail(what + " '" + s[i] + "'");
    }
    // a column, recall_score or recall_name by name
    CcType name_ref(const std::string& name) {
        if (name == "recall_name") return T_NAME;
        if (name == "recall_score") {
            push(OP_VAR, kCcVarScore, 0.0);
            return T_NUM;
        }
        uint32_t d = 0;
        for (; d < n_cols; ++d)
            if (name == cols[d].name) break;
        if (d == n_cols) {
            code = PG_ERR_INVALID;
            return fail("\"" + name + "\" is neither a declared column nor recall_name / recall_score (the reference's per-recall "
                        "Properties key is not served)");
        }
        size_t k = 0;
        for (; k < set->used.size(); ++k)
            if (set->used[k] == (int)d) break;
        if (k == set->used.size()) {
            if (k == kCondMaxCols) return fail("more than " + std::to_string(kCondMaxCols) + " referenced columns (\"" + name + "\")");
            set->used.push_back((int)d);
        }
        push(OP_VAR, (uint32_t)k, 0.0);
        return T_NUM;
    }
    // a literal of digits and '.' at the cursor → its value (govaluate's isNumeric)
    bool number(double* out) {
        if (s[i] == '0' && i + 1 < s.size() && (s[i + 1] == 'x' || s[i + 1] == 'X')) { fail("a hexadecimal literal is not in the served subset"); return false; }
        size_t j = i;
        while (j < s.size() && (is_digit(s[j]) || s[j] == '.')) ++j;
        const std::string lit = s.substr(i, j - i);
        size_t dots = 0, digits = 0;
        for (char d : lit) (d == '.' ? dots : digits)++;
        if (dots > 1 || digits == 0) { fail("malformed number '" + lit + "'"); return false; }
        if (j < s.size() && is_alpha(s[j])) { fail("malformed number '" + lit + s[j] + "…' (govaluate reads digits and '.' only)"); return false; }
        i = j;
        *out = strtod(lit.c_str(), nullptr);
        return true;
    }
    // a quoted literal at the cursor → str_lit.  govaluate tries every string as a date first; [A-Za-z_][A-Za-z0-9_]* never is one
    bool string_lit() {
        const char quote = s[i];
        const size_t close = s.find(quote, i + 1);
        if (close == std::string::npos) { fail("unterminated string literal"); return false; }
        const std::string text = s.substr(i + 1, close - i - 1);
        bool shape = !text.empty() && is_alpha(text[0]);
        for (char ch : text) shape = shape && (is_alpha(ch) || is_digit(ch));
        if (!shape) {
            fail("the string literal " + std::string(1, quote) + text.substr(0, 60) + quote + " is not in the served subset (a recall name [A-Za-z_][A-Za-z0-9_]*: "
                 "govaluate tries every other string as a date)");
            return false;
        }
        i = close + 1;
        str_lit = text;
        return true;
    }
    uint32_t recall_bit(const std::string& name) const {      // a literal that names no recall equals no source
        for (size_t r = 0; r < set->recall_names.size(); ++r)
            if (set->recall_names[r] == name) return 1u << r;
        return 0u;
    }
    CcType value() {
        ws();
        if (i >= s.size()) return fail("unexpected end of the expression");
        if (++nest > 64) return fail("nesting deeper than 64");
        const CcType t = value_inner();
        --nest;
        return t;
    }
    CcType value_inner() {
        const char c = s[i];
        if (c == '(') {
            ++i;
            const CcType t = or_();
            if (t == T_FAIL) return t;
            ws();
            if (i < s.size() && s[i] == ',') return fail("',' (an array) anywhere but behind \"in\" is not in the served subset");
            if (i >= s.size() || s[i] != ')') return unexpected("missing ')'");
            ++i;
            return t;
        }
        if (is_digit(c) || c == '.') {
            double v;
            if (!number(&v)) return T_FAIL;
            push(OP_CONST, 0, v);
            return T_NUM;
        }
        if (c == '[') {
            const size_t close = s.find(']', i + 1);
            if (close == std::string::npos || close == i + 1) return fail("unterminated or empty [name]");
            const std::string name = s.substr(i + 1, close - i - 1);
            i = close + 1;
            return name_ref(name);
        }
        if (c == '\'' || c == '"') return string_lit() ? T_STR : T_FAIL;
        if (is_alpha(c)) {
            size_t j = i;
            while (j < s.size() && (is_alpha(s[j]) || is_digit(s[j]) || s[j] == '.')) ++j;
            const std::string name = s.substr(i, j - i);
            if (name.find('.') != std::string::npos) return fail("the accessor \"" + name + "\" is not in the served subset");
            if (name == "true" || name == "false") return fail("the boolean literal \"" + name + "\" is not in the served subset");
            if (name == "in" || name == "IN") return fail("the comparator \"in\" without a left-hand side");
            i = j;
            ws();
            if (i < s.size() && s[i] == '(') {
                if (name != "round") return fail("the function \"" + name + "\" is not in the served subset (functions: round)");
                ++i;
                if (!num(add(), "round")) return T_FAIL;
                ws();
                if (i < s.size() && s[i] == ',') {
                    ++i;
                    if (!num(add(), "round")) return T_FAIL;
                    ws();
                    if (i < s.size() && s[i] == ',') return fail("round: wrong number of arguments");
                    if (i >= s.size() || s[i] != ')') return unexpected("round: missing ')'");
                    ++i;
                    push(OP_ROUND2, 0, 0.0);
                    return T_NUM;
                }
                if (i >= s.size() || s[i] != ')') return unexpected("round: missing ')'");
                ++i;
                push(OP_ROUND, 0, 0.0);
                return T_NUM;
            }
            if (name == "round") return fail("the function \"round\" needs its argument list");
            return name_ref(name);
        }
        return unexpected("unexpected");
    }
    CcType prefix() {
        ws();
        const bool minus = i < s.size() && s[i] == '-';
        const bool bang = i < s.size() && s[i] == '!' && !(i + 1 < s.size() && (s[i + 1] == '=' || s[i + 1] == '~'));
        if (!minus && !bang) return value();
        ++i;
        if (++nest > 64) return fail("nesting deeper than 64");
        const CcType t = prefix();
        --nest;
        if (minus) {
            if (!num(t, "unary '-'")) return T_FAIL;
            push(OP_NEG, 0, 0.0);
            return T_NUM;
        }
        if (!boolean(t, "'!'")) return T_FAIL;
        push(OP_NOT, 0, 0.0);
        return T_BOOL;
    }
    CcType power() {
        const CcType t = prefix();
        if (t == T_FAIL || !at("**")) return t;
        if (!num(t, "'**'")) return T_FAIL;
        i += 2;
        if (!num(prefix(), "'**'")) return T_FAIL;
        push(OP_POW, 0, 0.0);
        if (at("**")) return fail("a chained '**' is not in the served subset (write the parentheses)");
        return T_NUM;
    }
    CcType mul() {
        CcType t = power();
        for (;;) {
            if (t == T_FAIL) return t;
            ws();
            if (i >= s.size() || (s[i] != '*' && s[i] != '/' && s[i] != '%')) return t;
            const char op = s[i];
            const char where[4] = {'\'', op, '\'', 0};
            if (!num(t, where)) return T_FAIL;
            ++i;
            if (!num(power(), where)) return T_FAIL;
            push(op == '*' ? OP_MUL : op == '/' ? OP_DIVF : OP_FMOD, 0, 0.0);
            t = T_NUM;
        }
    }
    CcType add() {
        CcType t = mul();
        for (;;) {
            if (t == T_FAIL) return t;
            ws();
            if (i >= s.size() || (s[i] != '+' && s[i] != '-')) return t;
            const char op = s[i];
            const char where[4] = {'\'', op, '\'', 0};
            if (!num(t, where)) return T_FAIL;
            ++i;
            if (!num(mul(), where)) return T_FAIL;
            push(op == '+' ? OP_ADD : OP_SUB, 0, 0.0);
            t = T_NUM;
        }
    }
    // behind "in": ( literal, literal, … ) of two or more constants; strings: recall names → *mask, numbers → the list table
    bool in_list(bool strings, uint32_t* mask, uint32_t* arg) {
        ws();
        if (i >= s.size() || s[i] != '(') { fail("\"in\" takes a parenthesised list of constants"); return false; }
        ++i;
        std::vector<double> vals;
        uint32_t m = 0, n = 0;
        for (;;) {
            ws();
            if (i >= s.size()) { fail("\"in\": unterminated list"); return false; }
            if (strings) {
                if (s[i] != '\'' && s[i] != '"') { fail("recall_name in (…) takes string literals"); return false; }
                if (!string_lit()) return false;
                m |= recall_bit(str_lit);
            } else {
                const bool neg = s[i] == '-';
                if (neg) { ++i; ws(); }
                if (i >= s.size() || !(is_digit(s[i]) || s[i] == '.')) { fail("\"in\" takes a list of constant numbers"); return false; }
                double v;
                if (!number(&v)) return false;
                vals.push_back(neg ? -v : v);
            }
            ++n;
            ws();
            if (i < s.size() && s[i] == ',') { ++i; continue; }
            if (i < s.size() && s[i] == ')') { ++i; break; }
            if (i >= s.size()) { fail("\"in\": unterminated list"); return false; }
            fail("\"in\" takes a list of constants");
            return false;
        }
        if (n < 2) { fail("a one-element \"in\" list (govaluate makes no array of one parenthesised value and errors on every item)"); return false; }
        if (n > kCcMaxList) { fail("an \"in\" list of " + std::to_string(n) + " values (at most " + std::to_string(kCcMaxList) + ")"); return false; }
        if (strings) {
            *mask = m;
            return true;
        }
        if (set->lists.size() + n > kCcMaxListTotal) { fail("more than " + std::to_string(kCcMaxListTotal) + " \"in\" values in one set"); return false; }
        *arg = (uint32_t)set->lists.size() | (n << 16);
        set->lists.insert(set->lists.end(), vals.begin(), vals.end());
        return true;
    }
    CcType cmp() {
        CcType t = add();
        for (;;) {
            if (t == T_FAIL) return t;
            ws();
            if (at("<<") || at(">>") || at("=~") || at("!~")) return unexpected("unexpected");
            if (at_word("in") || at_word("IN")) {
                i += 2;
                if (t == T_NAME) {
                    uint32_t mask = 0;
                    if (!in_list(true, &mask, nullptr)) return T_FAIL;
                    set->reads_source = true;
                    push(OP_SRC, mask, 0.0);
                } else {
                    if (!num(t, "\"in\"")) return T_FAIL;
                    uint32_t arg = 0;
                    if (!in_list(false, nullptr, &arg)) return T_FAIL;
                    push(OP_IN, arg, 0.0);
                }
                t = T_BOOL;
                continue;
            }
            uint32_t op;
            const char* text;
            if (at("==")) op = OP_EQ, text = "'=='";
            else if (at("!=")) op = OP_NE, text = "'!='";
            else if (at(">=")) op = OP_GE, text = "'>='";
            else if (at("<=")) op = OP_LE, text = "'<='";
            else if (at(">")) op = OP_GT, text = "'>'";
            else if (at("<")) op = OP_LT, text = "'<'";
            else return t;
            const bool equality = op == OP_EQ || op == OP_NE;
            if (t == T_BOOL && equality) return fail(std::string(text) + " between bools is not in the served subset");
            if (t == T_NAME && equality) {
                i += 2;
                const CcType r = add();
                if (r == T_FAIL) return r;
                if (r != T_STR) return fail("recall_name compares with a string literal only");
                set->reads_source = true;
                push(OP_SRC, recall_bit(str_lit), 0.0);
                if (op == OP_NE) push(OP_NOT, 0, 0.0);
                t = T_BOOL;
                continue;
            }
            if (!num(t, text)) return T_FAIL;
            i += strlen(text) - 2;
            const CcType r = add();
            if (r == T_BOOL && equality) return fail(std::string(text) + " between bools is not in the served subset");
            if (!num(r, text)) return T_FAIL;
            push(op, 0, 0.0);
            t = T_BOOL;
        }
    }
    CcType and_() {
        CcType t = cmp();
        for (;;) {
            if (t == T_FAIL || !at("&&")) return t;
            if (!boolean(t, "'&&'")) return T_FAIL;
            i += 2;
            if (!boolean(cmp(), "'&&'")) return T_FAIL;
            push(OP_AND, 0, 0.0);
        }
    }
    CcType or_() {
        CcType t = and_();
        for (;;) {
            if (t == T_FAIL || !at("||")) return t;
            if (!boolean(t, "'||'")) return T_FAIL;
            i += 2;
            if (!boolean(and_(), "'||'")) return T_FAIL;
            push(OP_OR, 0, 0.0);
        }
    }
    // the whole expression: a bool
    bool top() {
        const CcType t = or_();
        if (t == T_FAIL) return false;
        ws();
        if (i != s.size()) { unexpected("unexpected"); return false; }
        if (t == T_NUM) { fail("the expression is a number, not a bool (the reference keeps an item only for `true`)"); return false; }
        return boolean(t, "the whole expression");
    }
};

int cc_refuse(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int cc_refuse(int code, const char* fmt, ...) {
    char buf[768];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    set_error("pg_classcut_compile: %s", buf);
    return code;
}

int classcut_compile(const pg_classcut_rule* rules, uint32_t n, const pg_cond_col* cols, uint32_t n_cols, const char* const* recall_names,
                     uint32_t n_recalls, pg_classcut* c) {
    if (!rules || n < 1) return cc_refuse(PG_ERR_INVALID, "no classes (the reference indexes configs[len - 1])");
    if (n > kCcMaxClasses) return cc_refuse(PG_ERR_UNSUPPORTED, "%u classes (at most %u)", n, kCcMaxClasses);
    if (n_cols && !cols) return cc_refuse(PG_ERR_INVALID, "NULL column declarations");
    if (n_cols > 256) return cc_refuse(PG_ERR_UNSUPPORTED, "%u declared columns (at most 256)", n_cols);
    for (uint32_t d = 0; d < n_cols; ++d) {
        if (!cols[d].name || !cols[d].name[0]) return cc_refuse(PG_ERR_INVALID, "declared column %u has no name", d);
        if (cols[d].dtype < PG_F_I32 || cols[d].dtype > PG_F_F64) return cc_refuse(PG_ERR_INVALID, "declared column \"%s\" has unknown dtype %d", cols[d].name, cols[d].dtype);
        if (!strcmp(cols[d].name, "recall_name") || !strcmp(cols[d].name, "recall_score"))
            return cc_refuse(PG_ERR_INVALID, "declared column \"%s\" hides the built-in of that name", cols[d].name);
        for (uint32_t e = 0; e < d; ++e)
            if (!strcmp(cols[e].name, cols[d].name)) return cc_refuse(PG_ERR_INVALID, "column \"%s\" is declared twice", cols[d].name);
        c->col_names.push_back(cols[d].name);
        c->col_dtypes.push_back(cols[d].dtype);
    }
    if (n_recalls && !recall_names) return cc_refuse(PG_ERR_INVALID, "NULL recall names");
    if (n_recalls > kCcMaxRecalls) return cc_refuse(PG_ERR_UNSUPPORTED, "%u recall names (at most %u)", n_recalls, kCcMaxRecalls);
    for (uint32_t r = 0; r < n_recalls; ++r) {
        if (!recall_names[r]) return cc_refuse(PG_ERR_INVALID, "recall name %u is NULL", r);
        c->recall_names.push_back(recall_names[r]);
    }
    for (uint32_t r = 0; r < n; ++r) {
        const pg_classcut_rule& ru = rules[r];
        if (ru.type != PG_TRIM_FIX && ru.type != PG_TRIM_ACCUMULATE)
            return cc_refuse(PG_ERR_INVALID, "class %u has type %u (PG_TRIM_FIX or PG_TRIM_ACCUMULATE)", r, ru.type);
        if (r > 0 && ru.type == PG_TRIM_ACCUMULATE && rules[r - 1].type == PG_TRIM_ACCUMULATE && ru.count < rules[r - 1].count)
            return cc_refuse(PG_ERR_INVALID, "class %u accumulates to %u directly after a class that accumulates to %u (the reference panics in its "
                             "constructor)", r, ru.count, rules[r - 1].count);
        if (!ru.expression) return cc_refuse(PG_ERR_INVALID, "class %u has no expression", r);
        const std::string src = ru.expression;
        CcParser p(src, c, cols, n_cols);
        bool ok = src.size() <= 16384;
        if (!ok) p.fail("expression too large (" + std::to_string(src.size()) + " bytes, at most 16384)");
        if (ok) ok = p.top();
        if (!ok)
            return cc_refuse(p.code, "class %u: %s at byte %zu of '%.200s' — the engine serves a typed boolean subset of govaluate (numbers, declared "
                             "columns, recall_score, recall_name ==/!=/in string literals, + - * / %% **, unary minus, round, == != > >= < <=, in over "
                             "constants, && || !, parentheses) and refuses the rest rather than evaluate it differently", r, p.err.c_str(), p.i, src.c_str());
        const size_t ops = c->progs.size() - p.prog0;
        if (ops > kCcMaxOps || (uint32_t)p.max_depth > kCcMaxDepth)
            return cc_refuse(PG_ERR_UNSUPPORTED, "class %u: expression '%.200s' has %zu operations at depth %d (at most %u at depth %u)", r, src.c_str(), ops,
                             p.max_depth, kCcMaxOps, kCcMaxDepth);
        c->rules.push_back(CcRule{(uint16_t)p.prog0, (uint16_t)ops});
        c->types.push_back(ru.type);
        c->counts.push_back(ru.count);
    }
    return PG_OK;
}

// out_cap = min(cap, the sum of the fix counts + the largest accumulator count): no request keeps more
uint32_t classcut_width(const pg_classcut* c, uint32_t cap) {
    uint64_t fix = 0, acc = 0;
    for (size_t r = 0; r < c->rules.size(); ++r) {
        if (c->types[r] == PG_TRIM_FIX) fix += c->counts[r];
        else acc = std::max<uint64_t>(acc, c->counts[r]);
    }
    return (uint32_t)std::min<uint64_t>(cap, fix + acc);
}

void classcut_program(const pg_classcut* c, const void* const* declared_base, const double* lists, const Instr* progs, uint64_t store_rows,
                      CcProgram* p) {
    memset(p, 0, sizeof *p);
    for (size_t k = 0; k < c->used.size(); ++k)
        p->cols[k] = CondCol{declared_base ? declared_base[c->used[k]] : nullptr, c->col_dtypes[(size_t)c->used[k]], 0};
    std::copy(c->rules.begin(), c->rules.end(), p->rules);
    p->lists = lists;
    p->progs = progs;
    p->n_used = (uint32_t)c->used.size();
    p->n_classes = (uint32_t)c->rules.size();
    p->store_rows = store_rows;
}

int classcut_host_check(const pg_classcut* c, const void* const* cols, const void* source, const char* who) {
    for (int d : c->used)
        if (!cols || !cols[d]) {
            set_error("%s: the values of column \"%s\" are missing", who, c->col_names[(size_t)d].c_str());
            return PG_ERR_INVALID;
        }
    PG_REQUIRE(source || !c->reads_source, "%s: an expression reads recall_name: source is needed", who);
    return PG_OK;
}

// binds the set to a store by name and makes sure its table is on the context's device; caller holds ctx->mu
int classcut_bind_locked(pg_ctx* ctx, pg_classcut* c, const pg_features* fs, const char* who, CcProgram* p) {
    std::vector<const void*> declared;
    int rc;
    if (!fs && !c->used.empty()) {
        set_error("%s: the set reads column \"%s\": a feature store is needed", who, c->col_names[(size_t)c->used[0]].c_str());
        return PG_ERR_INVALID;
    }
    if (fs && (rc = cond_resolve_columns(fs, c->col_names, c->col_dtypes, c->used, who, &declared))) return rc;
    if ((rc = c->table.ensure(ctx, who, {{c->lists.data(), c->lists.size() * 8}, {c->progs.data(), c->progs.size() * sizeof(Instr)}}))) return rc;
    classcut_program(c, declared.data(), c->table.part<double>(0), c->table.part<Instr>(1), fs ? fs->rows : 0, p);
    return PG_OK;
}

int classcut_masks_locked(pg_ctx* ctx, pg_classcut* c, const pg_features* fs, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                          const double* d_score, const uint8_t* d_source, const uint32_t* d_count, uint8_t* d_out, const char* who) {
    CcProgram p;
    int rc;
    if ((rc = classcut_bind_locked(ctx, c, fs, who, &p))) return rc;
    classcut_masks_kernel<<<dim3((cap + kCcMaskThreads - 1) / kCcMaskThreads, nq), kCcMaskThreads, 0, ctx->stream>>>(
        p, d_rows, reinterpret_cast<const unsigned long long*>(d_score), d_source, d_count, cap, d_out);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// the masks, the score sort and the cut on the context's stream; caller holds ctx->mu and has checked the arguments
int candidates_classcut_locked(pg_ctx* ctx, pg_classcut* c, const pg_features* fs, const CandIn& in, const CandOut& out, const char* who) {
    const uint32_t nq = in.nq, cap = in.cap;
    int rc;
    if (out.out_cap == 0) {                      // every count is 0: nothing is kept, nothing but the counts is written
        PG_HIP(hipMemsetAsync(out.count, 0, (size_t)nq * 4, ctx->stream));
        return PG_OK;
    }
    uint32_t *d_off, *d_ord;
    uint8_t* d_masks;
    if ((rc = scratch_carve(ctx, kSlotClasscut, [&](Carve& s) {
            d_off = s.take<uint32_t>((size_t)nq + 1);
            d_ord = s.take<uint32_t>((size_t)nq * cap);
            d_masks = s.take<uint8_t>((size_t)nq * cap);
        }))) return rc;
    if ((rc = classcut_masks_locked(ctx, c, fs, nq, cap, in.rows, reinterpret_cast<const double*>(in.score), in.source, in.count, d_masks, who))) return rc;
    if ((rc = uniform_offsets_locked(ctx, nq, cap, d_off))) return rc;
    // (what the sort makes of padding does not matter: padding is a member of no class wherever it lies in the order)
    if ((rc = sort_dev_locked(ctx, reinterpret_cast<const double*>(in.score), d_off, nq, nq * cap, cap, 1, d_ord))) return rc;
    CutArgs a{};
    a.in = in;
    a.out = out;
    a.order = d_ord;
    a.masks = d_masks;
    a.n_classes = (uint32_t)c->rules.size();
    for (size_t r = 0; r < c->rules.size(); ++r) {
        a.r_count[r] = c->counts[r];
        a.r_type[r] = c->types[r];
    }
    candidates_classcut_kernel<<<nq, kCcChunk, 0, ctx->stream>>>(a);
    PG_HIP(hipGetLastError());
    return PG_OK;
}

// one request of pg_candidates_classcut_host: masks [cap] → the input positions kept, in output order
void classcut_request_host(const pg_classcut* c, uint32_t cap, const uint64_t* rows, const double* score, uint32_t n_valid, const uint8_t* masks,
                           std::vector<uint32_t>* out) {
    out->clear();
    std::vector<uint32_t> real;
    for (uint32_t p = 0; p < n_valid && p < cap; ++p)
        if (rows[p] != kCandPad) real.push_back(p);
    std::stable_sort(real.begin(), real.end(), [&](uint32_t x, uint32_t y) { return cand_before(score[x], score[y]); });
    std::vector<uint8_t> taken(cap, 0);
    uint64_t acc = 0;
    for (size_t r = 0; r < c->rules.size(); ++r) {
        const uint64_t cnt = c->counts[r];
        const bool fix = c->types[r] == PG_TRIM_FIX;
        const uint64_t limit = fix ? cnt : (cnt > acc ? cnt - acc : 0);
        uint64_t rank = 0;
        for (size_t k = 0; k < real.size() && rank < limit; ++k) {
            const uint32_t p = real[k];
            if (!((masks[p] >> r) & 1u)) continue;
            ++rank;                                  // (a place in the window, taken already or not)
            if (taken[p]) continue;
            taken[p] = 1;
            out->push_back(p);
            if (!fix) ++acc;
        }
    }
}

}  // namespace
}  // namespace pg

extern "C" {

int pg_classcut_compile(const pg_classcut_rule* rules, uint32_t n, const pg_cond_col* cols, uint32_t n_cols, const char* const* recall_names,
                        uint32_t n_recalls, pg_classcut** out) {
    PG_REQUIRE(out, "pg_classcut_compile: NULL argument");
    std::unique_ptr<pg_classcut> c(new pg_classcut());
    const int rc = pg::classcut_compile(rules, n, cols, n_cols, recall_names, n_recalls, c.get());
    if (rc) return rc;
    *out = c.release();
    return PG_OK;
}

int pg_classcut_free(pg_classcut* c) {
    if (!c) return PG_OK;
    c->table.release();
    delete c;
    return PG_OK;
}

int pg_classcut_num_classes(const pg_classcut* c) { return c ? (int)c->rules.size() : 0; }
int pg_classcut_reads_recall_name(const pg_classcut* c) { return c && c->reads_source ? 1 : 0; }

int pg_classcut_out_cap(const pg_classcut* c, uint32_t cap, uint32_t* out_cap) {
    PG_REQUIRE(c && out_cap, "pg_classcut_out_cap: NULL argument");
    if (cap < 1 || cap > pg::kCandMaxCap) {
        pg::set_error("pg_classcut_out_cap: cap=%u unsupported (1..%u)", cap, pg::kCandMaxCap);
        return PG_ERR_UNSUPPORTED;
    }
    *out_cap = pg::classcut_width(c, cap);
    return PG_OK;
}

int pg_classcut_masks_host(const pg_classcut* c, uint32_t n, const uint8_t* item_in, const void* const* cols, const uint8_t* source,
                           const double* score, uint8_t* out_masks) {
    PG_REQUIRE(c && (n == 0 || (score && out_masks)), "pg_classcut_masks_host: NULL argument");
    int rc;
    if (n && (rc = pg::classcut_host_check(c, cols, source, "pg_classcut_masks_host"))) return rc;
    pg::CcProgram p;
    pg::classcut_program(c, nullptr, c->lists.data(), c->progs.data(), 0, &p);
    for (uint32_t i = 0; i < n; ++i) {
        pg::CondItem it;
        pg::cond_host_item(c->used, c->col_dtypes, cols, item_in, i, &it);
        out_masks[i] = (uint8_t)pg::cc_classes(p, it, score[i], source ? (uint32_t)source[i] : 0xFFu);
    }
    return PG_OK;
}

int pg_candidates_classcut_host(const pg_classcut* c, uint32_t nq, uint32_t cap, const uint8_t* item_in, const void* const* cols,
                                const uint64_t* rows, const double* score, const uint8_t* source, const uint32_t* count,
                                const double* planes_f64, uint32_t n_f64, const uint32_t* source_mask, const float* planes_f32, uint32_t n_f32,
                                uint64_t* out_rows, double* out_score, uint8_t* out_source, double* out_planes_f64, uint32_t* out_source_mask,
                                float* out_planes_f32, uint32_t* out_count) {
    const char* who = "pg_candidates_classcut_host";
    PG_REQUIRE(c && rows && score && out_count, "%s: NULL argument", who);
    int rc;
    if ((rc = pg::cond_check_shape(nq, cap, who))) return rc;
    const uint32_t out_cap = pg::classcut_width(c, cap);
    PG_REQUIRE(out_cap == 0 || (out_rows && out_score), "%s: NULL argument", who);
    const pg::CandCall l{rows, score, source, count, planes_f64, n_f64, source_mask, planes_f32, n_f32, out_rows, out_score,
                         out_source, out_planes_f64, out_source_mask, out_planes_f32, out_count};
    if ((rc = pg::cand_lists_check(l, pg::kCandMaxPlanes, who)) || (rc = pg::classcut_host_check(c, cols, source, who))) return rc;
    pg::CandIn in;
    pg::CandOut out;
    pg::cand_lists_bind(l, nq, cap, out_cap, &in, &out);
    pg::CcProgram p;
    pg::classcut_program(c, nullptr, c->lists.data(), c->progs.data(), 0, &p);
    std::vector<uint8_t> masks(cap);
    std::vector<uint32_t> picks;
    for (uint32_t q = 0; q < nq; ++q) {
        const size_t in0 = (size_t)q * cap, out0 = (size_t)q * out_cap;
        const uint32_t n_valid = pg::cand_n_valid(in, q);
        for (uint32_t pos = 0; pos < cap; ++pos) {
            uint32_t m = 0;
            if (pos < n_valid && rows[in0 + pos] != pg::kCandPad) {
                pg::CondItem it;
                pg::cond_host_item(c->used, c->col_dtypes, cols, item_in, in0 + pos, &it);
                m = pg::cc_classes(p, it, score[in0 + pos], source ? (uint32_t)source[in0 + pos] : 0xFFu);
            }
            masks[pos] = (uint8_t)m;
        }
        pg::classcut_request_host(c, cap, rows + in0, score + in0, n_valid, masks.data(), &picks);
        const uint32_t n = (uint32_t)std::min<size_t>(picks.size(), out_cap);
        for (uint32_t j = 0; j < n; ++j) pg::cand_carry(in, out, in0 + picks[j], out0 + j, true);
        pg::cand_pad(in, out, q, n, 1, pg::kCandNegInf);
        out_count[q] = n;
    }
    return PG_OK;
}

int pg_classcut_masks_dev(pg_ctx* ctx, pg_classcut* c, const pg_features* fs, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                          const double* d_score, const uint8_t* d_source, const uint32_t* d_count, uint8_t* d_out_masks) {
    const char* who = "pg_classcut_masks_dev";
    PG_REQUIRE(ctx && c && d_rows && d_score && d_out_masks, "%s: NULL argument", who);
    int rc;
    if ((rc = pg::cond_check_shape(nq, cap, who))) return rc;
    PG_REQUIRE(d_source || !c->reads_source, "%s: an expression reads recall_name: d_source is needed", who);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::classcut_masks_locked(ctx, c, fs, nq, cap, d_rows, d_score, d_source, d_count, d_out_masks, who);
}

int pg_candidates_classcut_dev(pg_ctx* ctx, pg_classcut* c, const pg_features* fs, uint32_t nq, uint32_t cap, const uint64_t* d_rows,
                               const double* d_score, const uint8_t* d_source, const uint32_t* d_count, const double* d_planes_f64,
                               uint32_t n_f64, const uint32_t* d_source_mask, const float* d_planes_f32, uint32_t n_f32, uint64_t* d_out_rows,
                               double* d_out_score, uint8_t* d_out_source, double* d_out_planes_f64, uint32_t* d_out_source_mask,
                               float* d_out_planes_f32, uint32_t* d_out_count) {
    const char* who = "pg_candidates_classcut_dev";
    const pg::CandCall l{d_rows, d_score, d_source, d_count, d_planes_f64, n_f64, d_source_mask, d_planes_f32, n_f32, d_out_rows, d_out_score,
                         d_out_source, d_out_planes_f64, d_out_source_mask, d_out_planes_f32, d_out_count};
    int rc;
    if ((rc = pg::cand_call_required(l, ctx && c, who)) || (rc = pg::cond_check_shape(nq, cap, who))) return rc;
    PG_REQUIRE(d_source || !c->reads_source, "%s: an expression reads recall_name: d_source is needed", who);
    const uint32_t out_cap = pg::classcut_width(c, cap);
    if ((rc = pg::cand_lists_check(l, pg::kCandMaxPlanes, who)) || (rc = pg::cand_call_apart(l, nq, cap, out_cap, who))) return rc;
    pg::CandIn in;
    pg::CandOut out;
    pg::cand_lists_bind(l, nq, cap, out_cap, &in, &out);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    return pg::candidates_classcut_locked(ctx, c, fs, in, out, who);
}

// ---- one request on host arrays (staged_run, cand_lists.hpp) ---------------------------------------------------------------------
int pg_candidates_classcut(pg_ctx* ctx, pg_classcut* c, const pg_features* fs, uint32_t n, const uint64_t* rows, const double* score,
                           const uint8_t* source, uint64_t* out_rows, double* out_score, uint8_t* out_source, uint32_t* out_count) {
    const char* who = "pg_candidates_classcut";
    PG_REQUIRE(ctx && c && out_count && (n == 0 || (rows && score)), "%s: NULL argument", who);
    PG_REQUIRE(!source == !out_source, "%s: source and out_source come in pairs", who);
    int rc;
    if (n == 0) {                                    // an empty request: an empty answer
        *out_count = 0;
        return PG_OK;
    }
    PG_REQUIRE(source || !c->reads_source, "%s: an expression reads recall_name: source is needed", who);
    if ((rc = pg::cond_check_shape(1, n, who))) return rc;
    const uint32_t out_cap = pg::classcut_width(c, n);
    if (out_cap == 0) {                              // every count is 0
        *out_count = 0;
        return PG_OK;
    }
    PG_REQUIRE(out_rows && out_score, "%s: NULL argument", who);
    std::lock_guard<std::mutex> g(ctx->mu);
    PG_HIP(hipSetDevice(ctx->device));
    using pg::Staged;
    enum { kRows, kScore, kOutRows, kOutScore, kSource, kOutSource, kCount };
    Staged st[] = {{rows, (size_t)n * 8, Staged::kIn},
                   {score, (size_t)n * 8, Staged::kIn},
                   {out_rows, (size_t)out_cap * 8, Staged::kOut},
                   {out_score, (size_t)out_cap * 8, Staged::kOut},
                   {source, n, Staged::in_if(source)},
                   {out_source, out_cap, Staged::out_if(source)},
                   {out_count, 4, Staged::kOut}};
    return pg::staged_run(ctx, pg::kSlotStaging, st, sizeof st / sizeof *st, false, [&] {
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
        out.out_cap = out_cap;
        return pg::candidates_classcut_locked(ctx, c, fs, in, out, who);
    });
}

}  // extern "C"
