// Compound WhereClauses: `pg_where`, a predicate over the integer columns of a feature store, compiled on the
// host from the SQL text a Hologres recall carries (HologresVectorConf.WhereClause, recconf.go:492-497) and evaluated on the
// device into a row bitmap that every consumer of a RowFilter reads (recall.hip, recall_filter.hip, index_where.hip).
//
//   expr  := and ( OR and )*
//   and   := unary ( AND unary )*
//   unary := NOT unary | '(' expr ')' | term
//   term  := column OP integer | column [NOT] IN '(' integer ( ',' integer )* ')' | column [NOT] BETWEEN integer AND integer
//
// The compiled program has no NOT and no evaluation stack to speak of.  Two-valued logic lets the compiler push every NOT into
// the terms (De Morgan; a term carries a `negated` flag), every comparison and BETWEEN is one inclusive range [lo, hi], and the
// AND / OR tree is emitted in postfix with the operand that needs the deeper stack first (Sethi-Ullman): 64 terms never need
// more than 7 levels.  A lane of the kernel owns 4 consecutive rows, a term's value is 4 bits, and the whole stack is ONE 32-bit
// register shifted by a nibble per push or pop: nothing is indexed dynamically, nothing spills.
#include "common.hpp"

#include <algorithm>
#include <climits>
#include <cstdarg>

namespace pg {
namespace {

constexpr uint32_t kMaxCols = 16, kMaxTerms = 64, kMaxIn = 1024, kMaxDepth = 64;
constexpr uint32_t kStackLevels = 8;               // nibbles of the kernel's stack register
constexpr uint32_t kTermNeg = 1u, kTermIn = 2u;
constexpr uint32_t kOpAnd = 64u, kOpOr = 65u;      // an op below kMaxTerms pushes that term
constexpr uint32_t kWhereBlockRows = 1024;

// a term of the program: v in [lo, hi], or v among in_vals[in_off, in_off + in_n) (sorted, distinct; lo / hi its ends); kTermNeg inverts
struct WhereTerm {
    long long lo, hi;
    uint32_t col, flags, in_off, in_n;
};
static_assert(sizeof(WhereTerm) == 32, "read as two 16-B scalar loads");

std::atomic<uint64_t> g_where_epoch{0};            // a bitmap build's epoch: process-wide, never reused (a cache key)

}  // namespace

// a bitmap built for one binding of a pg_where (a store's columns at their versions, a row count, a device); the callers that
// search with it hold a reference until their stream has synchronised, so a rebuild never frees it under a search
struct WhereBits {
    const pg_features* fs = nullptr;
    int device = -1;
    uint64_t rows = 0;
    std::vector<int> cols;
    std::vector<uint64_t> versions;
    void* d = nullptr;                   // the program (column pointers, terms, IN constants, ops, the count) and the bitmap
    uint32_t* bits = nullptr;            // [(rows + 31) / 32]
    uint64_t admitted = 0, epoch = 0;
    size_t bytes = 0;
    ~WhereBits() { if (d) (void)hipFree(d); }
};

}  // namespace pg

struct pg_where {
    std::vector<std::string> col_names;              // distinct, in order of first appearance
    std::vector<pg::WhereTerm> terms;                // sorted by column: the kernel loads a column once for all its terms
    std::vector<long long> in_vals;
    std::vector<uint32_t> ops;                       // postfix
    bool simple = false;                             // the clause is one plain comparison: served as RowFilter's single-column form
    int simple_op = 0;
    long long simple_val = 0;
    mutable std::mutex mu;                           // serialises the builds; guards cur and st
    mutable std::shared_ptr<pg::WhereBits> cur;
    mutable pg_where_stats_t st{};
};

namespace pg {
namespace {

// ---- the compiler --------------------------------------------------------------------------------------------------
enum Tok { T_END, T_IDENT, T_INT, T_OP, T_LP, T_RP, T_COMMA, T_AND, T_OR, T_NOT, T_IN, T_BETWEEN, T_BAD };
struct Node {
    int kind;          // 0 term (a = its index), 1 AND, 2 OR, 3 NOT (a only)
    int a, b;
};
struct RawTerm {
    uint32_t col;
    int kind;          // 0 comparison (op, v0), 1 BETWEEN v0 AND v1, 2 IN (ins)
    int op;
    long long v0, v1;
    bool neg;
    std::vector<long long> ins;
};

struct Parser {
    const char* s;
    size_t n, pos = 0;
    Tok tok = T_END;
    size_t tpos = 0;
    std::string ident;
    long long ival = 0;
    int op = 0;
    uint32_t depth = 0;
    size_t in_total = 0;
    bool failed = false;
    std::vector<Node> nodes;
    std::vector<RawTerm> terms;
    std::vector<std::string> cols;

    int fail(size_t at, const char* fmt, ...) {
        if (!failed) {
            char msg[160];
            va_list ap;
            va_start(ap, fmt);
            vsnprintf(msg, sizeof msg, fmt, ap);
            va_end(ap);
            set_error("pg_where_compile: %s at position %zu", msg, at);
            failed = true;
        }
        return -1;
    }
    static bool is_alpha(char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; }
    static bool is_digit(char c) { return c >= '0' && c <= '9'; }
    void next() {
        while (pos < n && (s[pos] == ' ' || s[pos] == '\t' || s[pos] == '\n' || s[pos] == '\r')) ++pos;
        tpos = pos;
        if (pos >= n) { tok = T_END; return; }
        const char c = s[pos];
        if (is_alpha(c)) {
            size_t e = pos;
            while (e < n && (is_alpha(s[e]) || is_digit(s[e]))) ++e;
            ident.assign(s + pos, e - pos);
            pos = e;
            std::string lower = ident;
            for (char& ch : lower) if (ch >= 'A' && ch <= 'Z') ch = (char)(ch - 'A' + 'a');
            tok = lower == "and" ? T_AND : lower == "or" ? T_OR : lower == "not" ? T_NOT : lower == "in" ? T_IN : lower == "between" ? T_BETWEEN : T_IDENT;
            return;
        }
        if (is_digit(c) || ((c == '-' || c == '+') && pos + 1 < n && is_digit(s[pos + 1]))) {
            const bool neg = c == '-';
            size_t e = pos + (is_digit(c) ? 0 : 1);
            const unsigned long long limit = neg ? (unsigned long long)LLONG_MAX + 1ull : (unsigned long long)LLONG_MAX;
            unsigned long long v = 0;
            for (; e < n && is_digit(s[e]); ++e) {
                const unsigned d = (unsigned)(s[e] - '0');
                if (v > (limit - d) / 10) {
                    fail(pos, "integer does not fit 64 bits");
                    tok = T_BAD;
                    return;
                }
                v = v * 10 + d;
            }
            ival = neg ? (long long)(0ull - v) : (long long)v;
            pos = e;
            tok = T_INT;
            return;
        }
        const char c1 = pos + 1 < n ? s[pos + 1] : '\0';
        tok = T_OP;
        if (c == '>') { op = c1 == '=' ? PG_WHERE_GE : PG_WHERE_GT; pos += c1 == '=' ? 2 : 1; return; }
        if (c == '<') { op = c1 == '=' ? PG_WHERE_LE : c1 == '>' ? PG_WHERE_NE : PG_WHERE_LT; pos += (c1 == '=' || c1 == '>') ? 2 : 1; return; }
        if (c == '=') { op = PG_WHERE_EQ; pos += c1 == '=' ? 2 : 1; return; }
        if (c == '!' && c1 == '=') { op = PG_WHERE_NE; pos += 2; return; }
        if (c == '(') { tok = T_LP; ++pos; return; }
        if (c == ')') { tok = T_RP; ++pos; return; }
        if (c == ',') { tok = T_COMMA; ++pos; return; }
        fail(pos, "unexpected character '%c'", c);
        tok = T_BAD;
    }
    int mk(int kind, int a, int b) {
        nodes.push_back(Node{kind, a, b});
        return (int)nodes.size() - 1;
    }
    int want_int(long long* out, const char* what) {
        if (tok != T_INT) return fail(tpos, "expected an integer %s", what);
        *out = ival;
        next();
        return 0;
    }
    int term() {
        if (tok != T_IDENT) return fail(tpos, tok == T_END ? "the clause ends where a term is expected" : "expected a column name");
        uint32_t col = 0;
        for (; col < cols.size() && cols[col] != ident; ++col) {}
        if (col == cols.size()) {
            if (cols.size() == kMaxCols) return fail(tpos, "more than %u distinct columns", kMaxCols);
            cols.push_back(ident);
        }
        if (terms.size() == kMaxTerms) return fail(tpos, "more than %u terms", kMaxTerms);
        RawTerm t{col, 0, 0, 0, 0, false, {}};
        next();
        if (tok == T_OP) {
            t.op = op;
            next();
            if (want_int(&t.v0, "after the operator")) return -1;
        } else {
            if (tok == T_NOT) {
                t.neg = true;
                next();
                if (tok != T_IN && tok != T_BETWEEN) return fail(tpos, "expected IN or BETWEEN after NOT");
            }
            if (tok == T_BETWEEN) {
                t.kind = 1;
                next();
                if (want_int(&t.v0, "after BETWEEN")) return -1;
                if (tok != T_AND) return fail(tpos, "expected AND between the bounds of BETWEEN");
                next();
                if (want_int(&t.v1, "after BETWEEN ... AND")) return -1;
            } else if (tok == T_IN) {
                t.kind = 2;
                next();
                if (tok != T_LP) return fail(tpos, "expected '(' after IN");
                do {
                    next();
                    long long v;
                    const size_t at = tpos;
                    if (want_int(&v, "in the IN list")) return -1;
                    if (++in_total > kMaxIn) return fail(at, "more than %u IN constants", kMaxIn);
                    t.ins.push_back(v);
                } while (tok == T_COMMA);
                if (tok != T_RP) return fail(tpos, "expected ',' or ')' in the IN list");
                next();
            } else {
                return fail(tpos, "expected a comparison operator, IN or BETWEEN after the column");
            }
        }
        terms.push_back(std::move(t));
        return mk(0, (int)terms.size() - 1, -1);
    }
    // NOT and '(' recurse: the depth limit bounds the recursion however long the clause is
    int unary() {
        if (tok == T_NOT || tok == T_LP) {
            const bool paren = tok == T_LP;
            if (++depth > kMaxDepth) return fail(tpos, "nesting deeper than %u", kMaxDepth);
            next();
            int c = paren ? expr() : unary();
            if (c < 0) return -1;
            if (paren) {
                if (tok != T_RP) return fail(tpos, "expected ')'");
                next();
            } else {
                c = mk(3, c, -1);
            }
            --depth;
            return c;
        }
        return tok == T_BAD ? -1 : term();
    }
    int conj() {
        int l = unary();
        while (l >= 0 && tok == T_AND) {
            next();
            const int r = unary();
            if (r < 0) return -1;
            l = mk(1, l, r);
        }
        return l;
    }
    int expr() {
        int l = conj();
        while (l >= 0 && tok == T_OR) {
            next();
            const int r = conj();
            if (r < 0) return -1;
            l = mk(2, l, r);
        }
        return l;
    }
};

// NOT pushed into the terms: the tree below `node` under `neg` pending negations (the nodes are rewritten in place; every term
// has exactly one parent)
void push_not(Parser& p, int node, bool neg, int* out) {
    Node& nd = p.nodes[(size_t)node];
    if (nd.kind == 3) return push_not(p, nd.a, !neg, out);
    if (nd.kind == 0) {
        if (neg) p.terms[(size_t)nd.a].neg = !p.terms[(size_t)nd.a].neg;
        *out = node;
        return;
    }
    if (neg) nd.kind = 3 - nd.kind;       // AND <-> OR
    int a, b;
    push_not(p, nd.a, neg, &a);
    push_not(p, p.nodes[(size_t)node].b, neg, &b);
    p.nodes[(size_t)node].a = a;
    p.nodes[(size_t)node].b = b;
    *out = node;
}
uint32_t stack_need(const Parser& p, int node, std::vector<uint32_t>& need) {
    const Node& nd = p.nodes[(size_t)node];
    if (nd.kind == 0) return need[(size_t)node] = 1;
    const uint32_t a = stack_need(p, nd.a, need), b = stack_need(p, nd.b, need);
    return need[(size_t)node] = a == b ? a + 1 : std::max(a, b);
}
void emit(const Parser& p, int node, const std::vector<uint32_t>& need, std::vector<uint32_t>& ops) {
    const Node& nd = p.nodes[(size_t)node];
    if (nd.kind == 0) {
        ops.push_back((uint32_t)nd.a);
        return;
    }
    const bool a_first = need[(size_t)nd.a] >= need[(size_t)nd.b];       // (AND and OR commute: the deeper operand first)
    emit(p, a_first ? nd.a : nd.b, need, ops);
    emit(p, a_first ? nd.b : nd.a, need, ops);
    ops.push_back(nd.kind == 1 ? kOpAnd : kOpOr);
}

int compile(const char* clause, pg_where* w) {
    Parser p{clause, strlen(clause)};
    p.next();
    int root = p.tok == T_BAD ? -1 : p.expr();
    if (root >= 0 && p.tok != T_END) root = p.fail(p.tpos, p.tok == T_RP ? "unmatched ')'" : "unexpected text after the clause");
    if (root < 0) return PG_ERR_PARSE;
    push_not(p, root, false, &root);
    std::vector<uint32_t> need(p.nodes.size(), 0);
    if (stack_need(p, root, need) > kStackLevels) {      // (cannot happen with kMaxTerms = 64: at most 7)
        set_error("pg_where_compile: the clause needs more than %u stack levels at position 0", kStackLevels);
        return PG_ERR_PARSE;
    }
    emit(p, root, need, w->ops);
    // the terms in column order (stable), the pushes renumbered
    std::vector<uint32_t> order(p.terms.size()), where_of(p.terms.size());
    for (uint32_t i = 0; i < order.size(); ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return p.terms[a].col < p.terms[b].col; });
    for (uint32_t i = 0; i < order.size(); ++i) where_of[order[i]] = i;
    for (uint32_t& o : w->ops) if (o < kMaxTerms) o = where_of[o];
    for (uint32_t i : order) {
        RawTerm& r = p.terms[i];
        WhereTerm t{1, 0, r.col, r.neg ? kTermNeg : 0u, 0, 0};       // (lo > hi: the empty range)
        if (r.kind == 2) {
            std::sort(r.ins.begin(), r.ins.end());
            r.ins.erase(std::unique(r.ins.begin(), r.ins.end()), r.ins.end());
            t.flags |= kTermIn;
            t.in_off = (uint32_t)w->in_vals.size();
            t.in_n = (uint32_t)r.ins.size();
            t.lo = r.ins.front();
            t.hi = r.ins.back();
            w->in_vals.insert(w->in_vals.end(), r.ins.begin(), r.ins.end());
        } else if (r.kind == 1) {
            t.lo = r.v0;
            t.hi = r.v1;
        } else {
            switch (r.op) {
                case PG_WHERE_GT: if (r.v0 != LLONG_MAX) { t.lo = r.v0 + 1; t.hi = LLONG_MAX; } break;
                case PG_WHERE_GE: t.lo = r.v0; t.hi = LLONG_MAX; break;
                case PG_WHERE_LT: if (r.v0 != LLONG_MIN) { t.lo = LLONG_MIN; t.hi = r.v0 - 1; } break;
                case PG_WHERE_LE: t.lo = LLONG_MIN; t.hi = r.v0; break;
                default: t.lo = t.hi = r.v0; if (r.op == PG_WHERE_NE) t.flags ^= kTermNeg; break;
            }
        }
        w->terms.push_back(t);
    }
    w->col_names = std::move(p.cols);
    if (p.terms.size() == 1 && p.terms[0].kind == 0) {
        static const int flipped[6] = {PG_WHERE_LE, PG_WHERE_LT, PG_WHERE_GE, PG_WHERE_GT, PG_WHERE_NE, PG_WHERE_EQ};
        w->simple = true;
        w->simple_op = p.terms[0].neg ? flipped[p.terms[0].op] : p.terms[0].op;
        w->simple_val = p.terms[0].v0;
    }
    return PG_OK;
}

// ---- evaluation ------------------------------------------------------------------------------------------------------
__host__ __device__ inline bool term_pass(const WhereTerm& t, long long v, const long long* __restrict__ in_vals) {
    bool hit;
    if (t.flags & kTermIn) {
        // pos = how many constants are below v (a branch-free binary search: the trip count depends on the list alone)
        const long long* c = in_vals + t.in_off;
        uint32_t pos = 0, step = 1;
        while (step * 2 <= t.in_n) step *= 2;
        for (; step; step >>= 1) {
            const uint32_t np = pos + step;
            if (np <= t.in_n && c[np - 1] < v) pos = np;
        }
        hit = pos < t.in_n && c[pos] == v;
    } else {
        hit = v >= t.lo && v <= t.hi;
    }
    return hit != ((t.flags & kTermNeg) != 0);
}

// One lane per tile: rows r0 .. r0 + 3 (r0 a multiple of 4), a 16-B load of an int32 column or two of an int64 one.  A column is read once
// for all its terms (the terms come sorted by column); a term's 4 bits are parked in the lane's own LDS words (8 terms a word),
// where the postfix program picks them up.  The program and the terms are uniform: scalar loads, uniform branches.
__global__ __launch_bounds__(256) void where_eval_kernel(const void* const* __restrict__ cols, uint32_t is64, const WhereTerm* __restrict__ terms,
                                                         uint32_t n_terms, const long long* __restrict__ in_vals, const uint32_t* __restrict__ ops,
                                                         uint32_t n_ops, uint64_t rows, uint32_t* __restrict__ bits,
                                                         unsigned long long* __restrict__ count) {
    __shared__ uint32_t tm[kMaxTerms / 8][256];
    __shared__ uint32_t wn[4];
    const uint32_t tid = threadIdx.x;
    const uint64_t tiles = (rows + kWhereBlockRows - 1) / kWhereBlockRows;
    uint32_t n = 0;
    // a block walks tiles of 1024 rows (the trip count is uniform over the block: every lane reaches the shuffles) and adds
    // its count once, so the count's one address sees a few thousand atomics, not one per tile
    for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint64_t r0 = tile * kWhereBlockRows + tid * 4;
        const uint32_t valid = r0 + 4 <= rows ? 0xFu : r0 < rows ? (1u << (uint32_t)(rows - r0)) - 1u : 0u;
        long long v0 = 0, v1 = 0, v2 = 0, v3 = 0;
        uint32_t cur = ~0u, acc = 0;
        for (uint32_t j = 0; j < n_terms; ++j) {
            const WhereTerm t = terms[j];
            if (t.col != cur) {
                cur = t.col;
                const void* base = cols[cur];
                if ((is64 >> cur) & 1u) {
                    const long long* c = reinterpret_cast<const long long*>(base) + r0;
                    if (valid == 0xFu) {
                        const longlong2 a = reinterpret_cast<const longlong2*>(c)[0], b = reinterpret_cast<const longlong2*>(c)[1];
                        v0 = a.x; v1 = a.y; v2 = b.x; v3 = b.y;
                    } else {
                        v0 = (valid & 1u) ? c[0] : 0; v1 = (valid & 2u) ? c[1] : 0; v2 = (valid & 4u) ? c[2] : 0; v3 = 0;
                    }
                } else {
                    const int32_t* c = reinterpret_cast<const int32_t*>(base) + r0;
                    if (valid == 0xFu) {
                        const int4 a = *reinterpret_cast<const int4*>(c);
                        v0 = a.x; v1 = a.y; v2 = a.z; v3 = a.w;
                    } else {
                        v0 = (valid & 1u) ? c[0] : 0; v1 = (valid & 2u) ? c[1] : 0; v2 = (valid & 4u) ? c[2] : 0; v3 = 0;
                    }
                }
            }
            const uint32_t m = (term_pass(t, v0, in_vals) ? 1u : 0u) | (term_pass(t, v1, in_vals) ? 2u : 0u) | (term_pass(t, v2, in_vals) ? 4u : 0u) |
                               (term_pass(t, v3, in_vals) ? 8u : 0u);
            acc |= m << (4 * (j & 7u));
            if ((j & 7u) == 7u || j + 1 == n_terms) {
                tm[j >> 3][tid] = acc;
                acc = 0;
            }
        }
        uint32_t s = 0;                        // the stack: a nibble per level, the top in bits 0-3
        for (uint32_t i = 0; i < n_ops; ++i) {
            const uint32_t op = ops[i];
            if (op < kMaxTerms) {
                s = (s << 4) | ((tm[op >> 3][tid] >> (4 * (op & 7u))) & 0xFu);
            } else {
                const uint32_t top = s & 0xFu;
                s >>= 4;
                s = op == kOpAnd ? s & (top | ~0xFu) : s | top;
            }
        }
        const uint32_t m = s & valid;          // (rows beyond the table leave zero bits)
        // 8 lanes make a word of the bitmap
        uint32_t word = m << (4 * (tid & 7u));
        word |= __shfl_xor(word, 1, 64);
        word |= __shfl_xor(word, 2, 64);
        word |= __shfl_xor(word, 4, 64);
        if ((tid & 7u) == 0 && r0 < rows) bits[r0 >> 5] = word;
        n += (uint32_t)__popc(m);
    }
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
    if ((tid & 63u) == 0) wn[tid >> 6] = n;
    __syncthreads();
    if (tid == 0 && wn[0] + wn[1] + wn[2] + wn[3]) atomicAdd(count, (unsigned long long)(wn[0] + wn[1] + wn[2] + wn[3]));
}

void eval_host(const pg_where* w, const void* const* cols, const int* dtypes, uint64_t rows, uint32_t* out_bits) {
    const size_t words = (size_t)((rows + 31) / 32);
    for (size_t i = 0; i < words; ++i) out_bits[i] = 0;
    uint8_t tv[kMaxTerms];
    for (uint64_t r = 0; r < rows; ++r) {
        for (size_t j = 0; j < w->terms.size(); ++j) {
            const WhereTerm& t = w->terms[j];
            const long long v = dtypes[t.col] == PG_F_I64 ? reinterpret_cast<const long long*>(cols[t.col])[r]
                                                          : (long long)reinterpret_cast<const int32_t*>(cols[t.col])[r];
            tv[j] = term_pass(t, v, w->in_vals.data()) ? 1 : 0;
        }
        uint32_t s = 0;
        for (uint32_t op : w->ops) {
            if (op < kMaxTerms) {
                s = (s << 1) | tv[op];
            } else {
                const uint32_t top = s & 1u;
                s >>= 1;
                s = op == kOpAnd ? s & (top | ~1u) : s | top;
            }
        }
        if (s & 1u) out_bits[r >> 5] |= 1u << (r & 31);
    }
}

// the clause's columns in `fs`, by name: where_check's rules for each
int where_resolve(const char* who, const pg_where* w, const pg_features* fs, uint64_t rows, int* cols) {
    PG_REQUIRE(fs->rows >= rows, "%s: the feature store holds %llu rows, the table %llu", who, (unsigned long long)fs->rows,
               (unsigned long long)rows);
    for (size_t i = 0; i < w->col_names.size(); ++i) {
        int c = -1;
        for (size_t j = 0; j < fs->cols.size() && c < 0; ++j)      // (names are unique: pg_features_set_column replaces a column of the name)
            if (fs->cols[j].name == w->col_names[i]) c = (int)j;
        PG_REQUIRE(c >= 0, "%s: the feature store has no column \"%s\"", who, w->col_names[i].c_str());
        const pg_features::Column& col = fs->cols[(size_t)c];
        PG_REQUIRE((col.dtype == PG_F_I32 || col.dtype == PG_F_I64) && col.d, "%s: column \"%s\" must be an int32 / int64 column with values", who,
                   col.name.c_str());
        cols[i] = c;
    }
    return PG_OK;
}

int where_build(pg_ctx* ctx, const pg_where* w, const pg_features* fs, uint64_t rows, const int* cols, std::shared_ptr<WhereBits>* out) {
    auto wb = std::make_shared<WhereBits>();
    const size_t nc = w->col_names.size(), nt = w->terms.size(), ni = w->in_vals.size(), no = w->ops.size();
    const size_t words = (size_t)((rows + 31) / 32);
    // program: [16 column pointers][terms][IN constants][ops][count], then the bitmap at a 256-B boundary
    const size_t o_terms = kMaxCols * 8, o_in = o_terms + nt * sizeof(WhereTerm), o_ops = o_in + ni * 8, o_cnt = (o_ops + no * 4 + 7) & ~(size_t)7;
    const size_t o_bits = align_up(o_cnt + 8);
    const size_t total = o_bits + words * 4 + 256;
    std::vector<unsigned char> h(o_bits, 0);
    uint32_t is64 = 0;
    for (size_t i = 0; i < nc; ++i) {
        const pg_features::Column& c = fs->cols[(size_t)cols[i]];
        reinterpret_cast<const void**>(h.data())[i] = c.d;
        if (c.dtype == PG_F_I64) is64 |= 1u << i;
        wb->cols.push_back(cols[i]);
        wb->versions.push_back(c.version);
    }
    memcpy(h.data() + o_terms, w->terms.data(), nt * sizeof(WhereTerm));
    if (ni) memcpy(h.data() + o_in, w->in_vals.data(), ni * 8);
    memcpy(h.data() + o_ops, w->ops.data(), no * 4);
    PG_HIP(hipSetDevice(ctx->device));
    if (hipMalloc(&wb->d, total) != hipSuccess) {
        (void)hipGetLastError();
        wb->d = nullptr;
        set_error("pg_where: hipMalloc(%zu) for the bitmap of %llu rows failed", total, (unsigned long long)rows);
        return PG_ERR_NOMEM;
    }
    char* d = (char*)wb->d;
    wb->bits = (uint32_t*)(d + o_bits);
    wb->fs = fs;
    wb->device = ctx->device;
    wb->rows = rows;
    wb->bytes = total;
    hipStream_t s = ctx->stream;
    hipEvent_t ev[2] = {nullptr, nullptr};
    PG_HIP(hipEventCreate(&ev[0]));
    if (hipEventCreate(&ev[1]) != hipSuccess) {
        (void)hipEventDestroy(ev[0]);
        set_error("pg_where: hipEventCreate failed");
        return PG_ERR_DEVICE;
    }
    auto done = [&](int rc) {
        (void)hipStreamSynchronize(s);           // (the staging vector and wb outlive everything enqueued)
        (void)hipEventDestroy(ev[0]);
        (void)hipEventDestroy(ev[1]);
        return rc;
    };
    unsigned long long h_n = 0;
    float ms = 0.0f;
    if (hipMemcpyAsync(d, h.data(), o_bits, hipMemcpyHostToDevice, s) != hipSuccess ||
        hipMemsetAsync(d + o_bits + words * 4, 0, 256, s) != hipSuccess || hipEventRecord(ev[0], s) != hipSuccess)
        return done(PG_ERR_DEVICE);
    const uint64_t tiles = (rows + kWhereBlockRows - 1) / kWhereBlockRows;
    where_eval_kernel<<<(uint32_t)std::min<uint64_t>(tiles, (uint64_t)ctx->num_cus * 8), 256, 0, s>>>(
        (const void* const*)d, is64, (const WhereTerm*)(d + o_terms), (uint32_t)nt, (const long long*)(d + o_in), (const uint32_t*)(d + o_ops),
        (uint32_t)no, rows, wb->bits, (unsigned long long*)(d + o_cnt));
    if (hipGetLastError() != hipSuccess || hipEventRecord(ev[1], s) != hipSuccess ||
        hipMemcpyAsync(&h_n, d + o_cnt, 8, hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess ||
        hipEventElapsedTime(&ms, ev[0], ev[1]) != hipSuccess) {
        set_error("pg_where: the bitmap build failed: %s", hipGetErrorString(hipGetLastError()));
        return done(PG_ERR_DEVICE);
    }
    wb->admitted = h_n;
    wb->epoch = g_where_epoch.fetch_add(1, std::memory_order_relaxed) + 1;
    w->st.builds++;
    w->st.last_build_ms = (double)ms;
    *out = std::move(wb);
    return done(PG_OK);
}

// A compiled clause bound to a store for a table of `rows` rows (caller holds ctx->mu; cols: where_resolve's): the filter, its
// identity for the caches that key on it and, for the bitmap form, the reference that keeps the bitmap alive — held until the
// caller's stream has synchronised.  A clause of one plain comparison binds to the single-column form and builds nothing
// (force_bits: the bitmap either way).
struct WhereBound {
    RowFilter f{};
    WhereId id{};
    std::shared_ptr<WhereBits> hold;
};
int where_bind(const char* who, pg_ctx* ctx, const pg_where* w, const pg_features* fs, uint64_t rows, const int* cols, bool force_bits,
               WhereBound* out) {
    int rc;
    PG_HIP(hipSetDevice(ctx->device));
    *out = WhereBound();
    if (w->simple && !force_bits) {
        const pg_features::Column& c = fs->cols[(size_t)cols[0]];
        out->f.col = c.d;
        out->f.dtype = c.dtype;
        out->f.op = w->simple_op;
        out->f.val = w->simple_val;
        out->id = WhereId{fs, cols[0], nullptr, 0};
        return PG_OK;
    }
    if (rows == 0 || rows >= (1ull << 32)) {
        set_error("%s: %llu rows unsupported", who, (unsigned long long)rows);
        return PG_ERR_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> g(w->mu);
    std::shared_ptr<WhereBits> wb = w->cur;
    bool hit = wb && wb->fs == fs && wb->device == ctx->device && wb->rows == rows && wb->cols.size() == w->col_names.size();
    for (size_t i = 0; hit && i < wb->cols.size(); ++i)
        hit = wb->cols[i] == cols[i] && wb->versions[i] == fs->cols[(size_t)cols[i]].version;
    if (hit) {
        w->st.hits++;
    } else {
        if ((rc = where_build(ctx, w, fs, rows, cols, &wb))) return rc;
        w->cur = wb;
        w->st.bytes = wb->bytes;
        w->st.epoch = wb->epoch;
        w->st.admitted = wb->admitted;
    }
    out->f.col = wb->bits;
    out->f.dtype = kFilterBits;
    out->f.admitted = (long long)wb->admitted;
    out->id = WhereId{fs, -1, w, wb->epoch};
    out->hold = wb;
    return PG_OK;
}

// the checks of pg_recall_topk_where in its order, the clause's columns in the place of its column
int where_ex_check(const char* who, const pg_ctx* ctx, const pg_table* t, const pg_features* fs, const pg_where* w, int metric,
                   const void* queries, const void* rows, const void* scores, uint32_t nq, uint32_t k, int* cols) {
    PG_REQUIRE(ctx && t && fs && w && queries && rows && scores, "%s: NULL argument", who);
    PG_REQUIRE(nq >= 1 && nq <= (uint32_t)kMaxQueries, "%s: nq=%u must be in [1,%d]", who, nq, kMaxQueries);
    PG_REQUIRE(t->dim <= 128 || nq <= 32, "%s: dim %u supports at most 32 queries per call", who, t->dim);
    PG_REQUIRE(metric == 0 || metric == 1, "%s: metric %d unknown (0 inner product, 1 squared Euclidean)", who, metric);
    int rc;
    if ((rc = where_resolve(who, w, fs, t->rows, cols))) return rc;
    if (k < 1 || k > 16384) {
        set_error("%s: k=%u unsupported (1..16384)", who, k);
        return PG_ERR_UNSUPPORTED;
    }
    return PG_OK;
}

// one filtered recall of host queries behind its checks: through `ix` (NULL: the table's own search, or its attached index when
// "index_route_where" is set)
int where_ex_recall(const char* who, pg_ctx* ctx, const pg_table* t, pg_index* ix, const pg_features* fs, const pg_where* w, int metric,
                    const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count) {
    int cols[kMaxCols];
    int rc;
    if ((rc = where_ex_check(who, ctx, t, fs, w, metric, queries, out_rows, out_scores, nq, k, cols))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    TableRead tr(t->rw);
    WhereBound b;
    if ((rc = where_bind(who, ctx, w, fs, t->rows, cols, false, &b))) return rc;
    if (!ix) ix = index_route_where(ctx, t);
    uint32_t counts[kMaxQueries];
    auto run = [&](const float* d_q, uint64_t* d_rows, float* d_sc) {
        return ix ? index_where_locked(ctx, ix, b.id, b.f, metric == 1, d_q, nq, k, d_rows, d_sc, counts)
                  : recall_where_locked(ctx, t, b.f, metric, d_q, nq, k, d_rows, d_sc, counts);
    };
    rc = recall_staged(ctx, t->dim, queries, nq, k, out_rows, out_scores, run);
    if (rc != PG_OK) {
        (void)hipStreamSynchronize(ctx->stream);      // (nothing enqueued reads the bitmap once b lets go of it)
        return rc;
    }
    if (out_count) memcpy(out_count, counts, (size_t)nq * 4);
    return PG_OK;
}
}  // namespace

int where_clause_check(const char* who, const pg_ctx* ctx, const pg_table* t, const pg_features* fs, const pg_where* w, int metric,
                       const void* queries, const void* rows, const void* scores, uint32_t nq, uint32_t k) {
    int cols[kMaxCols];
    return where_ex_check(who, ctx, t, fs, w, metric, queries, rows, scores, nq, k, cols);
}

int where_clause_bind(const char* who, pg_ctx* ctx, const pg_table* t, const pg_features* fs, const pg_where* w, WhereServe* out) {
    int cols[kMaxCols];
    int rc;
    if ((rc = where_resolve(who, w, fs, t->rows, cols))) return rc;
    WhereBound b;
    if ((rc = where_bind(who, ctx, w, fs, t->rows, cols, false, &b))) return rc;
    out->f = b.f;
    out->id = b.id;
    out->hold = b.hold;
    return PG_OK;
}

int where_bits_bind(const char* who, pg_ctx* ctx, const pg_where* w, const pg_features* fs, uint64_t rows, WhereServe* out) {
    int cols[kMaxCols];
    int rc;
    if ((rc = where_resolve(who, w, fs, rows, cols))) return rc;
    WhereBound b;
    if ((rc = where_bind(who, ctx, w, fs, rows, cols, true, &b))) return rc;
    out->f = b.f;
    out->id = b.id;
    out->hold = b.hold;
    return PG_OK;
}

}  // namespace pg

extern "C" {

int pg_where_compile(const char* clause, pg_where** out) {
    PG_REQUIRE(clause && out, "pg_where_compile: NULL argument");
    pg_where* w = new pg_where();
    const int rc = pg::compile(clause, w);
    if (rc != PG_OK) {
        delete w;
        return rc;
    }
    *out = w;
    return PG_OK;
}

int pg_where_free(pg_where* w) {
    delete w;
    return PG_OK;
}

int pg_where_num_columns(const pg_where* w) { return w ? (int)w->col_names.size() : 0; }

const char* pg_where_column_name(const pg_where* w, int i) {
    return w && i >= 0 && (size_t)i < w->col_names.size() ? w->col_names[(size_t)i].c_str() : nullptr;
}

int pg_where_eval_host(const pg_where* w, const void* const* cols, const int* dtypes, uint64_t rows, uint32_t* out_bits) {
    PG_REQUIRE(w && cols && dtypes && (out_bits || rows == 0), "pg_where_eval_host: NULL argument");
    for (size_t i = 0; i < w->col_names.size(); ++i) {
        PG_REQUIRE(cols[i] || rows == 0, "pg_where_eval_host: column \"%s\" has no values", w->col_names[i].c_str());
        PG_REQUIRE(dtypes[i] == PG_F_I32 || dtypes[i] == PG_F_I64, "pg_where_eval_host: column \"%s\" must be int32 / int64", w->col_names[i].c_str());
    }
    pg::eval_host(w, cols, dtypes, rows, out_bits);
    return PG_OK;
}

int pg_where_stats(const pg_where* w, pg_where_stats_t* out) {
    PG_REQUIRE(w && out, "pg_where_stats: NULL argument");
    std::lock_guard<std::mutex> g(w->mu);
    *out = w->st;
    return PG_OK;
}

int pg_where_bits(pg_ctx* ctx, const pg_where* w, const pg_features* fs, uint64_t rows, uint32_t* out_bits, uint64_t* out_admitted) {
    PG_REQUIRE(ctx && w && fs, "pg_where_bits: NULL argument");
    int cols[pg::kMaxCols];
    int rc;
    if ((rc = pg::where_resolve("pg_where_bits", w, fs, rows, cols))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::WhereBound b;
    if ((rc = pg::where_bind("pg_where_bits", ctx, w, fs, rows, cols, true, &b))) return rc;
    if (out_bits) {
        PG_HIP(hipMemcpyAsync(out_bits, b.f.col, (size_t)((rows + 31) / 32) * 4, hipMemcpyDeviceToHost, ctx->stream));
        PG_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (out_admitted) *out_admitted = (uint64_t)b.f.admitted;
    return PG_OK;
}

int pg_recall_topk_where_ex(pg_ctx* ctx, const pg_table* t, const pg_features* fs, const pg_where* w, int metric, const float* queries,
                            uint32_t nq, uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count) {
    return pg::where_ex_recall("pg_recall_topk_where_ex", ctx, t, nullptr, fs, w, metric, queries, nq, k, out_rows, out_scores, out_count);
}

int pg_index_recall_topk_where_ex(pg_ctx* ctx, const pg_index* ix, const pg_features* fs, const pg_where* w, int metric,
                                  const float* queries, uint32_t nq, uint32_t k, uint64_t* out_rows, float* out_scores, uint32_t* out_count) {
    PG_REQUIRE(ix, "pg_index_recall_topk_where_ex: NULL argument");
    return pg::where_ex_recall("pg_index_recall_topk_where_ex", ctx, pg::index_table(ix), const_cast<pg_index*>(ix), fs, w, metric, queries, nq, k, out_rows,
                               out_scores, out_count);
}

int pg_table_view_create_ex(pg_ctx* ctx, const pg_table* t, const pg_features* fs, const pg_where* w, pg_table** out_view) {
    PG_REQUIRE(ctx && t && fs && w && out_view, "pg_table_view_create_ex: NULL argument");
    PG_REQUIRE(!t->d_row_map, "pg_table_view_create_ex: the source is a view itself");
    int cols[pg::kMaxCols];
    int rc;
    if ((rc = pg::where_resolve("pg_table_view_create_ex", w, fs, t->rows, cols))) return rc;
    std::lock_guard<std::mutex> g(ctx->mu);
    pg::TableRead tr(t->rw);
    pg::WhereBound b;
    if ((rc = pg::where_bind("pg_table_view_create_ex", ctx, w, fs, t->rows, cols, false, &b))) return rc;
    return pg::view_create_locked("pg_table_view_create_ex", ctx, t, b.f, out_view);        // (ends synchronised)
}

}  // extern "C"
