// expr_prog.hpp — the postfix program the expression front ends compile to (expr.hip) and the pieces other evaluators of it
// share (cond.hip walks such programs per candidate with a register stack).
#pragma once
#include "common.hpp"

#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace pg {

enum OpCode : uint32_t { OP_CONST = 0, OP_VAR, OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_MOD, OP_POW, OP_FNZ,
                         OP_DIVF,   // antlr subset: float division as Go's `/` on float64 (no panic: ±Inf / NaN)
                         OP_NEG,    // antlr subset: unary minus
                         OP_FMOD,   // govaluate subset: `%` = math.Mod on float64 (no panic: NaN for a zero divisor)
                         OP_ROUND,  // govaluate subset: round(x) = math.Round (unary)
                         OP_ROUND2,  // govaluate subset: round(x, n) = math.Trunc(x * Pow(10, n)) / Pow(10, n) (binary)
                         // govaluate's boolean subset (classcut.hip only: no other front end emits them, no other evaluator
                         // meets them).  A bool travels on the value stack as 1.0 / 0.0, an error as a bit beside its slot.
                         OP_EQ, OP_NE, OP_GT, OP_GE, OP_LT, OP_LE,   // two numbers → bool, IEEE
                         OP_IN,     // unary: the number == one of the constants [arg & 0xFFFF, + arg >> 16) of the set's list table
                         OP_SRC,    // push: bit `source` of the mask `arg` (recall_name ==, in; a source >= 32 has no bit)
                         OP_AND, OP_OR,   // two bools, govaluate's short circuit: the left's error, else its verdict, else the right
                         OP_NOT,    // unary on a bool
                         OP_EXP };  // RealTimeU2I's weight expression only (rtu2i.hip): exp(x) = go_exp (unary); no other front end emits it

struct Instr {
    uint32_t op;
    uint32_t arg;     // variable index
    double val;       // constant
};

constexpr int kMaxStack = 32;
constexpr int kMaxProg = 128;

}  // namespace pg

struct pg_expr {
    std::string source;
    std::vector<pg::Instr> prog;
    std::vector<std::string> vars;
    int max_depth = 0;
    bool empty = false;       // "" → no expression (GetExpAST returns nil)
    bool antlr = false;       // compiled by pg_expr_compile_typed(…, "antlr"): the evaluation-error rule of ExprASTResultByAntlr applies on the host
    // RankConfig.ScoreRewrite of the scene this RankScore belongs to (pg_expr_set_score_rewrites): evaluated by the
    // recommend pipelines' fusion stage before the RankScore itself (pipeline.hip: post_fuse_sort_locked)
    struct Rewrite {
        std::string source;
        bool failed = false;  // the source's expression did not compile in the reference: the score is 0 (rank_service.go:349-351)
        std::vector<pg::Instr> prog;
        std::vector<std::string> vars;
    };
    std::vector<Rewrite> rewrites;
    mutable std::atomic<int> holders{0};     // bindings made from this expression that are still alive (pg::ExprHold)
};

namespace pg {

// expr.hip: the govaluate arithmetic subset parsed into e (source, prog, vars, max_depth) for the entry point `who`.  The front
// ends differ only in the function table they hand the parser: pg_expr_compile_govaluate utils.GovaluateFunctions' round,
// pg_rtu2i_compile the DAO's own table, which holds only exp.  PG_ERR_UNSUPPORTED with the construct named in the message.
enum GvFunctions : uint32_t { kGvRound = 1u, kGvExp = 2u };
int gv_compile(const char* who, const char* source, uint32_t functions, pg_expr* e);

// math.Pow as `^` sees it (utils/ast/ast.go:246; Go stdlib math/pow.go, go 1.24 per the reference's go.mod).  Go does not call a
// libm pow: Pow(x, 1) = x and Pow(x, +-0.5) = Sqrt(x), 1 / Sqrt(x) are exact special cases, and the INTEGER part of the exponent
// is applied by repeated squaring of Frexp(x)'s mantissa with the binary exponent carried on the side — so 400^4 is exactly
// 25 600 000 000 where pow() is an ulp off (and that ulp decides whether the power is an integer-valued exponent of the next
// `^`, or what an integer `%` of it leaves: found by scripts/soak_expr.py).  Integer-valued exponents therefore take Go's loop
// here, bit for bit (the oracle restates the same loop); fractional ones stay on pow(), within 2 ulp of Go's Exp(yf Log(x)) form.
__host__ __device__ __forceinline__ double go_pow(double x, double y) {
    if (y == 1.0) return x;
    const bool xfin = x == x && fabs(x) != __builtin_inf();
    if (y == 0.5 && xfin && x != 0.0) return sqrt(x);
    if (y == -0.5 && xfin && x != 0.0) return 1.0 / sqrt(x);
    const double ay = fabs(y);
    if (xfin && x != 0.0 && x != 1.0 && y != 0.0 && ay < 9223372036854775808.0 && ay == trunc(ay)) {
        double a1 = 1.0;
        long long ae = 0;
        int xe_i;
        double x1 = frexp(x, &xe_i);
        long long xe = xe_i;
        for (long long i = (long long)ay; i != 0; i >>= 1) {
            if (xe < -(1ll << 12) || (1ll << 12) < xe) {
                // overflow / underflow of the result: catch the exponent, stop
                ae += xe;
                break;
            }
            if (i & 1) {
                a1 *= x1;
                ae += xe;
            }
            x1 *= x1;
            xe <<= 1;
            if (x1 < 0.5) {
                x1 += x1;
                xe--;
            }
        }
        if (y < 0.0) {
            a1 = 1.0 / a1;
            ae = -ae;
        }
        if (ae > 4096) ae = 4096;                     // ldexp's int argument: far beyond the format either way
        if (ae < -4096) ae = -4096;
        return ldexp(a1, (int)ae);
    }
    return pow(x, y);
}

// math.Exp as the exp() of RealTimeU2IRecall's WeightExpression sees it (module/realtime_user2item_hologres_dao.go:23-30:
// real(cmplx.Exp(complex(v, 0))) = Exp(v) * cos(0) = Exp(v)).  Go's pure-Go exp (math/exp.go, the FreeBSD e_exp.c form) restated
// operation for operation: argument reduction x = k ln2 + r with ln2 split in two, a degree-5 rational approximation in r * r,
// then the scaling by 2^k.  This restatement IS the specification (Go's amd64 build has an assembly Exp, so parity with a Go
// binary is unpinned, like govaluate's); it differs from libm's exp by at most one unit in the last place.  No product feeds a
// sum as one fused operation here — host and device give the same bits —, and the scaling is two multiplications by powers of
// two, the first exact: one rounding, in the subnormal range too (what Go's Ldexp and C's ldexp give).
__host__ __device__ inline double go_exp(double x) {
#pragma clang fp contract(off)
    const double kLn2Hi = 6.93147180369123816490e-01, kLn2Lo = 1.90821492927058770002e-10, kLog2e = 1.44269504088896338700e+00;
    const double kP1 = 1.66666666666666657415e-01, kP2 = -2.77777777770155933842e-03, kP3 = 6.61375632143793436117e-05,
                 kP4 = -1.65339022054652515390e-06, kP5 = 4.13813679705723846039e-08;
    if (x != x || x == __builtin_inf()) return x;
    if (x == -__builtin_inf()) return 0.0;
    if (x > 7.09782712893383973096e+02) return __builtin_inf();
    if (x < -7.45133219101941108420e+02) return 0.0;
    if (-0x1p-28 < x && x < 0x1p-28) return 1.0 + x;
    const int k = x < 0.0 ? (int)(kLog2e * x - 0.5) : (int)(kLog2e * x + 0.5);      // (Go's int() truncates, as this cast does)
    const double kf = (double)k;
    const double hi = x - kf * kLn2Hi;
    const double lo = kf * kLn2Lo;
    const double r = hi - lo;
    const double t = r * r;
    const double c = r - t * (kP1 + t * (kP2 + t * (kP3 + t * (kP4 + t * kP5))));
    const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
    // Ldexp(y, k), k in [-1075, 1024]: both halves of k are exponents of normal numbers
    const int k1 = k >> 1, k2 = k - k1;
    const unsigned long long b1 = (unsigned long long)(k1 + 1023) << 52, b2 = (unsigned long long)(k2 + 1023) << 52;
    double p1, p2;
    memcpy(&p1, &b1, 8);
    memcpy(&p2, &b2, 8);
    return (y * p1) * p2;
}

// one binary operation of the program; false: the reference panics here (a zero divisor of OP_DIV / OP_MOD)
__host__ __device__ __forceinline__ bool expr_binop(uint32_t op, double l, double r, double* out) {
    double v = 0.0;
    bool ok = true;
    switch (op) {
        case OP_DIVF: v = l / r; break;
        case OP_ADD: v = l + r; break;
        case OP_SUB: v = l - r; break;
        case OP_MUL: v = l * r; break;
        case OP_DIV:
            if (r == 0.0) ok = false; else v = l / r;
            break;
        case OP_MOD: {
            // float64(int(l) % int(r)); Go's float→int of NaN/out-of-range gives MinInt64 on amd64
            const long long li = (l == l && fabs(l) < 9223372036854775808.0) ? (long long)l : (long long)0x8000000000000000ull;
            const long long ri = (r == r && fabs(r) < 9223372036854775808.0) ? (long long)r : (long long)0x8000000000000000ull;
            if (ri == 0) ok = false;
            else if (ri == -1) v = 0.0;
            else v = (double)(li % ri);
            break;
        }
        case OP_POW: v = go_pow(l, r); break;
        case OP_FNZ: v = (l != 0.0) ? l : r; break;
        case OP_FMOD: v = fmod(l, r); break;
        case OP_ROUND2: {
            const double m = go_pow(10.0, r);
            v = trunc(l * m) / m;
            break;
        }
    }
    *out = v;
    return ok;
}

}  // namespace pg
