// cond_host_san.cpp — the condition compiler, its host statements and the govaluate front end under ASan + UBSan: a stand-alone
// program (scripts/cond_host_san.sh builds the library's host code with the sanitizers and links this against it).  It feeds them
// the reference's own configs (sort/boost_score_sort_test.go's r1 / r2 and round cases, an `in` / `equal` FilterParam) and a few
// hundred mutations of them — operators, types, right-hand sides, nesting, list sizes, names, expression text, all drawn from a
// fixed generator — and evaluates whatever compiles on a handful of candidates.  Every call must return a status; nothing may
// trip a sanitizer.  No device is touched.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/pairec_gpu.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t n) {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return n ? (uint32_t)((g_state >> 11) % n) : 0;
}

static const char* const kNames[] = {"recall_name", "status", "price", "score", "", "nobody", "level"};
static const char* const kDomains[] = {"item", "", "user", "context"};
static const char* const kExprs[] = {"score * 100", "score * (-10)", "round(score * 3, 2)", "round(score * 3)", "score + price", "", "score >",
                                     "((((score", "score ** 2 ** 3", "[recall_name] % 0", "1 / 0 - price", "round()", "round(1,2,3)", "-", "nobody + 1",
                                     "1+(2+(3+(4+(5+(6+(7+(8+(9+score))))))))", "score * 1e5", "0x1F", "'r1'", "score ? 1 : 2"};

int main() {
    const pg_cond_col cols[] = {{"recall_name", PG_F_I32}, {"status", PG_F_I64}, {"price", PG_F_F32}, {"score", PG_F_F64}, {"level", PG_F_I32}};
    const int32_t c_recall[] = {0, 0, 1, 1, 2, 0};
    const int64_t c_status[] = {1, 0, 1, (1ll << 40), -5, 1};
    const float c_price[] = {0.5f, 20.f, 3.25f, 0.f, -1.f, 9.f};
    const double c_score[] = {0.1, 0.2, 0.3, 0.4, 0.5, 0.6};
    const int32_t c_level[] = {1, 2, 3, 4, 5, 6};
    const void* host_cols[] = {c_recall, c_status, c_price, c_score, c_level};
    const uint8_t item_in[] = {1, 1, 0, 1, 1, 0};
    const double score[] = {0.0, 1.0, 0.311, -2.5, 1e300, 7.0};
    const uint64_t user_vals[PG_COND_MAX_SLOTS] = {3, 0x4000000000000000ull, 1, 2, 3, 4, 5, 6};
    long long list[80];
    for (int i = 0; i < 80; ++i) list[i] = (long long)i * 3 - 7;
    unsigned compiled = 0, refused = 0, evaluated = 0;
    for (int round = 0; round < 600; ++round) {
        // rounds 0..3 are the reference's configs as they stand; the rest mutate them
        const bool golden = round < 4;
        pg_cond_term terms[4][12];
        pg_cond_rule rules[10];
        memset(terms, 0, sizeof terms);
        memset(rules, 0, sizeof rules);
        uint32_t n_rules = golden ? (round == 0 ? 2 : 1) : 1 + rnd(rnd(8) ? 3 : 9);
        const uint32_t boost = golden ? (round < 3) : rnd(2);
        for (uint32_t r = 0; r < n_rules && r < 10; ++r) {
            pg_cond_term* t = terms[r % 4];
            uint32_t n = golden ? (round == 0 || round == 3 ? 1 : 0) : rnd(rnd(4) ? 5 : 11);
            for (uint32_t i = 0; i < n; ++i) {
                // a term that compiles …
                static const struct { const char* name; int32_t type; } kLeft[] = {{"recall_name", PG_COND_STRING}, {"status", PG_COND_INT64},
                                                                                   {"price", PG_COND_FLOAT}, {"level", PG_COND_INT}};
                const auto& l = kLeft[golden ? (round == 3 ? 1 : 0) : rnd(4)];
                t[i].name = l.name;
                t[i].domain = golden ? "item" : kDomains[rnd(2)];
                t[i].type = golden && round == 3 ? PG_COND_INT : l.type;
                t[i].op = golden ? (round == 3 ? PG_COND_IN : PG_COND_EQUAL) : (l.type == PG_COND_FLOAT ? PG_COND_GREATER + (int32_t)rnd(4) : (int32_t)rnd(10));
                t[i].rhs = PG_COND_RHS_CONST;
                t[i].i = golden ? (long long)r : (long long)rnd(5) - 1;
                t[i].f = (double)rnd(7) * 0.5;
                t[i].list = list;
                t[i].n_list = golden ? 3 : rnd(9);
                if (golden) continue;
                if (rnd(5) == 0 && t[i].op < PG_COND_IN) {                     // user.x / item.x of the same kind
                    t[i].rhs = rnd(2) ? PG_COND_RHS_USER : PG_COND_RHS_ITEM;
                    t[i].rhs_name = t[i].rhs == PG_COND_RHS_USER ? (l.type == PG_COND_FLOAT ? "uf" : "ui") : l.name;
                }
                if (rnd(6) == 0 && i + 2 < n) {                                // a bool with the next terms as its children
                    t[i].op = PG_COND_BOOL;
                    t[i].bool_and = rnd(2);
                    t[i + 1].depth = 1;                                        // (kept by the terms generated next: only the fields below are rewritten)
                }
                if (i > 0 && t[i - 1].op == PG_COND_BOOL) t[i].depth = 1;
                // … and, one time in four, one thing wrong with it
                if (rnd(4) == 0) {
                    switch (rnd(10)) {
                        case 0: t[i].name = kNames[rnd(7)]; break;
                        case 1: t[i].domain = kDomains[rnd(4)]; break;
                        case 2: t[i].op = (int32_t)rnd(16) - 1; break;
                        case 3: t[i].type = (int32_t)rnd(6) - 1; break;
                        case 4: t[i].rhs = (int32_t)rnd(5); t[i].rhs_name = rnd(3) ? kNames[rnd(7)] : nullptr; break;
                        case 5: t[i].depth = rnd(3); break;
                        case 6: t[i].n_list = 64 + rnd(3); break;
                        case 7: t[i].list = nullptr; break;
                        case 8: t[i].name = nullptr; break;
                        default: t[i].op = PG_COND_BOOL; break;
                    }
                }
            }
            rules[r].terms = n || rnd(2) ? t : nullptr;
            rules[r].n_terms = n;
            rules[r].expression = golden ? (round < 3 ? kExprs[round == 0 ? r : round + 1] : nullptr) : (boost ? kExprs[rnd(rnd(3) ? 5 : 20)] : (rnd(8) ? nullptr : kExprs[rnd(20)]));
        }
        pg_cond* c = nullptr;
        const int rc = pg_cond_compile(rules, n_rules, cols, golden || rnd(8) ? 5 : rnd(6), boost, &c);
        if (rc != PG_OK) {
            if (golden) {
                fprintf(stderr, "golden config %d refused: %s\n", round, pg_last_error());
                return 1;
            }
            if (!pg_last_error()[0]) {
                fprintf(stderr, "round %d: status %d without a message\n", round, rc);
                return 1;
            }
            ++refused;
            continue;
        }
        ++compiled;
        uint8_t match[6], rule[6];
        double out[6];
        for (int r = 0; r < pg_cond_num_rules(c); ++r)
            if (pg_cond_match_host(c, (uint32_t)r, 6, rnd(2) ? item_in : nullptr, host_cols, user_vals, rnd(256), match) == PG_OK) ++evaluated;
        if (boost && pg_boost_scores_host(c, rnd(2), 6, item_in, host_cols, user_vals, rnd(256), score, out, rnd(2) ? rule : nullptr) == PG_OK) {
            ++evaluated;
            if (round == 0 && (out[0] != 0.0 || out[1] != 100.0 || out[2] != 0.311 || out[3] != 25.0)) {      // r1 x100, outside, r2 x(-10)
                fprintf(stderr, "the r1 / r2 case gives %g %g %g %g\n", out[0], out[1], out[2], out[3]);
                return 1;
            }
            if (round == 1 && out[2] != 0.93) {
                fprintf(stderr, "round(0.311 * 3, 2) gives %.17g\n", out[2]);
                return 1;
            }
        }
        for (int s = 0; s < pg_cond_num_user_slots(c); ++s) (void)strlen(pg_cond_user_slot_name(c, s));
        pg_cond_free(c);
    }
    // the front end alone: every text, and every prefix of it
    for (const char* src : kExprs) {
        const std::string s(src);
        for (size_t len = 0; len <= s.size(); ++len) {
            pg_expr* e = nullptr;
            if (pg_expr_compile_govaluate(s.substr(0, len).c_str(), &e) != PG_OK) continue;
            std::vector<double> vars((size_t)pg_expr_num_vars(e) * 3, 1.5), res(3);
            pg_expr_eval_host(e, vars.data(), 3, res.data());
            pg_expr_free(e);
        }
    }
    printf("cond_host_san: %u sets compiled, %u refused by name, %u host evaluations, no sanitizer report\n", compiled, refused, evaluated);
    return compiled > 100 && refused > 100 ? 0 : 1;
}
