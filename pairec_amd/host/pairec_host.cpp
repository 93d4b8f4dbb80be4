// pairec_host.cpp — implementation of the C++ host mirror (see pairec_host.hpp) and the small C
// driver API (ph_*) that the Python tests use to exercise it.
#include "pairec_host.hpp"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cerrno>
#include <cmath>
#include <cstring>
#include <ctime>
#include <deque>
#include <thread>

namespace pairec {

// ---- utils ---------------------------------------------------------------------------------------
double ToFloat(const json::Value& v, double def) {          // utils/type.go:43-69
    if (v.type == json::Value::Number) return v.num;
    if (v.type == json::Value::String) {
        char* e = nullptr;
        const double d = strtod(v.str.c_str(), &e);
        if (e != v.str.c_str() && *e == '\0') return d;
        return def;
    }
    return def;
}

namespace module {
bool Item::FloatExprData(const std::string& name, double* out) {
    if (name == "current_score") {                          // item.go:190-197
        algoScores["recall_score"] = Score;
        *out = Score;
        return true;
    }
    auto a = algoScores.find(name);
    if (a != algoScores.end()) { *out = a->second; return true; }
    auto p = Properties.find(name);
    if (p != Properties.end()) { *out = ToFloat(p->second, 0.0); return true; }
    return false;
}
bool InMemoryVectorDao::VectorString(const std::string& id, std::string* out, std::string* err) {
    auto it = vectors.find(id);
    if (it == vectors.end() || it->second.empty()) {
        if (err) *err = "vector empty";                     // module.VectoryEmptyError
        return false;
    }
    *out = it->second;
    return true;
}
}  // namespace module

namespace context {
std::string RecommendContext::GetParameter(const std::string& k) const {
    auto it = Param.find(k);
    return (it != Param.end() && it->second.type == json::Value::String) ? it->second.str : "";
}
double RecommendContext::GetFloat(const std::string& k, double def) const {
    if (HasExperiment() && ExperimentParamsJson.has(k)) return ToFloat(ExperimentParamsJson.at(k), def);
    auto it = ExperimentParams.find(k);
    return it != ExperimentParams.end() ? it->second : def;
}
long long RecommendContext::GetInt(const std::string& k, long long def) const {
    if (HasExperiment() && ExperimentParamsJson.has(k)) return (long long)ToFloat(ExperimentParamsJson.at(k), (double)def);
    auto it = ExperimentParams.find(k);
    return it != ExperimentParams.end() ? (long long)it->second : def;
}
}  // namespace context

// ---- fmt %v for float64 ------------------------------------------------------------------------------
std::string GoFmtFloat(double x) {
    if (x != x) return "NaN";
    if (std::isinf(x)) return x > 0 ? "+Inf" : "-Inf";
    if (x == 0) return std::signbit(x) ? "-0" : "0";
    // shortest digit string that round-trips (strconv 'g', precision -1)
    char buf[40];
    int prec = 1;
    for (; prec <= 17; ++prec) {
        snprintf(buf, sizeof buf, "%.*e", prec - 1, x);
        if (strtod(buf, nullptr) == x) break;
    }
    // buf = [-]d.ddddde[+-]XX
    std::string m(buf);
    const size_t epos = m.find('e');
    const int dexp = atoi(m.c_str() + epos + 1);
    std::string digits;
    for (size_t i = 0; i < epos; ++i)
        if (m[i] >= '0' && m[i] <= '9') digits.push_back(m[i]);
    while (digits.size() > 1 && digits.back() == '0') digits.pop_back();
    const std::string sign = x < 0 ? "-" : "";
    if (dexp < -4 || dexp >= 6) {               // strconv 'g', shortest: the %e form from exponent 6 on
        std::string out = sign + digits.substr(0, 1);
        if (digits.size() > 1) out += "." + digits.substr(1);
        char e[16];
        snprintf(e, sizeof e, "e%c%02d", dexp >= 0 ? '+' : '-', std::abs(dexp));
        return out + e;
    }
    if (dexp >= 0) {
        if ((int)digits.size() <= dexp + 1) return sign + digits + std::string((size_t)(dexp + 1) - digits.size(), '0');
        return sign + digits.substr(0, (size_t)dexp + 1) + "." + digits.substr((size_t)dexp + 1);
    }
    return sign + "0." + std::string((size_t)(-dexp - 1), '0') + digits;
}

// ---- cache --------------------------------------------------------------------------------------------
namespace cache {
namespace {
struct MemCache : Cache {            // go-cache semantics: per-entry expiry, lazy eviction on Get
    Value::Kind kind;
    struct Entry { std::string val; std::chrono::steady_clock::time_point until; bool forever; };
    std::mutex mu;
    std::map<std::string, Entry> m;
    explicit MemCache(Value::Kind k) : kind(k) {}
    void Put(const std::string& key, const std::string& val, int ttl) override {
        std::lock_guard<std::mutex> g(mu);
        m[key] = Entry{val, std::chrono::steady_clock::now() + std::chrono::seconds(ttl), ttl <= 0};
    }
    Value Get(const std::string& key) override {
        std::lock_guard<std::mutex> g(mu);
        auto it = m.find(key);
        if (it == m.end()) return Value{};
        if (!it->second.forever && std::chrono::steady_clock::now() >= it->second.until) {
            m.erase(it);
            return Value{};
        }
        return Value{kind, it->second.val};
    }
};
}  // namespace
std::shared_ptr<Cache> NewCache(const std::string& adapter, const std::string&, std::string* err) {
    if (adapter == "localCache") return std::make_shared<MemCache>(Value::kString);
    if (adapter == "localBytes") return std::make_shared<MemCache>(Value::kBytes);
    if (err) *err = "Cache:not found instance, name:" + adapter;           // cache.go:30
    return nullptr;
}
}  // namespace cache

// ---- recconf -------------------------------------------------------------------------------------
// ---- module.FilterParam → pg_cond_term ---------------------------------------------------------------------------
// [FilterParamConfig] (recconf.go:884-891) as pg_cond_compile takes it: a bool is followed by its children; an Operator that
// NewFilterParamWithConfig does not know adds nothing (filter_op.go:457-495).  Strings — literals, item properties, user
// properties — are dictionary-encoded per call through one map (equal strings, equal ids); without a map (a filter over the
// engine's integer columns) a string term is refused by name.  What pg_cond_compile refuses it refuses by name itself.
namespace {
struct CondBuild {
    std::map<std::string, long long>* dict = nullptr;
    std::deque<std::string> strs;
    std::deque<std::vector<long long>> lists;
    std::vector<std::string> item_names;                  // referenced item properties, in order of first use
    std::map<std::string, int> item_kind, user_kind;       // bit 0: read as a string, bit 1: read as a number
    std::string err;

    const char* keep(const std::string& x) { strs.push_back(x); return strs.back().c_str(); }
    void item(const std::string& name, int kind) {
        if (!item_kind.count(name)) item_names.push_back(name);
        item_kind[name] |= kind;
    }
    long long code(const std::string& x) { return dict->emplace(x, (long long)dict->size()).first->second; }
    bool constant(const json::Value& v, const std::string& type, const std::string& name, long long* i, double* f) {
        if (type == "string") {
            if (!dict) { err = "string term on \"" + name + "\": the store's columns are integers (encode the literal and use Type int)"; return false; }
            *i = code(v.type == json::Value::String ? v.str : v.type == json::Value::Number ? json::NumToString(v.num) : std::string());
            return true;
        }
        if (type == "float") { *f = ToFloat(v, 0.0); return true; }
        if (v.type == json::Value::Number) { *i = v.is_int ? v.i : (long long)v.num; return true; }      // utils.ToInt: int(float64)
        if (v.type == json::Value::String) {
            char* end = nullptr;
            errno = 0;
            const long long x = strtoll(v.str.c_str(), &end, 10);
            if (!v.str.empty() && end && !*end && errno == 0) { *i = x; return true; }
        }
        err = "Value of \"" + name + "\" is not an integer";
        return false;
    }
    bool build(const json::Value& configs, uint32_t depth, std::vector<pg_cond_term>* out) {
        static const std::map<std::string, int> ops = {{"equal", PG_COND_EQUAL}, {"not_equal", PG_COND_NOT_EQUAL}, {"greater", PG_COND_GREATER},
            {"greaterThan", PG_COND_GREATER_THAN}, {"less", PG_COND_LESS}, {"lessThan", PG_COND_LESS_THAN}, {"in", PG_COND_IN}, {"not_in", PG_COND_NOT_IN},
            {"is_null", PG_COND_IS_NULL}, {"is_not_null", PG_COND_IS_NOT_NULL}, {"bool", PG_COND_BOOL}, {"contains", PG_COND_CONTAINS},
            {"not_contains", PG_COND_NOT_CONTAINS}, {"expression", PG_COND_EXPRESSION}};
        static const std::map<std::string, int> types = {{"int", PG_COND_INT}, {"int64", PG_COND_INT64}, {"float", PG_COND_FLOAT}, {"string", PG_COND_STRING}};
        for (const auto& f : configs.arr) {
            const auto o = ops.find(f.s("Operator"));
            if (o == ops.end()) continue;
            pg_cond_term t;
            memset(&t, 0, sizeof t);
            t.op = o->second;
            t.depth = depth;
            if (t.op == PG_COND_BOOL) {
                std::string ty = f.s("Type");
                std::transform(ty.begin(), ty.end(), ty.begin(), [](unsigned char c) { return (char)std::tolower(c); });
                t.bool_and = ty.empty() || ty == "or" ? 0u : 1u;                                            // NewBoolFilterOp, :1640-1651
                out->push_back(t);
                if (!build(f.at("Configs"), depth + 1, out)) return false;
                continue;
            }
            const std::string name = f.s("Name"), domain = f.s("Domain"), type = f.s("Type");
            const bool user = domain == "user";
            t.name = keep(name);
            t.domain = keep(domain);
            const bool nullish = t.op == PG_COND_IS_NULL || t.op == PG_COND_IS_NOT_NULL;
            const auto ty = types.find(type);
            if (!nullish && ty == types.end()) { err = "Type \"" + type + "\" of \"" + name + "\" is not served (int, int64, float, string)"; return false; }
            if (!nullish) t.type = ty->second;
            const int kind = nullish ? 0 : type == "string" ? 1 : 2;
            if (user) user_kind[name] |= kind; else if (domain.empty() || domain == "item") item(name, kind);
            if (nullish || t.op >= PG_COND_CONTAINS) { out->push_back(t); continue; }
            const json::Value& v = f.at("Value");
            const bool listed = t.op == PG_COND_IN || t.op == PG_COND_NOT_IN;
            if (v.type == json::Value::String && (v.str.compare(0, 5, "user.") == 0 || v.str.compare(0, 5, "item.") == 0)) {
                const bool ru = v.str[0] == 'u';
                t.rhs = ru ? (listed ? PG_COND_RHS_USER_LIST : PG_COND_RHS_USER) : PG_COND_RHS_ITEM;
                t.rhs_name = keep(v.str.substr(5));
                if (ru) user_kind[v.str.substr(5)] |= kind; else if (!listed) item(v.str.substr(5), kind);
            } else if (listed) {
                lists.emplace_back();
                // (utils.ToStringArray drops empty strings from a []any; ToIntArray keeps every element)
                for (const auto& x : v.arr) {
                    if (type == "string" && x.type == json::Value::String && x.str.empty()) continue;
                    long long i = 0;
                    double d = 0.0;
                    if (type == "float" || type == "int64") continue;                                       // (never read: the switches list string and int)
                    if (!constant(x, type, name, &i, &d)) return false;
                    lists.back().push_back(i);
                }
                t.list = lists.back().data();
                t.n_list = (uint32_t)lists.back().size();
            } else if (!constant(v, type, name, &t.i, &t.f)) {
                return false;
            }
            out->push_back(t);
        }
        return true;
    }
};
}  // namespace

namespace recconf {
// a FilterParams list that the builder accepts (what pg_cond_compile refuses shows at the first request; this names the rest at load)
bool CheckFilterParams(const json::Value& params, bool strings, std::string* why) {
    std::map<std::string, long long> dict;
    CondBuild b;
    b.dict = strings ? &dict : nullptr;
    std::vector<pg_cond_term> terms;
    if (!b.build(params, 0, &terms)) { *why = b.err; return false; }
    if (terms.size() > PG_COND_MAX_TERMS) { *why = std::to_string(terms.size()) + " operators in one FilterParam (at most " + std::to_string(PG_COND_MAX_TERMS) + ")"; return false; }
    return true;
}
bool CheckBoostScoreConf(const json::Value& sc, std::string* why) {
    const auto& conds = sc.at("BoostScoreConditions").arr;
    if (conds.size() > PG_COND_MAX_RULES) { *why = "more than " + std::to_string(PG_COND_MAX_RULES) + " BoostScoreConditions"; return false; }
    for (const auto& c : conds) {
        if (!CheckFilterParams(c.at("Conditions"), true, why)) return false;
        // an empty Expression is a nil dereference in the reference when the condition matches (boost_score_sort.go:22-29,82)
        if (c.s("Expression").empty()) { *why = "a BoostScoreCondition without an Expression"; return false; }
        pg_expr* e = nullptr;
        if (pg_expr_compile_govaluate(c.s("Expression").c_str(), &e) != PG_OK) { *why = pg_last_error(); return false; }
        pg_expr_free(e);
    }
    return true;
}
// a DistinctIdSort entry (sort/distinct_id_sort.go:17-42).  The reference writes each condition's id under the condition's own
// DistinctIdName; the device writes one id per item, so one sort serves one name — two names are two sorts, which write the same
// properties (distinct_id_sort_test.go, "multi distinctid name").
bool CheckDistinctIdConf(const json::Value& sc, std::string* why) {
    const auto& conds = sc.at("DistinctIdConditions").arr;
    if (conds.size() > PG_COND_MAX_RULES) { *why = "more than " + std::to_string(PG_COND_MAX_RULES) + " DistinctIdConditions"; return false; }
    for (const auto& c : conds) {
        if (!CheckFilterParams(c.at("Conditions"), true, why)) return false;
        const json::Value& id = c.at("DistinctId");
        if (id.type != json::Value::Null && (id.type != json::Value::Number || id.num != std::floor(id.num) || std::fabs(id.num) >= 9e15)) {
            *why = "DistinctId is not an integer";
            return false;
        }
        auto name_of = [](const json::Value& x) { return x.s("DistinctIdName").empty() ? std::string("__distinct_id__") : x.s("DistinctIdName"); };
        if (name_of(c) != name_of(conds[0])) {
            *why = "DistinctIdName \"" + name_of(c) + "\" beside \"" + name_of(conds[0]) +
                   "\": the device serves one name per sort (declare one DistinctIdSort per name: they write the same properties)";
            return false;
        }
    }
    return true;
}
// a MultiRecallMixSort entry that pg_mix_compile accepts; what it refuses is named by key.  Rules with an unknown MixStrategy are
// skipped, as createMixStrategies skips them (multi_recall_mix_sort.go:47-58).
bool CheckMixSortConf(const json::Value& sc, std::string* why) {
    const double size = sc.d("Size");
    if (size < 0 || size > PG_MIX_MAX_SIZE) { *why = "Size " + json::NumToString(size) + " (0 .. " + std::to_string(PG_MIX_MAX_SIZE) + ")"; return false; }
    size_t known = 0;
    for (const auto& r : sc.at("MixSortRules").arr) {
        const std::string ms = r.s("MixStrategy");
        if (ms != "fix_position" && ms != "random_position") continue;
        ++known;
        if (!CheckFilterParams(r.at("Conditions"), true, why)) { *why = "MixSortRules: Conditions: " + *why; return false; }
        if (r.d("Number") < 0) { *why = "MixSortRules: a negative Number"; return false; }
        if (r.d("NumberRate") < 0) { *why = "MixSortRules: a negative NumberRate"; return false; }
        if (ms == "fix_position") {
            const auto& pos = r.at("Positions").arr;
            if (pos.size() > PG_MIX_MAX_POSITIONS) { *why = "MixSortRules: " + std::to_string(pos.size()) + " Positions (at most " + std::to_string(PG_MIX_MAX_POSITIONS) + ")"; return false; }
            for (const auto& p : pos)
                if (p.type != json::Value::Number || p.num < 1 || p.num > 2147483647.0) { *why = "MixSortRules: Positions count from 1 (the reference indexes items[-1])"; return false; }
        }
    }
    if (known > PG_MIX_MAX_STRATEGIES) { *why = std::to_string(known) + " MixSortRules (at most " + std::to_string(PG_MIX_MAX_STRATEGIES) + ")"; return false; }
    return true;
}
}  // namespace recconf

namespace recconf {
static std::vector<std::string> str_list(const json::Value& v) {
    std::vector<std::string> out;
    if (v.type == json::Value::Array)
        for (const auto& e : v.arr)
            if (e.type == json::Value::String) out.push_back(e.str);
    return out;
}
// the names a DiversityAdjustCountFilter expression reads besides recall_name / recall_score, appended to *names once each: bare
// and [bracketed] identifiers that are no keyword, no function call and no accessor (what the compile refuses it names itself)
static void ClasscutNames(const std::string& e, std::vector<std::string>* names) {
    auto alpha = [](char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || c == '_'; };
    auto digit = [](char c) { return c >= '0' && c <= '9'; };
    auto add = [&](const std::string& n) {
        if (n.empty() || n == "recall_name" || n == "recall_score" || n.find('.') != std::string::npos) return;
        if (std::find(names->begin(), names->end(), n) == names->end()) names->push_back(n);
    };
    for (size_t i = 0; i < e.size();) {
        const char c = e[i];
        if (c == '\'' || c == '"') {
            const size_t close = e.find(c, i + 1);
            i = close == std::string::npos ? e.size() : close + 1;
        } else if (c == '[') {
            const size_t close = e.find(']', i + 1);
            if (close == std::string::npos) return;
            add(e.substr(i + 1, close - i - 1));
            i = close + 1;
        } else if (digit(c) || c == '.') {
            while (i < e.size() && (digit(e[i]) || alpha(e[i]) || e[i] == '.')) ++i;
        } else if (alpha(c)) {
            size_t j = i;
            while (j < e.size() && (alpha(e[j]) || digit(e[j]) || e[j] == '.')) ++j;
            const std::string n = e.substr(i, j - i);
            size_t k = j;
            while (k < e.size() && (e[k] == ' ' || e[k] == '\t' || e[k] == '\n' || e[k] == '\r')) ++k;
            const bool keyword = n == "in" || n == "IN" || n == "true" || n == "false", call = k < e.size() && e[k] == '(';
            if (!keyword && !call) add(n);
            i = j;
        } else {
            ++i;
        }
    }
}

// pg_classcut_compile of a parsed DiversityAdjustCountFilter: its columns declared as the engine holds them (int32)
static bool CompileClasscut(const GpuFilterConfig& c, pg_classcut** out, std::string* why) {
    std::vector<pg_classcut_rule> rules(c.Classes.size());
    for (size_t i = 0; i < rules.size(); ++i) rules[i] = pg_classcut_rule{c.Classes[i].Expression.c_str(), c.Classes[i].Type, c.Classes[i].Count};
    std::vector<pg_cond_col> cols(c.ClassColumns.size());
    for (size_t i = 0; i < cols.size(); ++i) cols[i] = pg_cond_col{c.ClassColumns[i].c_str(), PG_F_I32};
    std::vector<const char*> recalls(c.ClassRecalls.size());
    for (size_t i = 0; i < recalls.size(); ++i) recalls[i] = c.ClassRecalls[i].c_str();
    if (recalls.size() > PG_CLASSCUT_MAX_RECALLS) recalls.resize(PG_CLASSCUT_MAX_RECALLS);      // (later recalls have names equal to no literal)
    if (pg_classcut_compile(rules.data(), (uint32_t)rules.size(), cols.data(), (uint32_t)cols.size(), recalls.data(), (uint32_t)recalls.size(), out) == PG_OK)
        return true;
    *why = pg_last_error();
    const size_t colon = why->find(": ");                                 // (the entry point's name says nothing here)
    if (colon != std::string::npos) *why = why->substr(colon + 2);
    return false;
}

// The targets of a pairec_gpu.Sorts TrafficControlSort entry as pg_traffic_compile takes them, and their ItemExpressions as one
// classcut set (class c is target class_target[c]; a target without an expression has no class: it controls every item).  What
// pg_traffic_compile or pg_classcut_compile refuse is named by key.  *set stays NULL when no target has an expression.
static bool CompileTrafficConf(const json::Value& sc, std::vector<pg_traffic_target>* targets, pg_classcut** set, std::vector<int>* class_target,
                               std::vector<std::string>* columns, std::string* why) {
    const auto& ts = sc.at("Targets").arr;
    if (ts.size() > PG_TRAFFIC_MAX_TARGETS) {
        *why = std::to_string(ts.size()) + " Targets (the device serves up to " + std::to_string(PG_TRAFFIC_MAX_TARGETS) + ")";
        return false;
    }
    GpuFilterConfig cc;
    for (size_t t = 0; t < ts.size(); ++t) {
        const json::Value& id = ts[t].at("TrafficControlTargetId");
        long long v = 0;
        if (id.type == json::Value::Number) v = id.is_int ? id.i : (long long)id.num;
        else if (id.type == json::Value::String) {
            char* end = nullptr;
            v = strtoll(id.str.c_str(), &end, 10);
            if (id.str.empty() || *end) { *why = "Targets[" + std::to_string(t) + "]: TrafficControlTargetId \"" + id.str + "\" is not an integer (strconv.Atoi)"; return false; }
        } else { *why = "Targets[" + std::to_string(t) + "]: no TrafficControlTargetId"; return false; }
        if (v <= -2147483648LL || v > 2147483647LL) { *why = "Targets[" + std::to_string(t) + "]: TrafficControlTargetId outside int32"; return false; }
        targets->push_back(pg_traffic_target{(int32_t)v, ts[t].s("ControlType") == "Percent" ? PG_TRAFFIC_PERCENT : PG_TRAFFIC_QUANTITY});
        if (ts[t].has("Alpha") && ts[t].at("Alpha").type != json::Value::Number) { *why = "Targets[" + std::to_string(t) + "]: Alpha is not a number"; return false; }
        const std::string expr = ts[t].s("ItemExpression");
        if (expr.empty()) continue;
        GpuFilterConfig::ClassConf cl;
        cl.Expression = expr;
        cl.Type = PG_TRIM_FIX;
        cl.Count = 1;                                                    // (the counts are ignored: only the masks are read)
        ClasscutNames(expr, &cc.ClassColumns);
        cc.Classes.push_back(cl);
        class_target->push_back((int)t);
    }
    pg_traffic* m = nullptr;
    if (pg_traffic_compile(targets->data(), (uint32_t)targets->size(), &m) != PG_OK) {
        *why = pg_last_error();
        return false;
    }
    pg_traffic_free(m);
    *columns = cc.ClassColumns;
    *set = nullptr;
    if (cc.Classes.empty()) return true;
    if (CompileClasscut(cc, set, why)) return true;
    *why = "ItemExpression: " + *why;
    return false;
}

bool RecommendConfig::Parse(const std::string& text, RecommendConfig* out, std::string* err) {
    json::Value root;
    if (!json::Parser(text).Parse(&root, err)) return false;
    if (root.type != json::Value::Object) { if (err) *err = "recconf: root is not an object"; return false; }
    for (const auto& a : root.at("AlgoConfs").arr) out->AlgoConfs.push_back({a.s("Name"), a.s("Type"), a});
    for (const auto& r : root.at("RecallConfs").arr) {
        RecallConfig c;
        c.Name = r.s("Name"); c.RecallType = r.s("RecallType"); c.RecallAlgo = r.s("RecallAlgo");
        c.ItemType = r.s("ItemType"); c.CachePrefix = r.s("CachePrefix");
        c.CacheAdapter = r.s("CacheAdapter"); c.CacheConfig = r.s("CacheConfig");
        c.RecallCount = (int)r.n("RecallCount"); c.CacheTime = (int)r.n("CacheTime");
        c.DaoAdapterType = r.at("DaoConf").s("AdapterType");
        c.VectorDaoAdapterType = r.at("VectorDaoConf").s("AdapterType");
        c.HologresName = r.at("VectorDaoConf").s("HologresName");
        c.VectorAlgoType = r.s("VectorAlgoType");
        out->RecallConfs.push_back(c);
    }
    for (const auto& kv : root.at("RankConf").obj) {
        RankConfig c;
        c.RankAlgoList = str_list(kv.second.at("RankAlgoList"));
        c.RankScore = kv.second.s("RankScore"); c.Processor = kv.second.s("Processor");
        c.ASTType = kv.second.s("ASTType"); c.BatchCount = (int)kv.second.n("BatchCount");
        for (const auto& rw : kv.second.at("ScoreRewrite").obj) c.ScoreRewrite[rw.first] = rw.second.str;
        out->RankConf[kv.first] = c;
    }
    for (const auto& kv : root.at("SortNames").obj) out->SortNames[kv.first] = str_list(kv.second);
    auto parse_scene_features = [&](const json::Value& scenes, std::map<std::string, SceneFeatureConfig>* dst) {
        for (const auto& sc : scenes.obj) {                        // recconf.go:52-53,169-176,256-265
            SceneFeatureConfig sf;
            sf.AsynLoadFeature = sc.second.at("AsynLoadFeature").type == json::Value::Bool && sc.second.at("AsynLoadFeature").b;
            for (const auto& lc : sc.second.at("FeatureLoadConfs").arr) {
                FeatureLoadConfig l;
                l.DaoAdapterType = lc.at("FeatureDaoConf").s("AdapterType");
                for (const auto& f : lc.at("Features").arr) {
                    FeatureConfig c;
                    c.FeatureType = f.s("FeatureType"); c.FeatureName = f.s("FeatureName"); c.FeatureSource = f.s("FeatureSource");
                    c.FeatureValue = f.s("FeatureValue"); c.FeatureStore = f.s("FeatureStore"); c.Normalizer = f.s("Normalizer");
                    c.Expression = f.s("Expression");
                    c.RemoveFeatureSource = f.at("RemoveFeatureSource").type == json::Value::Bool && f.at("RemoveFeatureSource").b;
                    l.Features.push_back(std::move(c));
                }
                sf.FeatureLoadConfs.push_back(std::move(l));
            }
            (*dst)[sc.first] = std::move(sf);
        }
    };
    parse_scene_features(root.at("FeatureConfs"), &out->FeatureConfs);
    parse_scene_features(root.at("UserFeatureConfs"), &out->UserFeatureConfs);
    for (const auto& sc : root.at("SceneConfs").obj)
        for (const auto& cat : sc.second.obj)
            out->SceneRecallNames[sc.first][cat.first] = str_list(cat.second.at("RecallNames"));
    auto is_false = [](std::string v) {
        std::transform(v.begin(), v.end(), v.begin(), ::tolower);
        return v == "false";
    };
    auto parse_dpp = [&](const json::Value& d, const std::string& name) {
        DPPSortConfig c;
        c.Name = name; c.Alpha = d.d("Alpha", 1.0); c.WindowSize = (int)d.n("WindowSize");
        c.CandidateCount = (int)d.n("CandidateCount"); c.MinScorePercent = d.d("MinScorePercent");
        c.NormalizeEmb = !is_false(d.s("NormalizeEmb"));    // dpp_sort.go:95-97
        c.EnsurePositiveSim = !is_false(d.s("EnsurePositiveSim"));   // :98-100
        c.AbortRunCount = (int)d.n("AbortRunCount");
        c.FilterRetrieveIds = str_list(d.at("FilterRetrieveIds"));
        c.EmbeddingHookNames = str_list(d.at("EmbeddingHookNames"));
        return c;
    };
    for (const auto& d : root.at("DPPConf").arr) out->DPPConf.push_back(parse_dpp(d, d.s("Name")));
    // SortConfs (recconf.go:86, sort/sort.go:162-200); the GPU diversity sorts of a pairec process are declared in
    // UserDefineConfs.pairec_gpu.Sorts with the same nested DPPConf / SSDConf objects (Engine::Create)
    auto parse_sort = [&](const json::Value& sc) {
        SortConfig c;
        c.Name = sc.s("Name"); c.SortType = sc.s("SortType");
        c.SortByField = sc.s("SortByField");
        c.SortOrder = sc.s("SortOrder");
        c.SwitchThreshold = sc.d("SwitchThreshold");
        if (c.SortType == "DPPSort") {
            c.DPPConf = parse_dpp(sc.at("DPPConf"), c.Name);
            c.HologresName = sc.at("DPPConf").at("DaoConf").s("HologresName");
        } else if (c.SortType == "SSDSort") {
            const json::Value& d = sc.at("SSDConf");
            c.HologresName = d.at("DaoConf").s("HologresName");
            SSDSortConfig& s = c.SSDConf;
            s.Name = c.Name;
            if (d.d("Gamma") > 0) s.Gamma = d.d("Gamma");                         // ssd_sort.go:81-83
            s.UseSSDStar = d.at("UseSSDStar").type == json::Value::Bool && d.at("UseSSDStar").b;
            s.WindowSize = (int)d.n("WindowSize") > 0 ? (int)d.n("WindowSize") : 5; // :84-86
            s.AbortRunCount = (int)d.n("AbortRunCount");
            s.CandidateCount = (int)d.n("CandidateCount");
            s.MinScorePercent = d.d("MinScorePercent");
            s.NormalizeEmb = !is_false(d.s("NormalizeEmb"));                      // :90-92
            s.EnsurePositiveSim = !is_false(d.s("EnsurePositiveSim"));            // :93-95
            s.FilterRetrieveIds = str_list(d.at("FilterRetrieveIds"));
        }
        return c;
    };
    for (const auto& sc : root.at("SortConfs").arr) out->SortConfs.push_back(parse_sort(sc));
    out->UserDefineConfs = root.at("UserDefineConfs");
    // the GPU plug-ins' own declarations, in the shapes of RecallConfig / SortConfig
    for (const auto& r : out->UserDefineConfs.at("pairec_gpu").at("Recalls").arr) {
        RecallConfig c;
        c.Name = r.s("Name"); c.Kind = r.s("Kind", "vector"); c.RecallAlgo = r.s("RecallAlgo");
        c.ItemType = r.s("ItemType"); c.CachePrefix = r.s("CachePrefix");
        c.CacheAdapter = r.s("CacheAdapter"); c.CacheConfig = r.s("CacheConfig");
        c.RecallCount = (int)r.n("RecallCount"); c.CacheTime = (int)r.n("CacheTime");
        c.RankScore = r.s("RankScore"); c.RankVar = r.s("RankVar");
        for (const auto& rw : r.at("ScoreRewrite").obj) c.ScoreRewrite[rw.first] = rw.second.str;
        // HologresVectorConf.WhereClause / TimeInterval (recconf.go:492-497) restrict the SQL's candidates.  The device serves
        // the form `column OP integer` over an int32 item column keyed by row, "${time}" standing for now - TimeInterval as in
        // hologres_vector_recall.go:56-61; anything else is refused here rather than answered over other candidates.
        c.WhereClause = !r.s("WhereClause").empty() ? r.s("WhereClause") : r.at("HologresVectorConf").s("WhereClause");
        c.TimeInterval = (int)(r.n("TimeInterval") != 0 ? r.n("TimeInterval") : r.at("HologresVectorConf").n("TimeInterval"));
        if (!c.WhereClause.empty()) {
            if (c.Kind != "hologres" && c.Kind != "hologres_v2" && c.Kind != "online_hologres") {
                if (err) *err = "pairec_gpu.Recalls: " + c.Name + ": WhereClause is not supported by Kind \"" + c.Kind + "\" (Kinds hologres, hologres_v2, online_hologres take one)";
                return false;
            }
            if (!recall::ParseWhereClause(c.WhereClause, c.TimeInterval, &c.WhereColumn, &c.WhereOp, &c.WhereValue)) {
                if (err) *err = "pairec_gpu.Recalls: " + c.Name + ": WhereClause \"" + c.WhereClause +
                                "\" is not supported (the device serves `column OP integer`, OP one of > >= < <= = != <>, the integer or ${time})";
                return false;
            }
        }
        out->GpuRecalls.push_back(c);
    }
    // DiversityRuleSort on the device (sort/diversity_rule_sort.go:25-67): what pg_diversity_rules cannot serve is refused here, by name
    auto parse_diversity = [&](const json::Value& sc, SortConfig* c) {
        auto refuse = [&](const std::string& what) {
            if (err) *err = "pairec_gpu.Sorts: " + c->Name + ": DiversityRuleSort: " + what;
            return false;
        };
        DiversityRuleSortConfig& dc = c->DiversityConf;
        dc.DiversitySize = (int)sc.n("DiversitySize");
        dc.ExploreItemSize = (int)sc.n("ExploreItemSize");
        dc.ExcludeRecalls = str_list(sc.at("ExcludeRecalls"));
        if (!sc.at("MultiValueDimensionConf").arr.empty()) return refuse("MultiValueDimensionConf (list-valued dimensions) is not supported");
        if (!sc.at("Conditions").arr.empty()) return refuse("Conditions (the sort's user-level gate) is not supported");
        if (sc.at("DiversityRules").arr.size() > PG_DIV_MAX_RULES) return refuse("more than " + std::to_string(PG_DIV_MAX_RULES) + " DiversityRules");
        if (sc.at("ExclusionRules").arr.size() > PG_DIV_MAX_EXCL) return refuse("more than " + std::to_string(PG_DIV_MAX_EXCL) + " ExclusionRules");
        for (const auto& r : sc.at("DiversityRules").arr) {
            DiversityRuleConfig rc;
            rc.Dimensions = str_list(r.at("Dimensions"));
            if (rc.Dimensions.empty() || rc.Dimensions.size() > PG_DIV_MAX_DIMS)
                return refuse("a rule needs 1.." + std::to_string(PG_DIV_MAX_DIMS) + " Dimensions");
            rc.WindowSize = (int)r.n("WindowSize"); rc.FrequencySize = (int)r.n("FrequencySize");
            rc.IntervalSize = (int)r.n("IntervalSize"); rc.Weight = (int)r.n("Weight");
            if (rc.WindowSize < 0 || rc.FrequencySize < 0 || rc.IntervalSize < 0) return refuse("a negative WindowSize, FrequencySize or IntervalSize");
            dc.DiversityRules.push_back(rc);
        }
        for (const auto& x : sc.at("ExclusionRules").arr) {
            ExclusionRuleConfig xc;
            for (const auto& p : x.at("Positions").arr) {
                if (p.type != json::Value::Number || p.num < 1 || p.num != std::floor(p.num)) return refuse("a position that is not a 1-based integer");
                xc.Positions.push_back((long long)p.num);
            }
            if (xc.Positions.empty() || x.at("Conditions").arr.empty()) continue;          // (never matches: diversity_exclusion_rule.go:38-43)
            if (x.at("Conditions").arr.size() > PG_DIV_MAX_TERMS) return refuse("more than " + std::to_string(PG_DIV_MAX_TERMS) + " Conditions in an exclusion rule");
            for (const auto& f : x.at("Conditions").arr) {
                ExclusionCondition ec;
                ec.Name = f.s("Name");
                const std::string op = f.s("Operator"), type = f.s("Type"), domain = f.s("Domain");
                const json::Value& v = f.at("Value");
                static const std::map<std::string, int> ops = {{"greater", PG_WHERE_GT}, {"greaterThan", PG_WHERE_GE}, {"less", PG_WHERE_LT},
                                                               {"lessThan", PG_WHERE_LE}, {"equal", PG_WHERE_EQ}, {"not_equal", PG_WHERE_NE}};
                const auto o = ops.find(op);
                ec.IsString = type == "string" && v.type == json::Value::String;
                const bool is_int = (type == "int" || type == "int64") && v.type == json::Value::Number && v.num == std::floor(v.num) && std::fabs(v.num) < 9e15;
                const bool served = o != ops.end() && !ec.Name.empty() && (domain.empty() || domain == "item") &&
                                    (is_int || (ec.IsString && (o->second == PG_WHERE_EQ || o->second == PG_WHERE_NE)));
                if (!served)
                    return refuse("exclusion condition on \"" + ec.Name + "\" (Operator \"" + op + "\", Type \"" + type +
                                  "\") is not an integer comparison: the device serves item properties under equal / not_equal / greater / "
                                  "greaterThan / less / lessThan against an integer literal, and strings under equal / not_equal");
                ec.Op = o->second;
                ec.Int = is_int ? (long long)v.num : 0;
                ec.Str = v.str;
                xc.Conditions.push_back(ec);
            }
            dc.ExclusionRules.push_back(xc);
        }
        return true;
    };
    for (const auto& sc : out->UserDefineConfs.at("pairec_gpu").at("Sorts").arr) {
        SortConfig c = parse_sort(sc);
        if (c.SortType == "DiversityRuleSort" && !parse_diversity(sc, &c)) return false;
        if (c.SortType == "BoostScoreSort") {
            c.BoostConf = sc;
            std::string why;
            if (!CheckBoostScoreConf(sc, &why)) {
                if (err) *err = "pairec_gpu.Sorts: " + c.Name + ": BoostScoreSort: " + why;
                return false;
            }
        }
        if (c.SortType == "MultiRecallMixSort") {
            c.MixConf = sc;
            std::string why;
            if (!CheckMixSortConf(sc, &why)) {
                if (err) *err = "pairec_gpu.Sorts: " + c.Name + ": MultiRecallMixSort: " + why;
                return false;
            }
        }
        if (c.SortType == "TrafficControlSort") {
            c.TrafficConf = sc;
            std::string why;
            std::vector<pg_traffic_target> targets;
            std::vector<int> class_target;
            std::vector<std::string> columns;
            pg_classcut* set = nullptr;
            if (!CompileTrafficConf(sc, &targets, &set, &class_target, &columns, &why)) {
                if (err) *err = "pairec_gpu.Sorts: " + c.Name + ": TrafficControlSort: " + why;
                return false;
            }
            pg_classcut_free(set);
        }
        if (c.SortType == "DistinctIdSort") {
            c.DistinctConf = sc;
            std::string why;
            if (!CheckDistinctIdConf(sc, &why)) {
                if (err) *err = "pairec_gpu.Sorts: " + c.Name + ": DistinctIdSort: " + why;
                return false;
            }
        }
        out->GpuSorts.push_back(c);
    }
    for (const auto& fc : out->UserDefineConfs.at("pairec_gpu").at("Filters").arr) {
        GpuFilterConfig c;
        c.Name = fc.s("Name"); c.FilterType = fc.s("FilterType"); c.FeatureStore = fc.s("FeatureStore");
        c.FilterParams = fc.at("FilterParams");
        std::string why;
        if (c.IsBlend()) {
            // NewSnakeFilter (snake_filter.go:118-164) / NewCompletelyFairCountFilter (completely_fair_count_filter.go:18-25): what
            // pg_blend_out_cap refuses is refused here, by name
            const bool snake = c.FilterType == "SnakeFilter";
            for (const auto& r : out->GpuRecalls) c.BlendSources.push_back(r.Name);
            const double retain = fc.d("RetainNum");
            c.Blend.mode = !snake ? PG_BLEND_FAIR : (fc.s("SnakeType") == "SKIP_ON_DUPLICATE" ? PG_BLEND_SNAKE_SKIP : PG_BLEND_SNAKE_REFILL);
            c.Blend.retain_num = retain >= 1 && retain <= 4294967295.0 ? (uint32_t)retain : 0u;
            const auto& confs = fc.at("AdjustCountConfs").arr;
            if (snake && confs.size() > PG_BLEND_MAX_SOURCES)
                why = std::to_string(confs.size()) + " AdjustCountConfs (the device serves up to " + std::to_string(PG_BLEND_MAX_SOURCES) + ")";
            for (size_t i = 0; snake && why.empty() && i < confs.size(); ++i) {
                const std::string name = confs[i].s("RecallName");
                const double weight = confs[i].d("Weight");
                const auto at = std::find(c.BlendSources.begin(), c.BlendSources.end(), name);
                if (at == c.BlendSources.end()) why = "RecallName \"" + name + "\" is no recall of pairec_gpu.Recalls";
                else if (at - c.BlendSources.begin() >= PG_BLEND_MAX_SOURCES)
                    why = "RecallName \"" + name + "\" is recall " + std::to_string(at - c.BlendSources.begin()) + " (the device serves the first " +
                          std::to_string(PG_BLEND_MAX_SOURCES) + " recalls)";
                else if (weight < 0 || weight > 4294967295.0 || weight != std::floor(weight)) why = "Weight of \"" + name + "\" is not a count";
                else {
                    c.Blend.source[i] = (uint8_t)(at - c.BlendSources.begin());
                    c.Blend.weight[i] = (uint32_t)weight;
                    c.Blend.n_entries = (uint32_t)i + 1;
                }
            }
            uint32_t width = 0;
            if (why.empty() && pg_blend_out_cap(&c.Blend, 1, &width) != PG_OK) {
                why = pg_last_error();
                const size_t colon = why.find(": ");                     // (the entry point's name says nothing here)
                if (colon != std::string::npos) why = why.substr(colon + 2);
                why = c.FilterType + ": " + why;
            }
        }
        else if (c.IsClasscut()) {
            // NewDiversityAdjustCountFilter (diversity_adjust_count_filter.go:44-66): what pg_classcut_compile refuses is refused here, by name
            for (const auto& r : out->GpuRecalls) c.ClassRecalls.push_back(r.Name);
            const auto& confs = fc.at("AdjustCountConfs").arr;
            for (size_t i = 0; why.empty() && i < confs.size(); ++i) {
                GpuFilterConfig::ClassConf cl;
                cl.Expression = confs[i].s("Expression");
                const double count = confs[i].d("Count");
                const std::string type = confs[i].s("Type");
                if (confs[i].at("Count").type != json::Value::Number || count < 0 || count > 4294967295.0 || count != std::floor(count))
                    why = "Count of class " + std::to_string(i) + " is not a count";
                else if (type != "fix" && type != "accumulator")
                    why = "Type \"" + type + "\" of class " + std::to_string(i) + " (the reference serves fix and accumulator)";
                cl.Count = why.empty() ? (uint32_t)count : 0u;
                cl.Type = type == "fix" ? PG_TRIM_FIX : PG_TRIM_ACCUMULATE;
                ClasscutNames(cl.Expression, &c.ClassColumns);
                c.Classes.push_back(cl);
            }
            if (why.empty()) {
                pg_classcut* set = nullptr;
                if (!CompileClasscut(c, &set, &why)) why = c.FilterType + ": " + why;
                else pg_classcut_free(set);
            }
        }
        else if (c.IsQuota()) {
            // NewPriorityAdjustCountFilter (priority_adjust_count_filter.go:44-78) / NewPriorityAdjustCountFilterV2
            // (priority_adjust_count_filter_v2.go:21-30): what pg_trim_out_cap / pg_trim2_out_cap refuse is refused here, by name
            const bool v2 = c.FilterType == "PriorityAdjustCountFilterV2";
            for (const auto& r : out->GpuRecalls) c.QuotaSources.push_back(r.Name);
            for (const char* key : {"EnsureDiversity", "DiversityMinCount", "DiversityDaoConf"})
                if (!v2 && why.empty() && fc.has(key)) why = std::string(key) + " (the filter's diversity branch is not served on the device)";
            const auto& confs = fc.at("AdjustCountConfs").arr;
            if (why.empty() && confs.empty()) why = "AdjustCountConfs is empty";
            if (why.empty() && confs.size() > PG_TRIM_MAX_RULES)
                why = std::to_string(confs.size()) + " AdjustCountConfs (the device serves up to " + std::to_string(PG_TRIM_MAX_RULES) + ")";
            for (size_t i = 0; why.empty() && i < confs.size(); ++i) {
                const std::string name = confs[i].s("RecallName"), type = confs[i].s("Type");
                const double count = confs[i].d("Count");
                const auto at = std::find(c.QuotaSources.begin(), c.QuotaSources.end(), name);
                if (at == c.QuotaSources.end()) why = "RecallName \"" + name + "\" is no recall of pairec_gpu.Recalls";
                else if (at - c.QuotaSources.begin() >= PG_TRIM_MAX_SOURCES)
                    why = "RecallName \"" + name + "\" is recall " + std::to_string(at - c.QuotaSources.begin()) + " (the device serves the first " +
                          std::to_string(PG_TRIM_MAX_SOURCES) + " recalls)";
                else if (confs[i].at("Count").type != json::Value::Number || count < 0 || count > 4294967295.0 || count != std::floor(count))
                    why = "Count of \"" + name + "\" is not a count";
                else if (type != "fix" && type != "accumulator")
                    why = "Type \"" + type + "\" of \"" + name + "\" (the reference serves fix and accumulator)";
                else
                    c.Quotas.push_back(pg_trim_rule{(uint8_t)(at - c.QuotaSources.begin()), (uint8_t)(type == "fix" ? PG_TRIM_FIX : PG_TRIM_ACCUMULATE),
                                                    (uint32_t)count});
            }
            uint32_t width = 0;
            if (why.empty() && (v2 ? pg_trim2_out_cap : pg_trim_out_cap)(c.Quotas.data(), (uint32_t)c.Quotas.size(), 1, &width) != PG_OK) {
                why = pg_last_error();
                const size_t colon = why.find(": ");                     // (the entry point's name says nothing here)
                if (colon != std::string::npos) why = why.substr(colon + 2);
            }
            if (!why.empty()) why = c.FilterType + ": " + why;
        }
        else if (c.IsDimcap()) {
            // NewDimensionFieldUniqueFilter (dimension_field_unique_filter.go:17-24) takes any Dimension; an empty one makes every
            // StringProperty "" and the filter a no-op, which a config never means
            c.Dimension = fc.s("Dimension");
            const json::Value& nv = fc.at("NullValue");
            if (c.Dimension.empty()) why = "DimensionFieldUniqueFilter: Dimension is empty";
            else if (!c.FeatureStore.empty() && c.FeatureStore != "item_features")
                why = "FeatureStore \"" + c.FeatureStore + "\" (the engine holds one store of item columns, \"item_features\")";
            else if (nv.type != json::Value::Null && (nv.type != json::Value::Number || nv.num != std::floor(nv.num) || std::fabs(nv.num) >= 9e15))
                why = "DimensionFieldUniqueFilter: NullValue is not an integer (the store's columns are integers: the code that stands for \"\")";
            else if (nv.type == json::Value::Number) {
                c.HasNullValue = true;
                c.NullValue = nv.is_int ? nv.i : (long long)nv.num;
            }
        }
        else if (c.FilterType != "ItemStateFilter") why = "unknown FilterType \"" + c.FilterType + "\" (the device serves ItemStateFilter)";
        else if (!c.FeatureStore.empty() && c.FeatureStore != "item_features")
            why = "FeatureStore \"" + c.FeatureStore + "\" (the engine holds one store of item columns, \"item_features\")";
        else CheckFilterParams(c.FilterParams, false, &why);
        if (!why.empty()) {
            if (err) *err = "pairec_gpu.Filters: " + c.Name + ": " + why;
            return false;
        }
        out->GpuFilters.push_back(c);
    }
    for (const auto& kv : out->UserDefineConfs.at("pairec_gpu").at("FilterNames").obj) out->GpuFilterNames[kv.first] = str_list(kv.second);
    return true;
}
}  // namespace recconf

// ---- algorithm -----------------------------------------------------------------------------------
namespace algorithm {
void AlgorithmFactory::RegisterAlgorithm(const std::string& name, std::shared_ptr<IAlgorithm> a) {
    std::lock_guard<std::mutex> g(mu_);
    algos_[name] = std::move(a);                            // overwrites (algorithm.go:164-168)
}
bool AlgorithmFactory::Run(const std::string& name, const AlgoData& data, AlgoResult* out, std::string* err) {
    std::shared_ptr<IAlgorithm> a;
    {
        std::lock_guard<std::mutex> g(mu_);
        auto it = algos_.find(name);
        if (it == algos_.end()) {
            if (err) *err = "not find algorithm, name:" + name;     // algorithm.go:113-115
            return false;
        }
        a = it->second;
    }
    return a->Run(data, out, err);
}
}  // namespace algorithm

// ---- response decoders ---------------------------------------------------------------------------
namespace algorithm {
namespace decode {
std::vector<AlgoResponse> EasyrecResponse(const std::vector<std::string>& item_ids,
                                          const std::map<std::string, std::vector<double>>& results) {
    std::vector<AlgoResponse> ret;                          // easyrec_response.go:226-232
    for (const auto& id : item_ids) {
        auto it = results.find(id);
        ret.emplace_back(it != results.end() && !it->second.empty() ? it->second[0] : 0.0);
    }
    return ret;
}
bool EasyrecMutValResponse(const std::vector<std::string>& item_ids, const std::vector<std::string>& outputs,
                           const std::map<std::string, std::vector<double>>& results,
                           std::vector<AlgoResponse>* out, std::string* err) {
    out->clear();                                           // easyrec_response.go:41-69
    for (const auto& id : item_ids) {
        AlgoResponse r;
        r.multiValModule = true;
        auto it = results.find(id);
        if (it != results.end()) {
            if (outputs.size() != it->second.size()) {
                if (err) *err = "outputs size is not equal scores";
                out->clear();
                return false;
            }
            for (size_t k = 0; k < outputs.size(); ++k) r.scoreArr[outputs[k]] = it->second[k];
        } else {
            for (const auto& o : outputs) r.scoreArr[o] = 0.0;
        }
        out->push_back(std::move(r));
    }
    return true;
}
bool EasyrecMutClassificationResponse(const std::vector<std::string>& item_ids,
                                      const std::map<std::string, std::pair<std::vector<float>, std::vector<long long>>>& tf_outputs,
                                      std::vector<AlgoResponse>* out, std::string* err) {
    out->assign(item_ids.size(), AlgoResponse());           // easyrec_response.go:145-199
    for (const auto& kv : tf_outputs) {
        const auto& vals = kv.second.first;
        const auto& shape = kv.second.second;
        const size_t width = shape.size() >= 2 ? (size_t)shape[1] : 1;        // [N, C] → C per item; [N] → 1
        if (vals.size() < item_ids.size() * width) {
            if (err) *err = "output " + kv.first + " holds fewer values than items";
            out->clear();
            return false;
        }
        for (size_t i = 0; i < item_ids.size(); ++i) {
            std::vector<double>& dst = (*out)[i].mulClassifyArr[kv.first];
            for (size_t c = 0; c < width; ++c) dst.push_back((double)vals[i * width + c]);   // float32 → float64
        }
    }
    return true;
}
double AlinkFMScore(double prediction_result, double prediction_score) {
    return prediction_result == 0.0 ? 1 - prediction_score : prediction_score;     // fm_response.go:28-34
}
std::vector<AlgoResponse> TFServingResponse(const std::vector<std::vector<double>>& outputs) {
    std::vector<AlgoResponse> ret;                          // tfserving/response.go:58-62
    for (const auto& val : outputs)
        for (double score : val) ret.emplace_back(score);
    return ret;
}
std::vector<AlgoResponse> WidenF32(const float* scores, size_t n) {
    std::vector<AlgoResponse> ret;
    for (size_t i = 0; i < n; ++i) ret.emplace_back((double)scores[i]);
    return ret;
}
std::vector<AlgoResponse> TfResponse(const std::vector<std::pair<std::string, OutputArray>>& outputs) {
    std::vector<AlgoResponse> ret;                          // tf_response.go:56-61: the first output only (`break`)
    if (!outputs.empty())
        for (float v : outputs[0].second.float_val) ret.emplace_back((double)v);
    return ret;
}
std::vector<AlgoResponse> TfMutValResponse(const std::vector<std::pair<std::string, OutputArray>>& outputs) {
    std::vector<AlgoResponse> ret;                          // tf_response.go:35-47
    for (const auto& kv : outputs)
        for (size_t i = 0; i < kv.second.float_val.size(); ++i) {
            if (i >= ret.size()) { ret.emplace_back(); ret.back().multiValModule = true; }
            ret[i].scoreArr[kv.first] = (double)kv.second.float_val[i];
        }
    return ret;
}
bool TorchrecMutValResponse(size_t n_items, const std::vector<std::pair<std::string, OutputArray>>& outputs,
                            std::vector<AlgoResponse>* out, std::string* err) {
    out->assign(n_items, AlgoResponse());                   // easyrec_response.go:474-491
    for (auto& r : *out) r.multiValModule = true;
    for (const auto& kv : outputs) {
        if (kv.second.size() < n_items) {                   // (the reference indexes FloatVal[i] and panics)
            if (err) *err = "output " + kv.first + " holds fewer values than items";
            out->clear();
            return false;
        }
        for (size_t i = 0; i < n_items; ++i) (*out)[i].scoreArr[kv.first] = kv.second.at(i);
    }
    return true;
}
bool TorchrecMutClassificationResponse(size_t n_items, const std::vector<std::pair<std::string, OutputArray>>& outputs,
                                       std::vector<AlgoResponse>* out, std::string* err) {
    out->assign(n_items, AlgoResponse());                   // easyrec_response.go:543-565
    for (const auto& kv : outputs) {
        const size_t dims = kv.second.shape.size();
        if (dims != 1 && dims != 2) continue;               // other ranks leave the output out of the map
        const size_t width = dims == 2 ? (size_t)kv.second.shape[1] : 1;
        if (kv.second.float_val.size() < n_items * width) {
            if (err) *err = "output " + kv.first + " holds fewer values than items";
            out->clear();
            return false;
        }
        for (size_t i = 0; i < n_items; ++i) {
            std::vector<double>& dst = (*out)[i].mulClassifyArr[kv.first];
            for (size_t c = 0; c < width; ++c) dst.push_back((double)kv.second.float_val[i * width + c]);
        }
    }
    return true;
}
bool TorchrecEmbeddingItemsResponse(const std::vector<std::string>& item_ids, const OutputArray* scores,
                                    std::vector<EmbeddingInfo>* out, std::string* err) {
    out->clear();                                           // easyrec_response.go:707-731
    for (size_t i = 0; i < item_ids.size(); ++i) {
        EmbeddingInfo info;
        info.ItemId = item_ids[i];
        if (scores) {
            if (i >= scores->size()) {
                if (err) *err = "match_item_scores holds fewer values than item_ids";
                out->clear();
                return false;
            }
            info.Score = scores->at(i);
        }
        out->push_back(info);
    }
    return true;
}
double PssmartScore(double score, const std::string& lable, const std::string& label) {
    return (lable == "0" || label == "0") ? 1 - score : score;       // pmml_response.go:24-31
}
}  // namespace decode
}  // namespace algorithm

// ---- recall --------------------------------------------------------------------------------------
namespace recall {
LoadOutcome CheckRecallConf(const recconf::RecallConfig& c) {
    const std::string& t = c.RecallType;
    auto panic = [](const std::string& m) { return LoadOutcome{LoadOutcome::kPanic, m}; };
    auto unavailable = [&](const std::string& what) {
        return LoadOutcome{LoadOutcome::kUnavailable, "recall " + c.Name + ": " + what + " is not available in the standalone mirror (no datasources)"};
    };
    auto one_of = [](const std::string& v, std::initializer_list<const char*> l) {
        for (const char* x : l) if (v == x) return true;
        return false;
    };
    if (t == "MockRecall" || t == "OnlineVectorRecall") return LoadOutcome{};       // constructors touch no datasource
    if (t == "VectorRecall") {                                // module.NewVectorDao (module/vector_dao.go:17-33)
        if (one_of(c.DaoAdapterType, {"redis", "hbase"}) || one_of(c.VectorDaoAdapterType, {"hologres", "mysql", "clickhouse", "be"}))
            return unavailable("a VectorDao over " + (c.DaoAdapterType.empty() ? c.VectorDaoAdapterType : c.DaoAdapterType));
        return panic("not found VectorDao implement");
    }
    if (t == "UserCustomRecall") {                            // module.NewUserCustomRecallDao (user_custom_recall_dao.go:12-28)
        if (one_of(c.DaoAdapterType, {"mysql", "tablestore", "hologres", "redis", "clickhouse", "featurestore"}))
            return unavailable("a UserCustomRecallDao over " + c.DaoAdapterType);
        return panic("not found UserCustomRecallDao implement");
    }
    if (one_of(t, {"HologresVectorRecall", "HologresVectorRecallV2", "I2IVectorRecall", "OnlineHologresVectorRecall"}))
        // holo.GetPostgres(VectorDaoConf.HologresName) → panic(err) (persist/holo: "Postgres not found, name:…")
        return panic("Postgres not found, name:" + c.HologresName);
    if (one_of(t, {"UserCollaborativeFilterRecall", "UserTopicRecall", "ItemCollaborativeFilterRecall", "UserGroupHotRecall",
                   "UserGlobalHotRecall", "ColdStartRecall", "BeRecall", "RealTimeU2IRecall", "GraphRecall", "OpenSearchRecall",
                   "RecallEngineRecall"}))
        return c.DaoAdapterType.empty() ? panic("not found " + t + " DAO implement (the constructor's DAO factory panics without DaoConf.AdapterType)")
                                        : unavailable("a DAO over " + c.DaoAdapterType);
    // unknown type — and "MilvusVectorRecall", whose constructor call is commented out (recall.go:78-79): recall stays nil
    return panic("recall empty, name:" + c.Name);
}
std::shared_ptr<Recall> Registry::GetRecall(const std::string& name, std::string* err) {
    auto it = recalls_.find(name);
    if (it == recalls_.end()) {
        if (err) *err = "recall:not found, name:" + name;
        return nullptr;
    }
    return it->second;
}
bool ParseWhereClause(const std::string& s, int time_interval, std::string* column, int* op, long long* value) {
    size_t p = 0;
    auto skip = [&]() { while (p < s.size() && isspace((unsigned char)s[p])) ++p; };
    skip();
    const size_t c0 = p;
    while (p < s.size() && (isalnum((unsigned char)s[p]) || s[p] == '_')) ++p;
    if (p == c0 || isdigit((unsigned char)s[c0])) return false;
    *column = s.substr(c0, p - c0);
    skip();
    static const struct { const char* text; int op; } kOps[] = {{">=", 1}, {"<=", 3}, {"!=", 5}, {"<>", 5}, {"==", 4}, {">", 0}, {"<", 2}, {"=", 4}};
    *op = -1;
    for (const auto& o : kOps)
        if (s.compare(p, strlen(o.text), o.text) == 0) { *op = o.op; p += strlen(o.text); break; }
    if (*op < 0) return false;
    skip();
    if (s.compare(p, 7, "${time}") == 0) {
        *value = (long long)time(nullptr) - (long long)time_interval;
        p += 7;
    } else {
        char* end = nullptr;
        errno = 0;
        *value = strtoll(s.c_str() + p, &end, 10);
        if (end == s.c_str() + p || errno) return false;
        p = (size_t)(end - s.c_str());
    }
    skip();
    return p == s.size();
}

std::vector<float> ParseVectorString(const std::string& s) {     // vector_recall.go:70-82
    std::vector<float> out;
    size_t p = 0;
    while (p <= s.size()) {
        size_t e = s.find(' ', p);
        if (e == std::string::npos) e = s.size();
        const std::string vc = s.substr(p, e - p);
        p = e + 1;
        const size_t c = vc.find(':');
        if (c == std::string::npos) continue;
        if (vc.find(':', c + 1) != std::string::npos) continue;       // len(vals) != 2
        const std::string val = vc.substr(c + 1);
        char* end = nullptr;
        const double d = strtod(val.c_str(), &end);
        // `value, _ := strconv.ParseFloat(vals[1], 32)`: a malformed number yields 0
        out.push_back((end != val.c_str() && *end == '\0') ? (float)d : 0.0f);
    }
    return out;
}
std::string FormatCacheString(const std::vector<module::ItemPtr>& items, const std::string& recall_name) {
    std::string out;                                               // vector_recall.go:105-110
    for (size_t i = 0; i < items.size(); ++i) {
        if (i) out.push_back(',');
        out += items[i]->Id + ":" + recall_name + ":" + GoFmtFloat(items[i]->Score);
    }
    return out;
}
bool ParseCacheString(const std::string& line, const std::string& recall_name, const std::string& item_type,
                      std::vector<module::ItemPtr>* out, std::string* err) {
    out->clear();                                                  // vector_recall.go:39-55
    size_t p = 0;
    while (p <= line.size()) {
        size_t e = line.find(',', p);
        if (e == std::string::npos) e = line.size();
        const std::string id = line.substr(p, e - p);
        p = e + 1;
        module::ItemPtr item;
        if (id.find(':') != std::string::npos) {
            std::vector<std::string> vars;
            size_t q = 0;
            while (q <= id.size()) {
                size_t c = id.find(':', q);
                if (c == std::string::npos) c = id.size();
                vars.push_back(id.substr(q, c - q));
                q = c + 1;
            }
            if (vars.size() < 3) {      // `vars[2]` would panic the reference (index out of range)
                if (err) *err = "recall cache entry \"" + id + "\": expected id:name:score";
                out->clear();
                return false;
            }
            item = std::make_shared<module::Item>(vars[0]);
            char* end = nullptr;
            const double f = strtod(vars[2].c_str(), &end);        // `f, _ := strconv.ParseFloat(vars[2], 64)`
            item->Score = (end != vars[2].c_str() && *end == '\0') ? f : 0.0;
        } else {
            item = std::make_shared<module::Item>(id);
        }
        item->RetrieveId = recall_name;
        item->ItemType = item_type;
        out->push_back(item);
        if (e == line.size()) break;
    }
    return true;
}
}  // namespace recall

// ---- filter --------------------------------------------------------------------------------------
namespace filter {
std::vector<module::ItemPtr> UniqueFilter(const std::vector<module::ItemPtr>& items) {
    std::vector<module::ItemPtr> out;
    std::map<module::ItemId, module::ItemPtr> uniq;
    for (const auto& item : items) {
        auto it = uniq.find(item->Id);
        if (it == uniq.end()) {
            uniq[item->Id] = item;
            out.push_back(item);
        } else {
            auto& exist = it->second;
            for (const auto& kv : item->algoScores) exist->AddAlgoScore(kv.first, kv.second);
            if (!exist->hasRecallScores) {
                exist->RecallScores = {{exist->RetrieveId, exist->Score}};
                exist->hasRecallScores = true;
            }
            exist->RecallScores[item->RetrieveId] = item->Score;
        }
    }
    return out;
}
}  // namespace filter

// ---- sort ----------------------------------------------------------------------------------------
namespace sort {
bool Registry::RegisterSort(const std::string& name, std::shared_ptr<ISort> s, std::string* err) {
    if (!s) { if (err) *err = "Sort is nil, name:" + name; return false; }      // sort.go:144-146 panics
    if (sorts_.count(name) == 0) sorts_[name] = std::move(s);                   // first registration wins
    return true;
}
std::shared_ptr<ISort> Registry::Get(const std::string& name) {
    auto it = sorts_.find(name);
    return it == sorts_.end() ? nullptr : it->second;
}
}  // namespace sort

// ---- GPU-backed plugins --------------------------------------------------------------------------
namespace {

std::string pg_err(const char* what) { return std::string(what) + ": " + pg_last_error(); }

// algorithm.IAlgorithm replacing FaissModel (algorithm/faiss/model.go:29-31)
struct GpuFaissAlgorithm : algorithm::IAlgorithm {
    Engine* e;
    explicit GpuFaissAlgorithm(Engine* eng) : e(eng) {}
    bool Init(const recconf::AlgoConfig&, std::string*) override { return true; }
    bool Run(const algorithm::AlgoData& data, algorithm::AlgoResult* out, std::string* err) override {
        if (data.kind != algorithm::AlgoData::kVector) { if (err) *err = "faiss: invalid request type"; return false; }
        const auto& req = data.vec;
        if (req.Vector.size() != e->dim) { if (err) *err = "faiss: vector dimension mismatch"; return false; }
        if (req.K == 0) return true;
        std::vector<uint64_t> rows(req.K);
        std::vector<float> scores(req.K);
        uint32_t cnt = 0;
        if (e->coalesce) {
            // one request per call, many calls at once (one goroutine per recall, service/recall.go:129-145): the library
            // batches them into shared table passes
            pg_coalescer* co = e->SceneCoalescer(req.K, err);
            if (!co) return false;
            if (pg_coalescer_recall(co, req.Vector.data(), rows.data(), scores.data(), &cnt) != PG_OK) {
                if (err) *err = pg_err("pg_coalescer_recall");
                return false;
            }
        } else if (pg_recall_topk(e->ctx, e->table, req.Vector.data(), 1, req.K, rows.data(), scores.data(), &cnt) != PG_OK) {
            if (err) *err = pg_err("pg_recall_topk");
            return false;
        }
        for (uint32_t i = 0; i < cnt; ++i) {
            out->reply.Retval.push_back(rows[i]);
            out->reply.Scores.push_back(scores[i]);
            out->reply.Labels.push_back(e->IdOfRow(rows[i]));
        }
        return true;
    }
};

// algorithm.IAlgorithm replacing EasModel / TFservingModel for the DNN rank model
struct GpuDnnAlgorithm : algorithm::IAlgorithm {
    Engine* e;
    std::string name;
    std::vector<std::string> outputs;            // empty: one score; else a multi-output model, one DNN3 head model per output
    GpuDnnAlgorithm(Engine* eng, std::string n, std::vector<std::string> outs) : e(eng), name(std::move(n)), outputs(std::move(outs)) {}
    bool Init(const recconf::AlgoConfig&, std::string*) override { return true; }
    bool Score(const pg_model* m, const algorithm::RankRequest& req, const std::vector<uint32_t>& rows, std::vector<float>* scores,
               std::string* err) {
        const uint32_t n = (uint32_t)rows.size();
        const uint32_t off[2] = {0, n};
        scores->resize(n);
        if (!m) { if (err) *err = "dnn: model of " + name + " not loaded"; return false; }
        if (e->coalesce && m == e->model) {
            // one call per 100-item batch and goroutine (rank_service.go:264-289): batched across callers by the library
            pg_coalescer* co = e->SceneCoalescer(0, err);
            if (!co) return false;
            if (pg_coalescer_rank_dnn3(co, req.UserVector.data(), rows.data(), n, scores->data()) != PG_OK) {
                if (err) *err = pg_err("pg_coalescer_rank_dnn3");
                return false;
            }
            return true;
        }
        if (pg_rank_dnn3(e->ctx, m, e->table, req.UserVector.data(), rows.data(), off, 1, scores->data()) != PG_OK) {
            if (err) *err = pg_err("pg_rank_dnn3");
            return false;
        }
        return true;
    }
    bool Run(const algorithm::AlgoData& data, algorithm::AlgoResult* out, std::string* err) override {
        if (data.kind != algorithm::AlgoData::kRank) { if (err) *err = "dnn: invalid request type"; return false; }
        const auto& req = data.rank;
        const uint32_t n = (uint32_t)req.ItemIds.size();
        std::vector<uint32_t> rows(n);
        for (uint32_t i = 0; i < n; ++i)
            if (!e->RowOfId(req.ItemIds[i], &rows[i])) { if (err) *err = "dnn: unknown item id " + req.ItemIds[i]; return false; }
        std::vector<float> scores;
        if (outputs.empty()) {
            if (!Score(e->model, req, rows, &scores, err)) return false;
            out->responses = algorithm::decode::WidenF32(scores.data(), n);             // float32 → float64 widening
            return true;
        }
        // multi-output model (EasyrecResponse.multiValModule, easyrec_response.go:35-70): GetModuleType() = true and a score
        // per output name; RankService writes them as "<algo>_<output>" (rank_service.go:315-319)
        out->responses.assign(n, algorithm::AlgoResponse());
        auto mh = e->named_models.find(name);
        if (mh != e->named_models.end()) {
            // the model as exported: ONE trunk, one head per output (PG_MODEL_DNN3_MULTI) — one gather, one launch
            uint32_t heads = 0;
            pg_model_num_outputs(mh->second, &heads);
            if (heads != outputs.size()) {
                if (err) *err = "dnn: model of " + name + " has " + std::to_string(heads) + " outputs, the algorithm names " +
                                std::to_string(outputs.size());
                return false;
            }
            std::vector<float> planes((size_t)heads * n);
            const uint32_t off[2] = {0, n};
            if (req.UserVector.empty()) { if (err) *err = "dnn: no user vector"; return false; }
            if (pg_rank_dnn3(e->ctx, mh->second, e->table, req.UserVector.data(), rows.data(), off, 1, planes.data()) != PG_OK) {
                if (err) *err = pg_err("pg_rank_dnn3");
                return false;
            }
            for (uint32_t i = 0; i < n; ++i) {
                out->responses[i].multiValModule = true;
                for (uint32_t o = 0; o < heads; ++o) out->responses[i].scoreArr[outputs[o]] = (double)planes[(size_t)o * n + i];
            }
            return true;
        }
        for (const auto& o : outputs) {
            auto it = e->named_models.find(name + "/" + o);
            if (!Score(it == e->named_models.end() ? nullptr : it->second, req, rows, &scores, err)) return false;
            for (uint32_t i = 0; i < n; ++i) {
                out->responses[i].multiValModule = true;
                out->responses[i].scoreArr[o] = (double)scores[i];
            }
        }
        return true;
    }
};

// algorithm.IAlgorithm for the EasyRec flavour (service/rank/algo_data.go:79-86, algorithm/eas/easyrec_request.go:20-73):
// the request names item ids; the per-item context features are device columns (pg_features_*), the user side arrives
// as a dense vector + dictionary-encoded categorical ids.  FM + two-tower predict (pg_rank_fm2t_rows).
struct GpuFm2tAlgorithm : algorithm::IAlgorithm {
    Engine* e;
    std::vector<std::string> columns;
    GpuFm2tAlgorithm(Engine* eng, std::vector<std::string> cols) : e(eng), columns(std::move(cols)) {}
    bool Init(const recconf::AlgoConfig&, std::string*) override { return true; }
    bool Run(const algorithm::AlgoData& data, algorithm::AlgoResult* out, std::string* err) override {
        if (data.kind != algorithm::AlgoData::kRank) { if (err) *err = "fm2t: invalid request type"; return false; }
        if (!e->fm2t || !e->feats) { if (err) *err = "fm2t: model or feature columns not loaded"; return false; }
        const auto& req = data.rank;
        const uint32_t n = (uint32_t)req.ItemIds.size();
        std::vector<uint32_t> rows(n);
        for (uint32_t i = 0; i < n; ++i)
            if (!e->RowOfId(req.ItemIds[i], &rows[i])) { if (err) *err = "fm2t: unknown item id " + req.ItemIds[i]; return false; }
        std::vector<int32_t> cols;
        for (const auto& c : columns) {
            const int idx = pg_features_column_index(e->feats, c.c_str());
            if (idx < 0) { if (err) *err = "fm2t: no feature column " + c; return false; }
            cols.push_back(idx);
        }
        const uint32_t off[2] = {0, n};
        std::vector<float> scores(n);
        if (req.UserVector.size() != e->fm2t_d_user || req.UserFieldIds.size() < e->fm2t_nuf) {
            if (err) *err = "fm2t: user vector / field ids do not match the model";
            return false;
        }
        if (e->coalesce && columns == e->fm2t_columns) {
            // 50 calls of 100 items per request, from as many goroutines (rank_service.go:264-289): one launch for all of them
            pg_coalescer* co = e->SceneCoalescer(0, err);
            if (!co) return false;
            if (pg_coalescer_rank_fm2t(co, req.UserVector.data(), req.UserFieldIds.data(), rows.data(), n, scores.data()) != PG_OK) {
                if (err) *err = pg_err("pg_coalescer_rank_fm2t");
                return false;
            }
        } else if (pg_rank_fm2t_rows(e->ctx, e->fm2t, e->feats, cols.data(), req.UserVector.data(), req.UserFieldIds.data(), rows.data(), off, 1,
                                     scores.data()) != PG_OK) {
            if (err) *err = pg_err("pg_rank_fm2t_rows");
            return false;
        }
        out->responses = algorithm::decode::WidenF32(scores.data(), n);
        return true;
    }
};

// algorithm.IAlgorithm of a vector model serving an OnlineVectorRecall: user features → user embedding → its
// FaissNeighNum nearest items (torchrecEmbeddingItemsResponseFunc, easyrec_response.go:700-734)
struct GpuOnlineVectorAlgorithm : algorithm::IAlgorithm {
    Engine* e;
    explicit GpuOnlineVectorAlgorithm(Engine* eng) : e(eng) {}
    bool Init(const recconf::AlgoConfig&, std::string*) override { return true; }
    bool Run(const algorithm::AlgoData& data, algorithm::AlgoResult* out, std::string* err) override {
        if (data.kind != algorithm::AlgoData::kEmbedding) { if (err) *err = "online vector: invalid request type"; return false; }
        if (!e->fm2t || !e->item_emb) { if (err) *err = "online vector: vector model or item-embedding table not loaded"; return false; }
        const uint32_t k = (uint32_t)std::max(data.emb.FaissNeighNum, 0);
        if (k == 0) return true;
        std::vector<uint64_t> rows(k);
        std::vector<float> scores(k);
        uint32_t cnt = 0;
        if (data.emb.UserVector.size() != e->fm2t_d_user) { if (err) *err = "online vector: user vector width does not match the model"; return false; }
        if (e->coalesce) {
            pg_coalescer* co = e->OnlineCoalescer(k, err);
            if (!co) return false;
            if (pg_coalescer_online_recall(co, data.emb.UserVector.data(), rows.data(), scores.data(), &cnt) != PG_OK) {
                if (err) *err = pg_err("pg_coalescer_online_recall");
                return false;
            }
        } else if (pg_online_vector_recall(e->ctx, e->fm2t, e->item_emb, data.emb.UserVector.data(), 1, k, rows.data(), scores.data(), &cnt) != PG_OK) {
            if (err) *err = pg_err("pg_online_vector_recall");
            return false;
        }
        for (uint32_t i = 0; i < cnt; ++i) out->embeddingItems.push_back({e->IdOfRow(rows[i]), (double)scores[i]});
        return true;
    }
};

// recall.Recall with the body of VectorRecall.GetCandidateItems (vector_recall.go:32-123, cache omitted)
struct GpuVectorRecall : recall::Recall, recall::ICloneRecall {
    Engine* e;
    recconf::RecallConfig conf;
    std::shared_ptr<cache::Cache> cache_;                      // BaseRecall.cache (recall.go:123-137)
    int cacheTime = 1800;
    std::mutex cloneMu;
    std::map<std::string, std::shared_ptr<recall::Recall>> cloneInstances;
    GpuVectorRecall(Engine* eng, recconf::RecallConfig c) : e(eng), conf(std::move(c)) {
        if (!conf.CacheAdapter.empty()) {
            std::string cerr;
            cache_ = cache::NewCache(conf.CacheAdapter, conf.CacheConfig, &cerr);   // error → logged, no cache
            if (conf.CacheTime > 0) cacheTime = conf.CacheTime;
        }
    }
    std::string GetRecallName() const override { return conf.Name; }
    // cloneWithBuilder (recall.go:167-214): instance-local cache keyed by the params' canonical JSON (Go
    // marshals maps with sorted keys and takes an md5 of that; the text itself is the key here), params
    // unmarshalled over a zero RecallConfig, Name forced to the original
    std::shared_ptr<recall::Recall> CloneWithConfig(const json::Value& params) override {
        if (params.type != json::Value::Object) return nullptr;
        std::string key;
        for (const auto& kv : params.obj) {                    // std::map iterates in key order
            key += kv.first + "=";
            key += kv.second.type == json::Value::String ? kv.second.str : json::NumToString(kv.second.num);
            key += ";";
        }
        std::lock_guard<std::mutex> g(cloneMu);
        auto it = cloneInstances.find(key);
        if (it != cloneInstances.end()) return it->second;
        recconf::RecallConfig c;
        c.Name = conf.Name;
        c.RecallType = params.s("RecallType"); c.RecallAlgo = params.s("RecallAlgo");
        c.ItemType = params.s("ItemType"); c.CacheAdapter = params.s("CacheAdapter");
        c.CacheConfig = params.s("CacheConfig"); c.CachePrefix = params.s("CachePrefix");
        c.RecallCount = (int)params.n("RecallCount"); c.CacheTime = (int)params.n("CacheTime");
        auto inst = std::make_shared<GpuVectorRecall>(e, c);
        cloneInstances[key] = inst;
        return inst;
    }
    std::vector<module::ItemPtr> GetCandidateItems(module::User* user, context::RecommendContext*) override {
        std::vector<module::ItemPtr> ret;
        std::string value, err;
        if (cache_) {                                                                   // vector_recall.go:35-58
            const cache::Value v = cache_->Get(conf.CachePrefix + user->Id);
            if (v.kind == cache::Value::kBytes) {                                       // `cacheRet.([]uint8)`
                if (recall::ParseCacheString(v.data, conf.Name, conf.ItemType, &ret, &err)) return ret;
                ret.clear();
            }
        }
        if (!e->user_vectors.VectorString(user->Id, &value, &err)) return ret;        // logged, empty result
        algorithm::AlgoData data;
        data.kind = algorithm::AlgoData::kVector;
        data.vec.K = (uint32_t)conf.RecallCount;
        data.vec.Vector = recall::ParseVectorString(value);
        if (data.vec.Vector.empty()) return ret;                                       // "user Vector empty"
        algorithm::AlgoResult result;
        if (!e->algorithms.Run(conf.RecallAlgo, data, &result, &err)) return ret;      // logged, empty result
        for (size_t i = 0; i < result.reply.Labels.size(); ++i) {
            auto item = std::make_shared<module::Item>(result.reply.Labels[i]);
            item->RetrieveId = conf.Name;
            item->ItemType = conf.ItemType;
            item->Score = (double)result.reply.Scores[i];
            ret.push_back(item);
        }
        if (cache_ && !ret.empty())                                                     // :103-120 (async in Go)
            cache_->Put(conf.CachePrefix + user->Id, recall::FormatCacheString(ret, conf.Name), cacheTime);
        return ret;
    }
};

// recall.Recall with the body of I2IVectorRecall.GetCandidateItems (item_2_item_vector_racall.go:51-152): the trigger is
// the request's "item_id" parameter, its embedding (dao.VectorString) the query
struct GpuI2IVectorRecall : recall::Recall {
    Engine* e;
    recconf::RecallConfig conf;
    GpuI2IVectorRecall(Engine* eng, recconf::RecallConfig c) : e(eng), conf(std::move(c)) {}
    std::vector<module::ItemPtr> GetCandidateItems(module::User*, context::RecommendContext* ctx) override {
        std::vector<module::ItemPtr> ret;
        uint32_t row = 0;
        if (!ctx || !e->RowOfId(ctx->GetParameter("item_id"), &row)) return ret;       // VectoryEmptyError: logged, empty
        const uint32_t k = (uint32_t)std::max(conf.RecallCount, 0);
        if (k == 0) return ret;
        std::vector<uint64_t> rows(k);
        std::vector<float> scores(k);
        uint32_t cnt = 0;
        if (e->coalesce) {
            std::string cerr;
            pg_coalescer* co = e->SceneCoalescer(k, &cerr);
            if (!co || pg_coalescer_i2i_recall(co, row, rows.data(), scores.data(), &cnt) != PG_OK) return ret;
        } else if (pg_i2i_recall(e->ctx, e->table, &row, 1, e->table, k, rows.data(), scores.data(), &cnt) != PG_OK) {
            return ret;
        }
        for (uint32_t i = 0; i < cnt; ++i) {
            auto item = std::make_shared<module::Item>(e->IdOfRow(rows[i]));
            item->RetrieveId = conf.Name;
            item->ItemType = conf.ItemType;
            item->Score = (double)scores[i];                                            // `distance float64` (:130-139)
            ret.push_back(item);
        }
        return ret;
    }
};

// recall.Recall with the bodies of HologresVectorRecall.GetCandidateItems (service/recall/hologres_vector_recall.go:94-206: "ORDER
// BY pm_approx_inner_product_distance(emb, $1) desc LIMIT RecallCount", :23) and HologresVectorRecallV2.GetCandidateItems
// (hologres_vector_recall_v2.go:96-206: "ORDER BY pm_approx_squared_euclidean_distance(emb, $1) LIMIT RecallCount", :23): the user's
// embedding from the VectorDao (handed to the SQL as it is — "v1,v2,…" or "{v1,v2,…}", module/vector_hologres_dao.go:67-114; the
// libsvm form of the other DAOs is accepted too), the RecallCount items of largest inner product (descending) / smallest squared
// Euclidean distance (ascending), Score = distance (v1 :175-183, v2 :181-189), among the rows the WhereClause admits (:56-61).
// (The user-vector cache of :100-115 is the VectorDao's business here; the result cache of :118-143 / :191-204 is GpuVectorRecall's.)
struct GpuHologresVectorRecall : recall::Recall {
    Engine* e;
    recconf::RecallConfig conf;
    bool l2;
    GpuHologresVectorRecall(Engine* eng, recconf::RecallConfig c, bool squared_euclidean = true) : e(eng), conf(std::move(c)), l2(squared_euclidean) {}
    static std::vector<float> ParseEmbedding(const std::string& s) {
        if (s.find(':') != std::string::npos) return recall::ParseVectorString(s);
        std::vector<float> out;
        size_t p = 0;
        while (p < s.size()) {
            while (p < s.size() && (s[p] == '{' || s[p] == '}' || s[p] == ',' || s[p] == ' ')) ++p;
            if (p >= s.size()) break;
            char* end = nullptr;
            const double d = strtod(s.c_str() + p, &end);
            if (end == s.c_str() + p) break;
            out.push_back((float)d);
            p = (size_t)(end - s.c_str());
        }
        return out;
    }
    std::vector<module::ItemPtr> GetCandidateItems(module::User* user, context::RecommendContext*) override {
        std::vector<module::ItemPtr> ret;
        std::string value, err;
        if (!e->user_vectors.VectorString(user->Id, &value, &err) || value.empty()) return ret;      // (:105-110) logged unless VectoryEmptyError
        user->Properties[conf.Name + "_embedding"] = json::Value::Str(value);                        // user.AddProperty (:111)
        const std::vector<float> vec = ParseEmbedding(value);
        const uint32_t k = (uint32_t)std::max(conf.RecallCount, 0);
        if (k == 0 || vec.size() != e->dim) return ret;                                               // the SQL would fail: logged, empty (:170-176)
        std::vector<uint64_t> rows(k);
        std::vector<float> dist(k);
        uint32_t cnt = 0;
        if (conf.WhereOp >= 0) {
            // the admitted rows as a view of the table, built by the first request of a table generation; concurrent requests
            // share its passes through the view's own coalescer
            const Engine::FilterView* fv = e->ViewFor(conf, k);
            if (!fv || fv->empty) return ret;               // unknown column: the SQL would fail (logged, empty :170-176); nothing admitted
            int rc;
            if (fv->co)
                rc = l2 ? pg_coalescer_recall_l2(fv->co, vec.data(), rows.data(), dist.data(), &cnt)
                        : pg_coalescer_recall(fv->co, vec.data(), rows.data(), dist.data(), &cnt);
            else if (fv->view)
                rc = l2 ? pg_recall_topk_l2(e->ctx, fv->view, vec.data(), 1, k, rows.data(), dist.data(), &cnt)
                        : pg_recall_topk(e->ctx, fv->view, vec.data(), 1, k, rows.data(), dist.data(), &cnt);
            else                                            // the view could not be built (memory): filter per call
                rc = pg_recall_topk_where(e->ctx, e->table, e->feats, pg_features_column_index(e->feats, conf.WhereColumn.c_str()), conf.WhereOp,
                                          conf.WhereValue, l2 ? 1 : 0, vec.data(), 1, k, rows.data(), dist.data(), &cnt);
            if (rc != PG_OK) return ret;
        } else if (e->coalesce) {                           // concurrent requests share the exact pass
            std::string cerr;
            pg_coalescer* co = e->SceneCoalescer(k, &cerr);
            if (!co) return ret;
            const int rc = l2 ? pg_coalescer_recall_l2(co, vec.data(), rows.data(), dist.data(), &cnt)
                              : pg_coalescer_recall(co, vec.data(), rows.data(), dist.data(), &cnt);
            if (rc != PG_OK) return ret;
        } else if ((l2 ? pg_recall_topk_l2(e->ctx, e->table, vec.data(), 1, k, rows.data(), dist.data(), &cnt)
                       : pg_recall_topk(e->ctx, e->table, vec.data(), 1, k, rows.data(), dist.data(), &cnt)) != PG_OK) {
            return ret;
        }
        for (uint32_t i = 0; i < cnt; ++i) {
            auto item = std::make_shared<module::Item>(e->IdOfRow(rows[i]));
            item->RetrieveId = conf.Name;
            item->ItemType = conf.ItemType;
            item->Score = (double)dist[i];                                                            // `item.Score = distance` (:189)
            ret.push_back(item);
        }
        return ret;
    }
};

// recall.Recall that returns the FINISHED page: recall → DNN rank → RankScore → ItemRankScore sort all happen where the
// rows live, one single-request call into the library's coalescer (pg_coalescer_recommend), and only ctx.Size items are
// materialised on the host.  A scene served this way names it as its only recall and leaves RankConf / SortNames empty
// (the default ItemRankScore sort keeps the order: Score is the fused score).  The reference has no such plug-in — it
// is what its Recall interface permits (recall.go:18-20) once the stages behind it are local.
struct GpuPageRecall : recall::Recall {
    Engine* e;
    recconf::RecallConfig conf;
    GpuPageRecall(Engine* eng, recconf::RecallConfig c) : e(eng), conf(std::move(c)) {}
    std::vector<module::ItemPtr> GetCandidateItems(module::User* user, context::RecommendContext* ctx) override {
        std::vector<module::ItemPtr> ret;
        std::string value, err;
        if (!e->user_vectors.VectorString(user->Id, &value, &err)) return ret;          // logged, empty result
        const std::vector<float> vec = recall::ParseVectorString(value);
        if (vec.size() != e->dim) return ret;                                           // (logged) the library copies exactly dim floats
        pg_coalescer* co = e->PageCoalescer(conf, &err);
        if (!co) return ret;                                                            // logged, empty result
        const uint32_t size = (uint32_t)std::max(1, std::min(ctx ? ctx->Size : 10, std::min(conf.RecallCount, 1000)));
        std::vector<uint64_t> rows(size);
        std::vector<float> rec(size), rnk(size);
        std::vector<double> fused(size);
        uint32_t cnt = 0;
        if (pg_coalescer_recommend(co, vec.data(), size, rows.data(), rec.data(), rnk.data(), fused.data(), &cnt) != PG_OK) return ret;
        for (uint32_t i = 0; i < cnt; ++i) {
            auto item = std::make_shared<module::Item>(e->IdOfRow(rows[i]));
            item->RetrieveId = conf.Name;
            item->ItemType = conf.ItemType;
            item->Score = fused[i];
            item->AddProperty("recall_score", json::Value::Num((double)rec[i]));                        // what ${current_score} leaves behind
            item->AddAlgoScore(conf.RankVar, (double)rnk[i]);
            ret.push_back(item);
        }
        return ret;
    }
};

// recall.Recall with the body of OnlineVectorRecall.GetCandidateItems (online_vector_recall.go:73-155, cache omitted):
// user features → PBRequest{FaissNeighNum = recallCount} → algorithm.Run(recallAlgo) → embedding items → Items
struct GpuOnlineVectorRecall : recall::Recall {
    Engine* e;
    recconf::RecallConfig conf;
    GpuOnlineVectorRecall(Engine* eng, recconf::RecallConfig c) : e(eng), conf(std::move(c)) {}
    std::vector<module::ItemPtr> GetCandidateItems(module::User* user, context::RecommendContext*) override {
        std::vector<module::ItemPtr> ret;
        std::string value, err;
        if (!e->user_vectors.VectorString(user->Id, &value, &err)) return ret;
        algorithm::AlgoData data;
        data.kind = algorithm::AlgoData::kEmbedding;
        data.emb.UserVector = recall::ParseVectorString(value);
        data.emb.FaissNeighNum = conf.RecallCount;
        algorithm::AlgoResult result;
        if (!e->algorithms.Run(conf.RecallAlgo, data, &result, &err)) return ret;       // logged, empty result
        // only the TorchRec vector flavours carry embedding items (:118-133)
        if (conf.VectorAlgoType != "torchrec_tdm" && conf.VectorAlgoType != "torchrec_vector") return ret;
        for (const auto& info : result.embeddingItems) {
            auto item = std::make_shared<module::Item>(info.ItemId);
            item->Score = info.Score;
            item->RetrieveId = conf.Name;
            ret.push_back(item);
        }
        if (conf.RecallCount > 0 && (int)ret.size() > conf.RecallCount) ret.resize((size_t)conf.RecallCount);
        return ret;
    }
};

// recall.Recall with the body of OnlineHologresVectorRecall.GetCandidateItems (online_hologres_vector_recall.go:105-237, result
// cache omitted): the user's features → the vector model's USER TOWER on the device (the reference asks a PAI-EAS model for
// EasyrecUserEmbResponse.GetUserEmb, :120-131, and keeps it in userVectorCache, :109-112,133) → the RecallCount rows of the
// Hologres vector table with the largest inner product (`pm_approx_inner_product_distance(...) ORDER BY distance desc`, :27),
// restricted by HologresVectorConf.WhereClause (:59-63) — Item.Score = distance, RetrieveId = the recall's name (:208-210).
// The vector table is the engine's item-embedding table (UserDefineConfs.pairec_gpu.OnlineVector), the clause's column an
// int32 feature column keyed by its rows.  One embedding per user (the reference splits GetUserEmb on "|" for multi-interest
// models and gives every part RecallCount / parts rows, :188-196).
struct GpuOnlineHologresVectorRecall : recall::Recall {
    Engine* e;
    recconf::RecallConfig conf;
    struct CachedEmb { std::vector<float> v; std::chrono::steady_clock::time_point used; };
    std::mutex mu;
    std::map<std::string, CachedEmb> userVectorCache;              // cache.WithMaximumSize(10000), expire-after-access cacheTime + 10 s (:74-77)
    GpuOnlineHologresVectorRecall(Engine* eng, recconf::RecallConfig c) : e(eng), conf(std::move(c)) {}
    bool UserEmbedding(const std::string& uid, const std::vector<float>& uv, std::vector<float>* emb) {
        const auto now = std::chrono::steady_clock::now();
        const auto ttl = std::chrono::seconds(std::max(conf.CacheTime, 0) + 10);
        {
            std::lock_guard<std::mutex> g(mu);
            auto it = userVectorCache.find(conf.CachePrefix + uid);
            if (it != userVectorCache.end() && now - it->second.used <= ttl) {
                it->second.used = now;
                *emb = it->second.v;
                return true;
            }
        }
        emb->assign(e->dim_item_emb(), 0.0f);
        if (pg_fm2t_user_embedding(e->ctx, e->fm2t, uv.data(), 1, emb->data()) != PG_OK) return false;     // logged, empty (:123-125)
        std::lock_guard<std::mutex> g(mu);
        if (userVectorCache.size() >= 10000) userVectorCache.erase(userVectorCache.begin());
        userVectorCache[conf.CachePrefix + uid] = CachedEmb{*emb, now};
        return true;
    }
    std::vector<module::ItemPtr> GetCandidateItems(module::User* user, context::RecommendContext*) override {
        std::vector<module::ItemPtr> ret;
        std::string value, err;
        if (!e->fm2t || !e->item_emb) return ret;                                                  // no model / vector table: logged, empty
        if (!e->user_vectors.VectorString(user->Id, &value, &err)) return ret;
        const std::vector<float> uv = recall::ParseVectorString(value);
        const uint32_t k = (uint32_t)std::max(conf.RecallCount, 0);
        if (k == 0 || uv.size() != e->fm2t_d_user) return ret;
        std::vector<uint64_t> rows(k);
        std::vector<float> dist(k);
        uint32_t cnt = 0;
        int rc;
        if (conf.WhereOp >= 0) {
            std::vector<float> emb;
            if (!UserEmbedding(user->Id, uv, &emb)) return ret;
            const Engine::FilterView* fv = e->ViewFor(conf, k, e->item_emb);
            if (!fv || fv->empty) return ret;                   // unknown column: the SQL would fail (logged, empty); nothing admitted
            if (fv->co) rc = pg_coalescer_recall(fv->co, emb.data(), rows.data(), dist.data(), &cnt);
            else if (fv->view) rc = pg_recall_topk(e->ctx, fv->view, emb.data(), 1, k, rows.data(), dist.data(), &cnt);
            else rc = pg_recall_topk_where(e->ctx, e->item_emb, e->feats, pg_features_column_index(e->feats, conf.WhereColumn.c_str()), conf.WhereOp,
                                           conf.WhereValue, 0, emb.data(), 1, k, rows.data(), dist.data(), &cnt);
        } else if (e->coalesce) {                               // tower + search of concurrent requests in one pass
            pg_coalescer* co = e->OnlineCoalescer(k, &err);
            if (!co) return ret;
            rc = pg_coalescer_online_recall(co, uv.data(), rows.data(), dist.data(), &cnt);
        } else {
            rc = pg_online_vector_recall(e->ctx, e->fm2t, e->item_emb, uv.data(), 1, k, rows.data(), dist.data(), &cnt);
        }
        if (rc != PG_OK) return ret;
        for (uint32_t i = 0; i < cnt; ++i) {
            auto item = std::make_shared<module::Item>(e->IdOfRow(rows[i]));
            item->RetrieveId = conf.Name;
            item->Score = (double)dist[i];
            ret.push_back(item);
        }
        return ret;
    }
};

// MockRecall (service/recall/mock_recall.go:27-41): recallCount random ids with random scores
struct MockRecall : recall::Recall {
    recconf::RecallConfig conf;
    explicit MockRecall(recconf::RecallConfig c) : conf(std::move(c)) {}
    std::vector<module::ItemPtr> GetCandidateItems(module::User*, context::RecommendContext*) override {
        std::vector<module::ItemPtr> ret;
        uint64_t s = 0x9E3779B97F4A7C15ull;
        while ((int)ret.size() < conf.RecallCount) {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            auto item = std::make_shared<module::Item>(std::to_string((uint32_t)(s >> 32)));
            item->RetrieveId = conf.Name;
            item->Score = (double)(s >> 11) * (1.0 / 9007199254740992.0);
            ret.push_back(item);
        }
        return ret;
    }
};

bool sort_items(Engine* e, sort::SortData* d, bool desc, std::string* err) {
    const uint32_t n = (uint32_t)d->Data.size();
    if (n == 0) return true;
    std::vector<double> s(n);
    for (uint32_t i = 0; i < n; ++i) s[i] = d->Data[i]->Score;
    const uint32_t seg[2] = {0, n};
    std::vector<uint32_t> order(n);
    if (pg_sort_scores(e->ctx, s.data(), seg, 1, desc ? 1 : 0, order.data()) != PG_OK) {
        if (err) *err = pg_err("pg_sort_scores");
        return false;                                   // caller ignores the error; Data left untouched
    }
    std::vector<module::ItemPtr> out(n);
    for (uint32_t i = 0; i < n; ++i) out[i] = d->Data[order[i]];
    d->Data.swap(out);
    return true;
}
struct GpuItemRankScoreSort : sort::ISort {              // sort/item_rank_score.go:26-32 (descending)
    Engine* e;
    explicit GpuItemRankScoreSort(Engine* eng) : e(eng) {}
    bool Sort(sort::SortData* d, std::string* err) override { return sort_items(e, d, true, err); }
};
struct GpuItemScoreSort : sort::ISort {                  // sort/item_score.go:36-41 (ascending)
    Engine* e;
    explicit GpuItemScoreSort(Engine* eng) : e(eng) {}
    bool Sort(sort::SortData* d, std::string* err) override { return sort_items(e, d, false, err); }
};
struct GpuDPPSort : sort::ISort {                        // sort/dpp_sort.go:108-351 (embedding table = item table)
    Engine* e;
    recconf::DPPSortConfig conf;
    GpuDPPSort(Engine* eng, recconf::DPPSortConfig c) : e(eng), conf(std::move(c)) {}
    // doSort (:271-351): experiment parameters override the config (:275-278,374,382)
    bool DoSort(std::vector<module::ItemPtr>* itemsp, sort::SortData* d, std::string* err) {
        auto& items = *itemsp;
        if (items.empty()) return true;
        const int size = d->Context ? d->Context->Size : 10;
        const context::RecommendContext none;
        const context::RecommendContext& cx = d->Context ? *d->Context : none;
        int window = (int)cx.GetInt("dpp_window_size", conf.WindowSize > 0 ? conf.WindowSize : 10);
        const int candidateCnt = (int)cx.GetInt("dpp_candidate_count", conf.CandidateCount);
        const double minScorePercent = cx.GetFloat("dpp_min_score_percent", conf.MinScorePercent);
        const double alpha = cx.GetFloat("dpp_alpha", conf.Alpha);
        const int doNorm = (int)cx.GetInt("dpp_norm_relevance_score", 0);
        if ((candidateCnt > 0 || minScorePercent > 0) && (int)items.size() > size) {   // :280-300
            sort::SortData tmp = *d;
            tmp.Data = items;
            if (!sort_items(e, &tmp, true, err)) return false;
            items.swap(tmp.Data);
            if (candidateCnt > 0) {
                const size_t cnt = (size_t)std::max(size, candidateCnt);
                if (cnt < items.size()) items.resize(cnt);
            }
            if (minScorePercent > 0 && (int)items.size() > size) {
                size_t idx = (size_t)size;
                const double mx = items[0]->Score;
                for (; idx < items.size(); ++idx)
                    if (items[idx]->Score / mx < minScorePercent) break;
                items.resize(idx);
            }
        }
        const uint32_t n = (uint32_t)items.size();
        std::vector<uint32_t> rows(n);
        std::vector<double> rel(n), used(n);
        for (uint32_t i = 0; i < n; ++i) {
            if (!e->RowOfId(items[i]->Id, &rows[i])) { if (err) *err = "dpp: unknown item id"; return false; }
            rel[i] = items[i]->Score;
        }
        pg_dpp_options o;
        memset(&o, 0, sizeof o);
        o.alpha = alpha;
        o.topn = (uint32_t)std::max(size, 0);
        o.window = (uint32_t)std::max(window, 0);
        o.normalize_emb = conf.NormalizeEmb ? 1 : 0;
        o.ensure_pos_similarity = conf.EnsurePositiveSim ? 1 : 0;
        o.norm_relevance_score = (doNorm == 1 || doNorm == 2) ? doNorm : 0;
        o.has_table = 1;
        std::vector<uint32_t> idx((size_t)std::max(size, 1));
        uint32_t cnt = 0;
        int rc;
        std::string cerr;                               // (a failed coalescer falls back to the direct call: not this call's error)
        pg_coalescer* co = e->coalesce ? e->SceneCoalescer(0, &cerr) : nullptr;
        // SortService.Sort runs once per request, requests overlap (sort/sort.go:65-125): equal-shaped DPP calls share a launch
        if (co && n <= 1024) rc = pg_coalescer_dpp(co, rows.data(), rel.data(), n, &o, nullptr, idx.data(), &cnt, used.data());
        else rc = pg_dpp_ex(e->ctx, e->table, rows.data(), rel.data(), n, &o, nullptr, idx.data(), &cnt, used.data());
        if (rc == PG_ERR_ARITH) return true;            // "all item score is zero": KernelMatrix errs, items stay as they are (:314-317)
        if (rc != PG_OK) {
            if (err) *err = pg_err("pg_dpp");
            return false;
        }
        for (uint32_t i = 0; i < n; ++i) items[i]->AddAlgoScore("dpp_relevance_score", used[i]);     // :410
        std::vector<module::ItemPtr> out;
        for (uint32_t i = 0; i < cnt; ++i) out.push_back(items[idx[i]]);
        items.swap(out);
        return true;
    }
    bool Sort(sort::SortData* d, std::string* err) override {
        auto& items = d->Data;
        if (items.empty()) return true;
        if (conf.AbortRunCount > 0 && (int)items.size() <= conf.AbortRunCount)      // :127-132
            return sort_items(e, d, true, err);
        if (!conf.FilterRetrieveIds.empty()) {                                       // :134-160
            std::vector<module::ItemPtr> backup, selected;
            for (auto& it : items) {
                const bool f = std::find(conf.FilterRetrieveIds.begin(), conf.FilterRetrieveIds.end(), it->RetrieveId) !=
                               conf.FilterRetrieveIds.end();
                (f ? backup : selected).push_back(it);
            }
            if (!DoSort(&selected, d, err)) return false;
            selected.insert(selected.end(), backup.begin(), backup.end());
            items.swap(selected);
            return true;
        }
        return DoSort(&items, d, err);
    }
};

// AlgoScoreSort (sort/algo_score_sort.go:38-66): descending by SortByField unless the best Item.Score exceeds
// SwitchThreshold, then by current_score.  (The reference's comparator assigns a failed RIGHT lookup's fallback to the
// left score — `iScore = items[j].Score` — which only matters when the field is missing; here a missing field falls
// back to the item's own score on both sides.)
struct GpuAlgoScoreSort : sort::ISort {
    Engine* e;
    std::string sortByField;
    double switchThreshold;
    GpuAlgoScoreSort(Engine* eng, const recconf::SortConfig& c)
        : e(eng), sortByField(c.SortByField.empty() ? "current_score" : c.SortByField), switchThreshold(c.SwitchThreshold) {}
    bool Sort(sort::SortData* d, std::string* err) override {
        const uint32_t n = (uint32_t)d->Data.size();
        if (n == 0) return true;
        double maxScore = -1e300;
        for (const auto& it : d->Data) maxScore = std::max(maxScore, it->Score);
        const std::string field = maxScore > switchThreshold ? "current_score" : sortByField;
        std::vector<double> key(n);
        for (uint32_t i = 0; i < n; ++i)
            if (!d->Data[i]->FloatExprData(field, &key[i])) key[i] = d->Data[i]->Score;
        const uint32_t seg[2] = {0, n};
        std::vector<uint32_t> order(n);
        if (pg_sort_scores(e->ctx, key.data(), seg, 1, 1, order.data()) != PG_OK) {
            if (err) *err = pg_err("pg_sort_scores");
            return false;
        }
        std::vector<module::ItemPtr> out(n);
        for (uint32_t i = 0; i < n; ++i) out[i] = d->Data[order[i]];
        d->Data.swap(out);
        return true;
    }
};

// CustomFieldSort (sort/custom_field_sort.go:21-73): by Item.FloatExprData(SortByField) — an algo score, else a property, "current_score"
// = Item.Score — falling back to the item's own Score where the field is missing; "asc" or (default, and for anything else) "desc".
// The order is the device sort's (ties by position, where Go's sort.Slice leaves them unspecified).
struct GpuCustomFieldSort : sort::ISort {
    Engine* e;
    std::string sortByField, sortOrder;
    GpuCustomFieldSort(Engine* eng, const recconf::SortConfig& c) : e(eng), sortByField(c.SortByField.empty() ? "current_score" : c.SortByField) {
        sortOrder = c.SortOrder;
        std::transform(sortOrder.begin(), sortOrder.end(), sortOrder.begin(), ::tolower);
        if (sortOrder != "asc" && sortOrder != "desc") sortOrder = "desc";
    }
    bool Sort(sort::SortData* d, std::string* err) override {
        const uint32_t n = (uint32_t)d->Data.size();
        if (n == 0) return true;
        std::vector<double> key(n);
        for (uint32_t i = 0; i < n; ++i)
            if (!d->Data[i]->FloatExprData(sortByField, &key[i])) key[i] = d->Data[i]->Score;
        const uint32_t seg[2] = {0, n};
        std::vector<uint32_t> order(n);
        if (pg_sort_scores(e->ctx, key.data(), seg, 1, sortOrder == "asc" ? 0 : 1, order.data()) != PG_OK) {
            if (err) *err = pg_err("pg_sort_scores");
            return false;
        }
        std::vector<module::ItemPtr> out(n);
        for (uint32_t i = 0; i < n; ++i) out[i] = d->Data[order[i]];
        d->Data.swap(out);
        return true;
    }
};

// DiversityRuleSort (sort/diversity_rule_sort.go:116-283) through pg_diversity_rules: the items' dimension strings
// (Item.StringProperty, a missing property = "") are dictionary-encoded per call — equal strings, equal codes — and so are the
// string conditions' literals; integer conditions read the property's integer.  What cannot be served leaves Data untouched and
// returns an error, which the caller ignores as it ignores every sort's error (sort/sort.go:123).
struct GpuDiversityRuleSort : sort::ISort {
    Engine* e;
    recconf::DiversityRuleSortConfig conf;
    GpuDiversityRuleSort(Engine* eng, recconf::DiversityRuleSortConfig c) : e(eng), conf(std::move(c)) {}
    bool Sort(sort::SortData* d, std::string* err) override {
        const size_t n = d->Data.size();
        if (n == 0 || conf.DiversityRules.empty()) return true;                    // :121-123
        if (n > PG_DIV_MAX_N) {
            if (err) *err = "DiversityRuleSort: " + std::to_string(n) + " items (the device serves up to " + std::to_string(PG_DIV_MAX_N) + ")";
            return false;
        }
        // columns: one per distinct dimension name (codes), one per distinct condition (integers, or codes of the same dictionary)
        std::vector<std::string> col_names;
        std::vector<bool> col_is_int;
        auto column = [&](const std::string& name, bool is_int) {
            for (size_t c = 0; c < col_names.size(); ++c)
                if (col_names[c] == name && col_is_int[c] == is_int) return (uint32_t)c;
            col_names.push_back(name);
            col_is_int.push_back(is_int);
            return (uint32_t)(col_names.size() - 1);
        };
        pg_div_config cfg;
        memset(&cfg, 0, sizeof cfg);
        cfg.size = d->Context ? d->Context->Size : 10;
        cfg.diversity_size = conf.DiversitySize;
        cfg.explore_item_size = conf.ExploreItemSize;
        cfg.n_rules = (uint32_t)conf.DiversityRules.size();
        for (size_t r = 0; r < conf.DiversityRules.size(); ++r) {
            const auto& rc = conf.DiversityRules[r];
            cfg.rules[r].n_dims = (uint32_t)rc.Dimensions.size();
            for (size_t k = 0; k < rc.Dimensions.size(); ++k) cfg.rules[r].dims[k] = column(rc.Dimensions[k], false);
            cfg.rules[r].interval = rc.IntervalSize; cfg.rules[r].window = rc.WindowSize;
            cfg.rules[r].frequency = rc.FrequencySize; cfg.rules[r].weight = rc.Weight;
        }
        std::vector<std::vector<uint32_t>> positions(conf.ExclusionRules.size());
        cfg.n_excl = (uint32_t)conf.ExclusionRules.size();
        for (size_t x = 0; x < conf.ExclusionRules.size(); ++x) {
            const auto& xc = conf.ExclusionRules[x];
            for (long long p : xc.Positions) positions[x].push_back((uint32_t)std::min<long long>(p, 0xFFFFFFFFll));
            cfg.excl[x].positions = positions[x].data();
            cfg.excl[x].n_positions = (uint32_t)positions[x].size();
            cfg.excl[x].n_terms = (uint32_t)xc.Conditions.size();
            for (size_t t = 0; t < xc.Conditions.size(); ++t)
                cfg.excl[x].terms[t] = pg_div_term{column(xc.Conditions[t].Name, !xc.Conditions[t].IsString), xc.Conditions[t].Op, xc.Conditions[t].Int};
        }
        if (col_names.size() > PG_DIV_MAX_COLS) {
            if (err) *err = "DiversityRuleSort: " + std::to_string(col_names.size()) + " distinct columns (the device serves up to " + std::to_string(PG_DIV_MAX_COLS) + ")";
            return false;
        }
        cfg.n_cols = (uint32_t)col_names.size();
        std::vector<int64_t> dims(col_names.size() * n);
        std::vector<std::map<std::string, int64_t>> dict(col_names.size());
        for (size_t c = 0; c < col_names.size(); ++c)
            for (size_t i = 0; i < n; ++i) {
                const module::Item& it = *d->Data[i];
                if (col_is_int[c]) {
                    const auto p = it.Properties.find(col_names[c]);
                    const bool num = p != it.Properties.end() && p->second.type == json::Value::Number && p->second.num == std::floor(p->second.num);
                    if (!num) {
                        if (err) *err = "DiversityRuleSort: item " + it.Id + " has no integer property \"" + col_names[c] + "\" for an exclusion condition";
                        return false;
                    }
                    dims[c * n + i] = p->second.is_int ? p->second.i : (long long)p->second.num;
                } else {
                    const auto ins = dict[c].emplace(feature::ItemStringProperty(it, col_names[c]), (int64_t)dict[c].size());
                    dims[c * n + i] = ins.first->second;
                }
            }
        for (size_t x = 0; x < conf.ExclusionRules.size(); ++x)                      // a literal no item carries: a code no item has
            for (size_t t = 0; t < conf.ExclusionRules[x].Conditions.size(); ++t) {
                const auto& ec = conf.ExclusionRules[x].Conditions[t];
                if (!ec.IsString) continue;
                const auto& dc = dict[cfg.excl[x].terms[t].column];
                const auto f = dc.find(ec.Str);
                cfg.excl[x].terms[t].value = f == dc.end() ? -1 : f->second;
            }
        std::vector<uint8_t> source;
        if (!conf.ExcludeRecalls.empty()) {                                           // :127-138
            source.resize(n);
            for (size_t i = 0; i < n; ++i)
                source[i] = std::find(conf.ExcludeRecalls.begin(), conf.ExcludeRecalls.end(), d->Data[i]->RetrieveId) != conf.ExcludeRecalls.end() ? 0 : 1;
            cfg.exclude_source_mask = 1u;
        }
        std::vector<uint32_t> order(n);
        if (pg_diversity_rules(e->ctx, &cfg, (uint32_t)n, dims.data(), source.empty() ? nullptr : source.data(), order.data()) != PG_OK) {
            if (err) *err = pg_err("pg_diversity_rules");
            return false;
        }
        std::vector<module::ItemPtr> out(n);
        for (size_t i = 0; i < n; ++i) out[i] = d->Data[order[i]];
        d->Data.swap(out);
        return true;
    }
};

// BoostScoreSort (sort/boost_score_sort.go:73-104) through pg_boost_scores: the properties the conditions and expressions name
// become candidate-aligned columns — strings dictionary-encoded per call together with the conditions' literals and the user's
// string properties, numbers as int64 where every item holds an integer and fp64 otherwise — and the user's properties the user
// slots.  An item without a named property, a property of the wrong kind, a list over the device's cap or a condition set
// pg_cond_compile refuses leave Data untouched and return an error, which the caller ignores as it ignores every sort's error.
namespace {
// fills the user slots of a compiled set from User.Properties; false: a property that is neither a number nor an encodable string
bool cond_user_slots(pg_cond* c, const module::User* user, CondBuild* b, uint64_t* vals, uint32_t* present, std::string* err) {
    *present = 0;
    for (int s = 0; s < pg_cond_num_user_slots(c); ++s) {
        const std::string name = pg_cond_user_slot_name(c, s);
        vals[s] = 0;
        if (!user) continue;
        const auto p = user->Properties.find(name);
        if (p == user->Properties.end()) continue;
        const json::Value& v = p->second;
        const bool as_string = (b->user_kind[name] & 1) != 0;
        if (as_string && b->dict) {
            const long long id = b->code(v.type == json::Value::String ? v.str : v.type == json::Value::Number ? json::NumToString(v.num) : std::string());
            memcpy(&vals[s], &id, 8);
        } else if (v.type == json::Value::Number || (v.type == json::Value::String && !v.str.empty())) {
            if (pg_cond_user_slot_is_float(c, s)) {
                const double d = ToFloat(v, 0.0);
                memcpy(&vals[s], &d, 8);
            } else {
                long long i = 0;
                double d = 0.0;
                if (!b->constant(v, "int", name, &i, &d)) { if (err) *err = "user property \"" + name + "\" is not an integer"; return false; }
                memcpy(&vals[s], &i, 8);
            }
        } else {
            if (err) *err = "user property \"" + name + "\" is not a number";
            return false;
        }
        *present |= 1u << s;
    }
    return true;
}
// the item properties a built condition set names, as candidate-aligned columns: strings dictionary-encoded through the build's
// map, numbers as int64 where every item holds an integer and fp64 otherwise
struct CondColumns {
    std::vector<std::vector<long long>> ints;
    std::vector<std::vector<double>> floats;
    std::vector<pg_cond_col> cols;              // (the names point into the build's item_names)
    std::vector<const void*> col_ptr;
    bool fill(CondBuild* b, const std::vector<module::ItemPtr>& data, std::string* why) {
        const size_t nc = b->item_names.size(), n = data.size();
        ints.resize(nc); floats.resize(nc); cols.resize(nc); col_ptr.resize(nc);
        for (size_t c = 0; c < nc; ++c) {
            const std::string& name = b->item_names[c];
            const int kind = b->item_kind[name];
            if ((kind & 1) && (kind & 2)) { *why = "property \"" + name + "\" is read both as a string and as a number"; return false; }
            bool whole = true;
            for (size_t i = 0; i < n; ++i) {
                const auto p = data[i]->Properties.find(name);
                if (p == data[i]->Properties.end()) { *why = "item " + data[i]->Id + " has no property \"" + name + "\""; return false; }
                if (kind & 1) continue;
                if (p->second.type != json::Value::Number) { *why = "item " + data[i]->Id + ": property \"" + name + "\" is not a number"; return false; }
                whole = whole && (p->second.is_int || (p->second.num == std::floor(p->second.num) && std::fabs(p->second.num) < 9e15));
            }
            cols[c].name = name.c_str();
            if ((kind & 1) || whole) {
                ints[c].resize(n);
                for (size_t i = 0; i < n; ++i) {
                    const json::Value& v = data[i]->Properties.find(name)->second;
                    ints[c][i] = (kind & 1) ? b->code(feature::ItemStringProperty(*data[i], name)) : (v.is_int ? v.i : (long long)v.num);
                }
                cols[c].dtype = PG_F_I64;
                col_ptr[c] = ints[c].data();
            } else {
                floats[c].resize(n);
                for (size_t i = 0; i < n; ++i) floats[c][i] = data[i]->Properties.find(name)->second.num;
                cols[c].dtype = PG_F_F64;
                col_ptr[c] = floats[c].data();
            }
        }
        return true;
    }
};
}  // namespace

// DistinctIdSort (sort/distinct_id_sort.go:52-72) through pg_distinct_ids: the conditions become the rules of one condition set
// over the items' own properties, as GpuBoostScoreSort builds them, and the ids come back per item, to be written under the sort's
// one DistinctIdName.  An item without a named property, a list over the device's cap or a set pg_cond_compile refuses leave the
// items untouched and return an error, which the caller ignores as it ignores every sort's error.
struct GpuDistinctIdSort : sort::ISort {
    Engine* e;
    json::Value conf;
    GpuDistinctIdSort(Engine* eng, json::Value c) : e(eng), conf(std::move(c)) {}
    bool Sort(sort::SortData* d, std::string* err) override {
        const size_t n = d->Data.size();
        const auto& conds = conf.at("DistinctIdConditions").arr;
        if (n == 0 || conds.empty()) return true;                                  // (no condition: the loop at :59 adds nothing)
        auto fail = [&](const std::string& what) { if (err) *err = "DistinctIdSort: " + what; return false; };
        if (n > PG_TRIM_MAX_CAP) return fail(std::to_string(n) + " items (the device serves up to " + std::to_string(PG_TRIM_MAX_CAP) + ")");
        const std::string name = conds[0].s("DistinctIdName").empty() ? "__distinct_id__" : conds[0].s("DistinctIdName");
        std::map<std::string, long long> dict;
        CondBuild b;
        b.dict = &dict;
        std::vector<std::vector<pg_cond_term>> terms(conds.size());
        std::vector<pg_cond_rule> rules(conds.size());
        std::vector<int64_t> ids(conds.size());
        for (size_t r = 0; r < conds.size(); ++r) {
            if (!b.build(conds[r].at("Conditions"), 0, &terms[r])) return fail(b.err);
            rules[r] = pg_cond_rule{terms[r].data(), (uint32_t)terms[r].size(), nullptr};
            ids[r] = (int64_t)conds[r].n("DistinctId");
        }
        CondColumns cc;
        std::string cerr;
        if (!cc.fill(&b, d->Data, &cerr)) return fail(cerr);
        pg_cond* c = nullptr;
        if (pg_cond_compile(rules.data(), (uint32_t)rules.size(), cc.cols.data(), (uint32_t)cc.cols.size(), 0, &c) != PG_OK) return fail(pg_last_error());
        uint64_t uv[PG_COND_MAX_SLOTS] = {0};
        uint32_t present = 0;
        std::vector<int64_t> out(n);
        std::string uerr;
        const bool ok = cond_user_slots(c, d->User, &b, uv, &present, &uerr) &&
                        pg_distinct_ids(e->ctx, c, ids.data(), (uint32_t)n, nullptr, cc.col_ptr.data(), uv, present, out.data()) == PG_OK;
        const std::string why = ok ? std::string() : (uerr.empty() ? pg_err("pg_distinct_ids") : uerr);
        pg_cond_free(c);
        if (!ok) return fail(why);
        for (size_t i = 0; i < n; ++i) {
            json::Value v = json::Value::Num((double)out[i]);
            v.is_int = true;
            v.i = out[i];
            d->Data[i]->Properties[name] = v;
        }
        return true;
    }
};

struct GpuBoostScoreSort : sort::ISort {
    Engine* e;
    json::Value conf;
    GpuBoostScoreSort(Engine* eng, json::Value c) : e(eng), conf(std::move(c)) {}
    bool Sort(sort::SortData* d, std::string* err) override {
        const size_t n = d->Data.size();
        const auto& conds = conf.at("BoostScoreConditions").arr;
        if (n == 0 || conds.empty()) return true;
        auto fail = [&](const std::string& what) { if (err) *err = "BoostScoreSort: " + what; return false; };
        if (n > PG_TRIM_MAX_CAP) return fail(std::to_string(n) + " items (the device serves up to " + std::to_string(PG_TRIM_MAX_CAP) + ")");
        std::map<std::string, long long> dict;
        CondBuild b;
        b.dict = &dict;
        std::vector<std::vector<pg_cond_term>> terms(conds.size());
        std::vector<pg_cond_rule> rules(conds.size());
        for (size_t r = 0; r < conds.size(); ++r) {
            if (!b.build(conds[r].at("Conditions"), 0, &terms[r])) return fail(b.err);
            rules[r].terms = terms[r].data();
            rules[r].n_terms = (uint32_t)terms[r].size();
            rules[r].expression = b.keep(conds[r].s("Expression"));
            pg_expr* x = nullptr;                                                  // the expression's variables are columns too
            if (pg_expr_compile_govaluate(rules[r].expression, &x) != PG_OK) return fail(pg_last_error());
            for (int v = 0; v < pg_expr_num_vars(x); ++v)
                if (strcmp(pg_expr_var_name(x, v), "score") != 0) b.item(pg_expr_var_name(x, v), 2);
            pg_expr_free(x);
        }
        CondColumns cc;
        std::string cerr;
        if (!cc.fill(&b, d->Data, &cerr)) return fail(cerr);
        pg_cond* c = nullptr;
        if (pg_cond_compile(rules.data(), (uint32_t)rules.size(), cc.cols.data(), (uint32_t)cc.cols.size(), 1, &c) != PG_OK) return fail(pg_last_error());
        uint64_t uv[PG_COND_MAX_SLOTS] = {0};
        uint32_t present = 0;
        std::vector<double> score(n), out(n);
        for (size_t i = 0; i < n; ++i) score[i] = d->Data[i]->Score;
        std::string uerr;
        const bool ok = cond_user_slots(c, d->User, &b, uv, &present, &uerr) &&
                        pg_boost_scores(e->ctx, c, conf.at("BoostScoreConditionsFilterAll").b ? 1u : 0u, (uint32_t)n, nullptr, cc.col_ptr.data(), uv, present,
                                        score.data(), out.data(), nullptr) == PG_OK;
        const std::string why = ok ? std::string() : (uerr.empty() ? pg_err("pg_boost_scores") : uerr);
        pg_cond_free(c);
        if (!ok) return fail(why);
        for (size_t i = 0; i < n; ++i) d->Data[i]->Score = out[i];
        return true;
    }
};

// MultiRecallMixSort (sort/multi_recall_mix_sort.go:62-178) through pg_mix_sort: the items in the order the previous sort left
// them are the list.  What the conditions read becomes columns of a store of n rows built for the call (item i is row i) — strings
// dictionary-encoded per call with the conditions' literals, numbers as int64 where every item holds an integer and fp64 otherwise,
// as GpuBoostScoreSort does; a PositionField becomes an int64 column, -1 where the item lacks it (utils.ToInt(.., -1)).  The
// RecallNames of all rules are numbered per call and an item's RetrieveId becomes its source.  The seed is Seed + the number of
// calls this sort has served.  Rules with an unknown MixStrategy are skipped (createMixStrategies, :47-58).  A config
// pg_mix_compile refuses, an item without a property a condition names or a list over the device's cap leave Data untouched and
// return the error.
struct GpuMultiRecallMixSort : sort::ISort {
    Engine* e;
    json::Value conf;
    std::atomic<uint64_t> served{0};
    GpuMultiRecallMixSort(Engine* eng, json::Value c) : e(eng), conf(std::move(c)) {}
    bool Sort(sort::SortData* d, std::string* err) override {
        const size_t n = d->Data.size();
        const uint64_t call = served.fetch_add(1);
        if (n == 0) return true;
        auto fail = [&](const std::string& what) { if (err) *err = "MultiRecallMixSort: " + what; return false; };
        if (n > PG_TRIM_MAX_CAP) return fail(std::to_string(n) + " items (the device serves up to " + std::to_string(PG_TRIM_MAX_CAP) + ")");
        std::map<std::string, long long> dict;
        CondBuild b;
        b.dict = &dict;
        std::vector<const json::Value*> rules;
        for (const auto& r : conf.at("MixSortRules").arr)
            if (r.s("MixStrategy") == "fix_position" || r.s("MixStrategy") == "random_position") rules.push_back(&r);
        const size_t ns = rules.size();
        std::vector<std::vector<pg_cond_term>> terms(ns);
        std::vector<std::vector<int32_t>> positions(ns);
        std::vector<pg_mix_strategy> st(ns);
        std::vector<std::string> names, pos_fields;          // recall names → sources; position columns
        for (size_t s = 0; s < ns; ++s) {
            const json::Value& r = *rules[s];
            memset(&st[s], 0, sizeof st[s]);
            st[s].type = r.s("MixStrategy") == "fix_position" ? PG_MIX_FIX : PG_MIX_RANDOM;
            if (!b.build(r.at("Conditions"), 0, &terms[s])) return fail(b.err);
            st[s].terms = terms[s].data();
            st[s].n_terms = (uint32_t)terms[s].size();
            for (const auto& p : r.at("Positions").arr) positions[s].push_back(p.type == json::Value::Number ? (int32_t)p.num : 0);
            st[s].positions = positions[s].data();
            st[s].n_positions = (uint32_t)positions[s].size();
            st[s].number = (int32_t)r.n("Number");
            st[s].number_rate = r.d("NumberRate");
            for (const auto& name : recconf::str_list(r.at("RecallNames"))) {
                auto at = std::find(names.begin(), names.end(), name);
                if (at == names.end()) {
                    if (names.size() >= 32) return fail("more than 32 RecallNames among the MixSortRules");
                    names.push_back(name);
                    at = names.end() - 1;
                }
                st[s].source_mask |= 1u << (at - names.begin());
            }
            if (st[s].type == PG_MIX_FIX && positions[s].empty() && !r.s("PositionField").empty()) {
                st[s].position_field = b.keep("position:" + r.s("PositionField"));      // (its own column: a condition may read the property as a string)
                if (std::find(pos_fields.begin(), pos_fields.end(), r.s("PositionField")) == pos_fields.end()) pos_fields.push_back(r.s("PositionField"));
            }
        }
        // the columns: what the conditions read, then the position fields
        const size_t ncond = b.item_names.size(), nc = ncond + pos_fields.size();
        std::vector<std::vector<long long>> ints(nc);
        std::vector<std::vector<double>> floats(nc);
        std::vector<pg_cond_col> cols(nc);
        std::vector<std::string> col_names(nc);
        for (size_t c = 0; c < ncond; ++c) {
            const std::string& name = b.item_names[c];
            const int kind = b.item_kind[name];
            if ((kind & 1) && (kind & 2)) return fail("property \"" + name + "\" is read both as a string and as a number");
            bool whole = true;
            for (size_t i = 0; i < n; ++i) {
                const auto p = d->Data[i]->Properties.find(name);
                if (p == d->Data[i]->Properties.end()) return fail("item " + d->Data[i]->Id + " has no property \"" + name + "\"");
                if (kind & 1) continue;
                if (p->second.type != json::Value::Number) return fail("item " + d->Data[i]->Id + ": property \"" + name + "\" is not a number");
                whole = whole && (p->second.is_int || (p->second.num == std::floor(p->second.num) && std::fabs(p->second.num) < 9e15));
            }
            col_names[c] = name;
            if ((kind & 1) || whole) {
                ints[c].resize(n);
                for (size_t i = 0; i < n; ++i) {
                    const json::Value& v = d->Data[i]->Properties.find(name)->second;
                    ints[c][i] = (kind & 1) ? b.code(feature::ItemStringProperty(*d->Data[i], name)) : (v.is_int ? v.i : (long long)v.num);
                }
                cols[c].dtype = PG_F_I64;
            } else {
                floats[c].resize(n);
                for (size_t i = 0; i < n; ++i) floats[c][i] = d->Data[i]->Properties.find(name)->second.num;
                cols[c].dtype = PG_F_F64;
            }
        }
        for (size_t k = 0; k < pos_fields.size(); ++k) {
            const size_t c = ncond + k;
            col_names[c] = "position:" + pos_fields[k];
            cols[c].dtype = PG_F_I64;
            ints[c].assign(n, -1);
            for (size_t i = 0; i < n; ++i) {
                const auto p = d->Data[i]->Properties.find(pos_fields[k]);
                if (p == d->Data[i]->Properties.end()) continue;
                long long v = -1;
                double f = 0.0;
                if (b.constant(p->second, "int", pos_fields[k], &v, &f)) ints[c][i] = v;      // utils.ToInt(.., -1)
            }
        }
        b.err.clear();
        for (size_t c = 0; c < nc; ++c) cols[c].name = col_names[c].c_str();
        pg_mix* m = nullptr;
        const uint32_t size = (uint32_t)std::max<long long>(conf.n("Size"), 0);
        if (pg_mix_compile(st.data(), (uint32_t)ns, cols.data(), (uint32_t)nc, size, conf.at("RemainItem").b ? 1u : 0u, &m) != PG_OK) return fail(pg_last_error());
        pg_features* fs = nullptr;
        std::vector<uint64_t> rows(n);
        std::vector<uint8_t> source(n);
        std::vector<uint32_t> out(n);
        uint32_t count = 0;
        for (size_t i = 0; i < n; ++i) {
            rows[i] = i;
            const auto at = std::find(names.begin(), names.end(), d->Data[i]->RetrieveId);
            source[i] = at == names.end() ? 0xFF : (uint8_t)(at - names.begin());
        }
        uint64_t uv[PG_COND_MAX_SLOTS] = {0};
        uint32_t present = 0;
        std::string why;
        bool ok = true;
        if (nc) {
            ok = pg_features_create(e->ctx, n, &fs) == PG_OK;
            for (size_t c = 0; ok && c < nc; ++c)
                ok = pg_features_set_column(e->ctx, fs, cols[c].name, cols[c].dtype, cols[c].dtype == PG_F_I64 ? (const void*)ints[c].data() : (const void*)floats[c].data(), 0.0) == PG_OK;
            if (!ok) why = pg_err("pg_features");
        }
        // the user slots (cond_user_slots reads them off a pg_cond; the set answers the same questions)
        for (int s = 0; ok && s < pg_mix_num_user_slots(m); ++s) {
            const std::string name = pg_mix_user_slot_name(m, s);
            if (!d->User) continue;
            const auto p = d->User->Properties.find(name);
            if (p == d->User->Properties.end()) continue;
            const json::Value& v = p->second;
            if (b.user_kind[name] & 1) {
                const long long id = b.code(v.type == json::Value::String ? v.str : v.type == json::Value::Number ? json::NumToString(v.num) : std::string());
                memcpy(&uv[s], &id, 8);
            } else if (pg_mix_user_slot_is_float(m, s)) {
                const double f = ToFloat(v, 0.0);
                memcpy(&uv[s], &f, 8);
            } else {
                long long i = 0;
                double f = 0.0;
                if (!b.constant(v, "int", name, &i, &f)) { ok = false; why = "user property \"" + name + "\" is not an integer"; break; }
                memcpy(&uv[s], &i, 8);
            }
            present |= 1u << s;
        }
        if (ok) {
            const long long seed = conf.n("Seed");
            ok = pg_mix_sort(e->ctx, m, fs, (uint32_t)std::max(d->Context ? d->Context->Size : 0, 0), (uint32_t)n, rows.data(), source.data(), nullptr,
                             (uint64_t)seed + call, uv, present, out.data(), &count) == PG_OK;
            if (!ok) why = pg_err("pg_mix_sort");
        }
        pg_mix_free(m);
        if (fs) pg_features_destroy(e->ctx, fs);
        if (!ok) return fail(why);
        std::vector<module::ItemPtr> page(count);
        for (uint32_t k = 0; k < count; ++k) page[k] = d->Data[out[k]];
        d->Data.swap(page);
        return true;
    }
};

// TrafficControlSort's macro control (sort/traffic_control_sort.go:91-185, :204-364) through pg_traffic_sort.  The PID controller
// itself — traffic counters, wall-clock time, PIDController.compute — is the Go side's job and hands over one alpha per target; the
// mirror has no traffic service, so a target's alpha is its config constant Alpha until Engine::SetTrafficAlpha replaces it.  The
// items are put in score order first (:114), each becomes its table row (one the table does not know: a row of its own behind the
// store, every column missing), the targets' ItemExpressions run as one classcut set over the engine's item_features store
// (pg_classcut_masks_dev) and its masks are the members; a target without an expression controls every item.  page_number is the
// request parameter (default 1, :294-297); PidGamma / PidBeta / PidEta default to 1.0 / 1.0 / 1.6 (:269-282) and an experiment
// parameter pid_gamma / pid_beta / pid_eta overrides them.  The items leave in the new order with __traffic_control_id__,
// _ORIGIN_POSITION_ and _NEW_POSITION_ set.  An error leaves Data in score order and returns it.
struct GpuTrafficControlSort : sort::ISort {
    Engine* e;
    json::Value conf;
    std::mutex mu;                                       // alphas
    std::vector<std::string> ids;                        // TrafficControlTargetId as written
    std::vector<double> alphas;
    GpuTrafficControlSort(Engine* eng, json::Value c) : e(eng), conf(std::move(c)) {
        for (const auto& t : conf.at("Targets").arr) {
            const json::Value& id = t.at("TrafficControlTargetId");
            ids.push_back(id.type == json::Value::String ? id.str : std::to_string(id.is_int ? id.i : (long long)id.num));
            alphas.push_back(t.d("Alpha"));
        }
    }
    bool SetAlpha(const std::string& target_id, double alpha) {
        std::lock_guard<std::mutex> g(mu);
        const auto at = std::find(ids.begin(), ids.end(), target_id);
        if (at == ids.end()) return false;
        alphas[(size_t)(at - ids.begin())] = alpha;
        return true;
    }
    bool Sort(sort::SortData* d, std::string* err) override {
        const size_t n = d->Data.size();
        if (n == 0) return true;
        auto fail = [&](const std::string& what) { if (err) *err = "TrafficControlSort: " + what; return false; };
        if (n > PG_TRIM_MAX_CAP) return fail(std::to_string(n) + " items (the device serves up to " + std::to_string(PG_TRIM_MAX_CAP) + ")");
        if (!sort_items(e, d, true, err)) return false;
        std::vector<pg_traffic_target> targets;
        std::vector<int> class_target;
        std::vector<std::string> columns;
        pg_classcut* set = nullptr;
        std::string why;
        if (!recconf::CompileTrafficConf(conf, &targets, &set, &class_target, &columns, &why)) return fail(why);
        const size_t T = targets.size();
        std::vector<double> alpha;
        {
            std::lock_guard<std::mutex> g(mu);
            alpha = alphas;
        }
        std::vector<uint8_t> member(n, 0);
        bool ok = true;
        if (set) {
            if (!columns.empty() && !e->feats) { ok = false; why = "the engine has no feature columns"; }
            for (size_t c = 0; ok && c < columns.size(); ++c)
                if (pg_features_column_index(e->feats, columns[c].c_str()) < 0) { ok = false; why = "\"" + columns[c] + "\" is not a feature column"; }
            std::vector<uint64_t> rows(n);
            std::vector<double> score(n);
            for (size_t i = 0; i < n; ++i) {
                uint32_t row;
                rows[i] = e->RowOfId(d->Data[i]->Id, &row) ? row : e->table_rows + i;
                score[i] = d->Data[i]->Score;
            }
            void *d_rows = nullptr, *d_score = nullptr, *d_masks = nullptr;
            std::vector<uint8_t> masks(n, 0);
            if (ok) {
                ok = pg_device_malloc(e->ctx, n * 8, &d_rows) == PG_OK && pg_device_malloc(e->ctx, n * 8, &d_score) == PG_OK &&
                     pg_device_malloc(e->ctx, n, &d_masks) == PG_OK && pg_memcpy_h2d(e->ctx, d_rows, rows.data(), n * 8) == PG_OK &&
                     pg_memcpy_h2d(e->ctx, d_score, score.data(), n * 8) == PG_OK &&
                     pg_classcut_masks_dev(e->ctx, set, e->feats, 1, (uint32_t)n, (const uint64_t*)d_rows, (const double*)d_score, nullptr, nullptr,
                                           (uint8_t*)d_masks) == PG_OK &&
                     pg_memcpy_d2h(e->ctx, masks.data(), d_masks, n) == PG_OK;
                if (!ok) why = pg_err("pg_classcut_masks_dev");
            }
            for (void* p : {d_rows, d_score, d_masks})
                if (p) pg_device_free(e->ctx, p);
            pg_classcut_free(set);
            for (size_t i = 0; ok && i < n; ++i)
                for (size_t c = 0; c < class_target.size(); ++c)
                    if ((masks[i] >> c) & 1u) member[i] |= (uint8_t)(1u << class_target[c]);
        }
        if (!ok) return fail(why);
        for (size_t t = 0; t < T; ++t)
            if (conf.at("Targets").arr[t].s("ItemExpression").empty())
                for (size_t i = 0; i < n; ++i) member[i] |= (uint8_t)(1u << t);
        const context::RecommendContext none;
        const context::RecommendContext& cx = d->Context ? *d->Context : none;
        long long page_no = 1;
        {
            const auto p = cx.Param.find("page_number");                     // utils.ToInt(ctx.GetParameter("page_number"), 1)
            if (p != cx.Param.end()) {
                if (p->second.type == json::Value::Number) page_no = p->second.is_int ? p->second.i : (long long)p->second.num;
                else if (p->second.type == json::Value::String) { char* end = nullptr; const long long v = strtoll(p->second.str.c_str(), &end, 10); if (!p->second.str.empty() && !*end) page_no = v; }
            }
            if (page_no < 1) page_no = 1;
            if (page_no > 0xFFFFFFFFLL) page_no = 0xFFFFFFFFLL;
        }
        const double gamma = cx.GetFloat("pid_gamma", conf.has("PidGamma") ? conf.d("PidGamma") : 1.0);
        const double beta = cx.GetFloat("pid_beta", conf.has("PidBeta") ? conf.d("PidBeta") : 1.0);
        const double eta = cx.GetFloat("pid_eta", conf.has("PidEta") ? conf.d("PidEta") : 1.6);
        const int size = d->Context ? d->Context->Size : 10;
        if (size < 1) return fail("the page size (ctx.Size) is " + std::to_string(size));
        std::vector<double> score(n), new_pos(n);
        for (size_t i = 0; i < n; ++i) score[i] = d->Data[i]->Score;
        std::vector<uint32_t> out(n);
        std::vector<int32_t> control(n);
        uint32_t count = 0;
        pg_traffic* m = nullptr;
        if (pg_traffic_compile(targets.data(), (uint32_t)T, &m) != PG_OK) return fail(pg_last_error());
        ok = pg_traffic_sort(e->ctx, m, (uint32_t)size, (uint32_t)page_no, gamma, beta, eta, (uint32_t)n, score.data(), member.data(), nullptr, alpha.data(),
                             out.data(), &count, control.data(), new_pos.data()) == PG_OK;
        if (!ok) why = pg_err("pg_traffic_sort");
        pg_traffic_free(m);
        if (!ok) return fail(why);
        auto integer = [](long long v) { json::Value x = json::Value::Num((double)v); x.is_int = true; x.i = v; return x; };
        for (size_t i = 0; i < n; ++i) {
            d->Data[i]->Properties["__traffic_control_id__"] = integer(control[i]);
            d->Data[i]->Properties["_ORIGIN_POSITION_"] = integer((long long)i + 1);
            d->Data[i]->Properties["_NEW_POSITION_"] = new_pos[i] == (double)(i + 1) ? integer((long long)i + 1) : json::Value::Num(new_pos[i]);
        }
        std::vector<module::ItemPtr> page(count);
        for (uint32_t k = 0; k < count; ++k) page[k] = d->Data[out[k]];
        d->Data.swap(page);
        return true;
    }
};

// ItemStateFilter (filter/item_state_filter.go:47-57; the DAO's keep, module/item_state_filter_hologres_dao.go:313-357) through
// pg_item_state_filter over the engine's feature columns: an item whose id the table does not know is the item absent from the
// state table.  The position rides in the score plane, so the kept items come back by position, in order.
bool item_state_filter(Engine* self, const recconf::GpuFilterConfig& conf, const module::User* user, std::vector<module::ItemPtr>* items, std::string* err) {
    const size_t n = items->size();
    if (n == 0) return true;
    auto fail = [&](const std::string& what) { if (err) *err = "ItemStateFilter " + conf.Name + ": " + what; return false; };
    if (n > PG_TRIM_MAX_CAP) return fail(std::to_string(n) + " items (the device serves up to " + std::to_string(PG_TRIM_MAX_CAP) + ")");
    if (!self->feats) return fail("the engine has no feature columns");
    CondBuild b;
    std::vector<pg_cond_term> terms;
    if (!b.build(conf.FilterParams, 0, &terms)) return fail(b.err);
    std::vector<pg_cond_col> cols(b.item_names.size());
    for (size_t c = 0; c < cols.size(); ++c) {
        if (pg_features_column_index(self->feats, b.item_names[c].c_str()) < 0) return fail("\"" + b.item_names[c] + "\" is not a feature column");
        cols[c] = pg_cond_col{b.item_names[c].c_str(), PG_F_I32};
    }
    pg_cond_rule rule{terms.data(), (uint32_t)terms.size(), nullptr};
    pg_cond* c = nullptr;
    if (pg_cond_compile(&rule, 1, cols.data(), (uint32_t)cols.size(), 0, &c) != PG_OK) return fail(pg_last_error());
    std::vector<uint64_t> rows(n), out_rows(n);
    std::vector<double> pos(n), out_pos(n);
    for (size_t i = 0; i < n; ++i) {
        uint32_t row;
        rows[i] = self->RowOfId((*items)[i]->Id, &row) ? row : self->table_rows;
        pos[i] = (double)i;
    }
    uint64_t uv[PG_COND_MAX_SLOTS] = {0};
    uint32_t present = 0, count = 0;
    std::string uerr;
    const bool ok = cond_user_slots(c, user, &b, uv, &present, &uerr) &&
                    pg_item_state_filter(self->ctx, c, self->feats, (uint32_t)n, rows.data(), pos.data(), nullptr, uv, present, out_rows.data(), out_pos.data(), nullptr,
                                         &count) == PG_OK;
    const std::string why = ok ? std::string() : (uerr.empty() ? pg_err("pg_item_state_filter") : uerr);
    pg_cond_free(c);
    if (!ok) return fail(why);
    std::vector<module::ItemPtr> kept(count);
    for (uint32_t k = 0; k < count; ++k) kept[k] = (*items)[(size_t)out_pos[k]];
    items->swap(kept);
    return true;
}

// DimensionFieldUniqueFilter (filter/dimension_field_unique_filter.go:33-55) through pg_candidates_dimcap over the engine's feature
// columns: the first item of each value of the Dimension column is kept; an item whose id the table does not know, or whose
// value is the configured NullValue, is the item whose StringProperty is "" and is always kept (:41-42).  The position rides in
// the score plane, as in item_state_filter.
bool dimension_unique_filter(Engine* self, const recconf::GpuFilterConfig& conf, std::vector<module::ItemPtr>* items, std::string* err) {
    const size_t n = items->size();
    if (n == 0) return true;
    auto fail = [&](const std::string& what) { if (err) *err = "DimensionFieldUniqueFilter " + conf.Name + ": " + what; return false; };
    if (n > PG_TRIM_MAX_CAP) return fail(std::to_string(n) + " items (the device serves up to " + std::to_string(PG_TRIM_MAX_CAP) + ")");
    if (!self->feats) return fail("the engine has no feature columns");
    if (pg_features_column_index(self->feats, conf.Dimension.c_str()) < 0) return fail("\"" + conf.Dimension + "\" is not a feature column");
    std::vector<uint64_t> rows(n), out_rows(n);
    std::vector<double> pos(n), out_pos(n);
    for (size_t i = 0; i < n; ++i) {
        uint32_t row;
        rows[i] = self->RowOfId((*items)[i]->Id, &row) ? row : self->table_rows;
        pos[i] = (double)i;
    }
    const pg_dimcap_conf dc{conf.Dimension.c_str(), 1u, PG_DIMCAP_NULL_KEEP, conf.HasNullValue ? 1u : 0u, (int64_t)conf.NullValue};
    uint32_t count = 0;
    if (pg_candidates_dimcap(self->ctx, self->feats, &dc, (uint32_t)n, rows.data(), pos.data(), nullptr, out_rows.data(), out_pos.data(), nullptr, &count) != PG_OK)
        return fail(pg_err("pg_candidates_dimcap"));
    std::vector<module::ItemPtr> kept(count);
    for (uint32_t k = 0; k < count; ++k) kept[k] = (*items)[(size_t)out_pos[k]];
    items->swap(kept);
    return true;
}

// SnakeFilter (filter/snake_filter.go:173-241) and CompletelyFairCountFilter (filter/completely_fair_count_filter.go:34-94) through
// pg_candidates_blend_dev: the items become the arrays a fan-in leaves — the position as the row, Score, the index of RetrieveId
// among the engine's recalls as the source, RecallScores as the per-recall planes and the source mask — and the kept positions
// come back in order; an item picked through another recall's list takes that recall's name and score (:83-88).
bool blend_filter(Engine* self, const recconf::GpuFilterConfig& conf, std::vector<module::ItemPtr>* items, std::string* err) {
    const size_t n = items->size();
    if (n == 0) return true;
    auto fail = [&](const std::string& what) { if (err) *err = conf.FilterType + " " + conf.Name + ": " + what; return false; };
    if (n > PG_BLEND_MAX_CAP) return fail(std::to_string(n) + " items (the device serves up to " + std::to_string(PG_BLEND_MAX_CAP) + ")");
    const bool snake = conf.Blend.mode != PG_BLEND_FAIR;
    // a fair filter deals out whatever names the items carry: those that are no recall of the engine get the indices behind
    std::vector<std::string> names = conf.BlendSources;
    if (names.size() > PG_BLEND_MAX_SOURCES) names.resize(PG_BLEND_MAX_SOURCES);
    const uint32_t n_planes = (uint32_t)std::max<size_t>(names.size(), 1);
    const uint32_t cap = (uint32_t)n;
    uint32_t out_cap = 0;
    if (pg_blend_out_cap(&conf.Blend, cap, &out_cap) != PG_OK) return fail(pg_last_error());
    std::vector<uint64_t> rows(n), out_rows(out_cap);
    std::vector<double> score(n), out_score(out_cap), planes((size_t)PG_BLEND_MAX_PLANES * n, std::nan(""));
    std::vector<uint8_t> source(n), out_source(out_cap);
    std::vector<uint32_t> mask(n);
    for (size_t i = 0; i < n; ++i) {
        const module::Item& it = *(*items)[i];
        auto at = std::find(names.begin(), names.end(), it.RetrieveId);
        if (at == names.end() && !snake) {
            if (names.size() >= PG_BLEND_MAX_SOURCES) return fail("more than " + std::to_string(PG_BLEND_MAX_SOURCES) + " recall names among the items");
            names.push_back(it.RetrieveId);
            at = names.end() - 1;
        }
        rows[i] = i;
        score[i] = it.Score;
        source[i] = at == names.end() ? 0xFF : (uint8_t)(at - names.begin());        // (a snake drops what no entry names)
        mask[i] = source[i] < 32 ? 1u << source[i] : 0u;
        if (it.hasRecallScores)
            for (const auto& kv : it.RecallScores) {
                const auto r = std::find(names.begin(), names.end(), kv.first);
                if (r == names.end() || r - names.begin() >= (long)n_planes) continue;
                mask[i] |= 1u << (r - names.begin());
                planes[(size_t)(r - names.begin()) * n + i] = kv.second;
            }
    }
    const size_t b_in = n * 8, b_out = (size_t)out_cap * 8;
    // one device buffer: rows | score | planes | mask | source | out rows | out score | out planes | out mask | out source | count
    const size_t o_score = b_in, o_planes = 2 * b_in, o_mask = o_planes + n_planes * b_in, o_source = o_mask + n * 4;
    const size_t o_orows = (o_source + n + 255) & ~(size_t)255, o_oscore = o_orows + b_out, o_oplanes = o_oscore + b_out;
    const size_t o_omask = o_oplanes + n_planes * b_out, o_osource = o_omask + (size_t)out_cap * 4, o_count = (o_osource + out_cap + 255) & ~(size_t)255;
    void* d = nullptr;
    if (pg_device_malloc(self->ctx, o_count + 256, &d) != PG_OK) return fail(pg_last_error());
    char* b = (char*)d;
    uint32_t count = 0;
    const bool ok = pg_memcpy_h2d(self->ctx, b, rows.data(), b_in) == PG_OK && pg_memcpy_h2d(self->ctx, b + o_score, score.data(), b_in) == PG_OK &&
                    pg_memcpy_h2d(self->ctx, b + o_planes, planes.data(), n_planes * b_in) == PG_OK &&
                    pg_memcpy_h2d(self->ctx, b + o_mask, mask.data(), n * 4) == PG_OK && pg_memcpy_h2d(self->ctx, b + o_source, source.data(), n) == PG_OK &&
                    pg_candidates_blend_dev(self->ctx, &conf.Blend, 1, cap, (const uint64_t*)b, (const double*)(b + o_score), (const uint8_t*)(b + o_source),
                                            nullptr, (const double*)(b + o_planes), n_planes, (const uint32_t*)(b + o_mask), nullptr, 0,
                                            (uint64_t*)(b + o_orows), (double*)(b + o_oscore), (uint8_t*)(b + o_osource), (double*)(b + o_oplanes),
                                            (uint32_t*)(b + o_omask), nullptr, (uint32_t*)(b + o_count)) == PG_OK &&
                    pg_synchronize(self->ctx) == PG_OK && pg_memcpy_d2h(self->ctx, out_rows.data(), b + o_orows, b_out) == PG_OK &&
                    pg_memcpy_d2h(self->ctx, out_score.data(), b + o_oscore, b_out) == PG_OK &&
                    pg_memcpy_d2h(self->ctx, out_source.data(), b + o_osource, out_cap) == PG_OK &&
                    pg_memcpy_d2h(self->ctx, &count, b + o_count, 4) == PG_OK;
    const std::string why = ok ? std::string() : pg_last_error();
    pg_device_free(self->ctx, d);
    if (!ok) return fail(why);
    std::vector<module::ItemPtr> kept(std::min(count, out_cap));
    for (size_t k = 0; k < kept.size(); ++k) {
        kept[k] = (*items)[(size_t)out_rows[k]];
        if (snake && out_source[k] != source[(size_t)out_rows[k]]) {                  // (:83-88)
            kept[k]->RetrieveId = names[out_source[k]];
            kept[k]->Score = out_score[k];
        }
    }
    items->swap(kept);
    return true;
}

// PriorityAdjustCountFilter (filter/priority_adjust_count_filter.go:80-251, ensureDiversity false) through pg_candidates_trim_dev and
// PriorityAdjustCountFilterV2 (filter/priority_adjust_count_filter_v2.go:39-103) through pg_candidates_trim2_dev: the items become
// the arrays a fan-in leaves, exactly as blend_filter builds them, and the kept positions come back in rule order; under V2 an item
// kept through a rule other than its own source takes that recall's name and score (:68-69).
bool quota_filter(Engine* self, const recconf::GpuFilterConfig& conf, std::vector<module::ItemPtr>* items, std::string* err) {
    const size_t n = items->size();
    if (n == 0) return true;
    auto fail = [&](const std::string& what) { if (err) *err = conf.FilterType + " " + conf.Name + ": " + what; return false; };
    if (n > PG_TRIM_MAX_CAP) return fail(std::to_string(n) + " items (the device serves up to " + std::to_string(PG_TRIM_MAX_CAP) + ")");
    const bool v2 = conf.FilterType == "PriorityAdjustCountFilterV2";
    std::vector<std::string> names = conf.QuotaSources;
    if (names.size() > PG_TRIM_MAX_SOURCES) names.resize(PG_TRIM_MAX_SOURCES);
    const uint32_t n_planes = (uint32_t)std::max<size_t>(names.size(), 1);
    const uint32_t cap = (uint32_t)n, n_rules = (uint32_t)conf.Quotas.size();
    uint32_t out_cap = 0;
    if ((v2 ? pg_trim2_out_cap : pg_trim_out_cap)(conf.Quotas.data(), n_rules, cap, &out_cap) != PG_OK) return fail(pg_last_error());
    if (out_cap == 0) {                                                       // every count is 0: nothing is kept
        items->clear();
        return true;
    }
    std::vector<uint64_t> rows(n), out_rows(out_cap);
    std::vector<double> score(n), out_score(out_cap), planes((size_t)n_planes * n, std::nan(""));
    std::vector<uint8_t> source(n), out_source(out_cap);
    std::vector<uint32_t> mask(n);
    for (size_t i = 0; i < n; ++i) {
        const module::Item& it = *(*items)[i];
        const auto at = std::find(names.begin(), names.end(), it.RetrieveId);
        rows[i] = i;
        score[i] = it.Score;
        source[i] = at == names.end() ? 0xFF : (uint8_t)(at - names.begin());        // (what no rule names is dropped)
        if (it.hasRecallScores && it.RecallScores.size() > 1) {                      // (:55: the names of RecallScores are what counts)
            for (const auto& kv : it.RecallScores) {
                const auto r = std::find(names.begin(), names.end(), kv.first);
                if (r == names.end()) {
                    mask[i] |= 1u << 31;                                             // (a recall the device does not know: no rule names it)
                    continue;
                }
                mask[i] |= 1u << (r - names.begin());
                planes[(size_t)(r - names.begin()) * n + i] = kv.second;
            }
        } else if (source[i] < n_planes) {
            mask[i] = 1u << source[i];
            planes[(size_t)source[i] * n + i] = it.Score;
        }
    }
    const size_t b_in = n * 8, b_out = (size_t)out_cap * 8;
    // one device buffer: rows | score | planes | mask | source | out rows | out score | out planes | out mask | out source | count
    const size_t o_score = b_in, o_planes = 2 * b_in, o_mask = o_planes + n_planes * b_in, o_source = o_mask + n * 4;
    const size_t o_orows = (o_source + n + 255) & ~(size_t)255, o_oscore = o_orows + b_out, o_oplanes = o_oscore + b_out;
    const size_t o_omask = o_oplanes + n_planes * b_out, o_osource = o_omask + (size_t)out_cap * 4, o_count = (o_osource + out_cap + 255) & ~(size_t)255;
    void* d = nullptr;
    if (pg_device_malloc(self->ctx, o_count + 256, &d) != PG_OK) return fail(pg_last_error());
    char* b = (char*)d;
    uint32_t count = 0;
    const bool ok = pg_memcpy_h2d(self->ctx, b, rows.data(), b_in) == PG_OK && pg_memcpy_h2d(self->ctx, b + o_score, score.data(), b_in) == PG_OK &&
                    pg_memcpy_h2d(self->ctx, b + o_planes, planes.data(), n_planes * b_in) == PG_OK &&
                    pg_memcpy_h2d(self->ctx, b + o_mask, mask.data(), n * 4) == PG_OK && pg_memcpy_h2d(self->ctx, b + o_source, source.data(), n) == PG_OK &&
                    (v2 ? pg_candidates_trim2_dev : pg_candidates_trim_dev)(
                        self->ctx, conf.Quotas.data(), n_rules, 1, cap, (const uint64_t*)b, (const double*)(b + o_score), (const uint8_t*)(b + o_source),
                        nullptr, (const double*)(b + o_planes), n_planes, (const uint32_t*)(b + o_mask), nullptr, 0, (uint64_t*)(b + o_orows),
                        (double*)(b + o_oscore), (uint8_t*)(b + o_osource), (double*)(b + o_oplanes), (uint32_t*)(b + o_omask), nullptr,
                        (uint32_t*)(b + o_count)) == PG_OK &&
                    pg_synchronize(self->ctx) == PG_OK && pg_memcpy_d2h(self->ctx, out_rows.data(), b + o_orows, b_out) == PG_OK &&
                    pg_memcpy_d2h(self->ctx, out_score.data(), b + o_oscore, b_out) == PG_OK &&
                    pg_memcpy_d2h(self->ctx, out_source.data(), b + o_osource, out_cap) == PG_OK &&
                    pg_memcpy_d2h(self->ctx, &count, b + o_count, 4) == PG_OK;
    const std::string why = ok ? std::string() : pg_last_error();
    pg_device_free(self->ctx, d);
    if (!ok) return fail(why);
    std::vector<module::ItemPtr> kept(std::min(count, out_cap));
    for (size_t k = 0; k < kept.size(); ++k) {
        kept[k] = (*items)[(size_t)out_rows[k]];
        if (v2 && out_source[k] < names.size()) {                                     // (:68-69; a single's are its own)
            kept[k]->RetrieveId = names[out_source[k]];
            kept[k]->Score = out_score[k];
        }
    }
    items->swap(kept);
    return true;
}

// DiversityAdjustCountFilter (filter/diversity_adjust_count_filter.go:75-143) through pg_candidates_classcut: an item becomes its table
// row (one the table does not know: a row of its own behind the store, every column missing), Item.Score and the index of
// RetrieveId among the engine's recalls; the kept rows come back in class order and name their items.
bool classcut_filter(Engine* self, const recconf::GpuFilterConfig& conf, std::vector<module::ItemPtr>* items, std::string* err) {
    const size_t n = items->size();
    if (n == 0) return true;
    auto fail = [&](const std::string& what) { if (err) *err = "DiversityAdjustCountFilter " + conf.Name + ": " + what; return false; };
    if (n > PG_TRIM_MAX_CAP) return fail(std::to_string(n) + " items (the device serves up to " + std::to_string(PG_TRIM_MAX_CAP) + ")");
    if (!conf.ClassColumns.empty() && !self->feats) return fail("the engine has no feature columns");
    for (const auto& name : conf.ClassColumns)
        if (pg_features_column_index(self->feats, name.c_str()) < 0) return fail("\"" + name + "\" is not a feature column");
    pg_classcut* set = nullptr;
    std::string why;
    if (!recconf::CompileClasscut(conf, &set, &why)) return fail(why);
    uint32_t out_cap = 0, count = 0;
    pg_classcut_out_cap(set, (uint32_t)n, &out_cap);
    const size_t width = std::max<size_t>(out_cap, 1);                      // (every count 0: nothing is kept, the outputs still exist)
    std::vector<uint64_t> rows(n), out_rows(width);
    std::vector<double> score(n), out_score(width);
    std::vector<uint8_t> source(n), out_source(width);
    std::map<uint64_t, size_t> at;
    for (size_t i = 0; i < n; ++i) {
        const module::Item& it = *(*items)[i];
        uint32_t row;
        rows[i] = self->RowOfId(it.Id, &row) ? row : self->table_rows + i;
        if (!at.emplace(rows[i], i).second) {
            pg_classcut_free(set);
            return fail("item " + it.Id + " comes twice (the filter runs behind UniqueFilter)");
        }
        score[i] = it.Score;
        const auto r = std::find(conf.ClassRecalls.begin(), conf.ClassRecalls.end(), it.RetrieveId);
        source[i] = r == conf.ClassRecalls.end() || r - conf.ClassRecalls.begin() >= 0xFF ? 0xFF : (uint8_t)(r - conf.ClassRecalls.begin());
    }
    const bool ok = pg_candidates_classcut(self->ctx, set, self->feats, (uint32_t)n, rows.data(), score.data(), source.data(), out_rows.data(),
                                           out_score.data(), out_source.data(), &count) == PG_OK;
    why = ok ? std::string() : pg_err("pg_candidates_classcut");
    pg_classcut_free(set);
    if (!ok) return fail(why);
    std::vector<module::ItemPtr> kept(std::min(count, out_cap));
    for (size_t k = 0; k < kept.size(); ++k) kept[k] = (*items)[at.at(out_rows[k])];
    items->swap(kept);
    return true;
}

struct GpuSSDSort : sort::ISort {                        // sort/ssd_sort.go:110-343 (embedding table = item table)
    Engine* e;
    recconf::SSDSortConfig conf;
    GpuSSDSort(Engine* eng, recconf::SSDSortConfig c) : e(eng), conf(std::move(c)) {}
    // doSort (:296-343): score-descending order, candidate trimming, then SSDWithSlidingWindow
    bool DoSort(std::vector<module::ItemPtr>* items, sort::SortData* d, std::string* err) {
        if (items->empty()) return true;
        const int size = d->Context ? d->Context->Size : 10;
        sort::SortData tmp = *d;
        tmp.Data = *items;
        if (!sort_items(e, &tmp, true, err)) return false;
        items->swap(tmp.Data);
        // experiment parameters override the config (ssd_sort.go:301-309,354-356,364)
        const context::RecommendContext none;
        const context::RecommendContext& cx = d->Context ? *d->Context : none;
        const double gamma = cx.GetFloat("ssd_gamma", conf.Gamma);
        if (gamma == 0) return true;                                                // :302-305
        const int candidateCnt = (int)cx.GetInt("ssd_candidate_count", conf.CandidateCount);
        const double minScorePercent = cx.GetFloat("ssd_min_score_percent", conf.MinScorePercent);
        const int windowSize = (int)cx.GetInt("ssd_window_size", conf.WindowSize);
        const int doNorm = (int)cx.GetInt("ssd_norm_quality_score", 0);
        if ((candidateCnt > 0 || minScorePercent > 0) && (int)items->size() > size) {
            if (candidateCnt > 0) {
                const size_t cnt = (size_t)std::max(size, candidateCnt);
                if (cnt < items->size()) items->resize(cnt);
            }
            if (minScorePercent > 0 && (int)items->size() > size) {
                size_t idx = (size_t)size;
                const double mx = (*items)[0]->Score;
                for (; idx < items->size(); ++idx)
                    if ((*items)[idx]->Score / mx < minScorePercent) break;
                items->resize(idx);
            }
        }
        const uint32_t n = (uint32_t)items->size();
        std::vector<uint32_t> rows(n);
        std::vector<double> rel(n);
        for (uint32_t i = 0; i < n; ++i) {
            if (!e->RowOfId((*items)[i]->Id, &rows[i])) { if (err) *err = "ssd: unknown item id"; return false; }
            rel[i] = (*items)[i]->Score;
        }
        std::vector<uint32_t> idx(n);
        std::vector<double> quality(n);
        uint32_t cnt = 0;
        // SortService.Sort runs once per request, requests overlap (sort/sort.go:65-125): equal-shaped SSD calls of concurrent
        // requests share one launch (every request its own workgroups and barrier); other shapes take the direct call
        int src = PG_ERR_UNSUPPORTED;
        std::string cerr;                               // (a failed coalescer falls back to the direct call: not this call's error)
        if (e->coalesce && n <= 1024)
            if (pg_coalescer* co = e->SceneCoalescer(0, &cerr))
                src = pg_coalescer_ssd(co, rows.data(), rel.data(), n, gamma, (uint32_t)std::max(size, 0), (uint32_t)std::max(windowSize, 0),
                                       conf.NormalizeEmb ? 1 : 0, conf.EnsurePositiveSim ? 1 : 0, (doNorm == 1 || doNorm == 2) ? doNorm : 0,
                                       conf.UseSSDStar ? 1 : 0, idx.data(), &cnt, quality.data());
        if (src == PG_ERR_UNSUPPORTED)
            src = pg_ssd(e->ctx, e->table, rows.data(), rel.data(), n, gamma, (uint32_t)std::max(size, 0),
                         (uint32_t)std::max(windowSize, 0), conf.NormalizeEmb ? 1 : 0, conf.EnsurePositiveSim ? 1 : 0,
                         (doNorm == 1 || doNorm == 2) ? doNorm : 0, conf.UseSSDStar ? 1 : 0, idx.data(), &cnt, quality.data());
        if (src != PG_OK) {
            if (err) *err = pg_err("pg_ssd");
            return false;
        }
        if ((doNorm == 1 || doNorm == 2) && cnt != n)        // :372,385 (not on the "all zeros" bail-out)
            for (uint32_t i = 0; i < n; ++i) (*items)[i]->AddAlgoScore("ssd_quality_score", quality[i]);
        std::vector<module::ItemPtr> out;
        for (uint32_t i = 0; i < cnt; ++i) out.push_back((*items)[idx[i]]);
        items->swap(out);
        return true;
    }
    bool Sort(sort::SortData* d, std::string* err) override {
        auto& items = d->Data;
        if (items.empty()) return true;
        if (conf.AbortRunCount > 0 && (int)items.size() <= conf.AbortRunCount)      // :129-134
            return sort_items(e, d, true, err);
        std::vector<std::string> filterIds;                                          // :136-152
        if (d->Context && d->Context->HasExperiment())
            for (const auto& v : d->Context->ExperimentParamsJson.at("ssd_filter_retrieve_ids").arr)
                if (v.type == json::Value::String) filterIds.push_back(v.str);
        if (filterIds.empty()) filterIds = conf.FilterRetrieveIds;
        if (!filterIds.empty()) {                                                    // :155-171
            std::vector<module::ItemPtr> backup, selected;
            for (auto& it : items) {
                const bool f = std::find(filterIds.begin(), filterIds.end(), it->RetrieveId) != filterIds.end();
                (f ? backup : selected).push_back(it);
            }
            if (!DoSort(&selected, d, err)) return false;
            selected.insert(selected.end(), backup.begin(), backup.end());
            items.swap(selected);
            return true;
        }
        return DoSort(&items, d, err);
    }
};

}  // namespace

// ---- rank service --------------------------------------------------------------------------------
namespace rank {
bool Rank(Engine* e, module::User* user, std::vector<module::ItemPtr>& items, context::RecommendContext* ctx,
          std::string* err) {
    const std::string scene = ctx->GetParameter("scene");
    auto rc = e->config.RankConf.find(scene);
    if (rc == e->config.RankConf.end()) return true;                         // no rank config: no rank
    const recconf::RankConfig& conf = rc->second;
    if (conf.RankAlgoList.empty() && conf.RankScore.empty()) return true;    // :168-171
    const int batch = conf.BatchCount > 0 ? conf.BatchCount : 100;           // :163-166
    std::string uv, verr;
    std::vector<float> user_vec;
    if (e->user_vectors.VectorString(user->Id, &uv, &verr)) user_vec = recall::ParseVectorString(uv);
    // batches × algos; a failing batch keeps its previous scores (:274-276,311)
    for (size_t b0 = 0; b0 < items.size(); b0 += (size_t)batch) {
        const size_t b1 = std::min(items.size(), b0 + (size_t)batch);
        for (const auto& algo : conf.RankAlgoList) {
            algorithm::AlgoData data;
            data.kind = algorithm::AlgoData::kRank;
            data.rank.UserVector = user_vec;
            auto uf = e->user_fields.find(user->Id);
            if (uf != e->user_fields.end()) data.rank.UserFieldIds = uf->second;
            for (size_t i = b0; i < b1; ++i) data.rank.ItemIds.push_back(items[i]->Id);
            algorithm::AlgoResult res;
            std::string aerr;
            if (!e->algorithms.Run(algo, data, &res, &aerr)) continue;       // logged; batch skipped
            for (size_t j = 0; j < res.responses.size() && b0 + j < b1; ++j) {          // rank_service.go:314-335
                const algorithm::AlgoResponse& r = res.responses[j];
                if (r.GetModuleType()) {
                    for (const auto& kv : r.GetScoreMap()) items[b0 + j]->AddAlgoScore(algo + "_" + kv.first, kv.second);
                } else if (r.IsMultiClassify()) {
                    for (const auto& kv : r.GetClassifyMap()) {
                        if (kv.second.size() == 1) items[b0 + j]->AddAlgoScore(algo + "_" + kv.first, kv.second[0]);
                        else for (size_t c = 0; c < kv.second.size(); ++c)
                            items[b0 + j]->AddAlgoScore(algo + "_" + kv.first + "_" + std::to_string(c), kv.second[c]);
                    }
                } else {
                    items[b0 + j]->AddAlgoScore(algo, r.GetScore());
                }
            }
        }
    }
    if (!conf.RankScore.empty()) {                                           // :339-363
        const uint32_t n = (uint32_t)items.size();
        // one expression over every item: variables from the AB parameters first, then the item (ast_parameter_data.go:30-40)
        auto eval = [&](pg_expr* ex, std::vector<double>* out) -> bool {
            const int nv = pg_expr_num_vars(ex);
            const bool antlr = pg_expr_is_antlr(ex) != 0;
            std::vector<double> vars((size_t)nv * n, 0.0);
            std::vector<char> failed(antlr ? n : 0, 0);
            out->assign(n, 0.0);
            for (int v = 0; v < nv; ++v) {
                const std::string name = pg_expr_var_name(ex, v);
                auto ab = ctx->ExperimentParams.find(name);
                if (!antlr) {
                    for (uint32_t i = 0; i < n; ++i) {
                        double x = 0.0;
                        if (ab != ctx->ExperimentParams.end() && ab->second != 0.0) x = ab->second;
                        else items[i]->FloatExprData(name, &x);
                        vars[(size_t)v * n + i] = x;
                    }
                    continue;
                }
                // ASTType "antlr": the data is AstParameterData.ExprData() — the experiment's parameters overlaid by the item's
                // algorithm scores and properties (ast_parameter_data.go:17-28, item.go:213-227; no "current_score" there); a
                // variable the map lacks, or one that is not a number, fails the evaluation: the item scores 0 (ast.go:374-383).
                // maxIndex(${p}) / maxValue(${p}) (antlr_functions.go:34-66,72-91) read the list property p.
                const bool fidx = name.rfind("maxIndex(", 0) == 0, fval = name.rfind("maxValue(", 0) == 0;
                const std::string inner = (fidx || fval) ? name.substr(9, name.size() - 10) : name;
                for (uint32_t i = 0; i < n; ++i) {
                    double x = 0.0;
                    bool ok = false;
                    const module::Item& it = *items[i];
                    auto a = it.algoScores.find(inner);
                    auto p = it.Properties.find(inner);
                    if (fidx || fval) {
                        if (p != it.Properties.end() && p->second.type == json::Value::Array && !p->second.arr.empty()) {
                            size_t best = 0;
                            double bv = ToFloat(p->second.arr[0], 0.0);
                            for (size_t j = 1; j < p->second.arr.size(); ++j) {
                                const double cv = ToFloat(p->second.arr[j], 0.0);
                                if (cv > bv) { bv = cv; best = j; }
                            }
                            x = fidx ? (double)best : bv;
                            ok = true;
                        }
                    } else if (p != it.Properties.end()) {                  // (the item's properties are written last: they win)
                        ok = p->second.type == json::Value::Number;
                        x = p->second.num;
                    } else if (a != it.algoScores.end()) {
                        x = a->second;
                        ok = true;
                    } else if (ab != ctx->ExperimentParams.end()) {
                        x = ab->second;
                        ok = true;
                    }
                    if (!ok) failed[i] = 1;
                    vars[(size_t)v * n + i] = x;
                }
            }
            if (n && pg_expr_eval(e->ctx, ex, nv ? vars.data() : nullptr, n, out->data()) != PG_OK) return false;
            for (uint32_t i = 0; antlr && i < n; ++i)
                if (failed[i]) (*out)[i] = 0.0;
            return true;
        };
        pg_expr* ex = nullptr;
        if (pg_expr_compile_typed(conf.RankScore.c_str(), conf.ASTType.c_str(), &ex) != PG_OK) { if (err) *err = pg_err("pg_expr_compile"); return false; }
        // ScoreRewrite (:296-306,343-353): every source's expression over the item as the algorithms left it, into a map
        // first, then written back (AddAlgoScores); a source whose expression does not compile scores 0
        if (!conf.ScoreRewrite.empty()) {
            std::vector<std::pair<std::string, std::vector<double>>> rewritten;
            for (const auto& rw : conf.ScoreRewrite) {
                std::vector<double> vals(n, 0.0);
                pg_expr* rex = nullptr;
                if (pg_expr_compile_typed(rw.second.c_str(), conf.ASTType.c_str(), &rex) == PG_OK) {
                    const bool ok = eval(rex, &vals);
                    pg_expr_free(rex);
                    if (!ok) { pg_expr_free(ex); if (err) *err = pg_err(("pg_expr_eval (ScoreRewrite[" + rw.first + "])").c_str()); return false; }
                }
                rewritten.emplace_back(rw.first, std::move(vals));
            }
            for (uint32_t i = 0; i < n; ++i) {
                std::map<std::string, double> scores;
                for (const auto& rw : rewritten) scores[rw.first] = rw.second[i];
                items[i]->AddAlgoScores(scores);
            }
        }
        std::vector<double> out;
        const bool ok = eval(ex, &out);
        pg_expr_free(ex);
        if (!ok) { if (err) *err = pg_err("pg_expr_eval"); return false; }
        for (uint32_t i = 0; i < n; ++i) items[i]->Score = out[i];
    }
    return true;
}
}  // namespace rank

// ---- engine --------------------------------------------------------------------------------------
Engine::~Engine() {
    if (ctx) {
        for (auto& kv : co_page) {
            pg_coalescer_destroy(kv.second.first);
            pg_expr_free(kv.second.second);
        }
        for (auto& kv : co_scene) pg_coalescer_destroy(kv.second);
        for (auto& kv : co_online) pg_coalescer_destroy(kv.second);
        DropViewsLocked();
        if (model) pg_model_destroy(ctx, model);
        for (auto& kv : named_models) pg_model_destroy(ctx, kv.second);
        if (fm2t) pg_model_destroy(ctx, fm2t);
        if (feats) pg_features_destroy(ctx, feats);
        if (staging_feats) pg_features_destroy(ctx, staging_feats);
        if (item_emb) pg_table_destroy(ctx, item_emb);
        if (staging) pg_table_destroy(ctx, staging);
        if (table) pg_table_destroy(ctx, table);
        pg_shutdown(ctx);
    }
}

// One coalescer per recall depth serves every per-request plug-in call of the scene: vector / i2i recalls, both rank
// algorithms (the DNN as algorithm 0, FM + two-tower behind it) and DPPSort.  k = 0: any (rank / sort calls do not
// depend on the recall depth).  At most kMaxSceneCoalescers depths are kept (each holds slots and a sibling context's
// scratch); a request with yet another K is served by the direct call.
pg_coalescer* Engine::SceneCoalescer(uint32_t k, std::string* err) {
    std::lock_guard<std::mutex> g(co_mu);
    if (k == 0 && !co_scene.empty()) return co_scene.begin()->second;
    if (k == 0) k = 5000;                          // sizes a rank batch: as many candidates as 256 requests x 5000
    auto it = co_scene.find(k);
    if (it != co_scene.end()) return it->second;
    if (co_scene.size() >= kMaxSceneCoalescers) {
        if (err) *err = "coalescer: too many distinct recall depths";
        return nullptr;
    }
    pg_scene_config sc;
    memset(&sc, 0, sizeof sc);
    sc.base.k = k;
    sc.base.max_wait_us = coalesce_wait_us;
    sc.base.depth = coalesce_depth;
    sc.base.max_rank_items = 16384;
    sc.base.timeout_us = coalesce_timeout_us;
    pg_rank_algo algos[2];
    memset(algos, 0, sizeof algos);
    std::vector<int32_t> cols;
    if (model) {
        algos[sc.n_algos].model = model;
        algos[sc.n_algos].name = "dnn";
        sc.n_algos++;
    }
    if (fm2t && feats && !fm2t_columns.empty()) {
        bool ok = true;
        for (const auto& cname : fm2t_columns) {
            const int idx = pg_features_column_index(feats, cname.c_str());
            ok = ok && idx >= 0;
            cols.push_back(idx);
        }
        if (ok) {
            algos[sc.n_algos].model = fm2t;
            algos[sc.n_algos].name = "fm2t";
            algos[sc.n_algos].features = feats;
            algos[sc.n_algos].item_field_cols = cols.data();
            sc.n_algos++;
        }
    }
    sc.algos = algos;
    pg_coalescer* c = nullptr;
    if (pg_coalescer_create_scene(ctx, table, &sc, &c) != PG_OK) {
        if (err) *err = std::string("pg_coalescer_create_scene: ") + pg_last_error();
        return nullptr;
    }
    co_scene[k] = c;
    return c;
}

// the OnlineVectorRecall's coalescer: user features → the vector model's user tower → top-k of the item-embedding table
pg_coalescer* Engine::OnlineCoalescer(uint32_t k, std::string* err) {
    std::lock_guard<std::mutex> g(co_mu);
    auto it = co_online.find(k);
    if (it != co_online.end()) return it->second;
    if (co_online.size() >= kMaxSceneCoalescers) {
        if (err) *err = "coalescer: too many distinct recall depths";
        return nullptr;
    }
    pg_scene_config sc;
    memset(&sc, 0, sizeof sc);
    sc.base.k = k;
    sc.base.max_wait_us = coalesce_wait_us;
    sc.base.depth = coalesce_depth;
    sc.base.timeout_us = coalesce_timeout_us;
    sc.query_model = fm2t;
    pg_coalescer* c = nullptr;
    if (pg_coalescer_create_scene(ctx, item_emb, &sc, &c) != PG_OK) {
        if (err) *err = std::string("pg_coalescer_create_scene: ") + pg_last_error();
        return nullptr;
    }
    co_online[k] = c;
    return c;
}

// configuration-time changes (a model or a feature column is replaced) retire the coalescers that hold the old objects;
// the next call builds new ones.  Not to be called while requests are in flight.
void Engine::DropCoalescers() {
    std::lock_guard<std::mutex> g(co_mu);
    for (auto& kv : co_page) {
        pg_coalescer_destroy(kv.second.first);
        pg_expr_free(kv.second.second);
    }
    co_page.clear();
    for (auto& kv : co_scene) pg_coalescer_destroy(kv.second);
    co_scene.clear();
    for (auto& kv : co_online) pg_coalescer_destroy(kv.second);
    co_online.clear();
    DropViewsLocked();
}

void Engine::DropViewsLocked() {
    for (auto& kv : co_views) {
        if (kv.second.co) pg_coalescer_destroy(kv.second.co);
        if (kv.second.view) pg_table_destroy(ctx, kv.second.view);
    }
    co_views.clear();
}

// The view of a filtered Hologres recall for the table's current generation.  The constant of the clause was fixed when the
// recall was built (hologres_vector_recall.go:56-61), so the admitted set only changes with the table (ingest.cpp: a commit is
// exclusive against every request, so no request sees two generations) or with the column (ph_engine_set_feature_column drops
// the views).  nullptr: no feature column of that name (the SQL would fail).
const Engine::FilterView* Engine::ViewFor(const recconf::RecallConfig& conf, uint32_t k, const pg_table* base) {
    if (!base) base = table;
    std::lock_guard<std::mutex> g(co_mu);
    const int col = feats ? pg_features_column_index(feats, conf.WhereColumn.c_str()) : -1;
    if (col < 0) return nullptr;
    FilterView& fv = co_views[conf.Name];
    const uint64_t gen = generation.load();
    if (fv.generation == gen) return &fv;
    if (fv.co) pg_coalescer_destroy(fv.co);
    if (fv.view) pg_table_destroy(ctx, fv.view);
    fv = FilterView();
    fv.generation = gen;
    const int rc = pg_table_view_create(ctx, base, feats, col, conf.WhereOp, conf.WhereValue, &fv.view);
    if (rc == PG_ERR_EMPTY) { fv.empty = true; return &fv; }             // no row passes: every answer is empty
    // (PG_ERR_INVALID is a misconfiguration — a feature store shorter than the table, a bad operator: the per-call path below
    // reports it on every request instead of serving empty pages for the whole generation)
    if (rc != PG_OK) { fv.failed = true; fv.view = nullptr; return &fv; }
    if (coalesce) {
        pg_scene_config sc;
        memset(&sc, 0, sizeof sc);
        sc.base.k = k;
        sc.base.max_wait_us = coalesce_wait_us;
        sc.base.depth = coalesce_depth;
        sc.base.timeout_us = coalesce_timeout_us;
        if (pg_coalescer_create_scene(ctx, fv.view, &sc, &fv.co) != PG_OK) fv.co = nullptr;    // direct calls on the view then
    }
    return &fv;
}

pg_coalescer* Engine::PageCoalescer(const recconf::RecallConfig& conf, std::string* err) {
    std::lock_guard<std::mutex> g(co_mu);
    auto it = co_page.find(conf.Name);
    if (it != co_page.end()) return it->second.first;
    if (!model) {
        if (err) *err = "page recall: no rank model loaded";
        return nullptr;
    }
    pg_expr* ex = nullptr;
    if (pg_expr_compile(conf.RankScore.c_str(), &ex) != PG_OK) {
        if (err) *err = std::string("pg_expr_compile: ") + pg_last_error();
        return nullptr;
    }
    if (!conf.ScoreRewrite.empty()) {
        // the scene's ScoreRewrite rides on the RankScore: the device evaluates every source from the un-rewritten scores
        // in front of it (a source that does not compile scores 0, as in rank_service.go:299-303,349-351)
        std::vector<const char*> src;
        std::vector<pg_expr*> rex;
        for (const auto& rw : conf.ScoreRewrite) {
            pg_expr* r = nullptr;
            if (pg_expr_compile(rw.second.c_str(), &r) != PG_OK) r = nullptr;
            src.push_back(rw.first.c_str());
            rex.push_back(r);
        }
        const int rc = pg_expr_set_score_rewrites(ex, (uint32_t)src.size(), src.data(), rex.data());
        for (pg_expr* r : rex) pg_expr_free(r);
        if (rc != PG_OK) {
            if (err) *err = std::string("pg_expr_set_score_rewrites: ") + pg_last_error();
            pg_expr_free(ex);
            return nullptr;
        }
    }
    pg_coalescer_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.k = (uint32_t)conf.RecallCount;
    cfg.max_wait_us = coalesce_wait_us;
    cfg.depth = coalesce_depth;
    cfg.max_top_n = (uint32_t)std::min(conf.RecallCount, 1000);
    cfg.timeout_us = coalesce_timeout_us;
    pg_coalescer* c = nullptr;
    if (pg_coalescer_create(ctx, table, model, ex, conf.RankVar.c_str(), &cfg, &c) != PG_OK) {
        if (err) *err = std::string("pg_coalescer_create: ") + pg_last_error();
        pg_expr_free(ex);
        return nullptr;
    }
    co_page[conf.Name] = std::make_pair(c, ex);
    return c;
}

Engine* Engine::Create(const std::string& config_json, std::string* err) {
    std::unique_ptr<Engine> e(new Engine());
    if (!recconf::RecommendConfig::Parse(config_json, &e->config, err)) return nullptr;
    // What the reference's own loaders would do with RecallConfs / SortConfs comes first (they run in runBeforeStart,
    // before any start hook): a config that panics pairec must not start here either.
    for (const auto& r : e->config.RecallConfs) {
        const recall::LoadOutcome o = recall::CheckRecallConf(r);
        if (o.kind == recall::LoadOutcome::kPanic) { if (err) *err = "panic: " + o.message; return nullptr; }
        if (o.kind == recall::LoadOutcome::kUnavailable) { if (err) *err = o.message; return nullptr; }
    }
    // RankConf.ASTType = "antlr" selects another expression language in the reference (GetExpASTWithType /
    // ExprASTResultWithType, utils/ast/ast.go:338-389: the valuate evaluator with AntlrFunctions — maxIndex, maxValue, …).
    // This engine evaluates the default grammar only; evaluating an "antlr" RankScore with it would silently change scores.
    // Round 5: the subset of that language the reference's tests pin is compiled to the device program
    // (pg_expr_compile_typed); a RankScore or ScoreRewrite expression outside it still stops the load, named.
    for (const auto& kv : e->config.RankConf)
        if (kv.second.ASTType == "antlr") {
            std::vector<std::pair<std::string, std::string>> exprs;
            exprs.emplace_back("RankScore", kv.second.RankScore);
            for (const auto& rw : kv.second.ScoreRewrite) exprs.emplace_back("ScoreRewrite[" + rw.first + "]", rw.second);
            for (const auto& ex : exprs) {
                pg_expr* probe = nullptr;
                if (pg_expr_compile_typed(ex.second.c_str(), "antlr", &probe) != PG_OK) {
                    if (err) *err = "RankConf[" + kv.first + "]." + ex.first + " with ASTType \"antlr\": " + pg_last_error();
                    return nullptr;
                }
                pg_expr_free(probe);
            }
        }
    // FeatureService.LoadFeatureConf (feature_service.go:33-58) / UserFeatureService: one Feature per FeatureLoadConfig.  An unknown
    // FeatureType is the reference's panic (op.go:32); an expression normalizer outside the stated subset stops the load, named.
    {
        auto build = [&](const std::map<std::string, recconf::SceneFeatureConfig>& src, const char* key,
                         std::map<std::string, std::vector<std::shared_ptr<feature::Feature>>>* dst) {
            for (const auto& sc : src)
                for (const auto& lc : sc.second.FeatureLoadConfs) {
                    auto f = std::make_shared<feature::Feature>();
                    std::string ferr;
                    if (!f->LoadWithConfig(lc.Features, &ferr)) {
                        if (err) *err = std::string(key) + "[" + sc.first + "]: " + ferr;
                        return false;
                    }
                    (*dst)[sc.first].push_back(std::move(f));
                }
            return true;
        };
        if (!build(e->config.FeatureConfs, "FeatureConfs", &e->sceneFeatures)) return nullptr;
        if (!build(e->config.UserFeatureConfs, "UserFeatureConfs", &e->sceneUserFeatures)) return nullptr;
    }
    for (const auto& sc : e->config.SortConfs) {
        // RegisterSortWithConfig (sort/sort.go:162-200): DPPSort / SSDSort open their Hologres datasource first
        // (NewDPPSort, dpp_sort.go:60-64; NewSSDSort, ssd_sort.go:52-56) and panic without it; an unknown SortType
        // leaves s nil → panic("Sort is nil, name:…")
        if (sc.SortType == "DPPSort" || sc.SortType == "SSDSort") {
            if (err) *err = "panic: Postgres not found, name:" + sc.HologresName + " (SortConfs entry \"" + sc.Name + "\": " + sc.SortType +
                            " opens its Hologres datasource in the constructor; GPU diversity sorts are declared in UserDefineConfs.pairec_gpu.Sorts)";
            return nullptr;
        }
        static const char* host_sorts[] = {"AlgoScoreSort", "MultiRecallMixSort", "BoostScoreSort", "DiversityRuleSort", "TrafficControlSort",
                                           "BoostScoreByWeight", "DistinctIdSort", "CustomFieldSort", "ConditionSort"};
        bool known = false;
        for (const char* r : host_sorts) known |= sc.SortType == r;
        if (!known) { if (err) *err = "panic: Sort is nil, name:" + sc.Name; return nullptr; }
    }
    // GPU plugin settings live in UserDefineConfs["pairec_gpu"]: they cannot be declared in RecallConfs / SortConfs
    const json::Value& g = e->config.UserDefineConfs.at("pairec_gpu");
    if (g.type != json::Value::Object) { if (err) *err = "UserDefineConfs.pairec_gpu missing"; return nullptr; }
    const json::Value& tb = g.at("Table");
    e->table_rows = (uint64_t)tb.n("Rows");
    e->dim = (uint32_t)tb.n("Dim", 128);
    e->id_prefix = tb.s("IdPrefix", "item_");
    if (pg_init((int)g.n("Device", 0), nullptr, &e->ctx) != PG_OK) { if (err) *err = pg_err("pg_init"); return nullptr; }
    if (pg_table_create(e->ctx, e->table_rows, e->dim, 0, &e->table) != PG_OK) { if (err) *err = pg_err("pg_table_create"); return nullptr; }
    const std::string table_path = tb.s("Path", "");
    if (!table_path.empty()) {
        // (item_id, embedding) rows from a file: the loader streams them in chunks and commits (ingest.cpp); the same
        // call replaces the table later while the engine serves (ph_engine_ingest_file)
        if (!e->IngestFile(table_path, err)) return nullptr;
    } else if (pg_table_fill_synthetic(e->ctx, e->table, (uint64_t)tb.n("SyntheticSeed", 0x5EED0001), 1) != PG_OK) {
        if (err) *err = pg_err("pg_table_fill_synthetic");
        return nullptr;
    }
    const json::Value& co = g.at("Coalesce");
    if (co.type == json::Value::Object) {
        e->coalesce = true;
        e->coalesce_wait_us = (uint32_t)co.n("MaxWaitUs", 0);
        e->coalesce_depth = (uint32_t)co.n("Depth", 0);
        e->coalesce_timeout_us = (uint32_t)co.n("TimeoutUs", 0);       // the EAS client's per-call timeout (eas/client.go:53-58)
    }
    const json::Value& ov = g.at("OnlineVector");          // the vector model's item side: item-tower outputs as a table
    if (ov.type == json::Value::Object) {
        e->item_emb_rows = (uint64_t)ov.n("Rows", (long long)e->table_rows);
        e->item_emb_dim = (uint32_t)ov.n("Dim", 64);
        if (pg_table_create(e->ctx, e->item_emb_rows, (uint32_t)ov.n("Dim", 64), 0, &e->item_emb) != PG_OK ||
            pg_table_fill_synthetic(e->ctx, e->item_emb, (uint64_t)ov.n("SyntheticSeed", 0x5EED0077), 1) != PG_OK) {
            if (err) *err = pg_err("online vector item table");
            return nullptr;
        }
    }
    // built-in sorts (sort.go init(): "ItemRankScore" is registered by default)
    e->sorts.RegisterSort("ItemRankScore", std::make_shared<GpuItemRankScoreSort>(e.get()), nullptr);
    e->sorts.RegisterSort("ItemScore", std::make_shared<GpuItemScoreSort>(e.get()), nullptr);
    for (const auto& d : e->config.DPPConf) e->sorts.RegisterSort(d.Name, std::make_shared<GpuDPPSort>(e.get(), d), nullptr);
    // SortConfs (validated above): AlgoScoreSort and CustomFieldSort are host logic over a GPU sort; the other rule-based sorts
    // are outside this engine's scope and are skipped
    for (const auto& sc : e->config.SortConfs) {
        if (sc.SortType == "AlgoScoreSort") e->sorts.RegisterSortWithConfig(sc.Name, std::make_shared<GpuAlgoScoreSort>(e.get(), sc));
        else if (sc.SortType == "CustomFieldSort") e->sorts.RegisterSortWithConfig(sc.Name, std::make_shared<GpuCustomFieldSort>(e.get(), sc));
    }
    // the GPU sorts of a pairec process: registered by name in the start hook (sort.RegisterSort — first registration wins)
    for (const auto& sc : e->config.GpuSorts) {
        if (sc.SortType == "DPPSort") e->sorts.RegisterSort(sc.Name, std::make_shared<GpuDPPSort>(e.get(), sc.DPPConf), nullptr);
        else if (sc.SortType == "SSDSort") e->sorts.RegisterSort(sc.Name, std::make_shared<GpuSSDSort>(e.get(), sc.SSDConf), nullptr);
        else if (sc.SortType == "AlgoScoreSort") e->sorts.RegisterSort(sc.Name, std::make_shared<GpuAlgoScoreSort>(e.get(), sc), nullptr);
        else if (sc.SortType == "CustomFieldSort") e->sorts.RegisterSort(sc.Name, std::make_shared<GpuCustomFieldSort>(e.get(), sc), nullptr);
        else if (sc.SortType == "ItemRankScore") e->sorts.RegisterSort(sc.Name, std::make_shared<GpuItemRankScoreSort>(e.get()), nullptr);
        else if (sc.SortType == "ItemScore") e->sorts.RegisterSort(sc.Name, std::make_shared<GpuItemScoreSort>(e.get()), nullptr);
        else if (sc.SortType == "DiversityRuleSort") e->sorts.RegisterSort(sc.Name, std::make_shared<GpuDiversityRuleSort>(e.get(), sc.DiversityConf), nullptr);
        else if (sc.SortType == "BoostScoreSort") e->sorts.RegisterSort(sc.Name, std::make_shared<GpuBoostScoreSort>(e.get(), sc.BoostConf), nullptr);
        else if (sc.SortType == "MultiRecallMixSort") e->sorts.RegisterSort(sc.Name, std::make_shared<GpuMultiRecallMixSort>(e.get(), sc.MixConf), nullptr);
        else if (sc.SortType == "TrafficControlSort") e->sorts.RegisterSort(sc.Name, std::make_shared<GpuTrafficControlSort>(e.get(), sc.TrafficConf), nullptr);
        else if (sc.SortType == "DistinctIdSort") e->sorts.RegisterSort(sc.Name, std::make_shared<GpuDistinctIdSort>(e.get(), sc.DistinctConf), nullptr);
        else { if (err) *err = "pairec_gpu.Sorts: unknown SortType " + sc.SortType; return nullptr; }
    }
    for (const auto& fc : e->config.GpuFilters) e->gpu_filters[fc.Name] = fc;
    // algorithms by name (the shim's start hook does the same with algorithm.RegisterAlgorithm)
    bool first_dnn = true, first_fm = true;
    for (const auto& a : g.at("Algorithms").arr) {
        const std::string name = a.s("Name"), kind = a.s("Kind");
        if (a.has("Precision")) {
            // the rank model's matrix layers: "f32" (bit-defined), "bf16" (fastest), "bf16x3" (split bf16: the fp32 scores of
            // the reference's model servers — eas/easyrec_response.go:479-483 — at matrix-pipe speed), "f16x2" / "f16" (dnn3 only: the same 1e-5 of the fp32 scores on scaled fp16 operands,
            // out-of-range tiles re-served in bf16x3)
            const std::string pr = a.s("Precision");
            const int pv = pr == "f32" ? PG_PREC_F32 : pr == "bf16" ? PG_PREC_BF16 : pr == "bf16x3" ? PG_PREC_BF16X3
                           : pr == "f16x2" ? PG_PREC_F16X2 : pr == "f16" ? PG_PREC_F16 : -1;
            if (pv < 0) {
                if (err) *err = "pairec_gpu.Algorithms: " + name + ": Precision \"" + pr + "\" (f32, bf16, bf16x3, f16x2 or f16)";
                return nullptr;
            }
            e->algo_precision[name] = pv;
            if (kind == "dnn3" && first_dnn) e->default_dnn_precision = pv;
            if (kind == "fm2t" && first_fm) e->default_fm2t_precision = pv;
        }
        first_dnn = first_dnn && kind != "dnn3";
        first_fm = first_fm && kind != "fm2t";
        if (kind == "faiss") e->algorithms.RegisterAlgorithm(name, std::make_shared<GpuFaissAlgorithm>(e.get()));
        else if (kind == "dnn3") {
            std::vector<std::string> outs;
            for (const auto& o : a.at("Outputs").arr) if (o.type == json::Value::String) outs.push_back(o.str);
            e->algorithms.RegisterAlgorithm(name, std::make_shared<GpuDnnAlgorithm>(e.get(), name, outs));
        }
        else if (kind == "online_vector") e->algorithms.RegisterAlgorithm(name, std::make_shared<GpuOnlineVectorAlgorithm>(e.get()));
        else if (kind == "fm2t") {
            std::vector<std::string> cols;
            for (const auto& c : a.at("ItemFieldColumns").arr) if (c.type == json::Value::String) cols.push_back(c.str);
            if (e->fm2t_columns.empty()) e->fm2t_columns = cols;       // the scene coalescer's FM algorithm uses the first one's columns
            e->algorithms.RegisterAlgorithm(name, std::make_shared<GpuFm2tAlgorithm>(e.get(), cols));
        }
    }
    // recall.Load over RecallConfs, with the reference's outcomes (service/recall/recall.go:47-107)
    for (const auto& r : e->config.RecallConfs) {
        if (r.RecallType == "MockRecall") e->recalls.RegisterRecall(r.Name, std::make_shared<MockRecall>(r));
        else if (r.RecallType == "OnlineVectorRecall") e->recalls.RegisterRecall(r.Name, std::make_shared<GpuOnlineVectorRecall>(e.get(), r));
    }
    // the GPU recalls: recall.RegisterRecall(name, impl) in the start hook (overwrites)
    for (const auto& r : e->config.GpuRecalls) {
        if (r.Kind == "vector") e->recalls.RegisterRecall(r.Name, std::make_shared<GpuVectorRecall>(e.get(), r));
        else if (r.Kind == "i2i") e->recalls.RegisterRecall(r.Name, std::make_shared<GpuI2IVectorRecall>(e.get(), r));
        else if (r.Kind == "hologres_v2") e->recalls.RegisterRecall(r.Name, std::make_shared<GpuHologresVectorRecall>(e.get(), r, true));
        else if (r.Kind == "hologres") e->recalls.RegisterRecall(r.Name, std::make_shared<GpuHologresVectorRecall>(e.get(), r, false));
        else if (r.Kind == "online_hologres") e->recalls.RegisterRecall(r.Name, std::make_shared<GpuOnlineHologresVectorRecall>(e.get(), r));
        else if (r.Kind == "page") {
            if (r.RankScore.empty() || r.RankVar.empty() || r.RecallCount <= 0) {
                if (err) *err = "pairec_gpu.Recalls: Kind \"page\" needs RecallCount, RankScore and RankVar";
                return nullptr;
            }
            e->recalls.RegisterRecall(r.Name, std::make_shared<GpuPageRecall>(e.get(), r));
        }
        else { if (err) *err = "pairec_gpu.Recalls: unknown Kind " + r.Kind; return nullptr; }
    }
    return e.release();
}

bool Engine::ItemStateFilter(const recconf::GpuFilterConfig& conf, const module::User* user, std::vector<module::ItemPtr>* items, std::string* err) {
    return item_state_filter(this, conf, user, items, err);
}
bool Engine::DimensionUniqueFilter(const recconf::GpuFilterConfig& conf, std::vector<module::ItemPtr>* items, std::string* err) {
    return dimension_unique_filter(this, conf, items, err);
}

bool Engine::BlendFilter(const recconf::GpuFilterConfig& conf, std::vector<module::ItemPtr>* items, std::string* err) {
    return blend_filter(this, conf, items, err);
}

bool Engine::SetTrafficAlpha(const std::string& sort_name, const std::string& target_id, double alpha, std::string* err) {
    auto s = std::dynamic_pointer_cast<GpuTrafficControlSort>(sorts.Get(sort_name));
    if (!s) { if (err) *err = "TrafficControlSort:not find, name:" + sort_name; return false; }
    if (!s->SetAlpha(target_id, alpha)) { if (err) *err = "TrafficControlSort " + sort_name + ": no target \"" + target_id + "\""; return false; }
    return true;
}

bool Engine::ClasscutFilter(const recconf::GpuFilterConfig& conf, std::vector<module::ItemPtr>* items, std::string* err) {
    return classcut_filter(this, conf, items, err);
}

bool Engine::QuotaFilter(const recconf::GpuFilterConfig& conf, std::vector<module::ItemPtr>* items, std::string* err) {
    return quota_filter(this, conf, items, err);
}

bool Engine::Recommend(const std::string& uid, int size, const std::string& scene,
                       std::vector<module::ItemPtr>* out, std::string* err) {
    return Recommend(uid, size, scene, json::Value(), out, err);
}

bool Engine::Recommend(const std::string& uid, int size, const std::string& scene, const json::Value& experiment_params,
                       std::vector<module::ItemPtr>* out, std::string* err) {
    VersionLock::Read generation_guard(version);     // one generation of rows and ids for the whole request
    module::User user(uid);
    context::RecommendContext ctx;
    ctx.Size = size;
    ctx.Param["scene"] = json::Value::Str(scene);
    // request parameters other than the scene ride in the experiment object under "_param" (the driver API has no
    // separate argument for them): "item_id" is what I2IVectorRecall reads with context.GetParameter
    for (const auto& kv : experiment_params.at("_param").obj) ctx.Param[kv.first] = kv.second;
    ctx.ExperimentParamsJson = experiment_params;
    // the request's user features ("features" of POST /api/recommend → User.Properties, web/recommend_controller.go) ride under
    // "_user_features"; UserFeatureService.LoadUserFeatures (user_recommend.go:64) transforms them before the recalls
    for (const auto& kv : experiment_params.at("_user_features").obj) user.Properties[kv.first] = kv.second;
    {
        auto uf = sceneUserFeatures.find(scene);
        if (uf != sceneUserFeatures.end()) {
            std::vector<module::ItemPtr> none;
            for (const auto& f : uf->second) f->LoadFeatures(&user, none, &ctx);
        }
    }
    // RecallService.GetItems (service/recall.go:53-153): scene → category → recall names, concatenated
    std::vector<module::ItemPtr> items;
    auto sc = config.SceneRecallNames.find(scene);
    if (sc != config.SceneRecallNames.end())
        for (const auto& cat : sc->second)
            for (const auto& name : cat.second) {
                std::string rerr;
                auto r = recalls.GetRecall(name, &rerr);
                if (!r) continue;
                // AB experiment: interface assertion + "recall.<name>" params object (service/recall.go:95-105)
                if (ctx.HasExperiment())
                    if (auto* cr = dynamic_cast<recall::ICloneRecall*>(r.get())) {
                        const json::Value& rc = ctx.ExperimentParamsJson.at("recall." + cr->GetRecallName());
                        if (rc.type == json::Value::Object)
                            if (auto cloned = cr->CloneWithConfig(rc)) r = cloned;
                    }
                auto got = r->GetCandidateItems(&user, &ctx);
                items.insert(items.end(), got.begin(), got.end());
            }
    items = filter::UniqueFilter(items);
    {   // FilterService.Filter (user_recommend.go:105-127): the scene's device filters, in order; an error leaves the items as they are
        auto fn = config.GpuFilterNames.find(scene);
        if (fn != config.GpuFilterNames.end())
            for (const auto& name : fn->second) {
                auto f = gpu_filters.find(name);
                std::string ferr;
                if (f != gpu_filters.end()) RunGpuFilter(f->second, &user, &items, &ferr);
            }
    }
    {   // FeatureService.LoadFeatures (user_recommend.go:129; feature_service.go:77-131): "features.scene.name" of the experiment first
        std::string fscene = ctx.HasExperiment() ? ctx.ExperimentParamsJson.s("features.scene.name") : "";
        if (fscene.empty()) fscene = scene;
        auto sf = sceneFeatures.find(fscene);
        if (sf != sceneFeatures.end())
            for (const auto& f : sf->second) f->LoadFeatures(&user, items, &ctx);
    }
    if (!rank::Rank(this, &user, items, &ctx, err)) return false;
    // SortService.Sort (sort/sort.go:65-125): SortNames[scene] else the default ItemRankScore
    std::vector<std::string> names;
    auto sn = config.SortNames.find(scene);
    if (sn != config.SortNames.end()) names = sn->second;
    if (names.empty()) names.push_back("ItemRankScore");
    sort::SortData sd;
    sd.Data = items;
    sd.Context = &ctx;
    sd.User = &user;
    for (const auto& n : names) {
        auto s = sorts.Get(n);
        if (!s) continue;
        // AB experiment: ICloneSort + "sort.<name>" params object (sort/sort.go:110-121)
        if (ctx.HasExperiment())
            if (auto* cs = dynamic_cast<sort::ICloneSort*>(s.get())) {
                const json::Value& sc2 = ctx.ExperimentParamsJson.at("sort." + cs->GetSortName());
                if (sc2.type == json::Value::Object)
                    if (auto cloned = cs->CloneWithConfig(sc2)) s = cloned;
            }
        std::string serr;
        s->Sort(&sd, &serr);                                          // error ignored (sort.go:123)
    }
    if ((int)sd.Data.size() > size) sd.Data.resize((size_t)size);     // items[:size]
    *out = sd.Data;
    return true;
}

// ---- EasyrecAlgoDataGenerator ------------------------------------------------------------------------
namespace rank {
static void value_json(const json::Value& v, std::string* o) {
    switch (v.type) {
        case json::Value::String: json::Escape(v.str, o); break;
        case json::Value::Number: *o += v.is_int ? std::to_string(v.i) : json::NumToString(v.num); break;
        case json::Value::Bool: *o += v.b ? "true" : "false"; break;
        default: *o += "null";
    }
}
json::Value EasyrecAlgoDataGenerator::Feature::Default() const {       // feature.defaultValue, :154-171
    json::Value v;
    if (type == json::Value::Number) {
        v.type = json::Value::Number;
        v.is_int = is_int;
        v.num = 0.0;
        v.i = 0;
    } else {
        v.type = json::Value::String;                                  // string and everything else: ""
    }
    return v;
}
EasyrecAlgoDataGenerator::EasyrecAlgoDataGenerator(const std::vector<std::string>& contextFeatures) {
    // parseFeature starts true (:187): the schema is the configured list, every column typed string
    for (const auto& n : contextFeatures) itemFeatures_.push_back(Feature{n, json::Value::String, false});
}
void EasyrecAlgoDataGenerator::SetItemFeatures(const std::vector<std::string>& in) {
    if (!in.empty()) {
        hasInputMap_ = true;
        if (in[0] != "*") {
            parseInputItemFeature_ = true;
            for (const auto& n : in) inputItemFeatures_.push_back(Feature{n, json::Value::String, false});
        }
    } else {
        parseInputItemFeature_ = true;
    }
}
void EasyrecAlgoDataGenerator::AddFeatures(const module::ItemPtr& item,
                                           const std::map<std::string, json::Value>& itemFeatures,
                                           const std::map<std::string, json::Value>& userFeatures) {
    if (item) requestItem_.push_back(item);
    if (!parseFeature_) {                       // (never taken after the constructor above; kept for fidelity)
        for (const auto& kv : itemFeatures) itemFeatures_.push_back(Feature{kv.first, kv.second.type, kv.second.is_int});
        userFeatures_ = userFeatures;
        parseFeature_ = true;
    }
    if (!parseInputItemFeature_) {              // "*": every feature of the first item that is not a context feature
        for (const auto& kv : itemFeatures) {
            bool ctxf = false;
            for (const auto& f : itemFeatures_) ctxf |= f.name == kv.first;
            if (!ctxf) inputItemFeatures_.push_back(Feature{kv.first, kv.second.type, kv.second.is_int});
        }
        parseInputItemFeature_ = true;
    }
    if (userFeatures_.empty()) userFeatures_ = userFeatures;
    for (const auto& f : itemFeatures_) {
        auto it = itemFeatures.find(f.name);
        contextFeatures_[f.name].push_back(it != itemFeatures.end() ? it->second : f.Default());
    }
    if (hasInputMap_)
        for (const auto& f : inputItemFeatures_) {
            auto it = itemFeatures.find(f.name);
            inputItemFeatureMap_[f.name].push_back(it != itemFeatures.end() ? it->second : f.Default());
        }
}
std::string EasyrecAlgoDataGenerator::GeneratorAlgoData() {
    std::string o = "{\"user_features\":{";
    bool first = true;
    for (const auto& kv : userFeatures_) {
        if (!first) o += ",";
        first = false;
        json::Escape(kv.first, &o);
        o += ":";
        value_json(kv.second, &o);
    }
    o += "},\"item_ids\":[";
    for (size_t i = 0; i < requestItem_.size(); ++i) {
        if (i) o += ",";
        json::Escape(requestItem_[i]->Id, &o);
    }
    o += "]";
    auto lists = [&](const char* key, std::map<std::string, std::vector<json::Value>>& m) {
        o += std::string(",\"") + key + "\":{";
        bool f2 = true;
        for (auto& kv : m) {
            if (!f2) o += ",";
            f2 = false;
            json::Escape(kv.first, &o);
            o += ":[";
            for (size_t i = 0; i < kv.second.size(); ++i) {
                if (i) o += ",";
                value_json(kv.second[i], &o);
            }
            o += "]";
            kv.second.clear();                   // g.contextFeatures[k] = g.contextFeatures[k][:0]
        }
        o += "}";
    };
    lists("context_features", contextFeatures_);
    lists("item_features", inputItemFeatureMap_);
    o += "}";
    requestItem_.clear();
    return o;
}
}  // namespace rank

}  // namespace pairec

// ---- C driver API for the tests ---------------------------------------------------------------------
using namespace pairec;
static thread_local std::string g_ph_err;
static thread_local std::string g_ph_out;

extern "C" {

const char* ph_last_error(void) { return g_ph_err.c_str(); }

void* ph_engine_create(const char* config_json) {
    std::string err;
    Engine* e = Engine::Create(config_json ? config_json : "", &err);
    if (!e) g_ph_err = err;
    return e;
}
void ph_engine_destroy(void* h) { delete (Engine*)h; }

// load the DNN3 rank model (blob format of pg_model_load) into the engine
int ph_engine_load_dnn3(void* h, int prec, const char* blob, size_t len) {
    Engine* e = (Engine*)h;
    if (!e || !blob) return -1;
    VersionLock::Write w(e->version);                  // no request is inside the coalescers / holds the model this replaces
    e->DropCoalescers();                               // they hold the old model
    if (e->model) { pg_model_destroy(e->ctx, e->model); e->model = nullptr; }
    if (prec < 0) prec = e->default_dnn_precision;     // pairec_gpu.Algorithms[].Precision of the scene's DNN
    const int rc = pg_model_load(e->ctx, PG_MODEL_DNN3, (pg_prec)prec, blob, len, &e->model);
    if (rc != PG_OK) g_ph_err = pg_last_error();
    return rc;
}

// the multi-output model of rank algorithm `algo` (blob format PG_MODEL_DNN3_MULTI: n_out heads on one trunk); its
// outputs are named by the algorithm's "Outputs" list, in order
int ph_engine_load_dnn3_multi(void* h, const char* algo, int prec, const char* blob, size_t len) {
    Engine* e = (Engine*)h;
    if (!e || !blob || !algo) return -1;
    VersionLock::Write w(e->version);                  // no request in flight holds the model this replaces
    pg_model* m = nullptr;
    if (prec < 0) prec = e->PrecisionOf(algo, e->default_dnn_precision);
    const int rc = pg_model_load(e->ctx, PG_MODEL_DNN3_MULTI, (pg_prec)prec, blob, len, &m);
    if (rc != PG_OK) { g_ph_err = pg_last_error(); return rc; }
    auto it = e->named_models.find(algo);
    if (it != e->named_models.end()) pg_model_destroy(e->ctx, it->second);
    e->named_models[algo] = m;
    return 0;
}

// one DNN3 model per output of a multi-output rank algorithm: key "<algo>/<output>"
int ph_engine_load_dnn3_named(void* h, const char* key, int prec, const char* blob, size_t len) {
    Engine* e = (Engine*)h;
    if (!e || !blob || !key) return -1;
    VersionLock::Write w(e->version);
    pg_model* m = nullptr;
    if (prec < 0) prec = e->PrecisionOf(std::string(key).substr(0, std::string(key).find('/')), e->default_dnn_precision);
    const int rc = pg_model_load(e->ctx, PG_MODEL_DNN3, (pg_prec)prec, blob, len, &m);
    if (rc != PG_OK) { g_ph_err = pg_last_error(); return rc; }
    auto it = e->named_models.find(key);
    if (it != e->named_models.end()) pg_model_destroy(e->ctx, it->second);
    e->named_models[key] = m;
    return 0;
}

// the vector model of the online recall (blob format of pg_model_load, PG_MODEL_FM_TWOTOWER)
int ph_engine_load_fm2t(void* h, int prec, const char* blob, size_t len) {
    Engine* e = (Engine*)h;
    if (!e || !blob) return -1;
    VersionLock::Write w(e->version);
    e->DropCoalescers();                               // they hold the old model
    if (e->fm2t) { pg_model_destroy(e->ctx, e->fm2t); e->fm2t = nullptr; }
    if (prec < 0) prec = e->default_fm2t_precision;
    const int rc = pg_model_load(e->ctx, PG_MODEL_FM_TWOTOWER, (pg_prec)prec, blob, len, &e->fm2t);
    if (rc != PG_OK) g_ph_err = pg_last_error();
    else if (len >= 16) {
        uint32_t hdr[4];
        memcpy(hdr, blob, sizeof hdr);                  // u32 n_user_fields, n_item_fields, k, d_user (include/pairec_gpu.h)
        e->fm2t_nuf = hdr[0];
        e->fm2t_d_user = hdr[3];
    }
    return rc;
}

// one int32 item feature column (dictionary-encoded categorical feature), keyed by item row
int ph_engine_set_feature_column(void* h, const char* name, const int32_t* values, uint64_t n) {
    Engine* e = (Engine*)h;
    if (!e || !name || !values || n != e->table_rows) { g_ph_err = "feature column: bad argument (one value per table row)"; return -1; }
    // exclusive against every request (they hold the version lock shared from their first plug-in call to their last label
    // lookup): the coalescers and views dropped here are not in use, and no request sees the column half-way.  A column
    // that belongs to a NEW generation of the table goes through ph_engine_ingest_feature_column instead.
    VersionLock::Write w(e->version);
    e->DropCoalescers();
    if (!e->feats && pg_features_create(e->ctx, e->table_rows, &e->feats) != PG_OK) { g_ph_err = pg_last_error(); return -1; }
    const int rc = pg_features_set_column(e->ctx, e->feats, name, PG_F_I32, values, 0.0);
    if (rc != PG_OK) g_ph_err = pg_last_error();
    return rc;
}

// the alpha of one target of a pairec_gpu.Sorts TrafficControlSort entry from the next request on (the PID controller's output:
// the Go side computes it and hands it over)
int ph_engine_set_traffic_alpha(void* h, const char* sort_name, const char* target_id, double alpha) {
    if (!h || !sort_name || !target_id) { g_ph_err = "ph_engine_set_traffic_alpha: NULL argument"; return -1; }
    std::string err;
    if (!((Engine*)h)->SetTrafficAlpha(sort_name, target_id, alpha, &err)) { g_ph_err = err; return -1; }
    return 0;
}

int ph_set_user_fields(void* h, const char* uid, const int32_t* ids, int n) {
    if (!h || !uid || !ids || n < 0) return -1;
    ((Engine*)h)->user_fields[uid] = std::vector<int32_t>(ids, ids + n);
    return 0;
}

int ph_set_user_vector(void* h, const char* uid, const char* vec) {
    if (!h || !uid || !vec) return -1;
    ((Engine*)h)->user_vectors.vectors[uid] = vec;
    return 0;
}

// → JSON {"items":[{"item_id":..,"score":..,"retrieve_id":..,"algo_scores":{..}}]}
static const char* items_to_json(const std::vector<module::ItemPtr>& items) {
    std::string& o = g_ph_out;
    o = "{\"items\":[";
    for (size_t i = 0; i < items.size(); ++i) {
        if (i) o += ",";
        o += "{\"item_id\":";
        json::Escape(items[i]->Id, &o);
        o += ",\"score\":" + json::NumToString(items[i]->Score) + ",\"retrieve_id\":";
        json::Escape(items[i]->RetrieveId, &o);
        o += ",\"item_type\":";
        json::Escape(items[i]->ItemType, &o);
        o += ",\"algo_scores\":{";
        bool first = true;
        for (const auto& kv : items[i]->algoScores) {
            if (!first) o += ",";
            first = false;
            json::Escape(kv.first, &o);
            o += ":" + json::NumToString(kv.second);
        }
        o += "}}";
    }
    o += "]}";
    return o.c_str();
}

// one registered sort over caller-made items: [{"id":..,"score":x,"properties":{..},"algo_scores":{..}}] → ["id", …] in the sorted order
const char* ph_engine_sort(void* h, const char* sort_name, const char* items_json, int size) {
    if (!h) { g_ph_err = "ph_engine_sort: NULL engine"; return nullptr; }
    Engine* e = (Engine*)h;
    json::Value root;
    std::string err;
    const std::string text = items_json ? items_json : "";
    if (!json::Parser(text).Parse(&root, &err)) { g_ph_err = err; return nullptr; }
    auto s = e->sorts.Get(sort_name ? sort_name : "");
    if (!s) { g_ph_err = std::string("Sort:not find, name:") + (sort_name ? sort_name : ""); return nullptr; }
    sort::SortData sd;
    context::RecommendContext ctx;
    ctx.Size = size;
    sd.Context = &ctx;
    for (const auto& it : root.arr) {
        auto item = std::make_shared<module::Item>(it.s("id"));
        item->Score = it.d("score");
        item->Properties = it.at("properties").obj;
        for (const auto& kv : it.at("algo_scores").obj) item->AddAlgoScore(kv.first, kv.second.num);
        sd.Data.push_back(item);
    }
    if (!s->Sort(&sd, &err)) { g_ph_err = err; return nullptr; }
    std::string& o = g_ph_out;
    o = "[";
    for (size_t i = 0; i < sd.Data.size(); ++i) { if (i) o += ","; json::Escape(sd.Data[i]->Id, &o); }
    o += "]";
    return o.c_str();
}

// one registered sort over caller-made items, as ph_engine_sort, with the user's properties (a JSON object or NULL); the answer
// carries the scores: {"items":[{"item_id","score",…}]}
static const char* engine_sort_user(void* h, const char* sort_name, const char* items_json, const char* user_json, int size, bool with_properties) {
    if (!h) { g_ph_err = "ph_engine_sort_scored: NULL engine"; return nullptr; }
    Engine* e = (Engine*)h;
    json::Value root, uroot;
    std::string err;
    const std::string text = items_json ? items_json : "", utext = user_json ? user_json : "{}";
    if (!json::Parser(text).Parse(&root, &err) || !json::Parser(utext).Parse(&uroot, &err)) { g_ph_err = err; return nullptr; }
    auto s = e->sorts.Get(sort_name ? sort_name : "");
    if (!s) { g_ph_err = std::string("Sort:not find, name:") + (sort_name ? sort_name : ""); return nullptr; }
    sort::SortData sd;
    context::RecommendContext ctx;
    module::User user("u");
    for (const auto& kv : uroot.obj) user.Properties[kv.first] = kv.second;
    ctx.Size = size;
    sd.Context = &ctx;
    sd.User = &user;
    for (const auto& it : root.arr) {
        auto item = std::make_shared<module::Item>(it.s("id"));
        item->Score = it.d("score");
        item->RetrieveId = it.s("retrieve_id");
        item->Properties = it.at("properties").obj;
        sd.Data.push_back(item);
    }
    if (!s->Sort(&sd, &err)) { g_ph_err = err; return nullptr; }
    if (!with_properties) return items_to_json(sd.Data);
    // {"items":[{"item_id","properties":{name: number | string}}]}: what a sort that tags its items (DistinctIdSort) leaves in them
    std::string& o = g_ph_out;
    o = "{\"items\":[";
    for (size_t i = 0; i < sd.Data.size(); ++i) {
        if (i) o += ",";
        o += "{\"item_id\":";
        json::Escape(sd.Data[i]->Id, &o);
        o += ",\"properties\":{";
        bool first = true;
        for (const auto& kv : sd.Data[i]->Properties) {
            if (kv.second.type != json::Value::Number && kv.second.type != json::Value::String) continue;
            if (!first) o += ",";
            first = false;
            json::Escape(kv.first, &o);
            o += ":";
            if (kv.second.type == json::Value::String) json::Escape(kv.second.str, &o);
            else o += kv.second.is_int ? std::to_string(kv.second.i) : json::NumToString(kv.second.num);
        }
        o += "}}";
    }
    o += "]}";
    return o.c_str();
}
const char* ph_engine_sort_scored(void* h, const char* sort_name, const char* items_json, const char* user_json, int size) {
    return engine_sort_user(h, sort_name, items_json, user_json, size, false);
}
// the same call; the answer carries the items' properties instead of their scores
const char* ph_engine_sort_props(void* h, const char* sort_name, const char* items_json, const char* user_json, int size) {
    return engine_sort_user(h, sort_name, items_json, user_json, size, true);
}

// one pairec_gpu.Filters entry over caller-made items [{"id","score"}, optionally "retrieve_id" and "recall_scores" {recall: score}
// as UniqueFilter leaves them] → the kept items, in order
const char* ph_engine_filter(void* h, const char* filter_name, const char* items_json, const char* user_json) {
    if (!h) { g_ph_err = "ph_engine_filter: NULL engine"; return nullptr; }
    Engine* e = (Engine*)h;
    json::Value root, uroot;
    std::string err;
    const std::string text = items_json ? items_json : "", utext = user_json ? user_json : "{}";
    if (!json::Parser(text).Parse(&root, &err) || !json::Parser(utext).Parse(&uroot, &err)) { g_ph_err = err; return nullptr; }
    auto f = e->gpu_filters.find(filter_name ? filter_name : "");
    if (f == e->gpu_filters.end()) { g_ph_err = std::string("Filter:not find, name:") + (filter_name ? filter_name : ""); return nullptr; }
    module::User user("u");
    for (const auto& kv : uroot.obj) user.Properties[kv.first] = kv.second;
    std::vector<module::ItemPtr> items;
    for (const auto& it : root.arr) {
        auto item = std::make_shared<module::Item>(it.s("id"));
        item->Score = it.d("score");
        item->RetrieveId = it.s("retrieve_id");
        for (const auto& kv : it.at("recall_scores").obj)
            if (kv.second.type == json::Value::Number) {
                item->RecallScores[kv.first] = kv.second.num;
                item->hasRecallScores = true;
            }
        items.push_back(item);
    }
    VersionLock::Read generation_guard(e->version);
    if (!e->RunGpuFilter(f->second, &user, &items, &err)) { g_ph_err = err; return nullptr; }
    return items_to_json(items);
}

const char* ph_recommend(void* h, const char* uid, int size, const char* scene) {
    if (!h) return nullptr;
    std::vector<module::ItemPtr> items;
    std::string err;
    if (!((Engine*)h)->Recommend(uid ? uid : "", size, scene ? scene : "", &items, &err)) {
        g_ph_err = err;
        return nullptr;
    }
    return items_to_json(items);
}

// the same request with an AB experiment attached: experiment_params_json = the layer params object
const char* ph_recommend_ab(void* h, const char* uid, int size, const char* scene, const char* experiment_params_json) {
    if (!h) return nullptr;
    json::Value params;
    std::string err;
    const std::string text = experiment_params_json ? experiment_params_json : "{}";
    if (!json::Parser(text).Parse(&params, &err) || params.type != json::Value::Object) {
        g_ph_err = "experiment params: " + (err.empty() ? std::string("not a JSON object") : err);
        return nullptr;
    }
    std::vector<module::ItemPtr> items;
    if (!((Engine*)h)->Recommend(uid ? uid : "", size, scene ? scene : "", params, &items, &err)) {
        g_ph_err = err;
        return nullptr;
    }
    return items_to_json(items);
}

// n_threads threads, each serving uids[t], uids[t + n_threads], … one request at a time (pairec's goroutines): the
// engine's plug-ins are called concurrently, and with "Coalesce" configured the library batches them.  → JSON array of the
// pages in uid order
const char* ph_recommend_concurrent(void* h, const char* uids_json, int size, const char* scene, int n_threads) {
    if (!h) return nullptr;
    Engine* e = (Engine*)h;
    json::Value uids;
    std::string err;
    const std::string text = uids_json ? uids_json : "[]";
    if (!json::Parser(text).Parse(&uids, &err) || uids.type != json::Value::Array) { g_ph_err = "uids: " + err; return nullptr; }
    const size_t n = uids.arr.size();
    std::vector<std::vector<module::ItemPtr>> pages(n);
    std::vector<std::string> errs(n);
    std::vector<std::thread> th;
    const std::string sc = scene ? scene : "";
    for (int t = 0; t < n_threads; ++t)
        th.emplace_back([&, t]() {
            for (size_t i = (size_t)t; i < n; i += (size_t)n_threads)
                if (!e->Recommend(uids.arr[i].str, size, sc, &pages[i], &errs[i]) && errs[i].empty()) errs[i] = "failed";
        });
    for (auto& x : th) x.join();
    for (size_t i = 0; i < n; ++i)
        if (!errs[i].empty()) { g_ph_err = errs[i]; return nullptr; }
    std::string o = "[";
    for (size_t i = 0; i < n; ++i) {
        if (i) o += ",";
        o += items_to_json(pages[i]);
    }
    o += "]";
    g_ph_out = o;
    return g_ph_out.c_str();
}

// recall.Load's outcome for one RecallConfs entry: "built" | "panic: <text>" | "unavailable: <text>"
const char* ph_check_recall_conf(const char* conf_json) {
    recconf::RecommendConfig c;
    std::string err;
    const std::string text = std::string("{\"RecallConfs\":[") + (conf_json ? conf_json : "{}") + "]}";
    if (!recconf::RecommendConfig::Parse(text, &c, &err) || c.RecallConfs.empty()) { g_ph_err = err; return nullptr; }
    const recall::LoadOutcome o = recall::CheckRecallConf(c.RecallConfs[0]);
    g_ph_out = o.kind == recall::LoadOutcome::kBuilt ? "built" : (o.kind == recall::LoadOutcome::kPanic ? "panic: " : "unavailable: ") + o.message;
    return g_ph_out.c_str();
}

// response decoders driven by JSON (tests): {"func": name, ...inputs} → [{"score":..,"score_map":{..},"module_type":b,"classify":{..}}]
const char* ph_decode_response(const char* spec_json) {
    json::Value sp;
    std::string err;
    const std::string text = spec_json ? spec_json : "";
    if (!json::Parser(text).Parse(&sp, &err)) { g_ph_err = err; return nullptr; }
    const std::string fn = sp.s("func");
    std::vector<std::string> ids, outs;
    for (const auto& v : sp.at("item_ids").arr) ids.push_back(v.str);
    for (const auto& v : sp.at("outputs").arr) outs.push_back(v.str);
    std::map<std::string, std::vector<double>> results;
    for (const auto& kv : sp.at("results").obj) for (const auto& x : kv.second.arr) results[kv.first].push_back(x.num);
    std::vector<algorithm::AlgoResponse> ret;
    if (fn == "easyrecResponseFunc") ret = algorithm::decode::EasyrecResponse(ids, results);
    else if (fn == "easyrecMutValResponseFunc") {
        if (!algorithm::decode::EasyrecMutValResponse(ids, outs, results, &ret, &err)) { g_ph_err = err; return nullptr; }
    } else if (fn == "easyrecMutClassificationResponseFunc") {
        std::map<std::string, std::pair<std::vector<float>, std::vector<long long>>> tf;
        for (const auto& kv : sp.at("tf_outputs").obj) {
            auto& dst = tf[kv.first];
            for (const auto& x : kv.second.at("float_val").arr) dst.first.push_back((float)x.num);
            for (const auto& x : kv.second.at("shape").arr) dst.second.push_back((long long)x.num);
        }
        if (!algorithm::decode::EasyrecMutClassificationResponse(ids, tf, &ret, &err)) { g_ph_err = err; return nullptr; }
    } else if (fn == "alinkFMResponseFunc") {
        for (const auto& v : sp.at("predictions").arr)
            ret.emplace_back(algorithm::decode::AlinkFMScore(v.d("prediction_result"), v.d("prediction_score")));
    } else if (fn == "tfservingResponseFunc") {
        std::vector<std::vector<double>> o2;
        for (const auto& row : sp.at("tf_rows").arr) { o2.emplace_back(); for (const auto& x : row.arr) o2.back().push_back(x.num); }
        ret = algorithm::decode::TFServingResponse(o2);
    } else if (fn == "tfResponseFunc" || fn == "tfMutValResponseFunc" || fn == "torchrecMutValResponseFunc" ||
               fn == "torchrecMutValResponseFuncDebug" || fn == "torchrecMutClassificationResponseFunc" ||
               fn == "torchrecMutClassificationResponseFuncDebug" || fn == "torchrecEmbeddingItemsResponseFunc") {
        // "outputs_list": [{"name":…, "dtype": "float"|"double", "values": […], "shape": […]}] in the message's order
        std::vector<std::pair<std::string, algorithm::decode::OutputArray>> outsl;
        for (const auto& ov : sp.at("outputs_list").arr) {
            algorithm::decode::OutputArray oa;
            oa.is_double = ov.s("dtype") == "double";
            for (const auto& x : ov.at("values").arr) { if (oa.is_double) oa.double_val.push_back(x.num); else oa.float_val.push_back((float)x.num); }
            for (const auto& x : ov.at("shape").arr) oa.shape.push_back((long long)x.num);
            outsl.emplace_back(ov.s("name"), std::move(oa));
        }
        bool ok = true;
        if (fn == "tfResponseFunc") ret = algorithm::decode::TfResponse(outsl);
        else if (fn == "tfMutValResponseFunc") ret = algorithm::decode::TfMutValResponse(outsl);
        else if (fn.rfind("torchrecMutVal", 0) == 0) ok = algorithm::decode::TorchrecMutValResponse(ids.size(), outsl, &ret, &err);
        else if (fn.rfind("torchrecMutClassification", 0) == 0) ok = algorithm::decode::TorchrecMutClassificationResponse(ids.size(), outsl, &ret, &err);
        else {
            const algorithm::decode::OutputArray* sc = nullptr;
            for (const auto& kv : outsl) if (kv.first == "match_item_scores") sc = &kv.second;
            std::vector<algorithm::EmbeddingInfo> items;
            ok = algorithm::decode::TorchrecEmbeddingItemsResponse(ids, sc, &items, &err);
            std::string o = "[";
            for (size_t i = 0; ok && i < items.size(); ++i) {
                if (i) o += ",";
                o += "{\"item_id\":";
                json::Escape(items[i].ItemId, &o);
                char buf[64];
                snprintf(buf, sizeof buf, ",\"score\":%.17g}", items[i].Score);
                o += buf;
            }
            o += "]";
            if (!ok) { g_ph_err = err; return nullptr; }
            g_ph_out = o;
            return g_ph_out.c_str();
        }
        if (!ok) { g_ph_err = err; return nullptr; }
    } else if (fn == "easyrecResponseFuncDebug") {
        ret = algorithm::decode::EasyrecResponse(ids, results);                    // (:237-268: the same scores + the debug strings)
    } else if (fn == "easyrecMutValResponseFuncDebug") {
        if (!algorithm::decode::EasyrecMutValResponse(ids, outs, results, &ret, &err)) { g_ph_err = err; return nullptr; }
    } else if (fn == "pssmartResponseFunc") {
        for (const auto& v : sp.at("predictions").arr)
            ret.emplace_back(algorithm::decode::PssmartScore(v.d("score"), v.s("lable"), v.s("label")));
    } else if (fn == "widenF32") {
        std::vector<float> f;
        for (const auto& x : sp.at("float_val").arr) f.push_back((float)x.num);
        ret = algorithm::decode::WidenF32(f.data(), f.size());
    } else { g_ph_err = "unknown decoder " + fn; return nullptr; }
    std::string o = "[";
    for (size_t i = 0; i < ret.size(); ++i) {
        if (i) o += ",";
        o += "{\"score\":" + json::NumToString(ret[i].GetScore()) + ",\"module_type\":" + (ret[i].GetModuleType() ? "true" : "false") + ",\"score_map\":{";
        bool first = true;
        for (const auto& kv : ret[i].GetScoreMap()) {
            if (!first) o += ",";
            first = false;
            json::Escape(kv.first, &o);
            o += ":" + json::NumToString(kv.second);
        }
        o += "},\"classify\":{";
        first = true;
        for (const auto& kv : ret[i].GetClassifyMap()) {
            if (!first) o += ",";
            first = false;
            json::Escape(kv.first, &o);
            o += ":[";
            for (size_t c = 0; c < kv.second.size(); ++c) o += (c ? "," : "") + json::NumToString(kv.second[c]);
            o += "]";
        }
        o += "}}";
    }
    o += "]";
    g_ph_out = o;
    return g_ph_out.c_str();
}

// fmt %v of a float64
const char* ph_go_fmt_float(double x) {
    g_ph_out = GoFmtFloat(x);
    return g_ph_out.c_str();
}

// recall result cache line: items JSON [{"id":..,"score":..}] → "id:name:score,…"
const char* ph_format_recall_cache(const char* items_json, const char* recall_name) {
    json::Value root;
    std::string err;
    const std::string text = items_json ? items_json : "";
    if (!json::Parser(text).Parse(&root, &err) || root.type != json::Value::Array) { g_ph_err = "items: " + err; return nullptr; }
    std::vector<module::ItemPtr> items;
    for (const auto& v : root.arr) {
        auto it = std::make_shared<module::Item>(v.s("id"));
        it->Score = v.d("score");
        items.push_back(it);
    }
    g_ph_out = recall::FormatCacheString(items, recall_name ? recall_name : "");
    return g_ph_out.c_str();
}

// … and back: "id:name:score,…" → items JSON; NULL (+ ph_last_error) where the reference would panic
const char* ph_parse_recall_cache(const char* line, const char* recall_name, const char* item_type) {
    std::vector<module::ItemPtr> items;
    std::string err;
    if (!recall::ParseCacheString(line ? line : "", recall_name ? recall_name : "", item_type ? item_type : "", &items, &err)) {
        g_ph_err = err;
        return nullptr;
    }
    return items_to_json(items);
}

// EasyrecAlgoDataGenerator driver: {"context_features":[names],"item_features":[names]|null,
// "user":{..},"items":[{"id":..,"features":{..}}], "batches": [n1, n2, ...]} → [request JSON per batch]
const char* ph_easyrec_generator(const char* spec_json) {
    json::Value root;
    std::string err;
    const std::string text = spec_json ? spec_json : "";
    if (!json::Parser(text).Parse(&root, &err)) { g_ph_err = err; return nullptr; }
    std::vector<std::string> ctxf, inf;
    for (const auto& v : root.at("context_features").arr) ctxf.push_back(v.str);
    rank::EasyrecAlgoDataGenerator g(ctxf);
    if (root.at("item_features").type == json::Value::Array) {
        for (const auto& v : root.at("item_features").arr) inf.push_back(v.str);
        g.SetItemFeatures(inf);
    }
    std::map<std::string, json::Value> user(root.at("user").obj.begin(), root.at("user").obj.end());
    std::string& o = g_ph_out;
    o = "[";
    size_t pos = 0;
    bool first = true;
    for (const auto& b : root.at("batches").arr) {
        for (long long k = 0; k < (long long)b.num && pos < root.at("items").arr.size(); ++k, ++pos) {
            const json::Value& it = root.at("items").arr[pos];
            std::map<std::string, json::Value> feats(it.at("features").obj.begin(), it.at("features").obj.end());
            g.AddFeatures(std::make_shared<module::Item>(it.s("id")), feats, user);
        }
        if (!first) o += ",";
        first = false;
        o += g.GeneratorAlgoData();
    }
    o += "]";
    return o.c_str();
}

// ---- service/feature drivers -------------------------------------------------------------------------------------
static void dyn_json(const json::Value& v, std::string* o) {        // floats keep a '.', so a reader can tell float64 10 from int 10
    switch (v.type) {
        case json::Value::String: json::Escape(v.str, o); break;
        case json::Value::Bool: *o += v.b ? "true" : "false"; break;
        case json::Value::Number:
            if (v.is_u64) *o += std::to_string((unsigned long long)v.i);
            else if (v.is_int) *o += std::to_string(v.i);
            else if (v.num != v.num || std::isinf(v.num)) *o += "null";
            else {
                std::string t = json::NumToString(v.num);
                if (t.find_first_of(".eEn") == std::string::npos) t += ".0";
                *o += t;
            }
            break;
        case json::Value::Array:
            *o += "[";
            for (size_t i = 0; i < v.arr.size(); ++i) { if (i) *o += ","; dyn_json(v.arr[i], o); }
            *o += "]";
            break;
        case json::Value::Object: {
            *o += "{";
            bool first = true;
            for (const auto& kv : v.obj) { if (!first) *o += ","; first = false; json::Escape(kv.first, o); *o += ":"; dyn_json(kv.second, o); }
            *o += "}";
            break;
        }
        default: *o += "null";
    }
}
static const char* go_type_of(const json::Value& v) {
    switch (v.type) {
        case json::Value::String: return "string";
        case json::Value::Bool: return "bool";
        case json::Value::Number: return v.is_u64 ? "uint64" : (v.is_int ? "int" : "float64");
        case json::Value::Array: return "slice";
        case json::Value::Object: return "map";
        default: return "nil";
    }
}
// NewNormalizer(name, expression).Apply(value): {"name":..,"expression":..,"value":..,"clock_ms":n?} →
// {"kind": Go type of the normalizer | null, "result": .., "type": Go type of the result}; an expression outside the subset → NULL + error
const char* ph_normalizer_apply(const char* spec_json) {
    json::Value root;
    std::string err;
    const std::string text = spec_json ? spec_json : "";
    if (!json::Parser(text).Parse(&root, &err)) { g_ph_err = err; return nullptr; }
    feature::SetClockForTest(root.n("clock_ms", 0));
    auto nz = feature::NewNormalizer(root.s("name"), root.s("expression"), &err);
    if (!nz && !err.empty()) { g_ph_err = err; return nullptr; }
    std::string& o = g_ph_out;
    if (!nz) { o = "{\"kind\":null}"; return o.c_str(); }
    const json::Value r = nz->Apply(root.at("value"));
    o = std::string("{\"kind\":\"") + nz->Kind() + "\",\"type\":\"" + go_type_of(r) + "\",\"result\":";
    dyn_json(r, &o);
    o += "}";
    return o.c_str();
}
// Feature.LoadFeatures: {"features":[FeatureConfig…], "user":{"id":..,"properties":{..}}|null,
// "items":[{"id":..,"retrieve_id":..,"properties":{..}}], "context_features":{..}?, "clock_ms":n?} → {"user":{..}|null,"items":[{..}]}
const char* ph_feature_load(const char* spec_json) {
    json::Value root;
    std::string err;
    const std::string text = spec_json ? spec_json : "";
    if (!json::Parser(text).Parse(&root, &err)) { g_ph_err = err; return nullptr; }
    feature::SetClockForTest(root.n("clock_ms", 0));
    std::vector<feature::FeatureConfig> confs;
    for (const auto& f : root.at("features").arr) {
        feature::FeatureConfig c;
        c.FeatureType = f.s("FeatureType"); c.FeatureName = f.s("FeatureName"); c.FeatureSource = f.s("FeatureSource");
        c.FeatureValue = f.s("FeatureValue"); c.FeatureStore = f.s("FeatureStore"); c.Normalizer = f.s("Normalizer");
        c.Expression = f.s("Expression");
        c.RemoveFeatureSource = f.at("RemoveFeatureSource").type == json::Value::Bool && f.at("RemoveFeatureSource").b;
        confs.push_back(std::move(c));
    }
    feature::Feature feat;
    if (!feat.LoadWithConfig(confs, &err)) { g_ph_err = err; return nullptr; }
    std::unique_ptr<module::User> user;
    if (root.at("user").type == json::Value::Object) {
        user.reset(new module::User(root.at("user").s("id")));
        user->Properties = root.at("user").at("properties").obj;
    }
    std::vector<module::ItemPtr> items;
    for (const auto& it : root.at("items").arr) {
        auto item = std::make_shared<module::Item>(it.s("id"));
        item->RetrieveId = it.s("retrieve_id");
        item->Properties = it.at("properties").obj;
        items.push_back(item);
    }
    context::RecommendContext ctx;
    if (root.at("context_features").type == json::Value::Object) ctx.Param["features"] = root.at("context_features");
    feat.LoadFeatures(user.get(), items, &ctx);
    std::string& o = g_ph_out;
    o = "{\"user\":";
    if (user) { json::Value u; u.type = json::Value::Object; u.obj = user->Properties; dyn_json(u, &o); } else o += "null";
    o += ",\"items\":[";
    for (size_t i = 0; i < items.size(); ++i) {
        if (i) o += ",";
        json::Value p; p.type = json::Value::Object; p.obj = items[i]->Properties;
        dyn_json(p, &o);
    }
    o += "]}";
    return o.c_str();
}

// cache adapters + clone hooks, self-checked in C++ (bit i set = check i passed)
int ph_cache_clone_semantics(void) {
    int ok = 0;
    std::string err;
    auto lc = cache::NewCache("localCache", "", &err);
    auto bc = cache::NewCache("localBytes", "", &err);
    if (lc && bc && !cache::NewCache("memcached", "", &err) && err == "Cache:not found instance, name:memcached") ok |= 1;
    if (lc && bc) {
        lc->Put("k", "a:r:1", 1800);
        bc->Put("k", "a:r:1", 1800);
        // localCache hands back a string (VectorRecall's []uint8 assertion misses), the byte store hits
        if (lc->Get("k").kind == cache::Value::kString && bc->Get("k").kind == cache::Value::kBytes) ok |= 2;
        if (bc->Get("absent").kind == cache::Value::kNone) ok |= 4;
        bc->Put("gone", "x", 0 + 1);
    }
    // ICloneSort: the hook swaps in the clone only when the experiment carries a "sort.<name>" object
    struct Rev : sort::ISort, sort::ICloneSort {
        bool reversed;
        explicit Rev(bool r) : reversed(r) {}
        bool Sort(sort::SortData* d, std::string*) override {
            if (reversed) std::reverse(d->Data.begin(), d->Data.end());
            return true;
        }
        std::shared_ptr<sort::ISort> CloneWithConfig(const json::Value& p) override {
            return std::make_shared<Rev>(p.at("reverse").type == json::Value::Bool && p.at("reverse").b);
        }
        std::string GetSortName() const override { return "rev"; }
    };
    {
        auto base = std::make_shared<Rev>(false);
        json::Value params;
        const std::string ptext = "{\"sort.rev\":{\"reverse\":true}}";     // (Parser keeps a reference)
        json::Parser(ptext).Parse(&params, &err);
        std::shared_ptr<sort::ISort> s = base;
        if (auto* cs = dynamic_cast<sort::ICloneSort*>(s.get())) {
            const json::Value& sc = params.at("sort." + cs->GetSortName());
            if (sc.type == json::Value::Object)
                if (auto c = cs->CloneWithConfig(sc)) s = c;
        }
        sort::SortData d;
        d.Data = {std::make_shared<module::Item>("a"), std::make_shared<module::Item>("b")};
        s->Sort(&d, &err);
        if (d.Data[0]->Id == "b" && s != base) ok |= 8;
    }
    return ok;
}

// host-only helpers (no GPU): used by the CPU tests of the mirror
int ph_parse_vector_string(const char* s, float* out, int cap) {
    const auto v = recall::ParseVectorString(s ? s : "");
    for (int i = 0; i < (int)v.size() && i < cap; ++i) out[i] = v[i];
    return (int)v.size();
}

// in: JSON [{"id":..,"score":..,"retrieve_id":..,"algo_scores":{..}}] → UniqueFilter → same shape + recall_scores
const char* ph_unique_filter(const char* items_json) {
    json::Value root;
    std::string err;
    if (!json::Parser(items_json ? items_json : "").Parse(&root, &err)) { g_ph_err = err; return nullptr; }
    std::vector<module::ItemPtr> items;
    for (const auto& v : root.arr) {
        auto it = std::make_shared<module::Item>(v.s("id"));
        it->Score = v.d("score");
        it->RetrieveId = v.s("retrieve_id");
        for (const auto& kv : v.at("algo_scores").obj) it->AddAlgoScore(kv.first, kv.second.num);
        items.push_back(it);
    }
    const auto out = filter::UniqueFilter(items);
    std::string& o = g_ph_out;
    o = "[";
    for (size_t i = 0; i < out.size(); ++i) {
        if (i) o += ",";
        o += "{\"id\":";
        json::Escape(out[i]->Id, &o);
        o += ",\"score\":" + json::NumToString(out[i]->Score) + ",\"algo_scores\":{";
        bool first = true;
        for (const auto& kv : out[i]->algoScores) {
            if (!first) o += ",";
            first = false;
            json::Escape(kv.first, &o);
            o += ":" + json::NumToString(kv.second);
        }
        o += "},\"recall_scores\":{";
        first = true;
        for (const auto& kv : out[i]->RecallScores) {
            if (!first) o += ",";
            first = false;
            json::Escape(kv.first, &o);
            o += ":" + json::NumToString(kv.second);
        }
        o += "}}";
    }
    o += "]";
    return o.c_str();
}

// registry semantics: returns a bitmask of checks that hold (all 5 bits set = 31)
int ph_registry_semantics(void) {
    struct DummySort : sort::ISort { int id; explicit DummySort(int i) : id(i) {} bool Sort(sort::SortData*, std::string*) override { return true; } };
    struct DummyAlgo : algorithm::IAlgorithm {
        double v; explicit DummyAlgo(double x) : v(x) {}
        bool Init(const recconf::AlgoConfig&, std::string*) override { return true; }
        bool Run(const algorithm::AlgoData&, algorithm::AlgoResult* out, std::string*) override { out->responses.assign(1, algorithm::AlgoResponse(v)); return true; }
    };
    int ok = 0;
    sort::Registry sr;
    std::string err;
    auto s1 = std::make_shared<DummySort>(1), s2 = std::make_shared<DummySort>(2);
    sr.RegisterSort("x", s1, &err);
    sr.RegisterSort("x", s2, &err);
    if (sr.Get("x") == s1) ok |= 1;                                   // first registration wins
    if (!sr.RegisterSort("nil", nullptr, &err)) ok |= 2;              // nil rejected (reference panics)
    algorithm::AlgorithmFactory f;
    f.RegisterAlgorithm("a", std::make_shared<DummyAlgo>(1.0));
    f.RegisterAlgorithm("a", std::make_shared<DummyAlgo>(2.0));
    algorithm::AlgoResult res;
    if (f.Run("a", algorithm::AlgoData{}, &res, &err) && res.responses[0].GetScore() == 2.0) ok |= 4;   // overwrite
    if (!f.Run("missing", algorithm::AlgoData{}, &res, &err) && err.find("not find algorithm") != std::string::npos) ok |= 8;
    recall::Registry rr;
    if (!rr.GetRecall("nope", &err)) ok |= 16;
    return ok;
}

// parse a recconf JSON and echo the subset the engine honours (for config tests)
const char* ph_parse_recconf(const char* text) {
    recconf::RecommendConfig c;
    std::string err;
    if (!recconf::RecommendConfig::Parse(text ? text : "", &c, &err)) { g_ph_err = err; return nullptr; }
    std::string& o = g_ph_out;
    o = "{\"recalls\":" + std::to_string(c.RecallConfs.size()) + ",\"gpu_recalls\":" + std::to_string(c.GpuRecalls.size()) +
        ",\"gpu_sorts\":" + std::to_string(c.GpuSorts.size()) + ",\"algos\":" + std::to_string(c.AlgoConfs.size()) +
        ",\"rank_scenes\":" + std::to_string(c.RankConf.size()) + ",\"dpp\":" + std::to_string(c.DPPConf.size());
    auto count_features = [](const std::map<std::string, recconf::SceneFeatureConfig>& m) {
        size_t n = 0;
        for (const auto& sc : m) for (const auto& lc : sc.second.FeatureLoadConfs) n += lc.Features.size();
        return n;
    };
    if (!c.FeatureConfs.empty() || !c.UserFeatureConfs.empty())
        o += ",\"feature_transforms\":" + std::to_string(count_features(c.FeatureConfs)) + ",\"user_feature_transforms\":" +
             std::to_string(count_features(c.UserFeatureConfs));
    auto echo = [&](const char* key, const recconf::RecallConfig& r) {
        o += std::string(",\"") + key + "\":{\"name\":";
        json::Escape(r.Name, &o);
        o += ",\"count\":" + std::to_string(r.RecallCount) + ",\"algo\":";
        json::Escape(r.RecallAlgo, &o);
        o += "}";
    };
    if (!c.RecallConfs.empty()) echo("recall0", c.RecallConfs[0]);
    if (!c.GpuRecalls.empty()) echo("gpu_recall0", c.GpuRecalls[0]);
    for (const auto& kv : c.RankConf) {
        o += ",\"rank_" + kv.first + "\":{\"batch\":" + std::to_string(kv.second.BatchCount) + ",\"score\":";
        json::Escape(kv.second.RankScore, &o);
        o += ",\"algos\":" + std::to_string(kv.second.RankAlgoList.size()) + ",\"score_rewrite\":{";
        bool first = true;
        for (const auto& rw : kv.second.ScoreRewrite) {
            if (!first) o += ",";
            first = false;
            json::Escape(rw.first, &o);
            o += ":";
            json::Escape(rw.second, &o);
        }
        o += "}}";
    }
    o += "}";
    return o.c_str();
}

}  // extern "C"
