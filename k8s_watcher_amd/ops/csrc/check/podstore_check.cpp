// podstore_check — the pod cache's store (../podstore.inc: PodStore with its
// per-namespace and per-timer-kind intrusive lists, store_take_due, store_put)
// as a stand-alone program, for a run under -fsanitize=address,undefined
// (scripts/podstore_check.sh). No Python.
//
//   podstore_check [STEPS] [SEED]
//
// A seeded random sequence of STEPS operations (default 5000) over a few dozen
// uids and four namespace ids: emplace, erase (by key and by iterator),
// set_ns, set_timer of every kind with and without a value (by iterator and
// by entry), keeping a core and then clearing a timer of a kind that keeps
// cores (the pending or the unready one: the core goes unless the other such
// kind's timer stands), the line that moves a pod from the one kind to the
// other (clear, set, keep), a send's core,
// a whole-entry replace (store_put), clear, and store_take_due. After every
// step the store is compared with a plain std::map model: for each timer kind
// timed() is the model's count and for_each_timed visits exactly the model's
// set, each entry once, with the model's time and mark; for each namespace id
// count() and for_each_in agree with the model; every entry's core and kept
// mark are the model's. A take returns exactly the entries the model expects,
// marks them, and the same take again returns none.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <memory>
#include <random>
#include <string>
#include <string_view>
#include <unordered_map>
#include <vector>

namespace {

#include "../podstore.inc"

constexpr uint32_t N_NS = 4;
constexpr int N_UIDS = 40;
const int64_t TIMES[] = {0, INT64_MIN, INT64_MAX, 100, -1, 1000};

struct Model {
    uint32_t ns = 0;
    bool has_core = false, kept = false;
    bool timed[N_TIMER] = {}, reported[N_TIMER] = {};
    int64_t at[N_TIMER] = {};
};
using ModelMap = std::map<std::string, Model>;

long g_step = 0;

[[noreturn]] void fail(const char* what, const std::string& uid = std::string()) {
    std::fprintf(stderr, "podstore_check: step %ld: %s %s\n", g_step, what, uid.c_str());
    std::exit(1);
}

void model_set_timer(Model& m, int k, bool has, int64_t at) {
    if (has) {
        m.timed[k] = true;
        m.at[k] = at;
        return;
    }
    m.timed[k] = m.reported[k] = false;
    // a kind that keeps cores: the kept core goes with it, unless the other such kind's timer holds it
    if ((k == TIMER_PENDING || k == TIMER_UNREADY) && m.kept && !m.timed[TIMER_PENDING] && !m.timed[TIMER_UNREADY])
        m.kept = m.has_core = false;
}

bool model_due(const Model& m, int k, int64_t now_s, int64_t after_s, bool scoped, uint32_t ns) {
    return m.timed[k] && !m.reported[k] && m.has_core && (!scoped || m.ns == ns) &&
           (__int128)now_s - (__int128)m.at[k] >= (__int128)after_s;
}

std::vector<std::string> sorted_keys(const std::vector<const CacheEntry*>& seen) {
    std::vector<std::string> keys;
    for (const CacheEntry* e : seen) keys.push_back(*e->key);
    std::sort(keys.begin(), keys.end());
    if (std::adjacent_find(keys.begin(), keys.end()) != keys.end()) fail("an entry visited twice");
    return keys;
}

void check(PodStore& st, const ModelMap& model) {
    if (st.size() != model.size()) fail("size");
    for (const auto& [uid, m] : model) {
        auto it = st.find(uid);
        if (it == st.end()) fail("entry missing", uid);
        const CacheEntry& e = it->second;
        if (*e.key != uid || e.ns_id != m.ns) fail("key or namespace", uid);
        if ((bool)e.core != m.has_core || e.core_kept != m.kept) fail("core", uid);
        for (int k = 0; k < N_TIMER; ++k)
            if (e.timed[k] != m.timed[k] || e.reported[k] != m.reported[k] || (m.timed[k] && e.timer[k].at != m.at[k]))
                fail("timer", uid);
    }
    for (int k = 0; k < N_TIMER; ++k) {
        std::vector<std::string> want;
        for (const auto& [uid, m] : model)
            if (m.timed[k]) want.push_back(uid);
        if (st.timed((TimerKind)k) != want.size()) fail("timed()");
        std::vector<const CacheEntry*> seen;
        st.for_each_timed((TimerKind)k, [&](CacheEntry& e) { seen.push_back(&e); });
        if (sorted_keys(seen) != want) fail("for_each_timed");
    }
    for (uint32_t ns = 0; ns < N_NS + 1; ++ns) {  // (+1: an id no entry ever had)
        std::vector<std::string> want;
        for (const auto& [uid, m] : model)
            if (m.ns == ns) want.push_back(uid);
        if (st.count(ns) != want.size()) fail("count(ns)");
        if ((st.any_in(ns) != nullptr) != !want.empty()) fail("any_in");
        std::vector<const CacheEntry*> seen;
        st.for_each_in(ns, [&](CacheEntry& e) { seen.push_back(&e); });
        if (sorted_keys(seen) != want) fail("for_each_in");
    }
}

}  // namespace

int main(int argc, char** argv) {
    const long steps = argc > 1 ? std::atol(argv[1]) : 5000;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 20261021);
    auto pick = [&](uint64_t n) { return (uint32_t)(rng() % n); };
    PodStore st;
    ModelMap model;
    long taken = 0, replaced = 0;
    for (g_step = 0; g_step < steps; ++g_step) {
        const std::string uid = "uid-" + std::to_string(pick(N_UIDS));
        const uint32_t ns = pick(N_NS);
        const int k = (int)pick(N_TIMER);
        const int64_t at = TIMES[pick(sizeof TIMES / sizeof *TIMES)];
        auto it = st.find(uid);
        auto mit = model.find(uid);
        if ((it == st.end()) != (mit == model.end())) fail("find", uid);
        const bool known = it != st.end();
        switch (pick(12)) {
            case 0:
            case 1: {  // emplace: an entry already there keeps its namespace
                bool inserted;
                CacheEntry& e = st.emplace(uid, ns, inserted);
                if (inserted == known || *e.key != uid) fail("emplace", uid);
                if (inserted) model[uid].ns = ns;
                break;
            }
            case 2:  // erase, by key or by iterator
                if (pick(2)) {
                    if (st.erase(uid) != known) fail("erase", uid);
                } else if (known) {
                    st.erase(it);
                }
                model.erase(uid);
                break;
            case 3:
                if (!known) break;
                st.set_ns(it->second, ns);
                mit->second.ns = ns;
                break;
            case 4:
            case 5:
            case 6: {  // a timer of any kind, with or without a value, through both overloads
                if (!known) break;
                const bool has = pick(3) != 0;
                if (pick(2)) st.set_timer((TimerKind)k, it, has, at);
                else st.set_timer((TimerKind)k, it->second, has, at);
                model_set_timer(mit->second, k, has, at);
                break;
            }
            case 7: {  // the core of an unsent Pending or unready line, kept; sometimes that timer goes right away
                if (!known) break;
                it->second.core = std::make_shared<const std::string>("{\"kept\":1}");
                it->second.core_kept = true;
                mit->second.has_core = mit->second.kept = true;
                const TimerKind keeper = pick(2) ? TIMER_PENDING : TIMER_UNREADY;
                const TimerKind other = keeper == TIMER_PENDING ? TIMER_UNREADY : TIMER_PENDING;
                switch (pick(3)) {
                    case 0: {
                        const bool held = it->second.timed[other];
                        st.set_timer(keeper, it->second, false, 0);
                        model_set_timer(mit->second, keeper, false, 0);
                        if ((bool)it->second.core != held) fail("a kept core and the timers that keep it", uid);
                        break;
                    }
                    case 1:  // the line that moves the pod to the other kind: clear, set, keep
                        st.set_timer(other, it, false, 0);
                        model_set_timer(mit->second, other, false, 0);
                        st.set_timer(keeper, it, false, 0);
                        model_set_timer(mit->second, keeper, false, 0);
                        if (it->second.core || it->second.core_kept) fail("the old kept core outlived both timers", uid);
                        st.set_timer(other, it, true, at);
                        model_set_timer(mit->second, other, true, at);
                        it->second.core = std::make_shared<const std::string>("{\"kept\":2}");
                        it->second.core_kept = true;
                        mit->second.has_core = mit->second.kept = true;
                        break;
                    default:
                        break;
                }
                break;
            }
            case 8:  // a send's core
                if (!known) break;
                it->second.core = std::make_shared<const std::string>("{\"sent\":1}");
                it->second.core_kept = false;
                mit->second.has_core = true;
                mit->second.kept = false;
                break;
            case 9: {  // a whole-entry replace: nothing of the old entry's alert state stays
                CacheEntry e;
                e.ns_id = ns;
                e.rv = std::to_string(g_step);
                if (pick(2)) e.core = std::make_shared<const std::string>("{\"put\":1}");
                const bool has_core = (bool)e.core;
                if (known) it->second.sig[pick(N_SIG)] = rng();
                store_put(st, uid, std::move(e));
                Model m;
                m.ns = ns;
                m.has_core = has_core;
                model[uid] = m;
                for (uint64_t s : st.find(uid)->second.sig)
                    if (s) fail("a signature outlived store_put", uid);
                ++replaced;
                break;
            }
            case 10:
                if (pick(40)) break;  // rare: the sequence is about a populated store
                st.clear();
                model.clear();
                break;
            default: {  // a sweep: exactly the model's due entries, each marked, none of them twice
                const int64_t now_s = TIMES[pick(sizeof TIMES / sizeof *TIMES)];
                const bool scoped = pick(2);
                std::vector<std::string> want;
                for (auto& [u, m] : model)
                    if (model_due(m, k, now_s, at, scoped, ns)) {
                        want.push_back(u);
                        m.reported[k] = true;
                    }
                std::vector<CacheEntry*> due;
                store_take_due(st, (TimerKind)k, now_s, at, scoped, ns, due);
                for (const CacheEntry* e : due)
                    if (!e->reported[k] || !e->core) fail("taken but not marked", *e->key);
                if (sorted_keys({due.begin(), due.end()}) != want) fail("store_take_due");
                taken += (long)due.size();
                due.clear();
                store_take_due(st, (TimerKind)k, now_s, at, scoped, ns, due);
                if (!due.empty()) fail("taken twice", *due[0]->key);
                break;
            }
        }
        check(st, model);
    }
    // a sequence that never took or replaced anything checked little
    if (steps >= 1000 && (taken < 20 || replaced < 20)) fail("the sequence took or replaced too little");
    std::printf("podstore_check: %ld steps, %ld entries taken, %ld replaced, %zu left\n", steps, taken, replaced,
                st.size());
    return 0;
}
