// prefilter_check — decode_line with the payload pre-filter (../engine.inc:
// payload_prefiltered, NsTextSet, DecodeCfg) as a stand-alone program, for a run
// under -fsanitize=address,undefined or -fsanitize=thread
// (scripts/prefilter_check.sh). The whole extension is compiled in, so it
// links what _kwcore links, but the interpreter is never started: decode
// touches no Python object.
//
//   prefilter_check LINES.ndjson SHARD_COUNT SHARD_INDEX BY_UID [NAMESPACE...]
//
// Every line is copied into a heap block of its exact size (an overread is
// seen) and decoded, the pre-filter on and off, by THREADS threads at once
// that share one DecodeCfg and one namespace set — the state decode workers
// share in the watcher. Each thread checks every line:
//   * on: a line is marked exactly when the rule written out again here says
//     so, and then has no core and no payload error;
//   * off (the payload half called again with the pre-filter off, as
//     line_core calls it): no line stays marked, and a line that was marked
//     gets its core or its payload error;
//   * everything else of the job is the same on and off.
// Then the module switch is turned off and the threads decode again: nothing
// is marked and every core is the one "off" built.
//   * the terminating signature (watcher.alerts.terminating is on) is the
//     pod's, marked or not, and the same on and off.
// stdout: one row per line, "tidx pre_dropped has_core(on) has_core(off)".

#include "../kwcore.cpp"

namespace {

struct Row {
    int tidx;
    bool pre, core_on, core_off;
    bool operator==(const Row& o) const {
        return tidx == o.tidx && pre == o.pre && core_on == o.core_on && core_off == o.core_off;
    }
};

// the rule, from the issue's words and not from payload_prefiltered's code
bool rule_drops(const DecodeCfg& C, const PodSpans& S) {
    auto plain = [](const Span& s) { return s.is_string() && !std::memchr(s.p, '\\', s.n); };
    auto text = [](const Span& s) { return std::string(s.p + 1, s.n - 2); };
    if (C.ns_texts && plain(S.ns) && !C.ns_texts->texts.count(text(S.ns))) return true;
    if (C.shard_count > 1) {
        const Span& k = C.shard_by_uid ? S.uid : S.ns;
        if (k.is_string() && !plain(k)) return false;
        const std::string key = k.is_string() ? text(k) : std::string();
        const uint32_t crc = (uint32_t)::crc32(0L, reinterpret_cast<const Bytef*>(key.data()), (uInt)key.size());
        return (int)(crc % (uint32_t)C.shard_count) != C.shard_index;
    }
    return false;
}

int check_lines(const DecodeCfg& C, const std::vector<std::unique_ptr<char[]>>& bufs, const std::vector<size_t>& sizes,
                std::vector<Row>& rows) {
    int bad = 0;
    LineJob on, off;
    for (size_t i = 0; i < bufs.size(); ++i) {
        for (LineJob* J : {&on, &off}) {
            J->p = bufs[i].get();
            J->n = sizes[i];
            J->bare = false;
            J->stage = JOB_FULL;
        }
        decode_line(C, on);
        // off: what line_core does for a pre-dropped line the apply wants after
        // all — the payload half again with the pre-filter off
        decode_line_impl(C, off);
        if (off.pre_dropped) decode_payload(C, off, false);
        const bool kept = on.has_core || on.payload_err || on.repr_fallback || on.pre_dropped;
        const bool want = g_payload_prefilter && kept && rule_drops(C, on.S);
        auto fail = [&](const char* what) {
            std::fprintf(stderr, "line %zu: %s\n", i, what);
            ++bad;
        };
        if (off.pre_dropped) fail("still marked pre-dropped after the payload half ran with the pre-filter off");
        if (!g_payload_prefilter && (on.pre_dropped || on.has_core != off.has_core))
            fail("the module switch is off, yet decode_line pre-filtered");
        if (on.pre_dropped != want) fail(want ? "not pre-dropped though the rule drops it" : "pre-dropped against the rule");
        if (on.pre_dropped != on.hot.pre_dropped) fail("hot.pre_dropped differs from the job's");
        if (on.pre_dropped && (on.has_core || on.payload_err || on.repr_fallback)) fail("pre-dropped, yet something built");
        if (on.pre_dropped && !(off.has_core || off.payload_err || off.repr_fallback)) fail("pre-dropped a line nothing is built for");
        if (!on.pre_dropped && (on.has_core != off.has_core || (on.has_core && on.core != off.core) ||
                                (on.payload_err == nullptr) != (off.payload_err == nullptr)))
            fail("payload differs between on and off");
        if (on.tidx != off.tidx || (on.err == nullptr) != (off.err == nullptr) || on.fail_sig != off.fail_sig ||
            on.cond_sig != off.cond_sig || on.term_sig != off.term_sig || on.hot.term_cand != (on.term_sig != 0))
            fail("fields differ between on and off");
        // the terminating signature is computed before the pre-filter: a marked line has it all the same
        const bool live = on.tidx == T_ADDED || on.tidx == T_MODIFIED;
        if (!on.err && live && on.obj_span.present() && on.term_sig != (pod_terminating(on.S) ? 1u : 0u))
            fail("terminating signature is not the pod's");
        rows.push_back(Row{on.tidx, on.pre_dropped, on.has_core, off.has_core});
    }
    return bad;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 5) {
        std::fprintf(stderr, "usage: %s LINES.ndjson SHARD_COUNT SHARD_INDEX BY_UID [NAMESPACE...]\n", argv[0]);
        return 2;
    }
    FILE* in = std::fopen(argv[1], "rb");
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::string all;
    char chunk[65536];
    for (size_t n; (n = std::fread(chunk, 1, sizeof chunk, in)) > 0;) all.append(chunk, n);
    std::fclose(in);
    std::vector<std::unique_ptr<char[]>> bufs;
    std::vector<size_t> sizes;
    for (size_t pos = 0; pos < all.size();) {
        size_t nl = all.find('\n', pos);
        if (nl == std::string::npos) nl = all.size();
        if (nl > pos) {
            bufs.emplace_back(new char[nl - pos]);
            std::memcpy(bufs.back().get(), all.data() + pos, nl - pos);
            sizes.push_back(nl - pos);
        }
        pos = nl + 1;
    }
    const std::string env_json = "\"production\"";
    const ReasonSet reasons = default_failure_reasons();
    const CondRules rules = default_condition_rules();
    NsTextSet set;
    for (int i = 5; i < argc; ++i) set.texts.insert(argv[i]);
    DecodeCfg C{};
    C.light = true;
    C.critical = true;
    C.env_json = &env_json;
    C.reasons = &reasons;
    C.rules = &rules;
    C.terminating = true;  // watcher.alerts.terminating: a terminating pod's line passes the critical filter
    C.ns_texts = argc > 5 ? &set : nullptr;
    C.shard_count = std::atoi(argv[2]);
    C.shard_index = std::atoi(argv[3]);
    C.shard_by_uid = std::atoi(argv[4]) != 0;

    constexpr int THREADS = 4;
    std::vector<Row> rows[THREADS];
    int bad[THREADS] = {};
    std::vector<std::thread> threads;
    for (int t = 0; t < THREADS; ++t)
        threads.emplace_back([&, t] { bad[t] = check_lines(C, bufs, sizes, rows[t]); });
    for (std::thread& t : threads) t.join();
    int total = 0;
    for (int t = 0; t < THREADS; ++t) {
        total += bad[t];
        if (!(rows[t] == rows[0])) {
            std::fprintf(stderr, "thread %d decoded differently from thread 0\n", t);
            ++total;
        }
    }
    // the module switch off (flipped while no thread decodes, as the tests flip it)
    g_payload_prefilter = false;
    std::vector<Row> rows_off[THREADS];
    threads.clear();
    for (int t = 0; t < THREADS; ++t)
        threads.emplace_back([&, t] { bad[t] = check_lines(C, bufs, sizes, rows_off[t]); });
    for (std::thread& t : threads) t.join();
    g_payload_prefilter = true;
    for (int t = 0; t < THREADS; ++t) {
        total += bad[t];
        for (size_t i = 0; i < rows_off[t].size(); ++i)
            if (rows_off[t][i].pre || rows_off[t][i].core_on != rows[0][i].core_off) {
                std::fprintf(stderr, "switch off, thread %d, line %zu: not what off built\n", t, i);
                ++total;
            }
    }
    for (const Row& r : rows[0]) std::printf("%d %d %d %d\n", r.tidx, (int)r.pre, (int)r.core_on, (int)r.core_off);
    std::fprintf(stderr, "%zu lines, %d threads, %d failures\n", bufs.size(), THREADS, total);
    return total ? 1 : 0;
}
