// findings_check — the container failure and pod condition findings walkers,
// the terminating finding, the deletion deadline, the pending-since and the unready-since (../findings.inc) over the scanner
// (../scanner.inc) as a stand-alone program, for a run under
// -fsanitize=address,undefined (scripts/findings_check.sh). No Python.
//
//   findings_check PODS.jsonl [MUTATIONS]
//
// PODS.jsonl holds one pod object per line. For each, the findings of the
// filter-first parse and of the full parse must agree (for the conditions:
// the walk over the raw span, the rules over the walked list, and the walk
// again after materialize()); the signature and the JSON of the container
// findings, then those of the condition findings, then the terminating
// signature and the JSON of the extra field termination, then the deletion
// deadline (or "-" for none), then the pending-since and the unready-since (likewise), go to stdout, one line per pod. Then every pod is mutated
// MUTATIONS times (bytes flipped, cut, doubled, swapped with JSON syntax;
// default 200) and walked again: the result is ignored, a malformed pod is a
// ParseError, and what counts is that the sanitizers stay silent. Every input
// is copied into a buffer of its exact size so an overread is seen.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <memory>
#include <string>
#include <string_view>
#include <vector>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace {

#include "../scanner.inc"
#include "../findings.inc"

struct Result {
    bool parsed = false;
    std::string json, cond_json, term_json;
    uint64_t sig = 0, cond_sig = 0, term_sig = 0;
    bool has_due = false, has_since = false, has_unready = false;
    int64_t due = 0, since = 0, unready = 0;
    bool same(const Result& o) const {
        return json == o.json && sig == o.sig && cond_json == o.cond_json && cond_sig == o.cond_sig &&
               term_json == o.term_json && term_sig == o.term_sig && has_due == o.has_due &&
               (!has_due || due == o.due) && has_since == o.has_since && (!has_since || since == o.since) &&
               has_unready == o.has_unready && (!has_unready || unready == o.unready);
    }
};

Result walk(const char* b, size_t n, bool light) {
    Result r;
    PodSpans S;
    try {
        Parser P(b, b + n);
        if (light) parse_pod_light(P, S); else parse_pod(P, S);
        P.ws();
        if (P.p_ != P.end_) throw ParseError{"trailing data"};
    } catch (const ParseError&) {
        return r;
    }
    r.parsed = true;
    std::vector<Finding> found;
    pod_findings(S, default_failure_reasons(), found);
    r.sig = findings_signature(found);
    findings_json(r.json, &found);
    std::vector<CondFinding> conds;
    const bool cond_ok = pod_conditions(S, default_condition_rules(), conds);
    r.cond_sig = condition_signature(conds);
    conditions_json(r.cond_json, &conds);
    r.term_sig = terminating_signature(S);
    termination_json(r.term_json, S);
    r.has_due = deletion_deadline(S, r.due);
    if (r.has_due && !r.term_sig) {
        std::fprintf(stderr, "a deadline on a pod that is not terminating\n");
        std::abort();
    }
    r.has_since = pending_since(S, r.since);
    if (r.has_since && r.term_sig) {
        std::fprintf(stderr, "a pending-since on a terminating pod\n");
        std::abort();
    }
    r.has_unready = unready_since(S, r.unready);
    if (r.has_unready && (r.term_sig || r.has_since)) {
        std::fprintf(stderr, "an unready-since on a terminating or Pending pod\n");
        std::abort();
    }
    try {
        materialize(S);
    } catch (const ParseError&) {
        return r;
    }
    // the walked list gives what the raw span gave
    std::vector<CondFinding> again;
    std::string again_json;
    pod_conditions(S, default_condition_rules(), again);
    conditions_json(again_json, &again);
    if (!cond_ok || again_json != r.cond_json || condition_signature(again) != r.cond_sig) {
        std::fprintf(stderr, "conditions differ after materialize: %s | %s\n", r.cond_json.c_str(), again_json.c_str());
        std::abort();
    }
    // materialize() walks status and spec only: the metadata spans stand as they stood
    std::string term_again;
    termination_json(term_again, S);
    int64_t due_again = 0;
    const bool has_again = deletion_deadline(S, due_again);
    if (term_again != r.term_json || terminating_signature(S) != r.term_sig || has_again != r.has_due ||
        (has_again && due_again != r.due)) {
        std::fprintf(stderr, "termination differs after materialize: %s | %s\n", r.term_json.c_str(), term_again.c_str());
        std::abort();
    }
    // ... and so do the phase and the creation time
    int64_t since_again = 0;
    if (pending_since(S, since_again) != r.has_since || (r.has_since && since_again != r.since)) {
        std::fprintf(stderr, "pending-since differs after materialize\n");
        std::abort();
    }
    // ... and the Ready condition: the walk runs over the raw span either way
    int64_t unready_again = 0;
    if (unready_since(S, unready_again) != r.has_unready || (r.has_unready && unready_again != r.unready)) {
        std::fprintf(stderr, "unready-since differs after materialize\n");
        std::abort();
    }
    return r;
}

// the bytes in a heap block of exactly their size
Result walk_exact(const std::string& text, bool light) {
    std::unique_ptr<char[]> buf(new char[text.size() ? text.size() : 1]);
    std::memcpy(buf.get(), text.data(), text.size());
    return walk(buf.get(), text.size(), light);
}

uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

void mutate(std::string& s) {
    static const char syntax[] = "{}[]\",:\\-0123456789.eEtfnu ";
    const int edits = 1 + (int)(rnd() % 4);
    for (int i = 0; i < edits && !s.empty(); ++i) {
        const size_t at = (size_t)(rnd() % s.size());
        switch (rnd() % 6) {
            case 0: s[at] = (char)(rnd() & 0xFF); break;
            case 1: s[at] = syntax[rnd() % (sizeof syntax - 1)]; break;
            case 2: s.erase(at, 1 + (size_t)(rnd() % 8)); break;
            case 3: s.insert(at, 1, syntax[rnd() % (sizeof syntax - 1)]); break;
            case 4: s.resize(at); break;
            case 5: {
                const size_t len = std::min<size_t>(1 + (size_t)(rnd() % 64), s.size() - at);
                s.insert(at, s.substr(at, len));
                break;
            }
        }
    }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s PODS.jsonl [MUTATIONS]\n", argv[0]);
        return 2;
    }
    const long mutations = argc > 2 ? std::atol(argv[2]) : 200;
    std::ifstream in(argv[1]);
    if (!in) {
        std::fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    std::vector<std::string> pods;
    for (std::string line; std::getline(in, line);)
        if (!line.empty()) pods.push_back(line);
    int bad = 0;
    for (int simd = 0; simd < 3; ++simd) {
#if defined(__x86_64__)
        // every scanner form this CPU has: scalar, AVX2, AVX-512BW
        if (simd == 1 && !simd_supported()) continue;
        if (simd == 2 && !avx512_supported()) continue;
        Parser::use_avx2 = simd >= 1;
        Parser::use_avx512 = simd == 2;
#else
        if (simd) break;
#endif
        for (const std::string& pod : pods) {
            const Result a = walk_exact(pod, true), b = walk_exact(pod, false);
            if (!a.parsed || !b.parsed || !a.same(b)) {
                std::fprintf(stderr, "parses disagree (simd %d): %.120s\n", simd, pod.c_str());
                ++bad;
            }
            if (simd == 0)
                std::cout << a.sig << '\t' << a.json << '\t' << a.cond_sig << '\t' << a.cond_json << '\t' << a.term_sig
                          << '\t' << a.term_json << '\t' << (a.has_due ? std::to_string(a.due) : std::string("-"))
                          << '\t' << (a.has_since ? std::to_string(a.since) : std::string("-")) << '\t'
                          << (a.has_unready ? std::to_string(a.unready) : std::string("-")) << '\n';
        }
    }
    long walked = 0;
    for (const std::string& pod : pods)
        for (long i = 0; i < mutations; ++i) {
            std::string m = pod;
            mutate(m);
#if defined(__x86_64__)
            Parser::use_avx2 = i % 3 >= 1 && simd_supported();
            Parser::use_avx512 = i % 3 == 2 && avx512_supported();
#endif
            const Result a = walk_exact(m, (i & 1) != 0);
            walked += a.parsed ? 1 : 0;
        }
    std::fprintf(stderr, "%zu pods, %ld mutations each, %ld of them still parsed, %d disagreements\n", pods.size(),
                 mutations, walked, bad);
    return bad ? 1 : 0;
}
