// findings.inc — container failure findings (watcher.alerts.container_failures,
// payload extra field container_failures). Unity-build fragment, #included
// into kwcore.cpp after the scanner (Parser, PodSpans) and before build_core.
// Nothing here touches Python.
//
// A pure function of the pod: status.initContainerStatuses, then
// status.containerStatuses, each element that is a JSON object, in order
// (models/findings.py is the semantic reference; both are held to one verdict
// by tests/test_container_failures.py):
//   waiting     state.waiting.reason is a string of the configured set
//   terminated  (no waiting finding) state.terminated.exitCode is an integer != 0
//   restarted   restartCount is an integer > 0 and lastState.terminated.exitCode
//               is an integer != 0
// "Integer" is a JSON integer token -?[0-9]+ (true, 1.0 and 1e2 are not; -0 is
// zero); a value of the wrong JSON type reads as absent; a repeated key is
// its last value, as json.loads; a reason is compared as decoded text.
//
// The walk runs over the raw spans the light parse kept (cstat_raw, init_raw):
// it needs lastState and the init containers, which parse_cstatuses does not
// record, and it runs for every ADDED/MODIFIED event when the filter option
// is on, where the payload walk runs only for the events that are sent.

enum : uint8_t { FK_WAITING = 0, FK_TERMINATED = 1, FK_RESTARTED = 2 };
const char* const k_finding_kind[] = {"waiting", "terminated", "restarted"};

struct Finding {
    Span name, reason, exit_code, restart_count;  // raw tokens of the right type; absent: null
    bool init;
    uint8_t kind;
};

using ReasonSet = std::vector<std::string>;

const ReasonSet& default_failure_reasons() {
    static const ReasonSet r = {"CrashLoopBackOff",  "ImagePullBackOff",           "ErrImagePull",
                                "ErrImageNeverPull", "InvalidImageName",           "CreateContainerConfigError",
                                "CreateContainerError", "RunContainerError"};
    return r;
}

// -?[0-9]+
inline bool int_token(const Span& s) {
    if (!s.present() || s.n == 0) return false;
    size_t i = s.p[0] == '-' ? 1 : 0;
    if (i == s.n) return false;
    for (; i < s.n; ++i)
        if (s.p[i] < '0' || s.p[i] > '9') return false;
    return true;
}

inline bool int_nonzero(const Span& s) {
    if (!int_token(s)) return false;
    for (size_t i = 0; i < s.n; ++i)
        if (s.p[i] >= '1' && s.p[i] <= '9') return true;
    return false;
}

inline bool int_positive(const Span& s) { return int_nonzero(s) && s.p[0] != '-'; }

inline bool object_span(const Span& s) { return s.present() && s.n >= 2 && s.p[0] == '{'; }

// "waiting" and "terminated" of a container state (state or lastState)
void state_members(const Span& state, Span& waiting, Span& terminated) {
    waiting = terminated = Span();
    if (!object_span(state)) return;
    Parser Q(state.p, state.p + state.n);
    Q.object([&](const char* k, size_t kn) {
        if (KEYIS("waiting")) waiting = Q.value();
        else if (KEYIS("terminated")) terminated = Q.value();
        else Q.value();
    });
}

// "exitCode" (an integer token, else absent) and "reason" (a string, else absent)
void terminated_members(const Span& term, Span& exit_code, Span& reason) {
    exit_code = reason = Span();
    if (!object_span(term)) return;
    Parser Q(term.p, term.p + term.n);
    Q.object([&](const char* k, size_t kn) {
        if (KEYIS("exitCode")) exit_code = Q.value();
        else if (KEYIS("reason")) reason = Q.value();
        else Q.value();
    });
    if (!int_token(exit_code)) exit_code = Span();
    if (!reason.is_string()) reason = Span();
}

Span waiting_reason(const Span& waiting) {
    Span reason;
    if (!object_span(waiting)) return reason;
    Parser Q(waiting.p, waiting.p + waiting.n);
    Q.object([&](const char* k, size_t kn) {
        if (KEYIS("reason")) reason = Q.value(); else Q.value();
    });
    return reason.is_string() ? reason : Span();
}

// the decoded text of a string token is one of the set's
bool reason_in(const Span& r, const ReasonSet& set) {
    if (!r.is_string()) return false;
    const char* p = r.p + 1;
    size_t n = r.n - 2;
    std::string text;
    if (__builtin_expect(std::memchr(p, '\\', n) != nullptr, 0)) {
        json_unescape(text, p, p + n);
        p = text.data();
        n = text.size();
    }
    for (const std::string& s : set)
        if (s.size() == n && std::memcmp(s.data(), p, n) == 0) return true;
    return false;
}

// One status array (raw span); throws ParseError on a malformed one.
void walk_statuses(const Span& raw, bool init, const ReasonSet& reasons, std::vector<Finding>& out) {
    if (!raw.present() || raw.n < 2 || raw.p[0] != '[') return;
    Parser P(raw.p, raw.p + raw.n);
    P.array([&]() {
        if (P.peek() != '{') {
            P.value();
            return;
        }
        Span name, rc, state, last;
        P.object([&](const char* k, size_t kn) {
            switch (kn) {
                case 4:
                    if (KEYIS("name")) { name = P.value(); return; }
                    break;
                case 5:
                    if (KEYIS("state")) { state = P.value(); return; }
                    break;
                case 9:
                    if (KEYIS("lastState")) { last = P.value(); return; }
                    break;
                case 12:
                    if (KEYIS("restartCount")) { rc = P.value(); return; }
                    break;
            }
            P.value();
        });
        if (!name.is_string()) name = Span();
        if (!int_token(rc)) rc = Span();
        Span waiting, term, ec, why;
        state_members(state, waiting, term);
        const Span wr = waiting_reason(waiting);
        if (reason_in(wr, reasons)) {
            out.push_back(Finding{name, wr, Span(), rc, init, FK_WAITING});
        } else {
            terminated_members(term, ec, why);
            if (int_nonzero(ec)) out.push_back(Finding{name, why, ec, rc, init, FK_TERMINATED});
        }
        if (int_positive(rc)) {
            state_members(last, waiting, term);
            terminated_members(term, ec, why);
            if (int_nonzero(ec)) out.push_back(Finding{name, why, ec, rc, init, FK_RESTARTED});
        }
    });
}

// The pod's findings, init containers first. false: a status array is
// malformed (nothing json.loads would have accepted): no findings.
bool pod_findings(const PodSpans& S, const ReasonSet& reasons, std::vector<Finding>& out) {
    out.clear();
    if (!S.status_present) return true;
    try {
        walk_statuses(S.init_raw, true, reasons, out);
        walk_statuses(S.cstat_raw, false, reasons, out);
    } catch (const ParseError&) {
        out.clear();
        return false;
    }
    return true;
}

// The failure signature: 0 for no findings, else a 64-bit hash (FNV-1a) of the
// list — strings as their decoded text, integers in one spelling (-0 is 0) —
// so equal lists give equal signatures however the JSON spelled them.
uint64_t findings_signature(const std::vector<Finding>& f) {
    if (f.empty()) return 0;
    uint64_t h = 1469598103934665603ULL;
    auto mix = [&](const char* p, size_t n) {
        for (size_t i = 0; i < n; ++i) {
            h ^= (uint8_t)p[i];
            h *= 1099511628211ULL;
        }
    };
    auto sized = [&](const char* p, size_t n) {
        const uint32_t len = (uint32_t)n;
        mix(reinterpret_cast<const char*>(&len), sizeof len);
        mix(p, n);
    };
    std::string text;
    auto str = [&](const Span& s) {
        if (!s.present()) {
            mix("\0", 1);
            return;
        }
        mix("\1", 1);
        const char* p = s.p + 1;
        size_t n = s.n - 2;
        if (std::memchr(p, '\\', n)) {
            text.clear();
            json_unescape(text, p, p + n);
            p = text.data();
            n = text.size();
        }
        sized(p, n);
    };
    auto integer = [&](const Span& s) {
        if (!s.present()) {
            mix("\0", 1);
            return;
        }
        mix("\1", 1);
        if (int_nonzero(s)) sized(s.p, s.n); else sized("0", 1);
    };
    for (const Finding& x : f) {
        const char head[2] = {(char)(x.init ? 1 : 0), (char)x.kind};
        mix(head, 2);
        str(x.name);
        str(x.reason);
        integer(x.exit_code);
        integer(x.restart_count);
    }
    return h ? h : 1;
}

inline void put_int_or_null(std::string& o, const Span& s) {
    if (!s.present()) o.append("null", 4);
    else if (int_nonzero(s)) o.append(s.p, s.n);
    else o.push_back('0');
}

// extra.container_failures: the list as JSON, strings copied as their raw
// tokens (the convention of every other payload field)
void findings_json(std::string& o, const std::vector<Finding>* f) {
    o.push_back('[');
    bool first = true;
    if (f)
        for (const Finding& x : *f) {
            if (!first) o.push_back(',');
            first = false;
            o.append("{\"container\":");
            if (x.name.present()) o.append(x.name.p, x.name.n); else o.append("null", 4);
            o.append(x.init ? ",\"init\":true,\"kind\":\"" : ",\"init\":false,\"kind\":\"");
            o.append(k_finding_kind[x.kind]);
            o.append("\",\"reason\":");
            if (x.reason.present()) o.append(x.reason.p, x.reason.n); else o.append("null", 4);
            o.append(",\"exit_code\":");
            put_int_or_null(o, x.exit_code);
            o.append(",\"restart_count\":");
            put_int_or_null(o, x.restart_count);
            o.push_back('}');
        }
    o.push_back(']');
}

// ----------------------------------------------------------------------------- pod condition findings
//
// watcher.alerts.pod_conditions, payload extra field pod_condition_alerts
// (models/findings.py condition_findings is the semantic reference; both are
// held to one verdict by tests/test_pod_condition_alerts.py). status.conditions,
// each element that is a JSON object, in order: a finding when a rule of
// pod_condition_rules has its type, its status and either no reason or its
// reason. type, status and reason are strings, any other JSON type reads as
// absent; a repeated key is its last value; text compares decoded. A finding
// is (type, status, reason) — never the message or the times, which the
// scheduler rewrites at every attempt.
//
// Before materialize() the walk runs over the raw span the light parse kept
// (cond_raw), for every ADDED/MODIFIED event when the filter option is on;
// the full parse and materialize() have walked the array already
// (PodSpans::conditions) and the rules are matched against that.

struct CondRule {
    std::string type, status, reason;
    bool any_reason = true;  // "Type=Status": whatever the reason, or none
};

using CondRules = std::vector<CondRule>;

constexpr size_t MAX_COND_RULES = 32;

const CondRules& default_condition_rules() {
    static const CondRules r = {{"PodScheduled", "False", "Unschedulable", false},
                                {"PodScheduled", "False", "SchedulerError", false},
                                {"DisruptionTarget", "True", "", true}};
    return r;
}

struct CondFinding {
    Span type, status, reason;  // raw string tokens; reason absent: null
};

// The decoded text of a string token: its raw bytes when it has no backslash
// (every condition the API server writes), else unescaped into `buf`.
inline std::string_view token_text(const Span& s, std::string& buf) {
    const char* p = s.p + 1;
    const size_t n = s.n - 2;
    if (__builtin_expect(std::memchr(p, '\\', n) != nullptr, 0)) {
        buf.clear();
        json_unescape(buf, p, p + n);
        return std::string_view(buf);
    }
    return std::string_view(p, n);
}

void match_condition(const Span& type, const Span& status, Span reason, const CondRules& rules,
                     std::vector<CondFinding>& out) {
    if (!type.is_string() || !status.is_string()) return;
    if (!reason.is_string()) reason = Span();
    std::string tb, sb, rb;
    const std::string_view t = token_text(type, tb), s = token_text(status, sb);
    std::string_view r;
    bool have_r = false;  // decoded only when a rule gets as far as asking
    for (const CondRule& rule : rules) {
        if (rule.type != t || rule.status != s) continue;
        if (!rule.any_reason) {
            if (!reason.present()) continue;
            if (!have_r) {
                r = token_text(reason, rb);
                have_r = true;
            }
            if (rule.reason != r) continue;
        }
        out.push_back(CondFinding{type, status, reason});
        return;
    }
}

// status.conditions as a raw span; throws ParseError on a malformed one.
void walk_conditions(const Span& raw, const CondRules& rules, std::vector<CondFinding>& out) {
    if (!raw.present() || raw.n < 2 || raw.p[0] != '[') return;
    Parser P(raw.p, raw.p + raw.n);
    P.array([&]() {
        if (P.peek() != '{') {
            P.value();
            return;
        }
        Span type, status, reason;
        P.object([&](const char* k, size_t kn) {
            switch (kn) {
                case 4:
                    if (KEYIS("type")) { type = P.value(); return; }
                    break;
                case 6:
                    if (KEYIS("status")) { status = P.value(); return; }
                    if (KEYIS("reason")) { reason = P.value(); return; }
                    break;
            }
            P.value();
        });
        match_condition(type, status, reason, rules, out);
    });
}

// A rule can match only where the span holds its type, its status and its
// reason. In a span without a backslash nothing is spelled with an escape, so
// their absence as raw bytes rules the rule out, and a span no rule is left
// for needs no walk: a few byte searches instead of a parse for nearly every
// pod (a healthy pod's conditions hold neither "Unschedulable" nor
// "DisruptionTarget"). A span with a backslash anywhere is always walked.
bool conditions_may_match(const Span& raw, const CondRules& rules) {
    if (!raw.present() || raw.n < 2 || raw.p[0] != '[') return false;
    if (std::memchr(raw.p, '\\', raw.n)) return true;
    const std::string_view text(raw.p, raw.n);
    for (const CondRule& r : rules) {
        if (!r.any_reason && text.find(r.reason) == std::string_view::npos) continue;  // the rarest first
        if (text.find(r.type) != std::string_view::npos && text.find(r.status) != std::string_view::npos) return true;
    }
    return false;
}

// The pod's condition findings. false: the conditions array is malformed
// (nothing json.loads would have accepted): no findings.
bool pod_conditions(const PodSpans& S, const CondRules& rules, std::vector<CondFinding>& out) {
    out.clear();
    if (!S.status_present) return true;
    if (!S.deferred) {
        for (const Condition& c : S.conditions) match_condition(c.type, c.status, c.reason, rules, out);
        return true;
    }
    if (!conditions_may_match(S.cond_raw, rules)) return true;
    try {
        walk_conditions(S.cond_raw, rules, out);
    } catch (const ParseError&) {
        out.clear();
        return false;
    }
    return true;
}

// As findings_signature, of the condition findings: 0 for none, else FNV-1a
// over the decoded text of each (type, status, reason), an absent reason
// apart from an empty one.
uint64_t condition_signature(const std::vector<CondFinding>& f) {
    if (f.empty()) return 0;
    uint64_t h = 1469598103934665603ULL;
    auto mix = [&](const char* p, size_t n) {
        for (size_t i = 0; i < n; ++i) {
            h ^= (uint8_t)p[i];
            h *= 1099511628211ULL;
        }
    };
    std::string buf;
    auto str = [&](const Span& s) {
        if (!s.present()) {
            mix("\0", 1);
            return;
        }
        mix("\1", 1);
        const std::string_view v = token_text(s, buf);
        const uint32_t len = (uint32_t)v.size();
        mix(reinterpret_cast<const char*>(&len), sizeof len);
        mix(v.data(), v.size());
    };
    for (const CondFinding& x : f) {
        str(x.type);
        str(x.status);
        str(x.reason);
    }
    return h ? h : 1;
}

// extra.pod_condition_alerts: the list as JSON, strings copied as their raw tokens
void conditions_json(std::string& o, const std::vector<CondFinding>* f) {
    o.push_back('[');
    bool first = true;
    if (f)
        for (const CondFinding& x : *f) {
            if (!first) o.push_back(',');
            first = false;
            o.append("{\"type\":");
            o.append(x.type.p, x.type.n);
            o.append(",\"status\":");
            o.append(x.status.p, x.status.n);
            o.append(",\"reason\":");
            if (x.reason.present()) o.append(x.reason.p, x.reason.n); else o.append("null", 4);
            o.push_back('}');
        }
    o.push_back(']');
}

// ----------------------------------------------------------------------------- terminating
//
// watcher.alerts.terminating, payload extra field termination
// (models/findings.py terminating is the semantic reference; both are held to
// one verdict by tests/test_terminating_alerts.py). A pod is terminating when
// its metadata is a JSON object whose deletionTimestamp is a JSON string, of
// any text; a value of any other JSON type reads as absent and a repeated key
// is its last value (parse_metadata keeps that one). The finding is the
// boolean alone, so its signature is 1 or 0: a later change of the timestamp
// is no new finding. Nothing to walk: both parses keep the span.

inline bool pod_terminating(const PodSpans& S) { return S.meta_present && S.del_time.is_string(); }

inline uint64_t terminating_signature(const PodSpans& S) { return pod_terminating(S) ? 1 : 0; }

// extra.termination: the three metadata values as their raw tokens, null when absent
void termination_json(std::string& o, const PodSpans& S) {
    auto raw = [&](const Span& s) {
        if (s.present()) o.append(s.p, s.n); else o.append("null", 4);
    };
    o.append("{\"deletion_timestamp\":");
    raw(S.del_time);
    o.append(",\"grace_period_seconds\":");
    raw(S.del_grace);
    o.append(",\"finalizers\":");
    raw(S.finalizers);
    o.push_back('}');
}

// ----------------------------------------------------------------------------- deletion deadline
//
// watcher.alerts.terminating_overdue_seconds (models/findings.py
// deletion_deadline is the semantic reference; tests/test_termination_overdue.py
// holds both to one verdict). Kubernetes sets deletionTimestamp to the time the
// pod is expected to be gone, so a terminating pod's deadline is that text
// read by one exact grammar, ASCII only:
//
//   YYYY-MM-DDTHH:MM:SS[.f{1,9}](Z|+HH:MM|-HH:MM)
//
// year 0001-9999, month 01-12, the day within the month by the proleptic
// Gregorian leap rule, hour 00-23, minute and second 00-59 (no second 60),
// offset 00:00-23:59. The value is seconds since 1970-01-01T00:00:00Z, the
// offset applied, the fraction dropped. Any other text has no deadline. The
// grammar is over the decoded text: the only escape that can spell one of its
// characters is \u00XX, so that one is decoded here and any other backslash
// ends the match — no allocation, no Python, safe on a decode worker.

constexpr size_t DEADLINE_TEXT_MAX = 35;  // 19 + a 9-digit fraction with its point + a 6-byte offset

// days from 1970-01-01 to y-m-d (proleptic Gregorian)
inline int64_t days_from_civil(int64_t y, int m, int d) {
    y -= m <= 2;
    const int64_t era = (y >= 0 ? y : y - 399) / 400;
    const int64_t yoe = y - era * 400;
    const int64_t doy = (153 * (m + (m > 2 ? -3 : 9)) + 2) / 5 + d - 1;
    const int64_t doe = yoe * 365 + yoe / 4 - yoe / 100 + doy;
    return era * 146097 + doe - 719468;
}

// the grammar over decoded text t[0..n)
inline bool timestamp_seconds(const char* t, size_t n, int64_t& out) {
    if (n < 20 || n > DEADLINE_TEXT_MAX) return false;
    auto two = [&](size_t i, int& v) {
        const unsigned a = (unsigned char)t[i] - '0', b = (unsigned char)t[i + 1] - '0';
        if (a > 9 || b > 9) return false;
        v = (int)(a * 10 + b);
        return true;
    };
    int yh, yl, mo, d, h, mi, s;
    if (!two(0, yh) || !two(2, yl) || t[4] != '-' || !two(5, mo) || t[7] != '-' || !two(8, d) || t[10] != 'T' ||
        !two(11, h) || t[13] != ':' || !two(14, mi) || t[16] != ':' || !two(17, s))
        return false;
    const int y = yh * 100 + yl;
    if (y < 1 || mo < 1 || mo > 12 || h > 23 || mi > 59 || s > 59) return false;
    static const int mdays[12] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    const bool leap = y % 4 == 0 && (y % 100 != 0 || y % 400 == 0);
    if (d < 1 || d > mdays[mo - 1] + (mo == 2 && leap ? 1 : 0)) return false;
    size_t i = 19;
    if (t[i] == '.') {
        size_t f = 0;
        for (++i; i < n && (unsigned)((unsigned char)t[i] - '0') <= 9; ++i) ++f;
        if (f < 1 || f > 9 || i >= n) return false;
    }
    int64_t off = 0;
    if (t[i] == 'Z') {
        if (i + 1 != n) return false;
    } else if (t[i] == '+' || t[i] == '-') {
        int oh, om;
        if (i + 6 != n || !two(i + 1, oh) || t[i + 3] != ':' || !two(i + 4, om) || oh > 23 || om > 59) return false;
        off = oh * 3600 + om * 60;
        if (t[i] == '-') off = -off;
    } else {
        return false;
    }
    out = days_from_civil(y, mo, d) * 86400 + h * 3600 + mi * 60 + s - off;
    return true;
}

// The grammar over a JSON string span (quotes included), its escapes decoded.
inline bool timestamp_span_seconds(const Span& t, int64_t& out) {
    const char* p = t.p + 1;
    const size_t n = t.n - 2;
    if (__builtin_expect(std::memchr(p, '\\', n) == nullptr, 1)) return timestamp_seconds(p, n, out);
    char text[DEADLINE_TEXT_MAX];
    size_t k = 0;
    for (const char* e = p + n; p < e;) {
        if (k == DEADLINE_TEXT_MAX) return false;
        if (*p != '\\') {
            text[k++] = *p++;
            continue;
        }
        uint32_t cp;  // \u00XX only: no other escape decodes to a character of the grammar
        if (e - p < 6 || p[1] != 'u' || !read_u4(p + 2, e, cp) || cp >= 0x80) return false;
        text[k++] = (char)cp;
        p += 6;
    }
    return timestamp_seconds(text, k, out);
}

// The deadline of a pod: false unless it is terminating and the decoded text
// of its deletionTimestamp matches the grammar.
inline bool deletion_deadline(const PodSpans& S, int64_t& out) {
    if (!pod_terminating(S)) return false;
    return timestamp_span_seconds(S.del_time, out);
}

// ----------------------------------------------------------------------------- pending since
//
// watcher.alerts.pending_overdue_seconds (models/findings.py pending_since is
// the semantic reference; tests/test_pending_overdue.py holds both to one
// verdict). A pod still Pending has a pending-since, its creation time: status
// is an object whose phase is the string "Pending" (as decoded: an escaped
// spelling counts), the pod is not terminating (the terminating alerts own
// that state, whatever watcher.alerts.terminating says), and
// metadata.creationTimestamp is a string the deadline grammar accepts. Both
// parses keep the three spans, so nothing is walked.
inline bool phase_is(const Span& ph, std::string_view want) {
    if (!ph.is_string()) return false;
    const char* p = ph.p + 1;
    const size_t n = ph.n - 2;
    if (__builtin_expect(std::memchr(p, '\\', n) == nullptr, 1)) return std::string_view(p, n) == want;
    std::string text;  // cold: a phase spelled with escapes
    json_unescape(text, p, p + n);
    return text == want;
}

inline bool phase_is_pending(const Span& ph) { return phase_is(ph, "Pending"); }

inline bool pending_since(const PodSpans& S, int64_t& out) {
    if (!S.status_present || !phase_is_pending(S.phase) || pod_terminating(S)) return false;
    if (!S.meta_present || !S.ctime.is_string()) return false;
    return timestamp_span_seconds(S.ctime, out);
}

// ----------------------------------------------------------------------------- unready since
//
// watcher.alerts.unready_overdue_seconds (models/findings.py unready_since is
// the semantic reference; tests/test_unready_overdue.py holds both to one
// verdict). A pod that is Running and not Ready has an unready-since, the time
// its Ready condition turned False: status is an object whose phase is the
// string "Running" (as decoded), the pod is not terminating, status.conditions
// is an array, the first element of it that is an object whose type is the
// string "Ready" has the string "False" as its status ("Unknown", "false" and
// false are not that), and that element's lastTransitionTime is a string the
// deadline grammar accepts. Later Ready elements are ignored; a repeated key
// is its last value; text compares decoded. Both parses keep the raw span of
// the array (cond_raw), and the walk runs over it, for a Running line only. In
// a span without a backslash nothing is spelled with an escape, so one that
// does not hold "False" as raw bytes (every healthy pod's) needs no walk.
inline bool unready_since(const PodSpans& S, int64_t& out) {
    if (!S.status_present || !phase_is(S.phase, "Running") || pod_terminating(S)) return false;
    const Span& raw = S.cond_raw;
    if (!raw.present() || raw.n < 2 || raw.p[0] != '[') return false;
    if (!std::memchr(raw.p, '\\', raw.n) &&
        std::string_view(raw.p, raw.n).find("\"False\"") == std::string_view::npos)
        return false;
    bool found = false;  // the first Ready element decides
    Span state, stamp;
    try {
        Parser P(raw.p, raw.p + raw.n);
        P.array([&]() {
            if (found || P.peek() != '{') {
                P.value();
                return;
            }
            Span type, status, time;
            P.object([&](const char* k, size_t kn) {
                switch (kn) {
                    case 4:
                        if (KEYIS("type")) { type = P.value(); return; }
                        break;
                    case 6:
                        if (KEYIS("status")) { status = P.value(); return; }
                        break;
                    case 18:
                        if (KEYIS("lastTransitionTime")) { time = P.value(); return; }
                        break;
                }
                P.value();
            });
            if (!type.is_string()) return;
            std::string tb;
            if (token_text(type, tb) != "Ready") return;
            found = true;
            state = status;
            stamp = time;
        });
    } catch (const ParseError&) {
        return false;  // nothing json.loads would have accepted
    }
    if (!found || !state.is_string() || !stamp.is_string()) return false;
    std::string sb;
    if (token_text(state, sb) != "False") return false;
    return timestamp_span_seconds(stamp, out);
}
