// _kwcore — native watch-event decoder for k8s-watcher-amd.
//
// Hot path of the watcher: one kube-apiserver watch line
// `{"type":"MODIFIED","object":{<Pod>}}` → the fields the filters need plus the
// clusterapi payload *core* (reference
// /root/reference/watcher/pod_watcher.py:159-202) as ready-to-send JSON bytes.
//
// The reference pays for this with json.loads + reflective V1Pod model
// construction inside the `kubernetes` library and then a Python dict build;
// here a single forward pass over the line records byte spans of the ~20
// fields that matter, skips everything else (managedFields, volumes, env, ...)
// with a structural scanner, and assembles the payload by copying raw JSON
// tokens. No Python object is created for the pod body.
//
// Semantics are pinned to the Python engine (models/payload.py::build_core),
// see tests/test_native_parity.py.

#define PY_SSIZE_T_CLEAN
#include <Python.h>

#include <arpa/inet.h>
#include <fcntl.h>
#include <openssl/err.h>
#include <openssl/evp.h>
#include <openssl/hmac.h>
#include <openssl/pem.h>
#include <openssl/ssl.h>
#include <openssl/x509v3.h>

#include <linux/futex.h>
#include <malloc.h>
#include <netinet/in.h>
#include <netinet/tcp.h>
#include <poll.h>
#include <sys/epoll.h>
#include <sys/ioctl.h>
#include <sys/mman.h>
#include <sys/sendfile.h>
#include <sys/resource.h>
#include <sys/eventfd.h>
#include <sys/socket.h>
#include <sys/syscall.h>
#include <sys/types.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <array>
#include <charconv>
#include <chrono>
#include <atomic>
#include <cctype>
#include <cerrno>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <string>
#include <thread>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#if defined(__x86_64__)
#include <immintrin.h>
#endif

namespace {

#include "scanner.inc"
#include "chunked.inc"

// ----------------------------------------------------------------------------- output

inline void put(std::string& o, const char* s, size_t n) { o.append(s, n); }
inline void put(std::string& o, const char* lit) { o.append(lit); }
inline void raw_or_null(std::string& o, const Span& s) {
    if (s.present()) o.append(s.p, s.n); else o.append("null", 4);
}

bool is_digit(char c) { return c >= '0' && c <= '9'; }

// JSON "falsy" per Python truthiness after json.loads: null, {}, [], "", 0, false.
bool falsy_token(const Span& s) {
    if (!s.present()) return true;
    const char* p = s.p;
    size_t n = s.n;
    if (n == 4 && std::memcmp(p, "null", 4) == 0) return true;
    if (n == 5 && std::memcmp(p, "false", 5) == 0) return true;
    if (n == 2 && std::memcmp(p, "\"\"", 2) == 0) return true;
    if (p[0] == '{' || p[0] == '[') {
        for (size_t i = 1; i + 1 < n; ++i) {
            char c = p[i];
            if (!(c == ' ' || c == '\n' || c == '\r' || c == '\t')) return false;
        }
        return true;
    }
    if (is_digit(p[0]) || p[0] == '-') {  // a number: falsy when float() of it is zero (1e-400 underflows to 0.0)
        const std::string num(p, n);
        return std::strtod(num.c_str(), nullptr) == 0.0;
    }
    return false;
}

// models/timefmt.py::k8s_time_to_isoformat on the raw string token.
void creation_time(std::string& o, const Span& s) {
    if (!s.present() || s.is_null()) {
        o.append("null", 4);
        return;
    }
    if (!s.is_string()) {  // non-string: passed through unchanged
        o.append(s.p, s.n);
        return;
    }
    const char* p = s.p + 1;
    size_t n = s.n - 2;
    std::string plain;
    if (std::memchr(p, '\\', n)) {  // never produced by the API: the decoded text decides, as in Python
        json_unescape(plain, p, p + n);
        p = plain.data();
        n = plain.size();
    }
    // YYYY-MM-DD[Tt ]HH:MM:SS(.frac)?(Z|z|[+-]HH:?MM)?
    auto digits = [&](size_t at, size_t cnt) {
        if (at + cnt > n) return false;
        for (size_t i = 0; i < cnt; ++i)
            if (!is_digit(p[at + i])) return false;
        return true;
    };
    bool ok = n >= 19 && digits(0, 4) && p[4] == '-' && digits(5, 2) && p[7] == '-' && digits(8, 2) &&
              (p[10] == 'T' || p[10] == 't' || p[10] == ' ') && digits(11, 2) && p[13] == ':' &&
              digits(14, 2) && p[16] == ':' && digits(17, 2);
    size_t i = 19;
    size_t fs = 0, fn = 0;
    if (ok && i < n && p[i] == '.') {
        fs = ++i;
        while (i < n && is_digit(p[i])) ++i;
        fn = i - fs;
        if (fn == 0) ok = false;
    }
    std::string tz;
    bool has_tz = false;
    if (ok && i < n) {
        if ((p[i] == 'Z' || p[i] == 'z') && i + 1 == n) {
            tz = "+00:00";
            has_tz = true;
        } else if ((p[i] == '+' || p[i] == '-') && (n - i == 6 || n - i == 5)) {
            if (n - i == 6 && digits(i + 1, 2) && p[i + 3] == ':' && digits(i + 4, 2)) {
                tz.assign(p + i, 6);
            } else if (n - i == 5 && digits(i + 1, 4)) {
                tz.assign(p + i, 3);
                tz.push_back(':');
                tz.append(p + i + 3, 2);
            } else {
                ok = false;
            }
            if (tz == "-00:00") tz = "+00:00";
            has_tz = true;
        } else {
            ok = false;
        }
    }
    if (!ok) {
        o.append(s.p, s.n);
        return;
    }
    o.push_back('"');
    o.append(p, 10);
    o.push_back('T');
    o.append(p + 11, 8);
    if (fn) {
        char micro[7];
        for (size_t k = 0; k < 6; ++k) micro[k] = k < fn ? p[fs + k] : '0';
        micro[6] = 0;
        bool nonzero = false;
        for (size_t k = 0; k < 6; ++k)
            if (micro[k] != '0') nonzero = true;
        if (nonzero) {
            o.push_back('.');
            o.append(micro, 6);
        }
    }
    if (has_tz) o.append(tz);
    o.push_back('"');
}

#include "findings.inc"

// extra: bit i = models/payload.py EXTRA_FIELDS[i]
// (pod_ip, host_ip, start_time, qos_class, resource_version, owner_references,
// container_failures: the findings the caller computed, [] without any,
// pod_condition_alerts: likewise the condition findings,
// termination: metadata.deletionTimestamp, deletionGracePeriodSeconds and
// finalizers, copied). The mask is an int everywhere: bit 8 is above a byte.
constexpr int EXTRA_FAILURES = 1 << 6;
constexpr int EXTRA_CONDITIONS = 1 << 7;
constexpr int EXTRA_TERMINATION = 1 << 8;

bool state_repr_json(std::string& o, const Span& state, const std::string& tz_utc);  // pyrepr.inc

// tz_utc non-null: watcher.state_format python_repr (pyrepr.inc); false when
// a state needs the Python formatter (the core is then incomplete).
bool build_core(std::string& o, const PodSpans& S, const std::string& env_json, int extra = 0,
                const std::string* tz_utc = nullptr, const std::vector<Finding>* findings = nullptr,
                const std::vector<CondFinding>* conds = nullptr) {
    o.clear();
    o.append("{\"name\":");
    raw_or_null(o, S.name);
    o.append(",\"namespace\":");
    raw_or_null(o, S.ns);
    o.append(",\"uid\":");
    raw_or_null(o, S.uid);
    o.append(",\"environment\":");
    o.append(env_json);
    o.append(",\"status\":{\"phase\":");
    if (S.status_present) {
        raw_or_null(o, S.phase);
        o.append(",\"conditions\":[");
        bool first = true;
        for (const auto& c : S.conditions) {
            if (!first) o.push_back(',');
            first = false;
            o.append("{\"type\":");
            raw_or_null(o, c.type);
            o.append(",\"status\":");
            raw_or_null(o, c.status);
            o.append(",\"reason\":");
            raw_or_null(o, c.reason);
            o.append(",\"message\":");
            raw_or_null(o, c.message);
            o.push_back('}');
        }
        o.append("],\"container_statuses\":[");
        first = true;
        for (const auto& c : S.cstatuses) {
            if (!first) o.push_back(',');
            first = false;
            o.append("{\"name\":");
            raw_or_null(o, c.name);
            o.append(",\"ready\":");
            raw_or_null(o, c.ready);
            o.append(",\"restart_count\":");
            raw_or_null(o, c.restart_count);
            o.append(",\"state\":");
            if (tz_utc) {
                if (!state_repr_json(o, c.state, *tz_utc)) return false;
            } else {
                raw_or_null(o, c.state);
            }
            o.push_back('}');
        }
        o.append("]}");
    } else {
        o.append("\"Unknown\",\"conditions\":[],\"container_statuses\":[]}");
    }
    o.append(",\"spec\":{\"node_name\":");
    if (S.spec_present) {
        raw_or_null(o, S.node_name);
        o.append(",\"containers\":[");
        bool first = true;
        for (const auto& c : S.containers) {
            if (!first) o.push_back(',');
            first = false;
            o.append("{\"name\":");
            raw_or_null(o, c.name);
            o.append(",\"image\":");
            raw_or_null(o, c.image);
            o.push_back('}');
        }
        o.append("]}");
    } else {
        o.append("null,\"containers\":[]}");
    }
    o.append(",\"metadata\":{\"labels\":");
    if (falsy_token(S.labels)) o.append("{}"); else o.append(S.labels.p, S.labels.n);
    o.append(",\"annotations\":");
    if (falsy_token(S.annotations)) o.append("{}"); else o.append(S.annotations.p, S.annotations.n);
    o.append(",\"creation_timestamp\":");
    creation_time(o, S.ctime);
    o.push_back('}');
    if (extra) {
        static const char* names[6] = {"pod_ip", "host_ip", "start_time", "qos_class", "resource_version",
                                       "owner_references"};
        const Span* vals[6] = {&S.pod_ip, &S.host_ip, &S.start_time, &S.qos, &S.rv, &S.owners};
        o.append(",\"extra\":{");
        bool first = true;
        for (int i = 0; i < 6; ++i) {
            if (!(extra >> i & 1)) continue;
            if (!first) o.push_back(',');
            first = false;
            o.push_back('"');
            o.append(names[i]);
            o.append("\":");
            raw_or_null(o, *vals[i]);
        }
        if (extra & EXTRA_FAILURES) {
            if (!first) o.push_back(',');
            o.append("\"container_failures\":");
            findings_json(o, findings);
            first = false;
        }
        if (extra & EXTRA_CONDITIONS) {
            if (!first) o.push_back(',');
            o.append("\"pod_condition_alerts\":");
            conditions_json(o, conds);
            first = false;
        }
        if (extra & EXTRA_TERMINATION) {
            if (!first) o.push_back(',');
            o.append("\"termination\":");
            termination_json(o, S);
        }
        o.push_back('}');
    }
    o.push_back('}');
    return true;
}

#include "validate.inc"

// watcher.validate: payload, for the string tokens extra.container_failures copies
const char* findings_invalid(const std::vector<Finding>& f) {
    for (const Finding& x : f)
        for (const Span* sp : {&x.name, &x.reason})
            if (const char* why = span_invalid(*sp)) return why;
    return nullptr;
}

// ... and for those extra.pod_condition_alerts copies
const char* conditions_invalid(const std::vector<CondFinding>& f) {
    for (const CondFinding& x : f)
        for (const Span* sp : {&x.type, &x.status, &x.reason})
            if (const char* why = span_invalid(*sp)) return why;
    return nullptr;
}

// ... and for the three metadata spans extra.termination copies
const char* termination_invalid(const PodSpans& S) {
    for (const Span* sp : {&S.del_time, &S.del_grace, &S.finalizers})
        if (const char* why = span_invalid(*sp)) return why;
    return nullptr;
}

// ----------------------------------------------------------------------------- Python glue

PyObject* g_json_loads = nullptr;
// WatchList (sendInitialEvents=true): the BOOKMARK that ends the initial
// state carries metadata.annotations["k8s.io/initial-events-end"] == "true".
bool initial_events_end(const Span& annotations) {
    if (!annotations.present() || annotations.n < 2 || annotations.p[0] != '{') return false;
    bool found = false;
    try {
        Parser P(annotations.p, annotations.p + annotations.n);
        P.object([&](const char* k, size_t kn) {
            Span v = P.value();
            if (!KEYIS("k8s.io/initial-events-end")) return;
            // a repeated key: the last one counts, as json.loads
            if (v.is_string() && std::memchr(v.p, '\\', v.n)) {
                std::string text;
                json_unescape(text, v.p + 1, v.p + v.n - 1);
                found = text == "true";
            } else {
                found = v.n == 6 && !std::memcmp(v.p, "\"true\"", 6);
            }
        });
    } catch (const ParseError&) {
        return false;
    }
    return found;
}

PyObject* g_types[6];  // ADDED MODIFIED DELETED BOOKMARK ERROR INVALID
enum { T_ADDED, T_MODIFIED, T_DELETED, T_BOOKMARK, T_ERROR, T_INVALID };

// JSON string token → Python str; non-string / absent → None (new reference).
PyObject* span_to_str(const Span& s) {
    if (!s.is_string()) Py_RETURN_NONE;
    const char* p = s.p + 1;
    size_t n = s.n - 2;
    if (!std::memchr(p, '\\', n)) {  // as json.loads(bytes) decodes: a raw lone surrogate passes
        PyObject* u = PyUnicode_DecodeUTF8(p, (Py_ssize_t)n, "surrogatepass");
        if (u) return u;
        PyErr_Clear();
        return PyUnicode_DecodeUTF8(p, (Py_ssize_t)n, "replace");
    }
    std::string o;
    o.reserve(n);
    json_unescape(o, p, p + n);
    return PyUnicode_DecodeUTF8(o.data(), (Py_ssize_t)o.size(), "surrogatepass");
}

#include "pyrepr.inc"

struct InternTable {
    std::unordered_map<std::string, PyObject*> map;
    ~InternTable() {
        for (auto& kv : map) Py_XDECREF(kv.second);
    }
    // Small-cardinality strings (namespaces, phases): reuse one object.
    PyObject* get(const Span& s) {
        if (!s.is_string() || s.n > 66 || std::memchr(s.p, '\\', s.n)) return span_to_str(s);
        std::string key(s.p + 1, s.n - 2);
        auto it = map.find(key);
        if (it != map.end()) {
            Py_INCREF(it->second);
            return it->second;
        }
        PyObject* v = span_to_str(s);
        if (!v) return nullptr;
        if (map.size() < 4096) {
            Py_INCREF(v);
            map.emplace(std::move(key), v);
        }
        return v;
    }
};

struct DecoderObject {
    PyObject_HEAD
    std::string* partial;
    std::string* env_json;
    std::string* out;
    PodSpans* spans;
    InternTable* interned;
    ChunkState chunk;  // feed_chunked's framing state (chunked.inc)
    long long n_events;
    long long n_bytes;
    int extra;  // watcher.payload_extra_fields mask
    int validate;  // watcher.validate: 0 off, 1 payload (default), 2 full
    std::string* tz_utc;     // state_format python_repr (pyrepr.inc); NULL: structured
    PyObject* repr_fallback; // object bytes -> core bytes, for states pyrepr.inc leaves to Python
    // watcher.alerts.container_failures: pod events carry a tenth field, the
    // failure signature (findings.inc); the reasons also serve the extra field
    bool failures;
    ReasonSet* reasons;
    std::vector<Finding>* findings;  // scratch
    // watcher.alerts.pod_conditions: pod events carry an eleventh field, the
    // signature of the condition findings; the rules also serve the extra field
    bool conditions;
    CondRules* rules;
    std::vector<CondFinding>* cond_findings;  // scratch
    // watcher.alerts.terminating: pod events carry a twelfth field, 1 when the
    // pod's graceful deletion has begun (findings.inc), else 0
    bool terminating;
    // watcher.alerts.terminating_overdue_seconds > 0 (with terminating): a
    // thirteenth field, the pod's deletion deadline or None (findings.inc)
    bool deadlines;
    // watcher.alerts.pending_overdue_seconds > 0: a fourteenth field, the
    // creation time of a pod still Pending or None (findings.inc); the four
    // before it are then present too, 0 / None while their options are off
    bool pending;
    // watcher.alerts.unready_overdue_seconds > 0: a fifteenth field, the time
    // the Ready condition of a Running pod turned False or None
    // (findings.inc); the five before it likewise present
    bool unready;
};

PyObject* make_invalid(const char* why, const char* line, size_t n) {
    PyObject* msg = PyUnicode_FromFormat("%s: %.200s", why, std::string(line, n < 200 ? n : 200).c_str());
    if (!msg) {
        PyErr_Clear();
        msg = PyUnicode_FromString(why);
    }
    PyObject* t = PyTuple_New(9);
    Py_INCREF(g_types[T_INVALID]);
    PyTuple_SET_ITEM(t, 0, g_types[T_INVALID]);
    for (int i = 1; i < 8; ++i) {
        PyObject* v = (i == 6) ? Py_False : Py_None;
        Py_INCREF(v);
        PyTuple_SET_ITEM(t, i, v);
    }
    PyTuple_SET_ITEM(t, 8, msg);
    return t;
}

int type_index(const Span& s) {
    if (!s.is_string()) return -1;
    const char* p = s.p + 1;
    size_t n = s.n - 2;
    if (n == 5 && !std::memcmp(p, "ADDED", 5)) return T_ADDED;
    if (n == 8 && !std::memcmp(p, "MODIFIED", 8)) return T_MODIFIED;
    if (n == 7 && !std::memcmp(p, "DELETED", 7)) return T_DELETED;
    if (n == 8 && !std::memcmp(p, "BOOKMARK", 8)) return T_BOOKMARK;
    if (n == 5 && !std::memcmp(p, "ERROR", 5)) return T_ERROR;
    if (std::memchr(p, '\\', n)) {  // "ADD\u0045D" is ADDED
        std::string text;
        json_unescape(text, p, p + n);
        if (!std::memchr(text.data(), '\\', text.size())) {
            text.insert(text.begin(), '"');
            text.push_back('"');
            return type_index(Span{text.data(), text.size()});
        }
    }
    return -2;  // unknown type string
}

// Build the event tuple for a parsed pod. `tidx` is the event type index.
PyObject* event_tuple(DecoderObject* self, int tidx, PyObject* type_obj, const Span& obj_span) {
    PodSpans& S = *self->spans;
    const bool pod_event = tidx >= T_ADDED && tidx <= T_DELETED;
    const bool with_unr = self->unready && pod_event;
    const bool with_pend = (self->pending || with_unr) && pod_event;
    const bool with_tsig = (self->terminating || with_pend) && pod_event;
    const bool with_csig = (self->conditions || with_tsig) && pod_event;
    const bool with_sig = (self->failures || with_csig) && pod_event;
    const bool with_due = with_tsig && ((self->terminating && self->deadlines) || with_pend);
    PyObject* t = PyTuple_New(with_unr ? 15 : with_pend ? 14 : with_due ? 13 : with_tsig ? 12 : with_csig ? 11 : with_sig ? 10 : 9);
    if (!t) return nullptr;
    if (with_sig) {  // filled below; a tuple is never left with an empty slot
        Py_INCREF(Py_None);
        PyTuple_SET_ITEM(t, 9, Py_None);
    }
    if (with_csig) {
        Py_INCREF(Py_None);
        PyTuple_SET_ITEM(t, 10, Py_None);
    }
    if (with_tsig) {
        Py_INCREF(Py_None);
        PyTuple_SET_ITEM(t, 11, Py_None);
    }
    if (with_due) {  // None stays unless the line is a terminating pod's with a deadline
        Py_INCREF(Py_None);
        PyTuple_SET_ITEM(t, 12, Py_None);
    }
    if (with_pend) {  // None stays unless the line is a live Pending pod's with a creation time
        Py_INCREF(Py_None);
        PyTuple_SET_ITEM(t, 13, Py_None);
    }
    if (with_unr) {  // None stays unless the line is a live Running pod's whose Ready is False since a time
        Py_INCREF(Py_None);
        PyTuple_SET_ITEM(t, 14, Py_None);
    }
    Py_INCREF(type_obj);
    PyTuple_SET_ITEM(t, 0, type_obj);
    if (tidx == T_ERROR) {
        for (int i = 1; i < 8; ++i) {
            PyObject* v = (i == 6) ? Py_False : Py_None;
            Py_INCREF(v);
            PyTuple_SET_ITEM(t, i, v);
        }
        PyObject* raw = PyBytes_FromStringAndSize(obj_span.p, (Py_ssize_t)obj_span.n);
        PyObject* st = raw ? PyObject_CallOneArg(g_json_loads, raw) : nullptr;
        Py_XDECREF(raw);
        if (!st) {
            PyErr_Clear();
            st = PyDict_New();
        }
        PyTuple_SET_ITEM(t, 8, st);
        return t;
    }
    PyObject* uid = span_to_str(S.uid);
    PyObject* ns = self->interned->get(S.ns);
    PyObject* name = span_to_str(S.name);
    PyObject* rv = span_to_str(S.rv);
    PyObject* phase = S.status_present ? self->interned->get(S.phase) : (Py_INCREF(Py_None), Py_None);
    if (!uid || !ns || !name || !rv || !phase) {
        Py_XDECREF(uid); Py_XDECREF(ns); Py_XDECREF(name); Py_XDECREF(rv); Py_XDECREF(phase);
        Py_DECREF(t);
        return nullptr;
    }
    PyTuple_SET_ITEM(t, 1, uid);
    PyTuple_SET_ITEM(t, 2, ns);
    PyTuple_SET_ITEM(t, 3, name);
    PyTuple_SET_ITEM(t, 4, rv);
    PyTuple_SET_ITEM(t, 5, phase);
    PyObject* hs = S.status_present ? Py_True : Py_False;
    Py_INCREF(hs);
    PyTuple_SET_ITEM(t, 6, hs);
    if (tidx == T_BOOKMARK || tidx < 0) {
        Py_INCREF(Py_None);
        PyTuple_SET_ITEM(t, 7, Py_None);
        if (tidx == T_BOOKMARK) {  // extra: True on the WatchList end-of-initial-events marker
            PyObject* end = initial_events_end(S.annotations) ? Py_True : Py_False;
            Py_INCREF(end);
            PyTuple_SET_ITEM(t, 8, end);
            return t;
        }
    } else {
        if (self->validate == 1) {  // no malformed sub-tree into a payload (validate.inc)
            if (const char* why = payload_spans_invalid(S)) {
                Py_DECREF(t);
                return make_invalid(why, obj_span.p, obj_span.n);
            }
        }
        const std::vector<Finding>* found = nullptr;
        if ((with_sig && self->failures) || (self->extra & EXTRA_FAILURES)) {
            pod_findings(S, *self->reasons, *self->findings);
            found = self->findings;
            if (self->validate == 1 && (self->extra & EXTRA_FAILURES)) {
                if (const char* why = findings_invalid(*found)) {
                    Py_DECREF(t);
                    return make_invalid(why, obj_span.p, obj_span.n);
                }
            }
        }
        if (with_sig) {
            PyObject* sig = PyLong_FromUnsignedLongLong(tidx == T_DELETED || !found ? 0 : findings_signature(*found));
            if (!sig) {
                Py_DECREF(t);
                return nullptr;
            }
            Py_DECREF(Py_None);
            PyTuple_SET_ITEM(t, 9, sig);
        }
        const std::vector<CondFinding>* cfound = nullptr;
        if ((with_csig && self->conditions) || (self->extra & EXTRA_CONDITIONS)) {
            pod_conditions(S, *self->rules, *self->cond_findings);
            cfound = self->cond_findings;
            if (self->validate == 1 && (self->extra & EXTRA_CONDITIONS)) {
                if (const char* why = conditions_invalid(*cfound)) {
                    Py_DECREF(t);
                    return make_invalid(why, obj_span.p, obj_span.n);
                }
            }
        }
        if (with_csig) {
            PyObject* sig = PyLong_FromUnsignedLongLong(tidx == T_DELETED || !cfound ? 0 : condition_signature(*cfound));
            if (!sig) {
                Py_DECREF(t);
                return nullptr;
            }
            Py_DECREF(Py_None);
            PyTuple_SET_ITEM(t, 10, sig);
        }
        if (self->validate == 1 && (self->extra & EXTRA_TERMINATION)) {
            if (const char* why = termination_invalid(S)) {
                Py_DECREF(t);
                return make_invalid(why, obj_span.p, obj_span.n);
            }
        }
        if (with_tsig) {
            PyObject* sig = PyLong_FromUnsignedLongLong(tidx == T_DELETED || !self->terminating ? 0
                                                                                                : terminating_signature(S));
            if (!sig) {
                Py_DECREF(t);
                return nullptr;
            }
            Py_DECREF(Py_None);
            PyTuple_SET_ITEM(t, 11, sig);
        }
        int64_t due;
        if (with_due && self->terminating && self->deadlines && tidx != T_DELETED && deletion_deadline(S, due)) {
            PyObject* d = PyLong_FromLongLong((long long)due);
            if (!d) {
                Py_DECREF(t);
                return nullptr;
            }
            Py_DECREF(Py_None);
            PyTuple_SET_ITEM(t, 12, d);
        }
        if (with_pend && self->pending && tidx != T_DELETED && pending_since(S, due)) {
            PyObject* d = PyLong_FromLongLong((long long)due);
            if (!d) {
                Py_DECREF(t);
                return nullptr;
            }
            Py_DECREF(Py_None);
            PyTuple_SET_ITEM(t, 13, d);
        }
        if (with_unr && tidx != T_DELETED && unready_since(S, due)) {
            PyObject* d = PyLong_FromLongLong((long long)due);
            if (!d) {
                Py_DECREF(t);
                return nullptr;
            }
            Py_DECREF(Py_None);
            PyTuple_SET_ITEM(t, 14, d);
        }
        PyObject* core;
        if (build_core(*self->out, S, *self->env_json, self->extra, self->tz_utc, found, cfound)) {
            core = PyBytes_FromStringAndSize(self->out->data(), (Py_ssize_t)self->out->size());
        } else {  // a container state the native repr leaves to models/payload.py
            PyObject* raw = self->repr_fallback ? PyBytes_FromStringAndSize(obj_span.p, (Py_ssize_t)obj_span.n)
                                                : nullptr;
            core = raw ? PyObject_CallOneArg(self->repr_fallback, raw) : nullptr;
            Py_XDECREF(raw);
            if (!core || !PyBytes_Check(core)) {
                PyErr_Clear();
                Py_XDECREF(core);
                Py_DECREF(t);
                return make_invalid("container state not representable", obj_span.p, obj_span.n);
            }
        }
        if (!core) {
            Py_DECREF(t);
            return nullptr;
        }
        PyTuple_SET_ITEM(t, 7, core);
    }
    Py_INCREF(Py_None);
    PyTuple_SET_ITEM(t, 8, Py_None);
    return t;
}

// Decode one watch line. Returns a new tuple, or nullptr with a Python error set.
PyObject* decode_line(DecoderObject* self, const char* b, size_t n) {
    PodSpans& S = *self->spans;
    S.clear();
    if (self->validate == 2) {
        if (const char* why = json_invalid(b, n)) return make_invalid(why, b, n);
    }
    Span type_span, obj_span;
    bool not_object = false;
    try {
        Parser P(b + (has_bom(b, n) ? 3 : 0), b + n);  // as json.loads(bytes): 'utf-8-sig'
        P.object([&](const char* k, size_t kn) {
            if (KEYIS("type")) {
                type_span = P.value();
            } else if (KEYIS("object")) {
                S.clear();  // a repeated "object" key: the last one is the pod
                obj_span = Span();
                if (P.peek() != '{') {  // not an object: INVALID, unless a later "object" key is one
                    P.value();
                    not_object = true;
                    return;
                }
                not_object = false;
                const char* start = P.p_;
                parse_pod(P, S);
                obj_span.p = start;
                obj_span.n = (size_t)(P.p_ - start);
            } else {
                P.value();
            }
        });
        P.ws();
        if (P.p_ != P.end_) throw ParseError{"trailing data"};
        if (not_object) throw ParseError{"object is not a JSON object"};
    } catch (const ParseError& e) {
        return make_invalid(e.msg, b, n);
    }
    int tidx = type_index(type_span);
    if (tidx == -1 || !obj_span.present()) return make_invalid("missing type or object", b, n);
    PyObject* type_obj;
    if (tidx >= 0) {
        type_obj = g_types[tidx];
        Py_INCREF(type_obj);
    } else {
        type_obj = span_to_str(type_span);
        if (!type_obj) return nullptr;
    }
    PyObject* t = event_tuple(self, tidx, type_obj, obj_span);
    Py_DECREF(type_obj);
    self->n_events++;
    return t;
}

// ----------------------------------------------------------------------------- methods

int Decoder_init(DecoderObject* self, PyObject* args, PyObject* kwds) {
    static const char* kwlist[] = {"environment", "state_format", nullptr};
    const char* env = nullptr;
    Py_ssize_t envn = 0;
    const char* sf = "structured";
    if (!PyArg_ParseTupleAndKeywords(args, kwds, "s#|s", (char**)kwlist, &env, &envn, &sf)) return -1;
    if (std::strcmp(sf, "structured") != 0 && std::strcmp(sf, "python_repr") != 0) {
        PyErr_SetString(PyExc_ValueError, "state_format must be 'structured' or 'python_repr'");
        return -1;
    }
    delete self->tz_utc;
    self->tz_utc = std::strcmp(sf, "python_repr") == 0 ? new std::string("tzutc()") : nullptr;
    // environment as a JSON string literal (via json.dumps for exact escaping)
    PyObject* envs = PyUnicode_FromStringAndSize(env, envn);
    if (!envs) return -1;
    PyObject* mod = PyImport_ImportModule("json");
    PyObject* dumped = mod ? PyObject_CallMethod(mod, "dumps", "O", envs) : nullptr;
    Py_XDECREF(mod);
    Py_DECREF(envs);
    if (!dumped) return -1;
    Py_ssize_t dn;
    const char* d = PyUnicode_AsUTF8AndSize(dumped, &dn);
    if (!d) {
        Py_DECREF(dumped);
        return -1;
    }
    self->env_json->assign(d, (size_t)dn);
    Py_DECREF(dumped);
    return 0;
}

PyObject* Decoder_new(PyTypeObject* type, PyObject*, PyObject*) {
    DecoderObject* self = (DecoderObject*)type->tp_alloc(type, 0);
    if (!self) return nullptr;
    self->partial = new std::string();
    self->env_json = new std::string("\"\"");
    self->out = new std::string();
    self->out->reserve(8192);
    self->spans = new PodSpans();
    self->interned = new InternTable();
    new (&self->chunk) ChunkState();
    self->n_events = 0;
    self->n_bytes = 0;
    self->validate = 1;
    self->tz_utc = nullptr;
    self->repr_fallback = nullptr;
    self->failures = false;
    self->reasons = new ReasonSet(default_failure_reasons());
    self->findings = new std::vector<Finding>();
    self->conditions = false;
    self->rules = new CondRules(default_condition_rules());
    self->cond_findings = new std::vector<CondFinding>();
    self->terminating = false;
    self->deadlines = false;
    self->pending = false;
    self->unready = false;
    return (PyObject*)self;
}

void Decoder_dealloc(DecoderObject* self) {
    delete self->partial;
    delete self->env_json;
    delete self->out;
    delete self->spans;
    delete self->interned;
    self->chunk.~ChunkState();
    delete self->tz_utc;
    delete self->reasons;
    delete self->findings;
    delete self->rules;
    delete self->cond_findings;
    Py_XDECREF(self->repr_fallback);
    Py_TYPE(self)->tp_free((PyObject*)self);
}

bool blank(const char* b, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (!(b[i] == ' ' || b[i] == '\r' || b[i] == '\t' || b[i] == '\n')) return false;
    return true;
}

// Split `data` into NDJSON lines (carrying a partial line across calls) and
// append one event tuple per complete non-blank line to `out`.
bool process_segment(DecoderObject* self, const char* data, size_t n, PyObject* out) {
    std::string& partial = *self->partial;
    bool open = !partial.empty();
    return split_lines(data, 0, n, open, [&](uint8_t kind, size_t off, size_t len) {
        return join_line(partial, kind, data + off, len, [&](const char* b, size_t blen, std::string*) {
            if (blen == 0 || blank(b, blen)) return true;
            PyObject* t = decode_line(self, b, blen);
            if (!t) return false;
            int r = PyList_Append(out, t);
            Py_DECREF(t);
            return r == 0;
        });
    });
}

PyObject* Decoder_feed(DecoderObject* self, PyObject* arg) {
    Py_buffer view;
    if (PyObject_GetBuffer(arg, &view, PyBUF_SIMPLE) < 0) return nullptr;
    self->n_bytes += (long long)view.len;
    PyObject* out = PyList_New(0);
    if (out && !process_segment(self, (const char*)view.buf, (size_t)view.len, out)) {
        Py_DECREF(out);
        out = nullptr;
    }
    PyBuffer_Release(&view);
    return out;
}

// HTTP/1.1 chunked transfer framing, decoded in place of the Python parser
// for the watch stream (chunked.inc).

// A framing error as the decoder's and the pipeline's ValueError (a size line
// that is not UTF-8 shows with replacement characters).
void set_chunk_error(const ChunkState& st, ChunkEnd e) {
    if (e == CE_TOO_LONG) PyErr_SetString(PyExc_ValueError, "chunk size line too long");
    else PyErr_Format(PyExc_ValueError, "bad chunk size line %.40s", st.line.c_str());
}

PyObject* Decoder_feed_chunked(DecoderObject* self, PyObject* arg) {
    Py_buffer view;
    if (PyObject_GetBuffer(arg, &view, PyBUF_SIMPLE) < 0) return nullptr;
    const char* data = (const char*)view.buf;
    size_t n = (size_t)view.len;
    self->n_bytes += (long long)n;
    PyObject* out = PyList_New(0);
    if (!out) {
        PyBuffer_Release(&view);
        return nullptr;
    }
    bool ok = true;  // false: a Python error is set
    size_t at;
    const ChunkEnd end = chunk_deframe(self->chunk, data, 0, n, at, [&](size_t off, size_t len) {
        return ok = process_segment(self, data + off, len, out);
    });
    if (end == CE_TOO_LONG || end == CE_BAD_SIZE) {
        set_chunk_error(self->chunk, end);
        ok = false;
    }
    PyBuffer_Release(&view);
    if (!ok) {
        Py_DECREF(out);
        return nullptr;
    }
    return out;
}

PyObject* Decoder_body_done(DecoderObject* self, PyObject*) {
    return PyBool_FromLong(self->chunk.done());
}

PyObject* Decoder_reset(DecoderObject* self, PyObject*) {
    self->partial->clear();
    self->chunk = ChunkState();
    Py_RETURN_NONE;
}

// decode_list(body) -> (resourceVersion, continue, [ADDED tuples])
PyObject* Decoder_decode_list(DecoderObject* self, PyObject* arg) {
    Py_buffer view;
    if (PyObject_GetBuffer(arg, &view, PyBUF_SIMPLE) < 0) return nullptr;
    const char* b = (const char*)view.buf;
    size_t n = (size_t)view.len;
    if (self->validate == 2) {
        if (const char* why = json_invalid(b, n)) {
            PyBuffer_Release(&view);
            PyErr_Format(PyExc_ValueError, "invalid list body: %s", why);
            return nullptr;
        }
    }
    PyObject* items = PyList_New(0);
    Span rv, cont;
    bool failed = false;
    try {
        Parser P(b, b + n);
        P.object([&](const char* k, size_t kn) {
            if (KEYIS("metadata")) {
                rv = cont = Span();  // a repeated key: the last one counts, as json.loads
                if (P.null_here()) return;
                if (P.peek() != '{') throw ParseError{"metadata is not an object"};
                P.object([&](const char* k2, size_t kn2) {
                    const char* k = k2; size_t kn = kn2;
                    if (KEYIS("resourceVersion")) rv = P.value();
                    else if (KEYIS("continue")) cont = P.value();
                    else P.value();
                });
            } else if (KEYIS("items")) {
                if (PyList_GET_SIZE(items) && PyList_SetSlice(items, 0, PyList_GET_SIZE(items), nullptr) < 0)
                    failed = true;  // (a repeated key: the last list is the list)
                if (P.null_here()) return;
                if (P.peek() != '[') throw ParseError{"items is not an array"};
                P.array([&]() {
                    if (failed) { P.value(); return; }
                    if (P.peek() != '{') { P.value(); return; }
                    self->spans->clear();
                    const char* start = P.p_;
                    parse_pod(P, *self->spans);
                    Span obj;
                    obj.p = start;
                    obj.n = (size_t)(P.p_ - start);
                    PyObject* t = event_tuple(self, T_ADDED, g_types[T_ADDED], obj);
                    if (!t || PyList_Append(items, t) < 0) failed = true;
                    Py_XDECREF(t);
                    self->n_events++;
                });
            } else {
                P.value();
            }
        });
        P.ws();
        if (P.p_ != P.end_) throw ParseError{"trailing data"};
    } catch (const ParseError& e) {
        PyBuffer_Release(&view);
        Py_DECREF(items);
        PyErr_Format(PyExc_ValueError, "invalid list body: %s", e.msg);
        return nullptr;
    }
    PyBuffer_Release(&view);
    if (failed) {
        Py_DECREF(items);
        return nullptr;
    }
    PyObject* rvo = span_to_str(rv);
    PyObject* co = span_to_str(cont);
    if (co && PyUnicode_Check(co) && PyUnicode_GET_LENGTH(co) == 0) {
        Py_DECREF(co);
        Py_INCREF(Py_None);
        co = Py_None;
    }
    PyObject* res = Py_BuildValue("(NNN)", rvo, co, items);
    return res;
}

PyObject* Decoder_core(DecoderObject*, PyObject* ev) {
    if (!PyTuple_Check(ev) || PyTuple_GET_SIZE(ev) < 8) {
        PyErr_SetString(PyExc_TypeError, "expected an event tuple");
        return nullptr;
    }
    PyObject* c = PyTuple_GET_ITEM(ev, 7);
    Py_INCREF(c);
    return c;
}

// core_from_summary(uid, ns, name, phase) -> bytes: payload core for a pod
// known only from the cache (synthesised DELETED after a relist).
PyObject* Decoder_core_from_summary(DecoderObject* self, PyObject* args) {
    PyObject *uid, *ns, *name, *phase;
    if (!PyArg_ParseTuple(args, "OOOO", &uid, &ns, &name, &phase)) return nullptr;
    PyObject* mod = PyImport_ImportModule("json");
    if (!mod) return nullptr;
    PyObject* dumps = PyObject_GetAttrString(mod, "dumps");
    Py_DECREF(mod);
    if (!dumps) return nullptr;
    std::string buf[4];
    PyObject* vals[4] = {uid, ns, name, phase};
    for (int i = 0; i < 4; ++i) {
        PyObject* kw = Py_BuildValue("{s:O}", "ensure_ascii", Py_False);
        PyObject* a = PyTuple_Pack(1, vals[i]);
        PyObject* r = (kw && a) ? PyObject_Call(dumps, a, kw) : nullptr;
        Py_XDECREF(kw);
        Py_XDECREF(a);
        if (!r) {
            Py_DECREF(dumps);
            return nullptr;
        }
        Py_ssize_t ln;
        const char* s = PyUnicode_AsUTF8AndSize(r, &ln);
        buf[i].assign(s, (size_t)ln);
        Py_DECREF(r);
    }
    Py_DECREF(dumps);
    PodSpans S;
    S.meta_present = true;
    S.uid = Span{buf[0].data(), buf[0].size()};
    S.ns = Span{buf[1].data(), buf[1].size()};
    S.name = Span{buf[2].data(), buf[2].size()};
    if (phase != Py_None) {
        S.status_present = true;
        S.phase = Span{buf[3].data(), buf[3].size()};
    }
    build_core(*self->out, S, *self->env_json, self->extra);
    return PyBytes_FromStringAndSize(self->out->data(), (Py_ssize_t)self->out->size());
}

// set_repr(tz_utc_repr, fallback): python_repr details (engine/pipeline.py::repr_settings)
PyObject* Decoder_set_repr(DecoderObject* self, PyObject* args) {
    const char* tz;
    PyObject* fn;
    if (!PyArg_ParseTuple(args, "sO", &tz, &fn)) return nullptr;
    if (!self->tz_utc) {
        PyErr_SetString(PyExc_ValueError, "set_repr: the decoder is not in python_repr mode");
        return nullptr;
    }
    *self->tz_utc = tz;
    Py_INCREF(fn);
    Py_XSETREF(self->repr_fallback, fn);
    Py_RETURN_NONE;
}

PyObject* Decoder_set_validate(DecoderObject* self, PyObject* arg) {
    long v = PyLong_AsLong(arg);
    if (PyErr_Occurred()) return nullptr;
    if (v < 0 || v > 2) {
        PyErr_SetString(PyExc_ValueError, "validate mode must be 0, 1 or 2");
        return nullptr;
    }
    self->validate = (int)v;
    Py_RETURN_NONE;
}

PyObject* Decoder_set_extra(DecoderObject* self, PyObject* arg) {
    self->extra = (int)PyLong_AsLong(arg);
    if (PyErr_Occurred()) return nullptr;
    Py_RETURN_NONE;
}

// An iterable of str -> ReasonSet; false with the error set.
bool reason_set_from(PyObject* arg, ReasonSet& out) {
    out.clear();
    PyObject* it = PyObject_GetIter(arg);
    if (!it) return false;
    PyObject* item;
    while ((item = PyIter_Next(it))) {
        Py_ssize_t n;
        const char* u = PyUnicode_Check(item) ? PyUnicode_AsUTF8AndSize(item, &n) : nullptr;
        if (u) out.emplace_back(u, (size_t)n);
        else if (!PyErr_Occurred()) PyErr_SetString(PyExc_TypeError, "failure reasons must be strings");
        Py_DECREF(item);
        if (!u) break;
    }
    Py_DECREF(it);
    return !PyErr_Occurred();
}

// set_container_failures(on, reasons | None): watcher.alerts.container_failures
// (pod events get the failure signature as a tenth field) and
// container_failure_reasons (None keeps the set; the extra field uses it too)
PyObject* Decoder_set_container_failures(DecoderObject* self, PyObject* args) {
    int on;
    PyObject* reasons = Py_None;
    if (!PyArg_ParseTuple(args, "p|O", &on, &reasons)) return nullptr;
    if (reasons != Py_None) {
        ReasonSet set;
        if (!reason_set_from(reasons, set)) return nullptr;
        *self->reasons = std::move(set);
    }
    self->failures = on;
    Py_RETURN_NONE;
}

// An iterable of (type, status, reason | None) -> CondRules; false with the
// error set. The rule strings are parsed in one place, models/findings.py.
bool cond_rules_from(PyObject* arg, CondRules& out) {
    out.clear();
    PyObject* it = PyObject_GetIter(arg);
    if (!it) return false;
    PyObject* item;
    while ((item = PyIter_Next(it))) {
        const char *t = nullptr, *s = nullptr, *r = nullptr;
        Py_ssize_t tn = 0, sn = 0, rn = 0;
        const bool ok = PyTuple_Check(item) && PyArg_ParseTuple(item, "s#s#z#", &t, &tn, &s, &sn, &r, &rn);
        if (ok) {
            CondRule rule;
            rule.type.assign(t, (size_t)tn);
            rule.status.assign(s, (size_t)sn);
            rule.any_reason = r == nullptr;
            if (r) rule.reason.assign(r, (size_t)rn);
            out.push_back(std::move(rule));
        } else if (!PyErr_Occurred()) {
            PyErr_SetString(PyExc_TypeError, "condition rules must be (type, status, reason or None) tuples");
        }
        Py_DECREF(item);
        if (!ok) break;
    }
    Py_DECREF(it);
    if (!PyErr_Occurred() && out.size() > MAX_COND_RULES) PyErr_SetString(PyExc_ValueError, "at most 32 condition rules");
    return !PyErr_Occurred();
}

// set_pod_conditions(on, rules | None): watcher.alerts.pod_conditions (pod
// events get the condition signature as an eleventh field) and
// pod_condition_rules (None keeps the set; the extra field uses it too)
PyObject* Decoder_set_pod_conditions(DecoderObject* self, PyObject* args) {
    int on;
    PyObject* rules = Py_None;
    if (!PyArg_ParseTuple(args, "p|O", &on, &rules)) return nullptr;
    if (rules != Py_None) {
        CondRules set;
        if (!cond_rules_from(rules, set)) return nullptr;
        *self->rules = std::move(set);
    }
    self->conditions = on;
    Py_RETURN_NONE;
}

// set_terminating(on): watcher.alerts.terminating (pod events get the
// terminating signature, 1 or 0, as a twelfth field)
PyObject* Decoder_set_terminating(DecoderObject* self, PyObject* arg) {
    const int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    self->terminating = on != 0;
    Py_RETURN_NONE;
}

// set_deadlines(on): watcher.alerts.terminating_overdue_seconds > 0 (with
// terminating on, pod events get the deletion deadline as a thirteenth field)
PyObject* Decoder_set_deadlines(DecoderObject* self, PyObject* arg) {
    const int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    self->deadlines = on != 0;
    Py_RETURN_NONE;
}

// set_pending(on): watcher.alerts.pending_overdue_seconds > 0 (pod events get
// the pending-since as a fourteenth field)
PyObject* Decoder_set_pending(DecoderObject* self, PyObject* arg) {
    const int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    self->pending = on != 0;
    Py_RETURN_NONE;
}

// set_unready(on): watcher.alerts.unready_overdue_seconds > 0 (pod events get
// the unready-since as a fifteenth field)
PyObject* Decoder_set_unready(DecoderObject* self, PyObject* arg) {
    const int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    self->unready = on != 0;
    Py_RETURN_NONE;
}

PyObject* Decoder_stats(DecoderObject* self, PyObject*) {
    return Py_BuildValue("{s:L,s:L}", "events", self->n_events, "bytes", self->n_bytes);
}

PyMethodDef Decoder_methods[] = {
    {"set_extra", (PyCFunction)Decoder_set_extra, METH_O, "set_extra(mask): watcher.payload_extra_fields"},
    {"set_validate", (PyCFunction)Decoder_set_validate, METH_O, "set_validate(0 off | 1 payload | 2 full)"},
    {"set_container_failures", (PyCFunction)Decoder_set_container_failures, METH_VARARGS,
     "set_container_failures(on, reasons=None): watcher.alerts.container_failures / container_failure_reasons"},
    {"set_pod_conditions", (PyCFunction)Decoder_set_pod_conditions, METH_VARARGS,
     "set_pod_conditions(on, rules=None): watcher.alerts.pod_conditions / pod_condition_rules"},
    {"set_terminating", (PyCFunction)Decoder_set_terminating, METH_O, "set_terminating(on): watcher.alerts.terminating"},
    {"set_deadlines", (PyCFunction)Decoder_set_deadlines, METH_O,
     "set_deadlines(on): watcher.alerts.terminating_overdue_seconds > 0"},
    {"set_pending", (PyCFunction)Decoder_set_pending, METH_O,
     "set_pending(on): watcher.alerts.pending_overdue_seconds > 0"},
    {"set_unready", (PyCFunction)Decoder_set_unready, METH_O,
     "set_unready(on): watcher.alerts.unready_overdue_seconds > 0"},
    {"set_repr", (PyCFunction)Decoder_set_repr, METH_VARARGS, "set_repr(tz_utc_repr, fallback): python_repr"},
    {"feed", (PyCFunction)Decoder_feed, METH_O, "feed(bytes) -> list of event tuples"},
    {"feed_chunked", (PyCFunction)Decoder_feed_chunked, METH_O,
     "feed_chunked(bytes) -> events; input keeps its HTTP chunked framing"},
    {"body_done", (PyCFunction)Decoder_body_done, METH_NOARGS, "True after the terminating 0-size chunk"},
    {"reset", (PyCFunction)Decoder_reset, METH_NOARGS, "drop partial line and chunk state"},
    {"decode_list", (PyCFunction)Decoder_decode_list, METH_O, "decode_list(body) -> (rv, continue, events)"},
    {"core", (PyCFunction)Decoder_core, METH_O, "core(event) -> payload core bytes"},
    {"core_from_summary", (PyCFunction)Decoder_core_from_summary, METH_VARARGS,
     "core_from_summary(uid, ns, name, phase) -> bytes"},
    {"stats", (PyCFunction)Decoder_stats, METH_NOARGS, "counters"},
    {nullptr, nullptr, 0, nullptr}};

PyTypeObject DecoderType = {PyVarObject_HEAD_INIT(nullptr, 0)};

// ----------------------------------------------------------------------------- ResponseScanner
//
// HTTP/1.1 response framing for the clusterapi notifier pool: one feed() per
// socket read returns every complete response in it. A 2xx keep-alive
// response is returned as its int status (no allocation); anything else as
// (status, keep_alive, body, retry_after) so the pool can log / close. Handles
// Content-Length, chunked bodies, 204/304 and read-until-close framing; interim
// 1xx responses are consumed and not returned, and after a response that
// closes the connection nothing more is returned until reset().

struct ScannerObject {
    PyObject_HEAD
    std::string* buf;
    size_t pos;
    bool closed;  // a response that closes the connection was reported: nothing more until reset()
};

bool ieq_prefix(const char* p, const char* e, const char* lit) {
    size_t n = std::strlen(lit);
    if ((size_t)(e - p) < n) return false;
    for (size_t i = 0; i < n; ++i) {
        char c = p[i];
        if (c >= 'A' && c <= 'Z') c = (char)(c - 'A' + 'a');
        if (c != lit[i]) return false;
    }
    return true;
}

bool contains_token_ci(const char* p, const char* e, const char* tok) {
    size_t n = std::strlen(tok);
    for (const char* q = p; q + n <= e; ++q)
        if (ieq_prefix(q, e, tok)) return true;
    return false;
}

bool ieq_name(const char* p, const char* e, const char* lit) {
    return (size_t)(e - p) == std::strlen(lit) && ieq_prefix(p, e, lit);
}

// Retry-After (docs/DEVIATIONS.md "Hostile clusterapi responses", P5):
// [blanks] 1*DIGIT ["." *DIGIT] [blanks] seconds, capped at 300 s, rounded as
// Python's float() rounds it; -1 for anything else (an HTTP-date, a sign, an
// exponent, inf, nan: the pool's own backoff then).
double parse_retry_after(const char* v, const char* e) {
    while (v < e && (*v == ' ' || *v == '\t')) ++v;
    while (e > v && (e[-1] == ' ' || e[-1] == '\t')) --e;
    if (v >= e || !is_digit(*v)) return -1.0;
    const char* q = v;
    while (q < e && is_digit(*q)) ++q;
    const char* int_end = q;
    if (q < e && *q == '.')
        for (++q; q < e && is_digit(*q); ++q) {
        }
    if (q != e) return -1.0;
    double secs = 0.0;
    const auto r = std::from_chars(v, e, secs, std::chars_format::fixed);
    if (r.ec == std::errc::result_out_of_range) {  // too large, or a fraction too small for a double
        while (v < int_end && *v == '0') ++v;
        return v < int_end ? 300.0 : 0.0;
    }
    if (r.ec != std::errc()) return -1.0;
    return secs > 300.0 ? 300.0 : secs;
}

// Try to parse one complete response at b[0..n). Returns bytes consumed (0 =
// incomplete, SIZE_MAX = malformed); fills status, keep_alive, body span and
// retry_after (seconds, -1 = no usable Retry-After header). An interim
// response (1xx but 101) is returned like any other: the caller reports it
// to nobody. What is malformed is listed in docs/DEVIATIONS.md, "Hostile
// clusterapi responses"; net/http.py's ResponseParser follows the same list.
const size_t MAX_HEAD = 65536;  // status line + headers + blank line

size_t scan_response(const char* b, size_t n, int& status, bool& keep_alive, std::string& body,
                     bool& until_close, double& retry_after) {
    const char* e = b + n;
    const size_t incomplete = n >= MAX_HEAD ? SIZE_MAX : 0;  // a head still open after 64 KiB is malformed
    bool http10 = false;
    long long clen = -1;
    retry_after = -1.0;
    int n_retry_after = 0;
    bool chunked = false, conn_close = false, conn_keep = false;
    // One pass over the head, line by line, up to the blank line. A fault in a
    // line is reported when the line is here, the rest of the head or not.
    const char* he = nullptr;  // the CR that ends the last header line
    for (const char* ls = b; !he;) {
        const char* le = (const char*)std::memchr(ls, '\r', (size_t)(e - ls));
        if (!le || le + 1 >= e) return incomplete;
        if (le[1] != '\n' || std::memchr(ls, '\n', (size_t)(le - ls))) return SIZE_MAX;  // bare CR / bare LF
        if (ls == b) {
            // status line: HTTP/1.0 or HTTP/1.1, SP, exactly three digits, SP or CRLF
            if (le - b < 12 || std::memcmp(b, "HTTP/1.", 7) != 0 || (b[7] != '0' && b[7] != '1') || b[8] != ' ')
                return SIZE_MAX;
            http10 = b[7] == '0';
            status = 0;
            for (int i = 9; i < 12; ++i) {
                if (!is_digit(b[i])) return SIZE_MAX;
                status = status * 10 + (b[i] - '0');
            }
            if (le - b > 12 && b[12] != ' ') return SIZE_MAX;
            if (status < 100 || status == 101) return SIZE_MAX;  // 101: nothing here ever asks to switch protocols
        } else {
            if (*ls == ' ' || *ls == '\t') return SIZE_MAX;  // blank in front of the name (obs-fold)
            const char* colon = (const char*)std::memchr(ls, ':', (size_t)(le - ls));
            if (colon) {
                if (colon > ls && (colon[-1] == ' ' || colon[-1] == '\t')) return SIZE_MAX;
                const char* v = colon + 1;
                if (ieq_name(ls, colon, "content-length")) {
                    const char* ve = le;
                    while (v < ve && (*v == ' ' || *v == '\t')) ++v;
                    while (ve > v && (ve[-1] == ' ' || ve[-1] == '\t')) --ve;
                    if (clen >= 0 || v == ve) return SIZE_MAX;  // repeated, or empty
                    clen = 0;
                    for (; v < ve; ++v) {
                        if (!is_digit(*v) || clen > (INT64_MAX - (*v - '0')) / 10) return SIZE_MAX;
                        clen = clen * 10 + (*v - '0');
                    }
                } else if (ieq_name(ls, colon, "transfer-encoding")) {
                    chunked |= contains_token_ci(v, le, "chunked");
                } else if (ieq_name(ls, colon, "connection")) {
                    conn_close |= contains_token_ci(v, le, "close");
                    conn_keep |= contains_token_ci(v, le, "keep-alive");
                } else if (ieq_name(ls, colon, "retry-after")) {
                    retry_after = ++n_retry_after == 1 ? parse_retry_after(v, le) : -1.0;
                }
            }
        }
        ls = le + 2;
        if (ls >= e) return incomplete;
        if (*ls == '\r') {  // the blank line, or a bare CR
            if (ls + 1 >= e) return incomplete;
            if (ls[1] != '\n') return SIZE_MAX;
            he = le;
        }
    }
    if ((size_t)(he + 4 - b) > MAX_HEAD) return SIZE_MAX;
    keep_alive = http10 ? (conn_keep && !conn_close) : !conn_close;
    const char* bs = he + 4;
    body.clear();
    until_close = false;
    if (status < 200 || status == 204 || status == 304) return (size_t)(bs - b);
    if (chunked) {
        const char* q = bs;
        while (true) {
            const char* nl = (const char*)std::memchr(q, '\n', (size_t)(e - q));
            if (!nl) return 0;
            if (nl == q || nl[-1] != '\r') return SIZE_MAX;  // bare LF
            size_t sz = 0;
            if (!parse_chunk_size(q, (size_t)(nl - 1 - q), sz, false) || sz > (size_t)INT64_MAX) return SIZE_MAX;
            q = nl + 1;
            if (sz == 0) {
                while (true) {  // trailers up to the empty line
                    const char* t = (const char*)std::memchr(q, '\n', (size_t)(e - q));
                    if (!t) return 0;
                    if (t == q || t[-1] != '\r') return SIZE_MAX;
                    const bool empty = t == q + 1;
                    q = t + 1;
                    if (empty) return (size_t)(q - b);
                }
            }
            if ((size_t)(e - q) < sz + 2) return 0;  // sz < 2^63: no wrap
            if (q[sz] != '\r' || q[sz + 1] != '\n') return SIZE_MAX;
            body.append(q, sz);
            q += sz + 2;
        }
    }
    if (clen >= 0) {
        if ((size_t)(e - bs) < (size_t)clen) return 0;
        body.assign(bs, (size_t)clen);
        return (size_t)(bs - b) + (size_t)clen;
    }
    // no framing: body runs to EOF; report what is here and let the caller close
    until_close = true;
    keep_alive = false;
    body.assign(bs, (size_t)(e - bs));
    return n;
}

PyObject* Scanner_new(PyTypeObject* type, PyObject*, PyObject*) {
    ScannerObject* self = (ScannerObject*)type->tp_alloc(type, 0);
    if (!self) return nullptr;
    self->buf = new std::string();
    self->pos = 0;
    self->closed = false;
    return (PyObject*)self;
}

void Scanner_dealloc(ScannerObject* self) {
    delete self->buf;
    Py_TYPE(self)->tp_free((PyObject*)self);
}

PyObject* Scanner_feed(ScannerObject* self, PyObject* arg) {
    Py_buffer view;
    if (PyObject_GetBuffer(arg, &view, PyBUF_SIMPLE) < 0) return nullptr;
    if (self->closed) {  // what follows a closing response is not a response
        PyBuffer_Release(&view);
        return PyList_New(0);
    }
    std::string& buf = *self->buf;
    const char* data;
    size_t n;
    bool direct = buf.empty();
    if (direct) {
        data = (const char*)view.buf;
        n = (size_t)view.len;
    } else {
        buf.append((const char*)view.buf, (size_t)view.len);
        data = buf.data();
        n = buf.size();
    }
    PyObject* out = PyList_New(0);
    std::string body;
    size_t pos = 0;
    bool ok = out != nullptr;
    while (ok && pos < n) {
        int status = 0;
        bool keep = true, until_close = false;
        double retry_after = -1.0;
        size_t used = scan_response(data + pos, n - pos, status, keep, body, until_close, retry_after);
        if (used == 0) break;
        if (used == SIZE_MAX) {
            PyErr_SetString(PyExc_ValueError, "malformed HTTP response");
            ok = false;
            break;
        }
        pos += used;
        if (status < 200) continue;  // interim (100, 102, 103): belongs to no request
        PyObject* item;
        if (status >= 200 && status < 300 && keep) {
            item = PyLong_FromLong(status);
        } else {
            item = Py_BuildValue("(iOy#d)", status, keep ? Py_True : Py_False, body.data(),
                                 (Py_ssize_t)body.size(), retry_after);
        }
        if (!item || PyList_Append(out, item) < 0) ok = false;
        Py_XDECREF(item);
        if (!keep) {
            self->closed = true;
            pos = n;
            break;
        }
    }
    if (ok) {
        if (direct) {
            if (pos < n) buf.assign(data + pos, n - pos);
        } else {
            buf.erase(0, pos);
        }
    }
    PyBuffer_Release(&view);
    if (!ok) {
        Py_XDECREF(out);
        return nullptr;
    }
    return out;
}

PyObject* Scanner_reset(ScannerObject* self, PyObject*) {
    self->buf->clear();
    self->closed = false;
    Py_RETURN_NONE;
}

PyObject* Scanner_pending(ScannerObject* self, PyObject*) {
    return PyLong_FromSize_t(self->buf->size());
}

PyMethodDef Scanner_methods[] = {
    {"feed", (PyCFunction)Scanner_feed, METH_O,
     "feed(bytes) -> [status | (status, keep_alive, body)] for each complete response"},
    {"reset", (PyCFunction)Scanner_reset, METH_NOARGS, "drop buffered bytes"},
    {"pending", (PyCFunction)Scanner_pending, METH_NOARGS, "buffered byte count"},
    {nullptr, nullptr, 0, nullptr}};

PyTypeObject ScannerType = {PyVarObject_HEAD_INIT(nullptr, 0)};

// format_event_timestamp(utc: bool) -> str: datetime.now().isoformat() equivalent
// stamp_fields(buf, rv_off, rvs, ndigits, uid_off, uid_text): benchmark
// fixtures (testing/cluster_replay.py) re-stamp a prerendered watch stream per
// step — rvs[i] as ndigits zero-padded decimal digits at buf[rv_off[i]], and
// uid_text at every buf[uid_off[j]] — bounds-checked, in place. The numpy
// version of this was most of the fixture's time at ~1.5M events/s.
PyObject* kw_stamp_fields(PyObject*, PyObject* args) {
    Py_buffer buf, rvo, rvs, uo;
    int nd;
    const char* ut;
    Py_ssize_t un;
    if (!PyArg_ParseTuple(args, "w*y*y*iy*y#", &buf, &rvo, &rvs, &nd, &uo, &ut, &un)) return nullptr;
    bool ok = rvo.len == rvs.len && rvo.len % 8 == 0 && uo.len % 8 == 0 && nd > 0 && nd <= 19;
    const int64_t* ro = (const int64_t*)rvo.buf;
    const int64_t* rv = (const int64_t*)rvs.buf;
    const int64_t* uof = (const int64_t*)uo.buf;
    const size_t n = (size_t)rvo.len / 8, m = (size_t)uo.len / 8, blen = (size_t)buf.len;
    char* b = (char*)buf.buf;
    for (size_t i = 0; ok && i < n; ++i) {
        if (ro[i] < 0 || (size_t)ro[i] + (size_t)nd > blen || rv[i] < 0) {
            ok = false;
            break;
        }
        int64_t v = rv[i];
        for (int d = nd - 1; d >= 0; --d) {
            b[ro[i] + d] = (char)('0' + v % 10);
            v /= 10;
        }
    }
    for (size_t j = 0; ok && j < m; ++j) {
        if (uof[j] < 0 || (size_t)uof[j] + (size_t)un > blen) {
            ok = false;
            break;
        }
        std::memcpy(b + uof[j], ut, (size_t)un);
    }
    PyBuffer_Release(&buf);
    PyBuffer_Release(&rvo);
    PyBuffer_Release(&rvs);
    PyBuffer_Release(&uo);
    if (!ok) {
        PyErr_SetString(PyExc_ValueError, "stamp_fields: offsets out of range or arrays mismatched");
        return nullptr;
    }
    Py_RETURN_NONE;
}

PyObject* kw_event_timestamp(PyObject*, PyObject* arg) {
    int utc = PyObject_IsTrue(arg);
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    struct tm tmv;
    time_t secs = ts.tv_sec;
    if (utc) gmtime_r(&secs, &tmv); else localtime_r(&secs, &tmv);
    long micro = ts.tv_nsec / 1000;
    char buf[64];
    int n = std::snprintf(buf, sizeof buf, "%04d-%02d-%02dT%02d:%02d:%02d", tmv.tm_year + 1900, tmv.tm_mon + 1,
                          tmv.tm_mday, tmv.tm_hour, tmv.tm_min, tmv.tm_sec);
    if (micro) n += std::snprintf(buf + n, sizeof buf - n, ".%06ld", micro);
    if (utc) n += std::snprintf(buf + n, sizeof buf - n, "+00:00");
    return PyUnicode_FromStringAndSize(buf, n);
}

PyObject* kw_cpu_features(PyObject*, PyObject*) {
#if defined(__x86_64__)
    return Py_BuildValue("{s:O,s:O}", "avx2", Parser::use_avx2 ? Py_True : Py_False, "avx512",
                         Parser::use_avx512 ? Py_True : Py_False);
#else
    return Py_BuildValue("{s:O,s:O}", "avx2", Py_False, "avx512", Py_False);
#endif
}

// set_simd(True) = best supported level, False = scalar, "avx2" = cap at AVX2.
PyObject* kw_set_simd(PyObject*, PyObject* arg) {
#if defined(__x86_64__)
    bool cap_avx2 = PyUnicode_Check(arg) && PyUnicode_CompareWithASCIIString(arg, "avx2") == 0;
    int on = PyObject_IsTrue(arg);
    if (on < 0) return nullptr;
    Parser::use_avx2 = on && simd_supported();
    Parser::use_avx512 = on && !cap_avx2 && avx512_supported();
#endif
    Py_RETURN_NONE;
}

// bench_parse(data, mode, repeat) -> seconds. Times the pure C++ stages on
// newline-separated lines without creating Python objects:
// mode 0 = structural skip of each line, 1 = field extraction (spans),
// 2 = extraction + payload core assembly, 3 = filter-first light extraction,
// 4 = light extraction + materialize + core assembly.
PyObject* kw_bench_parse(PyObject*, PyObject* args) {
    Py_buffer view;
    int mode = 2, repeat = 1;
    if (!PyArg_ParseTuple(args, "y*|ii", &view, &mode, &repeat)) return nullptr;
    const char* b = (const char*)view.buf;
    const char* e = b + view.len;
    std::vector<std::pair<const char*, const char*>> lines;
    for (const char* p = b; p < e;) {
        const char* nl = (const char*)std::memchr(p, '\n', (size_t)(e - p));
        if (!nl) nl = e;
        if (nl > p) lines.emplace_back(p, nl);
        p = nl + 1;
    }
    PodSpans S;
    std::string out;
    out.reserve(8192);
    std::string env = "\"production\"";
    size_t sink = 0;
    struct timespec t0, t1;
    clock_gettime(CLOCK_MONOTONIC, &t0);
    try {
        for (int r = 0; r < repeat; ++r) {
            for (auto& ln : lines) {
                Parser P(ln.first, ln.second);
                if (mode == 0) {
                    sink += (size_t)(P.value().n);
                    continue;
                }
                S.clear();
                const bool light = mode >= 3;
                P.object([&](const char* k, size_t kn) {
                    if (KEYIS("object")) {
                        if (light) parse_pod_light(P, S); else parse_pod(P, S);
                    } else {
                        P.value();
                    }
                });
                if (mode == 2 || mode == 4 || mode == 5) {
                    static const std::string tz_utc = "tzutc()";
                    materialize(S);
                    build_core(out, S, env, 0, mode == 5 ? &tz_utc : nullptr);  // 5: state_format python_repr
                    sink += out.size();
                } else {
                    sink += S.name.n;
                }
            }
        }
    } catch (const ParseError& err) {
        PyBuffer_Release(&view);
        PyErr_SetString(PyExc_ValueError, err.msg);
        return nullptr;
    }
    clock_gettime(CLOCK_MONOTONIC, &t1);
    PyBuffer_Release(&view);
    double secs = (double)(t1.tv_sec - t0.tv_sec) + 1e-9 * (double)(t1.tv_nsec - t0.tv_nsec);
    return Py_BuildValue("(dn)", secs, (Py_ssize_t)sink);
}

#include "podstore.inc"
#include "podcache.inc"
#include "logsink.inc"
#include "engine.inc"
#include "checkpoint.inc"
#include "relist.inc"
#include "tls13.inc"
#include "readerhub.inc"
#include "sinkserver.inc"
#include "looplag.inc"

// json_invalid(data) -> None if json.loads(data) accepts it, else the reason (validate.inc)
PyObject* kw_json_invalid(PyObject*, PyObject* arg) {
    Py_buffer view;
    if (PyObject_GetBuffer(arg, &view, PyBUF_SIMPLE) < 0) return nullptr;
    const char* why = json_invalid((const char*)view.buf, (size_t)view.len);
    PyBuffer_Release(&view);
    if (!why) Py_RETURN_NONE;
    return PyUnicode_FromString(why);
}

// bench_validate(data, repeat) -> seconds: json_invalid over every line of data
PyObject* kw_bench_validate(PyObject*, PyObject* args) {
    Py_buffer view;
    int repeat = 1;
    if (!PyArg_ParseTuple(args, "y*|i", &view, &repeat)) return nullptr;
    const char* b = (const char*)view.buf;
    const char* e = b + view.len;
    std::vector<std::pair<const char*, size_t>> lines;
    for (const char* p = b; p < e;) {
        const char* nl = (const char*)std::memchr(p, '\n', (size_t)(e - p));
        if (!nl) nl = e;
        if (nl > p) lines.emplace_back(p, (size_t)(nl - p));
        p = nl + 1;
    }
    size_t bad = 0;
    const int64_t t0 = mono_ns();
    for (int r = 0; r < repeat; ++r)
        for (auto& ln : lines) bad += json_invalid(ln.first, ln.second) != nullptr;
    const int64_t t1 = mono_ns();
    PyBuffer_Release(&view);
    return Py_BuildValue("(dn)", (double)(t1 - t0) * 1e-9, (Py_ssize_t)bad);
}

// malloc_info() -> the C heap (glibc mallinfo2, every arena): bytes in use
// (small chunks + mmapped blocks), free inside the heap (retained, not
// returned to the kernel), and the arenas' size. Memory accounting for the
// watcher's RSS beyond the cache / owed notifications / read buffers.
PyObject* kw_malloc_info(PyObject*, PyObject*) {
    struct mallinfo2 mi = mallinfo2();
    return Py_BuildValue("{s:n,s:n,s:n,s:n}", "in_use_bytes", (Py_ssize_t)(mi.uordblks + mi.hblkhd), "free_bytes",
                         (Py_ssize_t)mi.fordblks, "arena_bytes", (Py_ssize_t)mi.arena, "mmap_bytes",
                         (Py_ssize_t)mi.hblkhd);
}

// malloc_arenas() -> [(arena, free_bytes, system_bytes)]: glibc's
// malloc_info() per arena (0 is the main arena, the event loop's; the others
// belong to native threads) — where the retained free bytes of the C heap sit
// (soak attribution: benchmarks/soak.py samples it).
PyObject* kw_malloc_arenas(PyObject*, PyObject*) {
    char* buf = nullptr;
    size_t len = 0;
    FILE* f = open_memstream(&buf, &len);
    if (!f) return PyErr_SetFromErrno(PyExc_OSError);
    malloc_info(0, f);
    std::fclose(f);
    std::string xml(buf ? buf : "", len);
    std::free(buf);
    PyObject* out = PyList_New(0);
    if (!out) return nullptr;
    auto attr = [](const std::string& x, size_t from, size_t to, const char* tag, const char* key) -> long long {
        const size_t t = x.find(tag, from);
        if (t == std::string::npos || t >= to) return 0;
        const size_t k = x.find(key, t);
        if (k == std::string::npos || k >= to) return 0;
        return std::atoll(x.c_str() + k + std::strlen(key));
    };
    size_t pos = 0;
    for (;;) {
        const size_t h = xml.find("<heap nr=\"", pos);
        if (h == std::string::npos) break;
        const size_t e = xml.find("</heap>", h);
        if (e == std::string::npos) break;
        const int nr = std::atoi(xml.c_str() + h + 10);
        const long long fr = attr(xml, h, e, "<total type=\"fast\"", "size=\"") +
                             attr(xml, h, e, "<total type=\"rest\"", "size=\"");
        const long long sys = attr(xml, h, e, "<system type=\"current\"", "size=\"");
        PyObject* t = Py_BuildValue("(iLL)", nr, fr, sys);
        if (!t || PyList_Append(out, t) < 0) {
            Py_XDECREF(t);
            Py_DECREF(out);
            return nullptr;
        }
        Py_DECREF(t);
        pos = e;
    }
    return out;
}

// malloc_trim() -> bool: give the C heap's free pages back to the kernel
// (every arena; the decode workers' arenas keep what their threads freed).
// Runs without the GIL: the service calls it from an executor thread.
PyObject* kw_malloc_trim(PyObject*, PyObject*) {
    int r;
    Py_BEGIN_ALLOW_THREADS
    r = malloc_trim(0);
    Py_END_ALLOW_THREADS
    return PyBool_FromLong(r);
}

// malloc_tune(mmap_threshold, trim_threshold) -> bool: fixed glibc thresholds.
// Left dynamic, glibc raises its mmap threshold to the size of every large
// block freed (up to 32 MiB), so after one 4 MiB read buffer or relist batch
// goes, later multi-MiB transients are carved from the arenas between
// long-lived chunks and what they free stays there as holes that neither
// trimming nor malloc_trim can return (round-5 soak: RSS +12 MiB, all of it
// retained free bytes). A fixed threshold keeps every block at or above it
// on its own mapping, unmapped when freed. Process-wide; call once at start.
PyObject* kw_malloc_tune(PyObject*, PyObject* args) {
    Py_ssize_t mmap_thr = 0, trim_thr = 0;
    if (!PyArg_ParseTuple(args, "nn", &mmap_thr, &trim_thr)) return nullptr;
    if (mmap_thr <= 0 || trim_thr <= 0 || mmap_thr > (Py_ssize_t)(32 << 20) || trim_thr > ((Py_ssize_t)1 << 30)) {
        PyErr_SetString(PyExc_ValueError, "malloc_tune: thresholds out of range");
        return nullptr;
    }
    const int a = mallopt(M_MMAP_THRESHOLD, (int)mmap_thr);
    const int b = mallopt(M_TRIM_THRESHOLD, (int)trim_thr);
    return PyBool_FromLong(a == 1 && b == 1);
}

PyMethodDef module_methods[] = {
    {"malloc_tune", (PyCFunction)kw_malloc_tune, METH_VARARGS,
     "malloc_tune(mmap_threshold, trim_threshold) -> ok (glibc mallopt; fixes both, disabling their sliding)"},
    {"malloc_trim", (PyCFunction)kw_malloc_trim, METH_NOARGS, "malloc_trim() -> released (glibc malloc_trim(0), no GIL)"},
    {"malloc_arenas", (PyCFunction)kw_malloc_arenas, METH_NOARGS,
     "malloc_arenas() -> [(arena, free_bytes, system_bytes)] (glibc malloc_info per arena)"},
    {"malloc_info", (PyCFunction)kw_malloc_info, METH_NOARGS,
     "malloc_info() -> {in_use_bytes, free_bytes, arena_bytes, mmap_bytes} (glibc mallinfo2)"},
    {"json_invalid", (PyCFunction)kw_json_invalid, METH_O, "json_invalid(data) -> None | reason (json.loads semantics)"},
    {"bench_validate", (PyCFunction)kw_bench_validate, METH_VARARGS, "bench_validate(lines, repeat) -> (seconds, invalid)"},
    {"bench_parse", (PyCFunction)kw_bench_parse, METH_VARARGS, "bench_parse(data, mode=2, repeat=1)"},
    {"event_timestamp", (PyCFunction)kw_event_timestamp, METH_O, "event_timestamp(utc) -> str"},
    {"stamp_fields", (PyCFunction)kw_stamp_fields, METH_VARARGS,
     "stamp_fields(buf, rv_off, rvs, ndigits, uid_off, uid_text): fixture re-stamping (int64 arrays)"},
    {"cpu_features", (PyCFunction)kw_cpu_features, METH_NOARGS, "SIMD paths in use"},
    {"set_simd", (PyCFunction)kw_set_simd, METH_O, "enable/disable the AVX2 scanner"},
    {"apply_stats", (PyCFunction)kw_apply_stats, METH_NOARGS,
     "apply_stats() -> cumulative counts of the partitioned and serial apply paths"},
    {"probe", (PyCFunction)kw_probe, METH_O, "probe(enable) -> event-loop thread time in native calls since the last call"},
    {"set_partitioned_apply", (PyCFunction)kw_set_partitioned_apply, METH_O,
     "set_partitioned_apply(on) -> previous: batches' apply phase split by pod-cache shard over the decode pool"},
    {"set_payload_prefilter", (PyCFunction)kw_set_payload_prefilter, METH_O,
     "set_payload_prefilter(on) -> previous: decode builds no payload for events the namespace or shard filter drops"},
    {"apply_partition", (PyCFunction)kw_apply_partition, METH_O,
     "apply_partition(uid) -> which of the partitioned apply's partitions takes the pod's lines"},
    {nullptr, nullptr, 0, nullptr}};

PyModuleDef moddef = {PyModuleDef_HEAD_INIT, "_kwcore", "native watch-event decoder", -1, module_methods};

}  // namespace

PyMODINIT_FUNC PyInit__kwcore(void) {
    DecoderType.tp_name = "_kwcore.StreamDecoder";
    DecoderType.tp_basicsize = sizeof(DecoderObject);
    DecoderType.tp_flags = Py_TPFLAGS_DEFAULT;
    DecoderType.tp_doc = "StreamDecoder(environment, state_format='structured')";
    DecoderType.tp_methods = Decoder_methods;
    DecoderType.tp_new = Decoder_new;
    DecoderType.tp_init = (initproc)Decoder_init;
    DecoderType.tp_dealloc = (destructor)Decoder_dealloc;
    if (PyType_Ready(&DecoderType) < 0) return nullptr;
    PyObject* m = PyModule_Create(&moddef);
    if (!m) return nullptr;
    Py_INCREF(&DecoderType);
    PyModule_AddObject(m, "StreamDecoder", (PyObject*)&DecoderType);
    ScannerType.tp_name = "_kwcore.ResponseScanner";
    ScannerType.tp_basicsize = sizeof(ScannerObject);
    ScannerType.tp_flags = Py_TPFLAGS_DEFAULT;
    ScannerType.tp_doc = "ResponseScanner(): incremental HTTP/1.1 response framing";
    ScannerType.tp_methods = Scanner_methods;
    ScannerType.tp_new = Scanner_new;
    ScannerType.tp_dealloc = (destructor)Scanner_dealloc;
    if (PyType_Ready(&ScannerType) < 0) return nullptr;
    Py_INCREF(&ScannerType);
    PyModule_AddObject(m, "ResponseScanner", (PyObject*)&ScannerType);
    if (register_engine(m) < 0 || register_podcache(m) < 0 || register_pipeline(m) < 0 || register_logsink(m) < 0 ||
        register_checkpoint(m) < 0 || register_relist(m) < 0 || register_readerhub(m) < 0 || register_tls13(m) < 0 || register_sinkserver(m) < 0 ||
        register_looplag(m) < 0)
        return nullptr;
    const char* names[6] = {"ADDED", "MODIFIED", "DELETED", "BOOKMARK", "ERROR", "INVALID"};
    for (int i = 0; i < 6; ++i) {
        g_types[i] = PyUnicode_InternFromString(names[i]);
        if (!g_types[i]) return nullptr;
    }
    PyObject* json = PyImport_ImportModule("json");
    if (!json) return nullptr;
    g_json_loads = PyObject_GetAttrString(json, "loads");
    Py_DECREF(json);
    if (!g_json_loads) return nullptr;
#if defined(__x86_64__)
    __builtin_cpu_init();
    Parser::use_avx2 = simd_supported();
    Parser::use_avx512 = avx512_supported();
#endif
    return m;
}
