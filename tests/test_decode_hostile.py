"""Both decode engines on hostile but valid JSON (docs/DEVIATIONS.md, "Hostile
but valid JSON"): lines ``json.loads`` accepts but that no Python dict spells
and no other fuzz here generates — containers of the wrong type, escaped
spellings of keys and values, repeated keys, lone surrogates, deep nesting,
timestamp look-alikes, numbers that underflow.

Every consumer with parsing code of its own sees every case: ``PyDecoder``
against ``NativeDecoder`` (``validate`` payload and full, every SIMD level),
the Python ``EventPipeline.handle_batch`` against the fused native
``handle_raw`` (production: the critical filter reads ``phase``; staging),
``decode_list`` in both engines and the native relist against the Python
reconcile. They must give the same type, identity fields, INVALID verdict,
parsed payload core and ``submit`` calls, and raise ``ValueError`` — nothing
else — exactly where the policy says so.
"""

import json
import random

import pytest
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from k8s_watcher_amd.engine.pipeline import EventPipeline
from k8s_watcher_amd.metrics import Metrics
from k8s_watcher_amd.ops.decode import INVALID, PyDecoder
from k8s_watcher_amd.ops.native import NativeDecoder, load

from k8s_watcher_amd.utils.config import load_settings

ENV = "production"
LEVELS = (True, "avx2", False)  # AVX-512 where the CPU has it, AVX2, the portable scanner
POD_TYPES = ("ADDED", "MODIFIED", "DELETED")
COUNTERS = ("events_received", "events_filtered_critical", "events_filtered_namespace", "bookmarks")


# ----------------------------------------------------------------------------- the consumers

class Recorder:
    def __init__(self):
        self.calls = []

    def submit(self, uid, et, ns, name, core, read_ns, ts):
        self.calls.append((uid, et, ns, name, core))

    def flush(self):
        pass


_SETTINGS = {}


def pipeline(env, validate, fmt, native):
    key = (env, validate, fmt)
    if key not in _SETTINGS:
        _SETTINGS[key] = load_settings(env, overrides={"watcher": {"validate": validate, "state_format": fmt}},
                                       environ={})
    rec = Recorder()
    p = EventPipeline(_SETTINGS[key], PyDecoder(env, fmt), rec, Metrics())
    p.log_events_setting = False
    if native:
        p.attach_native()
    return p, rec


def parsed(calls):
    return [c[:4] + (json.loads(c[4]),) for c in calls]


def outcome(p, rec, ctrl):
    return {"submits": parsed(rec.calls), "ctrl": [c[0] for c in ctrl], "last_rv": p.last_rv,
            "counters": {k: p.metrics.c[k] for k in COUNTERS}}


def python_answers(line, fmt):
    """What the Python engine says of one watch line: (decoder view, {env: pipeline view})."""
    data = line + b"\n"
    py = PyDecoder(ENV, fmt)
    evs = py.feed(data)
    view = [event_view(py, ev) for ev in evs]
    pipes = {}
    for env in ("production", "staging"):
        p, rec = pipeline(env, "payload", fmt, native=False)
        ctrl = p.handle_batch(PyDecoder(env, fmt).feed(data), 0)
        pipes[env] = outcome(p, rec, ctrl)
    return view, pipes


def event_view(dec, ev):
    """An event as both engines must report it: verdict, type, identity fields, the parsed core."""
    if ev[0] == INVALID:
        return (INVALID,)
    core = json.loads(dec.core(ev)) if ev[0] in POD_TYPES else None
    extra = ev[8] if ev[0] in ("BOOKMARK", "ERROR") else None
    return (ev[0], ev[1:7], core, extra)


def native_answers(line, fmt):
    """[(what, view)] for every native consumer at every SIMD level."""
    data = line + b"\n"
    mod = load()
    out = []
    try:
        for level in LEVELS:
            mod.set_simd(level)
            for validate in ("payload", "full"):
                nat = NativeDecoder(ENV, fmt, validate=validate)
                out.append((f"decoder {validate} simd={level}", [event_view(nat, ev) for ev in nat.feed(data)]))
                for env in ("production", "staging"):
                    p, rec = pipeline(env, validate, fmt, native=True)
                    ctrl = p.handle_raw(data, 0, framed=False)
                    out.append((f"pipeline {env} {validate} simd={level}", outcome(p, rec, ctrl)))
    finally:
        mod.set_simd(True)
    return out


def assert_engines_agree(line, fmt="structured"):
    """Every native consumer answers the watch line as the Python engine does; returns Python's view."""
    view, pipes = python_answers(line, fmt)
    # A state python_repr cannot render is found by the fused pipeline only when
    # it formats the payload, after the event was counted and its
    # resourceVersion kept; PyDecoder.feed says INVALID before the Python
    # pipeline sees an event. For such a line the two agree on what goes out.
    late = fmt == "python_repr" and view == [(INVALID,)]
    for what, got in native_answers(line, fmt):
        want = pipes[what.split()[1]] if what.startswith("pipeline") else view
        if late and what.startswith("pipeline"):
            got, want = [(o["submits"], o["ctrl"]) for o in (got, want)]
        assert got == want, (what, line[:300])
    return view, pipes


# ----------------------------------------------------------------------------- Test 1: the pinned corpus

MD = '"metadata":{"name":"a","namespace":"default","uid":"u1","resourceVersion":"7"}'
FAILED = '"status":{"phase":"Failed"}'


def ev(body, etype='"ADDED"'):
    return ('{"type":' + etype + ',"object":{' + body + "}}").encode("utf-8")


def md(extra):
    return MD[:-1] + "," + extra + "}"


END = "k8s.io/initial-events-end"

# id -> (line, event type both engines must report (or INVALID), {field: value} the answer must hold)
WATCH_ROWS = {
    # wrong container types read as absent
    "status-string": (ev(MD + ',"status":"x"'), "ADDED", {"has_status": False, "phase": "Unknown"}),
    "status-array": (ev(MD + ',"status":[1]'), "ADDED", {"has_status": False, "phase": "Unknown"}),
    "status-number": (ev(MD + ',"status":0'), "ADDED", {"has_status": False}),
    "status-dup-last-number": (ev(MD + "," + FAILED + ',"status":3'), "ADDED", {"has_status": False}),
    "status-dup-last-object": (ev(MD + ',"status":3,' + FAILED), "ADDED", {"has_status": True, "phase": "Failed"}),
    "status-dup-last-null": (ev(MD + "," + FAILED + ',"status":null'), "ADDED", {"has_status": False}),
    "spec-number": (ev(MD + ',"spec":5,' + FAILED), "ADDED", {"node_name": None}),
    "spec-string": (ev(MD + ',"spec":"x",' + FAILED), "ADDED", {"node_name": None}),
    "spec-dup": (ev(MD + ',"spec":{"nodeName":"n1"},"spec":[],' + FAILED), "ADDED", {"node_name": None}),
    "metadata-string": (ev('"metadata":"x",' + FAILED), "ADDED", {"name": None, "uid": None}),
    "metadata-array": (ev('"metadata":[{"name":"a"}],' + FAILED), "ADDED", {"name": None}),
    "metadata-dup-last-string": (ev(MD + ',"metadata":"x",' + FAILED), "ADDED", {"name": None}),
    "metadata-dup-last-object": (ev('"metadata":7,' + MD + "," + FAILED), "ADDED", {"name": "a", "uid": "u1"}),
    "conditions-mixed": (ev(MD + ',"status":{"phase":"Failed","conditions":[5,{"type":"Ready","status":"True"},"s",'
                                 'null,[{"type":"x"}]]}'), "ADDED", {"n_conditions": 1}),
    "conditions-string": (ev(MD + ',"status":{"phase":"Failed","conditions":"abc"}'), "ADDED", {"n_conditions": 0}),
    "conditions-object": (ev(MD + ',"status":{"phase":"Failed","conditions":{"a":1}}'), "ADDED", {"n_conditions": 0}),
    "conditions-dup": (ev(MD + ',"status":{"phase":"Failed","conditions":[{"type":"a"}],"conditions":7}'), "ADDED",
                       {"n_conditions": 0}),
    "cstatuses-array-of-strings": (ev(MD + ',"status":{"phase":"Failed","containerStatuses":["x"]}'), "ADDED",
                                   {"n_cstatuses": 0}),
    "cstatuses-string": (ev(MD + ',"status":{"phase":"Failed","containerStatuses":"x"}'), "ADDED", {"n_cstatuses": 0}),
    "cstatuses-mixed": (ev(MD + ',"status":{"phase":"Failed","containerStatuses":[1,{"name":"c","ready":true},[]]}'),
                        "ADDED", {"n_cstatuses": 1}),
    "containers-object": (ev(MD + ',"spec":{"containers":{"a":1}},' + FAILED), "ADDED", {"n_containers": 0}),
    "containers-null-element": (ev(MD + ',"spec":{"containers":[null,{"name":"c","image":"i"}]},' + FAILED), "ADDED",
                                {"n_containers": 1}),
    "containers-number": (ev(MD + ',"spec":{"nodeName":"n","containers":1.5},' + FAILED), "ADDED",
                          {"n_containers": 0, "node_name": "n"}),
    "state-string-structured": (ev(MD + ',"status":{"phase":"Failed","containerStatuses":[{"name":"c","state":"x"}]}'),
                                "ADDED", {"n_cstatuses": 1}),
    # identity fields that are no strings
    "identity-not-strings": (ev('"metadata":{"name":5,"namespace":true,"uid":[1],"resourceVersion":{"a":1}},' + FAILED),
                             "ADDED", {"name": None, "uid": None}),
    # falsy labels / annotations
    "labels-underflow": (ev(md('"labels":1e-400') + "," + FAILED), "ADDED", {"labels": {}}),
    "labels-negative-underflow": (ev(md('"labels":-1E-999') + "," + FAILED), "ADDED", {"labels": {}}),
    "labels-zero-spellings": (ev(md('"labels":0.000e+5,"annotations":-0') + "," + FAILED), "ADDED",
                              {"labels": {}, "annotations": {}}),
    "labels-denormal-is-truthy": (ev(md('"labels":1e-320') + "," + FAILED), "ADDED", {"labels": 1e-320}),
    "labels-number": (ev(md('"labels":10,"annotations":0.5') + "," + FAILED), "ADDED",
                      {"labels": 10, "annotations": 0.5}),
    "labels-false-empty": (ev(md('"labels":false,"annotations":""') + "," + FAILED), "ADDED",
                           {"labels": {}, "annotations": {}}),
    "labels-spaced-empty": (ev(md('"labels":[ \t],"annotations":{ }') + "," + FAILED), "ADDED",
                            {"labels": {}, "annotations": {}}),
    "labels-dup": (ev(md('"labels":{"a":"b"},"labels":{"c":"d"}') + "," + FAILED), "ADDED", {"labels": {"c": "d"}}),
    # timestamp look-alikes
    "ctime-trailing-newline": (ev(md('"creationTimestamp":"2025-07-09T01:51:28Z\\n"')), "ADDED",
                               {"ctime": "2025-07-09T01:51:28Z\n"}),
    "ctime-arabic-digit": (ev(md('"creationTimestamp":"٢025-07-09 01:51:28Z"')), "ADDED",
                           {"ctime": "٢025-07-09 01:51:28Z"}),
    "ctime-escaped-z": (ev(md('"creationTimestamp":"2025-07-09T01:51:28\\u005a"')), "ADDED",
                        {"ctime": "2025-07-09T01:51:28+00:00"}),
    "ctime-escaped-digits": (ev(md('"creationTimestamp":"\\u0032025-07-09t01:51:28.5\\u002B0900"')), "ADDED",
                             {"ctime": "2025-07-09T01:51:28.500000+09:00"}),
    "ctime-escaped-arabic-digit": (ev(md('"creationTimestamp":"\\u0662025-07-09T01:51:28Z"')), "ADDED",
                                   {"ctime": "٢025-07-09T01:51:28Z"}),
    # escaped spellings of keys and values
    "key-escaped-name": (ev('"metadata":{"na\\u006de":"a","u\\u0069d":"u1","namespac\\u0065":"default"},' + FAILED),
                         "ADDED", {"name": "a", "uid": "u1"}),
    "key-escaped-phase": (ev(MD + ',"status":{"ph\\u0061se":"Failed"}'), "ADDED", {"phase": "Failed"}),
    "key-escaped-upper-hex": (ev(MD + ',"status":{"\\u0070\\u0068\\u0061\\u0073\\u0065":"Failed",'
                                      '"c\\u006Fnditions":[{"typ\\u0065":"Ready"}]}'), "ADDED",
                              {"phase": "Failed", "n_conditions": 1}),
    "key-escaped-containers": (ev('"met\\u0061data":{"name":"a","namespace":"default","uid":"u1"},'
                                  '"sp\\u0065c":{"nod\\u0065Name":"n","cont\\u0061iners":[{"nam\\u0065":"c"}]},'
                                  '"st\\u0061tus":{"phase":"Failed","containerSt\\u0061tuses":[{"n\\u0061me":"c"}]}'),
                               "ADDED", {"name": "a", "node_name": "n", "n_containers": 1, "n_cstatuses": 1,
                                         "phase": "Failed"}),
    "key-escaped-slash": (ev(md('"labels":{"a\\/b":"c\\/d"}') + "," + FAILED), "ADDED", {"labels": {"a/b": "c/d"}}),
    "key-escaped-type": (b'{"ty\\u0070e":"ADDED","object":{' + (MD + "," + FAILED).encode() + b"}}", "ADDED",
                         {"phase": "Failed"}),
    "key-escaped-object": (b'{"type":"ADDED","obj\\u0065ct":{' + (MD + "," + FAILED).encode() + b"}}", "ADDED",
                           {"phase": "Failed"}),
    "type-escaped-added": (ev(MD + "," + FAILED, '"ADD\\u0045D"'), "ADDED", {"phase": "Failed"}),
    "type-escaped-deleted": (ev(MD + ',"status":{"phase":"Running"}', '"\\u0044ELETED"'), "DELETED",
                             {"phase": "Running"}),
    "type-escaped-bookmark": (ev(MD, '"BOOKM\\u0041RK"'), "BOOKMARK", {}),
    "phase-value-escaped": (ev(MD + ',"status":{"phase":"Fail\\u0065d"}', '"MODIFIED"'), "MODIFIED",
                            {"phase": "Failed"}),
    "phase-value-escaped-succeeded": (ev(MD + ',"status":{"phase":"\\u0053ucceeded"}', '"MODIFIED"'), "MODIFIED",
                                      {"phase": "Succeeded"}),
    "phase-value-escaped-running": (ev(MD + ',"status":{"phase":"Runn\\u0069ng"}', '"MODIFIED"'), "MODIFIED",
                                    {"phase": "Running"}),
    "identity-values-escaped": (ev('"metadata":{"name":"\\u0061","namespace":"d\\u0065fault","uid":"u\\u0031",'
                                   '"resourceVersion":"\\u0037"},' + FAILED), "ADDED", {"name": "a", "uid": "u1"}),
    "type-dup": (b'{"type":"ADDED","type":"DELETED","object":{' + MD.encode() + b"}}", "DELETED", {}),
    "object-dup": (b'{"type":"ADDED","object":{"metadata":{"name":"first"}},"object":{' + (MD + "," + FAILED).encode()
                   + b"}}", "ADDED", {"name": "a"}),
    "type-after-object-spaced": (b'\t{ "object" :\r{ ' + (MD + " , " + FAILED).encode() + b' } , "type" : "ADDED" } \r',
                                 "ADDED", {"phase": "Failed"}),
    # a type that is no JSON string
    "type-number": (ev(MD, "5"), INVALID, {}),
    "type-null": (ev(MD, "null"), INVALID, {}),
    "type-bool": (ev(MD, "true"), INVALID, {}),
    "type-array": (ev(MD, '["ADDED"]'), INVALID, {}),
    "type-dup-last-number": (b'{"type":"ADDED","type":5,"object":{' + MD.encode() + b"}}", INVALID, {}),
    "type-unknown-string": (ev(MD, '"FOO"'), "FOO", {}),
    # lone surrogates are delivered
    "surrogate-escaped-name": (ev('"metadata":{"name":"\\ud800","namespace":"default","uid":"u1"},' + FAILED), "ADDED",
                               {"name": "\ud800"}),
    "surrogate-raw-uid": (b'{"type":"ADDED","object":{"metadata":{"name":"a","namespace":"default",'
                          b'"uid":"\xed\xa0\x80"},"status":{"phase":"Failed"}}}', "ADDED", {"uid": "\ud800"}),
    "surrogate-low-in-label": (ev(md('"labels":{"k\\udc00":"v\\udfff"}') + "," + FAILED), "ADDED",
                               {"labels": {"k\udc00": "v\udfff"}}),
    "surrogate-pair-escaped": (ev('"metadata":{"name":"\\ud83d\\ude00","namespace":"default","uid":"u1"},' + FAILED),
                               "ADDED", {"name": "\U0001f600"}),
    # BOOKMARK: the WatchList end marker
    "bookmark-end-dup-last-false": (ev(md('"annotations":{"' + END + '":"true","' + END + '":"false"}'), '"BOOKMARK"'),
                                    "BOOKMARK", {"end": False}),
    "bookmark-end-dup-last-true": (ev(md('"annotations":{"' + END + '":"false","' + END + '":"true"}'), '"BOOKMARK"'),
                                   "BOOKMARK", {"end": True}),
    "bookmark-end-escaped-value": (ev(md('"annotations":{"' + END + '":"tru\\u0065"}'), '"BOOKMARK"'), "BOOKMARK",
                                   {"end": True}),
    "bookmark-end-escaped-key": (ev(md('"annotations":{"k8s.io\\/initial-\\u0065vents-end":"true"}'), '"BOOKMARK"'),
                                 "BOOKMARK", {"end": True}),
    "bookmark-end-not-a-string": (ev(md('"annotations":{"' + END + '":true}'), '"BOOKMARK"'), "BOOKMARK",
                                  {"end": False}),
    "bookmark-annotations-dup": (ev(md('"annotations":{"' + END + '":"true"},"annotations":[]'), '"BOOKMARK"'),
                                 "BOOKMARK", {"end": False}),
}

# python_repr: a container state that is no object is INVALID, from feed, in both engines
REPR_ROWS = {
    "state-string": ev(MD + ',"status":{"phase":"Failed","containerStatuses":[{"name":"c","state":"x"}]}'),
    "state-array": ev(MD + ',"status":{"phase":"Failed","containerStatuses":[{"name":"c","state":[1]}]}'),
    "state-number": ev(MD + ',"status":{"phase":"Failed","containerStatuses":[5,{"name":"c","state":0}]}'),
    "sub-state-string": ev(MD + ',"status":{"phase":"Failed","containerStatuses":[{"state":{"running":"x"}}]}'),
    "sub-state-number": ev(MD + ',"status":{"phase":"Failed","containerStatuses":[{"state":{"waiting":5}}]}'),
}

ITEM = '{' + MD + "," + FAILED + "}"
ITEM2 = '{"metadata":{"name":"b","namespace":"default","uid":"u2","resourceVersion":"8"},' + FAILED + "}"
LIST_MD = '"metadata":{"resourceVersion":"99","continue":"tok"}'

# id -> (body, True where policy 4 says ValueError, (resourceVersion, continue, uids) otherwise)
LIST_ROWS = {
    "items-mixed": (('{' + LIST_MD + ',"items":[5,' + ITEM + ',"s",null,[' + ITEM2 + "]]}").encode(), False,
                    ("99", "tok", ["u1"])),
    "items-string": (('{' + LIST_MD + ',"items":"abc"}').encode(), True, None),
    "items-object": (('{' + LIST_MD + ',"items":{"a":1}}').encode(), True, None),
    "items-number": (('{' + LIST_MD + ',"items":0}').encode(), True, None),
    "items-null": (('{' + LIST_MD + ',"items":null}').encode(), False, ("99", "tok", [])),
    "metadata-string": (('{"metadata":"x","items":[' + ITEM + "]}").encode(), True, None),
    "metadata-array": (('{"metadata":[],"items":[' + ITEM + "]}").encode(), True, None),
    "metadata-null": (('{"metadata":null,"items":[' + ITEM + "]}").encode(), False, (None, None, ["u1"])),
    "top-level-array": (b"[]", True, None),
    "top-level-string": (b'"x"', True, None),
    "top-level-number": (b"7", True, None),
    "not-json": (b'{"items":[', True, None),
    "trailing-data": (b'{"items":[]} x', True, None),
    "trailing-object": (('{"items":[' + ITEM + "]}{}").encode(), True, None),
    "identity-not-strings": (b'{"metadata":{"resourceVersion":7,"continue":5},"items":[]}', False, (None, None, [])),
    "continue-empty": (b'{"metadata":{"resourceVersion":"5","continue":""},"items":[]}', False, ("5", None, [])),
    "items-dup": (('{' + LIST_MD + ',"items":[' + ITEM + '],"items":[' + ITEM2 + "]}").encode(), False,
                  ("99", "tok", ["u2"])),
    "items-dup-last-null": (('{' + LIST_MD + ',"items":[' + ITEM + '],"items":null}').encode(), False,
                            ("99", "tok", [])),
    "items-dup-last-string": (('{' + LIST_MD + ',"items":[' + ITEM + '],"items":"x"}').encode(), True, None),
    "metadata-dup": (('{' + LIST_MD + ',"items":[' + ITEM + '],"metadata":{"resourceVersion":"5"}}').encode(), False,
                     ("5", None, ["u1"])),
    "keys-escaped": (('{"met\\u0061data":{"resourc\\u0065Version":"9\\u0039","continu\\u0065":"tok"},'
                      '"it\\u0065ms":[' + ITEM + "]}").encode(), False, ("99", "tok", ["u1"])),
    "spaced": (('\t{ "items" : [ ' + ITEM + " ,\r" + ITEM2 + " ] , " + LIST_MD + " } \r").encode(), False,
               ("99", "tok", ["u1", "u2"])),
}

CASES = ([("watch", k) for k in WATCH_ROWS] + [("repr", k) for k in REPR_ROWS] + [("list", k) for k in LIST_ROWS])


def held(view, pipes):
    """The fields a corpus row pins, read from the Python engine's answer."""
    etype, ident, core, extra = view
    uid, ns, name, rv, phase, has_status = ident
    out = {"uid": uid, "ns": ns, "name": name, "has_status": has_status, "end": extra}
    if core is not None:
        out.update(phase=core["status"]["phase"], node_name=core["spec"]["node_name"],
                   n_conditions=len(core["status"]["conditions"]),
                   n_cstatuses=len(core["status"]["container_statuses"]),
                   n_containers=len(core["spec"]["containers"]), labels=core["metadata"]["labels"],
                   annotations=core["metadata"]["annotations"], ctime=core["metadata"]["creation_timestamp"])
    else:
        out["phase"] = phase
    return out


def list_answer(dec, body):
    """decode_list's answer: ("raises", class) or (rv, continue, [event views])."""
    try:
        rv, cont, evs = dec.decode_list(body)
    except Exception as exc:  # noqa: BLE001 - the class is what the caller asserts
        return ("raises", ValueError if isinstance(exc, ValueError) else type(exc))
    return (rv, cont, [event_view(dec, e) for e in evs])


def python_relist(env, body):
    p, rec = pipeline(env, "payload", "structured", native=False)
    try:
        rv, cont, evs = PyDecoder(env).decode_list(body)
    except Exception as exc:  # noqa: BLE001
        return ("raises", ValueError if isinstance(exc, ValueError) else type(exc))
    ctrl = p.reconcile(evs, 0)
    return (rv, cont, parsed(rec.calls), [c[0] for c in ctrl], sorted(u or "" for u, _ in p.cache.items()))


def native_relist(env, validate, body):
    p, rec = pipeline(env, validate, "structured", native=True)
    rl = p.native.relist(None, True)
    rl.page(body)
    ctrl = []
    try:
        done = False
        while not done:
            done, c = p.native_slice(rl.step, 1e6, 0)
            ctrl += c
    except Exception as exc:  # noqa: BLE001
        assert rec.calls == [], "a body that raises must not have applied any item"
        return ("raises", ValueError if isinstance(exc, ValueError) else type(exc))
    rv, cont = rl.page_meta()
    done = False
    while not done:
        done, c = p.native_slice(rl.sweep, 1e6, 0)
        ctrl += c
    return (rv, cont, parsed(rec.calls), [c[0] for c in ctrl], sorted(u or "" for u, _ in p.cache.items()))


def assert_list_agrees(body):
    """decode_list in both engines and the native relist against the Python reconcile."""
    want = list_answer(PyDecoder(ENV), body)
    relisted = {env: python_relist(env, body) for env in ("production", "staging")}
    mod = load()
    try:
        for level in LEVELS:
            mod.set_simd(level)
            for validate in ("payload", "full"):
                got = list_answer(NativeDecoder(ENV, validate=validate), body)
                assert got == want, (f"decode_list {validate} simd={level}", body[:300])
                for env in ("production", "staging"):
                    assert native_relist(env, validate, body) == relisted[env], (
                        f"relist {env} {validate} simd={level}", body[:300])
    finally:
        mod.set_simd(True)
    return want


@pytest.mark.parametrize("kind,row", CASES, ids=[f"{k}-{r}" for k, r in CASES])
def test_pinned_corpus(kind, row):
    if kind == "watch":
        line, etype, want = WATCH_ROWS[row]
        assert json.loads(line)  # hostile, but valid
        view, pipes = assert_engines_agree(line)
        assert len(view) == 1 and view[0][0] == etype
        if etype != INVALID:
            got = held(view[0], pipes)
            assert {k: got[k] for k in want} == want
            if etype in POD_TYPES and got["ns"] == "default" and want.get("phase") in ("Failed", "Succeeded"):
                # the critical-events filter (production) saw the phase: the event went out
                assert [c[:2] for c in pipes["production"]["submits"]] == [(got["uid"], etype)]
            elif etype == "MODIFIED" and want.get("phase") == "Running":
                assert pipes["production"]["submits"] == []
                assert pipes["production"]["counters"]["events_filtered_critical"] == 1
        else:
            assert pipes["staging"]["ctrl"] == [INVALID] and pipes["staging"]["submits"] == []
        # the same answers in python_repr (no row here has a state it cannot render)
        assert_engines_agree(line, "python_repr")
    elif kind == "repr":
        line = REPR_ROWS[row]
        assert json.loads(line)
        view, pipes = assert_engines_agree(line, "python_repr")
        assert view == [(INVALID,)]
        assert pipes["staging"]["ctrl"] == [INVALID] and pipes["staging"]["submits"] == []
        structured, _ = assert_engines_agree(line)  # structured passes the state through
        assert structured[0][0] == "ADDED"
    else:
        body, raises, want = LIST_ROWS[row]
        got = assert_list_agrees(body)
        if raises:
            assert got == ("raises", ValueError)
        else:
            assert (got[0], got[1], [e[1][0] for e in got[2]]) == want


# ----------------------------------------------------------------------------- Test 2: structural fuzz

class Raw(str):
    """A number token the encoder writes as it stands."""


_char = st.one_of(st.characters(blacklist_categories=("Cs",)), st.characters(blacklist_categories=("Cs",)),
                  st.sampled_from("\ud800􏰀\udfff/\\\"\n\x00\x7f"))
text = st.text(alphabet=_char, max_size=10)
number = st.one_of(st.integers(-5, 10 ** 6), st.floats(allow_nan=False, allow_infinity=False),
                   st.sampled_from([Raw("1e-400"), Raw("-0"), Raw("0.0E+7"), Raw("-1E-999"), Raw("1e-320"), Raw("0")]))
scalar = st.one_of(st.none(), st.booleans(), number, text)
wrong = st.one_of(st.none(), st.booleans(), number, text, st.just([]), st.lists(scalar, min_size=1, max_size=2),
                  st.just({}), st.dictionaries(text, scalar, min_size=1, max_size=2))


def sub(s):
    """`s`, or with probability about 1/4 a value of the wrong type."""
    return st.one_of(s, s, s, wrong)


def obj(fields):
    return sub(st.fixed_dictionaries({}, optional=fields))


def arr(element):
    return sub(st.lists(sub(element), max_size=3))


leaf = sub(text)
timestamp = sub(st.sampled_from(["2025-07-09T01:51:28Z", "2025-07-09t01:51:28.120+0900", "2025-07-09 01:51:28Z\n",
                                 "٢025-07-09T01:51:28Z", "not a time", ""]))
state_obj = obj({"running": obj({"startedAt": leaf}), "waiting": obj({"reason": leaf, "message": leaf})})
pod = st.fixed_dictionaries({}, optional={
    "kind": st.just("Pod"),
    "metadata": obj({
        "name": leaf, "namespace": sub(st.sampled_from(["default", "production", "batch"])), "uid": leaf,
        "resourceVersion": leaf, "labels": sub(st.dictionaries(text, text, max_size=3)),
        "annotations": sub(st.dictionaries(text, text, max_size=3)), "creationTimestamp": timestamp,
        "managedFields": st.lists(st.dictionaries(text, scalar, max_size=3), max_size=2)}),
    "spec": obj({"nodeName": leaf, "containers": arr(st.fixed_dictionaries({}, optional={"name": leaf, "image": leaf}))}),
    "status": obj({
        "phase": sub(st.sampled_from(["Pending", "Running", "Succeeded", "Failed", "Unknown"])),
        "conditions": arr(st.fixed_dictionaries({}, optional={
            "type": leaf, "status": leaf, "reason": leaf, "message": leaf})),
        "containerStatuses": arr(st.fixed_dictionaries({}, optional={
            "name": leaf, "ready": sub(st.booleans()), "restartCount": sub(st.integers(0, 9)), "state": state_obj}))}),
})

JUNK = [None, True, 0, 7, Raw("1e-400"), "x", [], [1], {}, {"name": "junk", "phase": "Failed", "type": "x"}]


class Encoder:
    """JSON text for a value, spelled the hostile way its flags ask for: any
    character of any key or string as a \\uXXXX escape (upper or lower hex, an
    astral character as its pair), ``/`` as ``\\/``, a key twice with another
    first value, ``[ \\t\\r]`` around structural characters."""

    def __init__(self, rng, escape, dup, space):
        self.rng, self.escape, self.dup, self.space = rng, escape, dup, space

    def ws(self):
        if not self.space or self.rng.random() < 0.5:
            return ""
        return "".join(self.rng.choice(" \t\r") for _ in range(self.rng.randint(1, 3)))

    def u(self, code):
        return "\\u" + format(code, "04X" if self.rng.random() < 0.5 else "04x")

    def string(self, s):
        out = ['"']
        for ch in s:
            o = ord(ch)
            if 0xD800 <= o <= 0xDFFF and self.rng.random() < 0.5:
                out.append(ch)  # a lone surrogate, raw: three bytes json.loads(bytes) lets pass
            elif 0xD800 <= o <= 0xDFFF or o < 0x20 or self.rng.random() < self.escape:
                if o > 0xFFFF:
                    o -= 0x10000
                    out.append(self.u(0xD800 + (o >> 10)) + self.u(0xDC00 + (o & 0x3FF)))
                else:
                    out.append(self.u(o))
            elif ch in '"\\':
                out.append("\\" + ch)
            elif ch == "/" and self.rng.random() < 0.5:
                out.append("\\/")
            else:
                out.append(ch)
        out.append('"')
        return "".join(out)

    def member(self, k, v):
        return self.ws() + self.string(k) + self.ws() + ":" + self.ws() + self.value(v) + self.ws()

    def members(self, pairs):
        parts = []
        for k, v in pairs:
            if self.rng.random() < self.dup:  # the key twice: the first value is another one
                parts.append(self.member(k, self.rng.choice(JUNK)))
            parts.append(self.member(k, v))
        return "{" + (",".join(parts) if parts else self.ws()) + "}"

    def value(self, v):
        if isinstance(v, Raw):
            return str(v)
        if v is None or isinstance(v, (bool, int, float)):
            return json.dumps(v)
        if isinstance(v, str):
            return self.string(v)
        if isinstance(v, list):
            return "[" + (",".join(self.ws() + self.value(x) + self.ws() for x in v) if v else self.ws()) + "]"
        return self.members(list(v.items()))

    def line(self, etype, pod, type_last):
        top = [("type", etype), ("object", pod)]
        if type_last:
            top.reverse()
        return (self.ws() + self.members(top) + self.ws()).encode("utf-8", "surrogatepass")


@settings(max_examples=300, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(pod=pod, etype=st.sampled_from(["ADDED", "MODIFIED", "DELETED", "BOOKMARK"]),
       seed=st.integers(0, 2 ** 32 - 1), escape=st.sampled_from([0.0, 0.0, 0.15, 1.0]),
       dup=st.sampled_from([0.0, 0.3]), space=st.booleans(), type_last=st.booleans(),
       fmt=st.sampled_from(["structured", "structured", "python_repr"]))
def test_structural_fuzz(pod, etype, seed, escape, dup, space, type_last, fmt):
    """Every generated case is compared (no assume, no filter): all native
    consumers answer the hostile spelling as the Python engine does, and the
    Python engine answers it as it answers the plain json.dumps spelling of the
    document json.loads reads from it."""
    line = Encoder(random.Random(seed), escape, dup, space).line(etype, pod, type_last)
    doc = json.loads(line)
    assert doc["type"] == etype
    view, pipes = assert_engines_agree(line, fmt)
    assert len(view) == 1
    plain = json.dumps(doc).encode()  # ensure_ascii: lone surrogates as escapes
    assert python_answers(plain, fmt) == (view, pipes), line[:300]
    if view[0][0] != INVALID:
        assert view[0][0] == etype
    else:  # only a state python_repr cannot render makes such a line INVALID
        assert fmt == "python_repr"


# ----------------------------------------------------------------------------- Test 3: creationTimestamp fuzz

_digits = st.sampled_from("0123456789")
_frac = st.one_of(st.just(""), st.sampled_from([".0", ".000000", ".000000000000", ".5", ".123456789", ".", ".01"]),
                  st.text(alphabet=_digits, min_size=0, max_size=12).map(lambda d: "." + d))
_tz = st.sampled_from(["Z", "z", "", "+00:00", "-00:00", "+0000", "-0000", "+02:00", "-05:30", "+0530", "+5:30",
                       "+05:3", "+05-30", "ZZ", "Z ", "Z\n", " ", "\n", "+02:00\n", "z\t"])
_stamp = st.builds(
    lambda y, mo, d, sep, h, mi, s, frac, tz: f"{y:04d}-{mo:02d}-{d:02d}{sep}{h:02d}:{mi:02d}:{s:02d}{frac}{tz}",
    st.integers(0, 9999), st.integers(0, 19), st.integers(0, 39), st.sampled_from(["T", "t", " ", "_", ""]),
    st.integers(0, 29), st.integers(0, 69), st.integers(0, 69), _frac, _tz)


def _mangle(draw_pos, s, repl):
    i = draw_pos % max(1, len(s))
    return s[:i] + repl + s[i + 1:]


timestamps = st.one_of(
    _stamp,
    # a non-ASCII digit in place of any character: str.isdigit() / \d say yes, the format says no
    st.builds(_mangle, st.integers(0, 40), _stamp, st.sampled_from(["٢", "２", "৩", "¹", "𝟙"])),
    # short strings: a cut anywhere
    st.builds(lambda s, n: s[:n], _stamp, st.integers(0, 25)),
    st.sampled_from(["", "Z", "2025", "2025-07-09", "2025-07-09T01:51", "2025-07-09T01:51:2", "2025-07-09T01:51:28",
                     "2025-07-09T01:51:28.", "2025-07-09T01:51:28+", "2025-07-09T01:51:28+0", "\n", "not a time"]))


@settings(max_examples=300, deadline=None, suppress_health_check=[HealthCheck.too_slow])
@given(stamp=timestamps, seed=st.integers(0, 2 ** 32 - 1), escape=st.sampled_from([0.0, 0.1, 1.0]))
def test_creation_timestamp_fuzz(stamp, seed, escape):
    """structured mode: both engines recognise exactly the same timestamps, on
    the unescaped value — the cores are equal after json.loads, for the plain
    and for an escaped spelling of the same string."""
    spelled = Encoder(random.Random(seed), escape, 0.0, False).string(stamp)
    cores = []
    for token in (json.dumps(stamp), spelled):
        line = ('{"type":"ADDED","object":{"metadata":{"creationTimestamp":' + token + "}}}\n").encode()
        py, nat = PyDecoder(ENV), NativeDecoder(ENV)
        a, b = py.feed(line), nat.feed(line)
        assert len(a) == len(b) == 1 and a[0][0] == b[0][0] == "ADDED"
        ca, cb = json.loads(py.core(a[0])), json.loads(nat.core(b[0]))
        assert ca == cb, (stamp, token)
        cores.append(ca)
    assert cores[0] == cores[1], (stamp, spelled)
    out = cores[0]["metadata"]["creation_timestamp"]
    if out != stamp:  # reformatted: only a string the format describes, to isoformat() text
        assert stamp.isascii() and len(stamp) >= 19 and stamp[-1] not in "\n \t"
        assert out[:10] == stamp[:10] and out[10] == "T" and out[11:19] == stamp[11:19]


# ----------------------------------------------------------------------------- Test 4: the depth ladder

JV_MAX_DEPTH = 2048  # ops/csrc/validate.inc
AGREE_DEPTH = 200    # json.loads follows this well inside CPython's default recursion limit


def nest(depth):
    return "[" * depth + "]" * depth


def deep_pod(where, depth):
    n = nest(depth)
    if where == "ignored":
        return '{' + MD + "," + FAILED + ',"x":' + n + "}"
    if where == "labels":
        return '{' + md('"labels":{"k":' + n + "}") + "," + FAILED + "}"
    return ('{' + MD + ',"status":{"phase":"Failed","containerStatuses":[{"name":"c","state":{"running":' + n
            + "}}]}}")


def flat(core, depth):
    """The parsed core with the nest cut out of its bytes first (json.loads cannot follow a deep one)."""
    assert core.count(nest(depth).encode()) <= 1
    return json.loads(core.replace(nest(depth).encode(), b'"@"'))


def deep_views(dec, data, depth):
    out = []
    for e in dec.feed(data):
        out.append((INVALID,) if e[0] == INVALID else (e[0], e[1:7], flat(dec.core(e), depth)))
    return out


@pytest.mark.parametrize("where", ["ignored", "labels", "state"])
@pytest.mark.parametrize("depth", [100, 200, 1000, 2048, 2049, 5000])
def test_depth_ladder(depth, where):
    """Policy 6. No call raises, at any depth. Up to 200 levels both engines
    accept and agree. Above, the Python engine may answer INVALID; the native
    engine then answers INVALID, or else exactly what the Python engine answers
    for the same pod at 200 levels. validate: full is INVALID above
    JV_MAX_DEPTH; validate: payload only where the depth lies in a copied span.
    decode_list has no INVALID to answer with: past 200 levels it may raise
    ValueError (policy 4's only class), and nothing else."""
    podtext = deep_pod(where, depth)
    line = ('{"type":"ADDED","object":' + podtext + "}").encode()
    body = ('{"metadata":{"resourceVersion":"1"},"items":[' + podtext + "]}").encode()
    if depth <= AGREE_DEPTH:
        view, pipes = assert_engines_agree(line)
        assert view[0][0] == "ADDED" and len(pipes["production"]["submits"]) == 1
        got = assert_list_agrees(body)
        assert got[0] == "1" and [e[0] for e in got[2]] == ["ADDED"]
        return
    data = line + b"\n"
    ref_line = ('{"type":"ADDED","object":' + deep_pod(where, AGREE_DEPTH) + "}\n").encode()
    want = deep_views(PyDecoder(ENV), ref_line, AGREE_DEPTH)
    assert want[0][0] == "ADDED"
    py_view = deep_views(PyDecoder(ENV), data, depth)  # feed and core do not raise
    assert py_view in ([(INVALID,)], want)
    total = depth + {"ignored": 2, "labels": 4, "state": 6}[where]  # containers open around the innermost "["
    span = depth + 1  # {"k":[[..]]} / {"running":[[..]]}
    mod = load()
    try:
        for level in LEVELS:
            mod.set_simd(level)
            for validate in ("payload", "full"):
                got = deep_views(NativeDecoder(ENV, validate=validate), data, depth)
                assert got in ([(INVALID,)], want), (validate, level)
                if validate == "full" and total > JV_MAX_DEPTH:
                    assert got == [(INVALID,)], (validate, level)
                if validate == "payload" and where == "ignored":
                    assert got == want, level  # no copied span holds the depth
                if validate == "payload" and where != "ignored" and span > JV_MAX_DEPTH:
                    assert got == [(INVALID,)], level
                for env in ("production", "staging"):
                    p, rec = pipeline(env, validate, "structured", native=True)
                    ctrl = p.handle_raw(data, 0, framed=False)
                    if got == [(INVALID,)]:
                        assert [c[0] for c in ctrl] == [INVALID] and rec.calls == []
                    else:
                        assert ctrl == [] and [c[:4] for c in rec.calls] == [("u1", "ADDED", "default", "a")]
                nat = NativeDecoder(ENV, validate=validate)
                try:
                    rv, cont, evs = nat.decode_list(body)
                    assert (rv, cont, [e[0] for e in evs]) in (("1", None, ["ADDED"]), ("1", None, [INVALID]))
                except ValueError:
                    pass
    finally:
        mod.set_simd(True)
    for env in ("production", "staging"):  # the Python pipeline: INVALID or delivered, never an exception
        p, rec = pipeline(env, "payload", "structured", native=False)
        ctrl = p.handle_batch(PyDecoder(env).feed(data), 0)
        assert ([c[0] for c in ctrl], len(rec.calls)) == (([INVALID], 0) if py_view == [(INVALID,)] else ([], 1))
    try:
        rv, cont, evs = PyDecoder(ENV).decode_list(body)
        assert (rv, cont, [e[0] for e in evs]) == ("1", None, ["ADDED"])
    except ValueError:
        pass
