"""Pods still Pending N seconds after creation
(``watcher.alerts.pending_overdue_seconds``).

The finding (``models/findings.py`` ``pending_since`` and its native twin in
``ops/csrc/findings.inc``), ``E_PENDING_SINCE`` from both decoders, the
pending-since, its own reported mark and the kept core in both caches, where an
event stores them (watch path serial and partitioned, native relist, Python
reconcile, the unchanged items of a notifying relist), the sweep
(``EventPipeline.report_overdue``) in both engines, and the service's loop.
Every sweep but the end-to-end test's takes its clock as an argument.
"""

import calendar
import collections
import datetime
import json
import random

import pytest

from conftest import run
from k8s_watcher_amd.engine.pipeline import EventPipeline
from k8s_watcher_amd.metrics import Metrics
from k8s_watcher_amd.ops.cache import CORE, make_pod_cache
from k8s_watcher_amd.ops.decode import E_PENDING_SINCE, E_UID, make_decoder
from k8s_watcher_amd.testing.podgen import PodFactory, event_line
from k8s_watcher_amd.utils.config import ConfigError, load_settings, parse_override
from test_pod_condition_alerts import RV_EXTRA, alerts, escaped, lines, merged, with_rv
from test_terminating_alerts import NAMESPACES, T1, deleting, md, settings_for, shard_of, warm_up
from test_termination_overdue import RawRecorder, feed, mutated_timestamp, valid_timestamp

KEY = "watcher.alerts.pending_overdue_seconds"
N = 300  # the option's value in these tests
C1 = "2025-07-09T01:51:28Z"  # a creation time, and its seconds since 1970
C1_S = 1752025888
COUNTERS = ("events_received", "events_filtered_critical", "events_filtered_namespace", "events_unchanged",
            "events_other_shard", "events_container_failure", "events_pod_condition", "events_terminating",
            "events_termination_overdue", "events_pending_overdue", "bookmarks")


def PO(n=N, **kw):
    return alerts(pending_overdue_seconds=n, **kw)


# ----------------------------------------------------------------------------- config (test 1)

def test_config():
    for env in ("development", "staging", "production"):
        assert load_settings(env, environ={}).watcher.pending_overdue_seconds == 0
    w = load_settings("production", environ={}, overrides=PO(45)).watcher
    # it needs no other option: terminating stays off, and may be on
    assert w.pending_overdue_seconds == 45 and w.terminating is False and w.terminating_overdue_seconds == 0
    w = load_settings("production", environ={}, overrides=PO(45, terminating=True, terminating_overdue_seconds=7)).watcher
    assert (w.pending_overdue_seconds, w.terminating, w.terminating_overdue_seconds) == (45, True, 7)
    assert load_settings("staging", environ={}, overrides=parse_override(KEY + "=30")).watcher.pending_overdue_seconds == 30
    assert load_settings("staging", environ={}, overrides=PO("30")).watcher.pending_overdue_seconds == 30
    assert load_settings("staging", environ={}, overrides=PO(" 4000000000 ")).watcher.pending_overdue_seconds == 4000000000
    for bad in (True, False, 1.5, 30.0, [30], {"seconds": 30}, -1, "soon", "-1", "1.5", "", "3e2", "0x10", None):
        with pytest.raises(ConfigError, match=KEY):
            load_settings("staging", environ={}, overrides=PO(bad))


def test_print_config_shows_the_key(capsys):
    from k8s_watcher_amd.utils.config import dump_effective
    dump_effective(load_settings("production", environ={}))
    assert "pending_overdue_seconds: 0" in capsys.readouterr().out
    dump_effective(load_settings("production", environ={}, overrides=PO(45)))
    assert "pending_overdue_seconds: 45" in capsys.readouterr().out


# ----------------------------------------------------------------------------- the corpus (test 2)

CT = ',"creationTimestamp":"%s"' % C1
TS = ',"deletionTimestamp":"%s"' % T1


def st(phase='"Pending"', more=""):
    """A "status" member as raw JSON text."""
    return '"status":{"phase":%s,"podIP":"10.244.0.7"%s}' % (phase, more)


# (id, the raw "metadata" member(s), the raw "status" member(s) or None, the event type, pending_since of the pod)
CORPUS = [
    ("pending", md(CT), st(), "MODIFIED", C1_S),
    ("pending-added", md(CT), st(), "ADDED", C1_S),
    ("pending-deleted-line", md(CT), st(), "DELETED", C1_S),  # the function's value; a DELETED line is never examined
    ("running", md(CT), st('"Running"'), "MODIFIED", None),
    ("succeeded", md(CT), st('"Succeeded"'), "MODIFIED", None),
    ("failed", md(CT), st('"Failed"'), "MODIFIED", None),
    ("unknown", md(CT), st('"Unknown"'), "MODIFIED", None),
    ("lower-case", md(CT), st('"pending"'), "MODIFIED", None),
    ("trailing-blank", md(CT), st('"Pending "'), "MODIFIED", None),
    ("empty-phase", md(CT), st('""'), "MODIFIED", None),
    ("no-status", md(CT), None, "MODIFIED", None),
    ("status-null", md(CT), '"status":null', "MODIFIED", None),
    ("status-array", md(CT), '"status":["Pending"]', "MODIFIED", None),
    ("status-string", md(CT), '"status":"Pending"', "MODIFIED", None),
    ("status-number", md(CT), '"status":7', "MODIFIED", None),
    ("status-without-phase", md(CT), '"status":{"podIP":"10.244.0.7"}', "MODIFIED", None),
    ("phase-null", md(CT), st("null"), "MODIFIED", None),
    ("phase-number", md(CT), st("7"), "MODIFIED", None),
    ("phase-true", md(CT), st("true"), "MODIFIED", None),
    ("phase-array", md(CT), st('["Pending"]'), "MODIFIED", None),
    ("phase-object", md(CT), st('{"phase":"Pending"}'), "MODIFIED", None),
    ("phase-escaped", md(CT), st('"P\\u0065nding"'), "MODIFIED", C1_S),
    ("phase-escaped-first", md(CT), st('"\\u0050ending"'), "MODIFIED", C1_S),
    ("phase-escaped-all", md(CT), st('"\\u0050\\u0065\\u006e\\u0064\\u0069\\u006E\\u0067"'), "MODIFIED", C1_S),
    ("phase-escaped-other", md(CT), st('"Pendin\\u0067\\u0020"'), "MODIFIED", None),
    ("phase-escaped-backslash", md(CT), st('"P\\\\u0065nding"'), "MODIFIED", None),
    ("phase-escaped-solidus", md(CT), st('"Pen\\/ding"'), "MODIFIED", None),
    ("phase-key-escaped", md(CT), '"status":{"ph\\u0061se":"Pending"}', "MODIFIED", C1_S),
    ("phase-repeated-last-running", md(CT), st(more=',"phase":"Running"'), "MODIFIED", None),
    ("phase-repeated-last-pending", md(CT), st('"Running"', more=',"phase":"Pending"'), "MODIFIED", C1_S),
    ("phase-repeated-last-null", md(CT), st(more=',"phase":null'), "MODIFIED", None),
    ("status-repeated-last-running", md(CT), st() + "," + st('"Running"'), "MODIFIED", None),
    ("status-repeated-last-pending", md(CT), st('"Running"') + "," + st(), "MODIFIED", C1_S),
    ("status-repeated-last-null", md(CT), st() + ',"status":null', "MODIFIED", None),
    ("status-repeated-last-array", md(CT), st() + ',"status":[]', "MODIFIED", None),
    ("status-repeated-last-empty", md(CT), st() + ',"status":{}', "MODIFIED", None),
    ("creation-missing", md(), st(), "MODIFIED", None),
    ("creation-null", md(',"creationTimestamp":null'), st(), "MODIFIED", None),
    ("creation-number", md(',"creationTimestamp":%d' % C1_S), st(), "MODIFIED", None),
    ("creation-array", md(',"creationTimestamp":["%s"]' % C1), st(), "MODIFIED", None),
    ("creation-object", md(',"creationTimestamp":{"time":"%s"}' % C1), st(), "MODIFIED", None),
    ("creation-no-zone", md(',"creationTimestamp":"2025-07-09T01:51:28"'), st(), "MODIFIED", None),
    ("creation-blank-for-t", md(',"creationTimestamp":"2025-07-09 01:51:28Z"'), st(), "MODIFIED", None),
    ("creation-empty", md(',"creationTimestamp":""'), st(), "MODIFIED", None),
    ("creation-leap-day-that-is-none", md(',"creationTimestamp":"2100-02-29T00:00:00Z"'), st(), "MODIFIED", None),
    ("creation-any-text", md(',"creationTimestamp":"soon, été ✓"'), st(), "MODIFIED", None),
    ("creation-offset", md(',"creationTimestamp":"2025-07-09T10:51:28+09:00"'), st(), "MODIFIED", C1_S),
    ("creation-fraction", md(',"creationTimestamp":"2025-07-09T01:51:28.75Z"'), st(), "MODIFIED", C1_S),
    ("creation-before-1970", md(',"creationTimestamp":"1969-12-31T23:59:59Z"'), st(), "MODIFIED", -1),
    ("creation-escaped", md(',"creationTimestamp":"2025-07-09T01:51:28\\u005a"'), st(), "MODIFIED", C1_S),
    ("creation-escaped-other", md(',"creationTimestamp":"2025-07-09T01:51:28\\u007a"'), st(), "MODIFIED", None),
    ("creation-key-escaped", md(',"creation\\u0054imestamp":"%s"' % C1), st(), "MODIFIED", C1_S),
    ("creation-repeated-last-null", md(CT + ',"creationTimestamp":null'), st(), "MODIFIED", None),
    ("creation-repeated-last-string", md(',"creationTimestamp":null' + CT), st(), "MODIFIED", C1_S),
    ("creation-repeated-last-other", md(CT + ',"creationTimestamp":"1970-01-01T00:00:00Z"'), st(), "MODIFIED", 0),
    ("17-bytes-other-key", md(',"creationTimestamq":"%s"' % C1), st(), "MODIFIED", None),
    ("metadata-array", '"metadata":["creationTimestamp","%s"]' % C1, st(), "MODIFIED", None),
    ("metadata-null", '"metadata":null', st(), "MODIFIED", None),
    ("metadata-repeated-last-without", md(CT) + "," + md(), st(), "MODIFIED", None),
    ("metadata-repeated-last-with", md() + "," + md(CT), st(), "MODIFIED", C1_S),
    ("metadata-repeated-last-array", md(CT) + ',"metadata":[]', st(), "MODIFIED", None),
    ("terminating", md(CT + TS), st(), "MODIFIED", None),
    ("terminating-any-text", md(CT + ',"deletionTimestamp":""'), st(), "MODIFIED", None),
    ("deletion-null", md(CT + ',"deletionTimestamp":null'), st(), "MODIFIED", C1_S),
    ("deletion-number", md(CT + ',"deletionTimestamp":1752025892'), st(), "MODIFIED", C1_S),
    ("deletion-repeated-last-null", md(CT + TS + ',"deletionTimestamp":null'), st(), "MODIFIED", C1_S),
    ("deletion-repeated-last-string", md(CT + ',"deletionTimestamp":null' + TS), st(), "MODIFIED", None),
    ("status-before-metadata", None, None, "MODIFIED", C1_S),  # (written out in corpus_object)
]


def corpus_object(members, status, uid="u-corpus"):
    """The pod as JSON text around the raw metadata and status member(s)."""
    if members is None:
        return ('{%s,"kind":"Pod","spec":{"nodeName":"n","containers":[{"name":"c","image":"i"}]},%s}'
                % (st(), md(CT).replace("@UID@", uid)))
    return ('{"kind":"Pod","apiVersion":"v1",%s,"spec":{"nodeName":"mi355x-node-01","containers":[{"name":"c",'
            '"image":"registry.example.com/team/c:v1"}]}%s}'
            % (members.replace("@UID@", uid), "" if status is None else "," + status))


def corpus_line(members, status, etype="MODIFIED", uid="u-corpus"):
    return ('{"type":"%s","object":%s}\n' % (etype, corpus_object(members, status, uid))).encode()


def corpus_pods():
    """The corpus as pod objects (raw JSON text) with the expected pending-since: findings_check's input."""
    return [(corpus_object(members, status), want) for _, members, status, _, want in CORPUS]


@pytest.mark.parametrize("case", CORPUS, ids=[c[0] for c in CORPUS])
def test_finding_table(case):
    from k8s_watcher_amd.models.findings import pending_since
    _, members, status, _, want = case
    got = pending_since(json.loads(corpus_object(members, status)))
    assert got == want and (got is None or type(got) is int)


def test_finding_of_odd_pods():
    from k8s_watcher_amd.models.findings import pending_since
    for pod in ({}, {"status": None}, {"status": {"phase": "Pending"}}, {"status": {"phase": "Pending"}, "metadata": None},
                {"status": {"phase": "Pending"}, "metadata": []}, {"status": [], "metadata": {"creationTimestamp": C1}},
                {"status": {"phase": b"Pending"}, "metadata": {"creationTimestamp": C1}}):
        assert pending_since(pod) is None, pod


def decoder_for(s, engine="python"):
    w = s.watcher
    return make_decoder(engine, s.environment, w.state_format, w.payload_extra, w.validate,
                        w.container_failures, w.container_failure_reasons, w.pod_conditions, w.pod_condition_rules,
                        w.terminating, w.terminating_overdue_seconds > 0, w.pending_overdue_seconds > 0)


def pipeline(s, native, cache=None, notifier=None):
    rec, m = RawRecorder(), Metrics()
    p = EventPipeline(s, decoder_for(s), notifier if notifier is not None else rec, m, cache)
    p.log_events_setting = False
    if native:
        p.attach_native()
    return p, rec, m


def expected_cache(events):
    """uid -> pending-since after the decoded ``events`` in order, as the issue states the rule."""
    want = {}
    for ev in events:
        if ev[0] == "DELETED":
            want.pop(ev[E_UID], None)
        elif ev[0] in ("ADDED", "MODIFIED"):
            want[ev[E_UID]] = ev[E_PENDING_SINCE]
    return want


def same_core(a, b, spelled):
    """Two payload cores are the same bytes. ``spelled``: the line holds a
    backslash; the native engine copies a string token as the line spells it
    and the Python engine writes it as ``json.dumps`` does, so such a line's
    cores are the same JSON value (what the engines have always answered on
    escaped text: tests/test_terminating_alerts.py ``VALUES``)."""
    if a is None or b is None or not spelled:
        return a == b
    return json.loads(a) == json.loads(b)


def check_decoders(data, want_of):
    """``data``: watch lines; ``want_of(line) -> pending_since`` of its pod by
    the Python twin. ``E_PENDING_SINCE``, ``INVALID`` and the core bytes from
    both decoders (the native one under validate payload and full).
    -> the Python decoder's events."""
    py = make_decoder("python", "staging", pending=True)
    a = [py.feed(ln)[0] for ln in data]
    for ev, ln in zip(a, data):
        if ev[0] == "INVALID":
            continue
        assert len(ev) == 14 and ev[9:13] == (0, 0, 0, None), ln  # the earlier slots, filled as their options' off
        assert ev[E_PENDING_SINCE] == (None if ev[0] == "DELETED" else want_of(ln)), ln
    for validate in ("payload", "full"):
        nat = make_decoder("native", "staging", validate=validate, pending=True)
        for ea, ln in zip(a, data):
            eb = nat.feed(ln)[0]
            assert ea[0] == eb[0], ln  # INVALID included
            if ea[0] == "INVALID":
                continue
            assert len(eb) == 14 and eb[:7] == ea[:7] and eb[9:] == ea[9:], (validate, ln)
            assert type(eb[E_PENDING_SINCE]) is type(ea[E_PENDING_SINCE]), ln
            assert same_core(py.core(ea), nat.core(eb), b"\\" in ln), ln  # byte-identical
    return a


def check_pipelines(data, a, overrides=()):
    """The lines as one batch through both fused pipelines, full parse
    (staging) and filter-first (production): the pending-since each stores,
    what is tracked, the notifications' bytes, the INVALID reports."""
    batch = b"".join(data)
    want = expected_cache(a)
    spelled = {e[E_UID] for e, ln in zip(a, data) if b"\\" in ln and e[0] != "INVALID"}
    invalid = [e[0] for e in a if e[0] == "INVALID"]
    for env, ov in (("staging", PO()), ("production", merged(PO(), {"watcher": {"namespaces": []}}))):
        for validate in ("payload", "full"):
            s = settings_for(env, merged(ov, {"watcher": {"validate": validate}}, *overrides))
            got = {}
            for native in (False, True):
                p, rec, m = pipeline(s, native)
                assert [c[0] for c in feed(p, native, batch)] == invalid
                uids = [u for u, _ in p.cache.items()]
                got[native] = ({u: p.cache.pending_since(u) for u in uids}, p.cache.pending_tracked(),
                               {u: p.cache.core_kept(u) for u in uids}, [c[:4] for c in rec.calls],
                               list(zip((c[0] for c in rec.calls), rec.raw)), {u: p.cache.get(u)[CORE] for u in uids})
            assert got[False][:4] == got[True][:4], (env, validate)
            for (u, x), (_, y) in zip(got[False][4], got[True][4]):  # the notifications' bytes
                assert same_core(x, y, u in spelled), (env, validate, u)
            for u, x in got[False][5].items():  # ... and the cached cores', kept or sent
                assert same_core(x, got[True][5][u], u in spelled), (env, validate, u)
            assert got[True][0] == want, (env, validate)
            assert got[True][1] == sum(v is not None for v in want.values())
    return want


def check_corpus():
    from k8s_watcher_amd.models.findings import pending_since
    data = [corpus_line(members, status, etype, "c%d" % i) for i, (_, members, status, etype, _) in enumerate(CORPUS)]
    table = {ln: want for ln, (*_, want) in zip(data, CORPUS)}
    for ln, want in table.items():
        assert pending_since(json.loads(ln)["object"]) == want, ln
    a = check_decoders(data, table.__getitem__)
    assert all(e[0] != "INVALID" for e in a)
    want = check_pipelines(data, a)
    assert sum(v is not None for v in want.values()) >= 15 and sum(v is None for v in want.values()) >= 30
    # with the option off the tuples are what they were
    for eng in ("python", "native"):
        assert all(len(make_decoder(eng, "staging").feed(ln)[0]) == 9 for ln in data[:10])
        assert all(len(make_decoder(eng, "staging", terminating=True, overdue=True).feed(ln)[0]) == 13 for ln in data[:10])
        d = make_decoder(eng, "staging", terminating=True, overdue=True, pending=True)
        evs = [d.feed(ln)[0] for ln in data]
        assert all(len(e) == 14 for e in evs)
        by_id = {c[0]: e for c, e in zip(CORPUS, evs)}
        assert by_id["terminating"][11:] == (1, 1752025892, None) and by_id["pending"][11:] == (0, None, C1_S)


def test_corpus_one_verdict_from_both_engines():
    check_corpus()


# ----------------------------------------------------------------------------- seeded mutations (test 3)

PHASES = ['"Pending"'] * 6 + ['"Running"', '"Succeeded"', '"Failed"', '"Unknown"', '"pending"', '"Pending "', '""']
RETYPED = ["null", "true", "0", "-1.5", "[]", "{}", '["Pending"]', '{"phase":"Pending"}']
BLANKS = ["", "", "", " ", "\t", "  ", "\r"]


def mutated_line(rng, i):
    """A corpus-like line, mutated in the phase (value, type, escapes,
    repetition), the status (type, repetition), the creation time (the
    overdue tests' mutated timestamps: valid or one step off the grammar), the
    deletion timestamp and the event type; all of it valid JSON."""
    ws = lambda: rng.choice(BLANKS)  # noqa: E731
    phase = rng.choice(PHASES)
    r = rng.random()
    if r < 0.08:
        phase = rng.choice(RETYPED)
    elif r < 0.30:
        phase = escaped(rng, json.loads(phase))
    fields = [["phase", phase], ["podIP", '"10.244.0.7"']]
    r = rng.random()
    if r < 0.07:
        fields.append(["phase", rng.choice(PHASES + RETYPED)])  # repeated: the last one counts
    elif r < 0.10:
        fields = fields[1:]
    elif r < 0.14:
        fields[0][0] = escaped(rng, "phase")[1:-1]
    rng.shuffle(fields)
    status = '"status":%s{%s}' % (ws(), ",".join('%s"%s"%s:%s%s' % (ws(), k, ws(), ws(), v) for k, v in fields))
    r = rng.random()
    if r < 0.04:
        status = '"status":%s' % rng.choice(RETYPED + ['"Pending"'])
    elif r < 0.08:
        status = rng.choice(('"status":null,', '"status":{"phase":"Running"},', '"status":{"phase":"Pending"},')) + status
    elif r < 0.11:
        status = status + rng.choice((',"status":null', ',"status":{"phase":"Running"}', ',"status":{}'))
    elif r < 0.13:
        status = None
    more = ""
    r = rng.random()
    if r < 0.40:  # one step off the grammar, more often than not
        more += ',%s"creationTimestamp"%s:%s%s' % (ws(), ws(), ws(), mutated_timestamp(rng))
    elif r < 0.80:
        more += ',%s"creationTimestamp"%s:%s"%s"' % (ws(), ws(), ws(), valid_timestamp(rng)[0])
    elif r < 0.90:
        more += ',"creationTimestamp":%s' % rng.choice(RETYPED + [str(C1_S)])
    if rng.random() < 0.06:
        more += ',"creationTimestamp":%s' % rng.choice(('"%s"' % C1, "null"))
    if rng.random() < 0.12:
        more += ',"deletionTimestamp":%s' % rng.choice(('"%s"' % T1, '""', "null", "17"))
    members = md(more, rv=str(i + 1))
    if rng.random() < 0.03:
        members = rng.choice(('"metadata":null', '"metadata":[]', md(CT) + "," + members, members + "," + md(CT)))
    etype = "MODIFIED" if rng.random() < 0.85 else rng.choice(("ADDED", "DELETED"))
    return corpus_line(members, status, etype, "u%d" % i)


def fuzz_lines(n=2000, seed=29):
    rng = random.Random(seed)
    return [mutated_line(rng, i) for i in range(n)]


def fuzz_pods(n=200, seed=29):
    """The pod objects (raw JSON text) of the first ``n`` mutated lines: findings_check's input."""
    return [ln[ln.index(b'"object":') + 9:-2].decode() for ln in fuzz_lines(n, seed)]


def check_fuzz():
    from k8s_watcher_amd.models.findings import pending_since
    data = fuzz_lines()
    assert len(data) == 2000
    twin = {ln: pending_since(json.loads(ln)["object"]) for ln in data}
    # the condition on the mutator, by the Python twin alone: both outcomes are common
    assert sum(v is not None for v in twin.values()) >= 200 and sum(v is None for v in twin.values()) >= 200
    a = check_decoders(data, twin.__getitem__)
    live = [e for e in a if e[0] in ("ADDED", "MODIFIED")]
    assert len(live) >= 1500 and sum(e[E_PENDING_SINCE] is not None for e in live) >= 200
    check_pipelines(data, a)
    check_pipelines(data, a, [{"watcher": {"notify_on": "phase_change"}}])


def test_seeded_mutation_fuzz():
    check_fuzz()


# ----------------------------------------------------------------------------- both caches, one API (test 4)

@pytest.mark.parametrize("native", [False, True], ids=["python-cache", "native-cache"])
def test_both_caches_one_api(native):
    cache = make_pod_cache(native)
    # an unknown uid is a no-op
    cache.set_pending_since("nobody", 5)
    cache.keep_core("nobody", b"{}")
    assert cache.pending_since("nobody") is None and cache.pending_tracked() == 0 and len(cache) == 0
    assert cache.take_pending_overdue(10 ** 9, 0) == [] and cache.core_kept("nobody") is False
    cache.observe("ADDED", "u", "1", "Pending", "default", "n")
    assert cache.pending_since("u") is None and cache.pending_tracked() == 0
    cache.set_pending_since("u", 100)
    assert cache.pending_since("u") == 100 and cache.pending_tracked() == 1
    assert cache.tracked() == 0 and cache.deadline("u") is None and cache.take_overdue(10 ** 9, 0) == []  # deadlines only
    # no core: neither returned nor marked; a later core makes it reportable
    assert cache.take_pending_overdue(1000, 30) == []
    cache.set_core("u", b'{"a":1}')
    # the boundary: now - since == after fires, one second earlier does not
    assert cache.take_pending_overdue(129, 30) == []
    assert cache.take_pending_overdue(130, 30) == [("u", "default", "n", b'{"a":1}', 100)]
    assert cache.take_pending_overdue(131, 30) == [] and cache.take_pending_overdue(10 ** 9, 0) == []  # marked
    # a value keeps the mark, None clears the value and the mark
    cache.set_pending_since("u", 50)
    assert cache.pending_since("u") == 50 and cache.take_pending_overdue(10 ** 9, 0) == []
    cache.set_pending_since("u", None)
    assert cache.pending_since("u") is None and cache.pending_tracked() == 0 and cache.get("u")[CORE] == b'{"a":1}'
    cache.set_pending_since("u", None)  # twice is fine
    cache.set_pending_since("u", 60)
    assert cache.take_pending_overdue(89, 30) == []
    assert cache.take_pending_overdue(90, 30) == [("u", "default", "n", b'{"a":1}', 60)]
    # the marks are per kind: reported pending-overdue, then terminating, still reported termination-overdue, once
    cache.set_deadline("u", 70)
    assert cache.tracked() == 1 and cache.pending_tracked() == 1
    assert cache.take_overdue(100, 30) == [("u", "default", "n", b'{"a":1}', 70)] and cache.take_overdue(100, 30) == []
    cache.set_pending_since("u", None)  # ... and clearing one leaves the other
    assert cache.deadline("u") == 70 and cache.tracked() == 1 and cache.take_overdue(10 ** 9, 0) == []
    cache.set_pending_since("u", 60)
    cache.set_deadline("u", None)
    assert cache.pending_since("u") == 60 and cache.pending_tracked() == 1 and cache.tracked() == 0
    assert cache.take_pending_overdue(10 ** 9, 0) == [("u", "default", "n", b'{"a":1}', 60)]  # (cleared above: marked anew)
    # a kept core: reported from, dropped when the pending-since is cleared
    cache.put("k", "1", "Pending", "default", "k", None)
    cache.set_pending_since("k", 10)
    cache.keep_core("k", b'{"k":1}')
    assert cache.core_kept("k") is True and cache.get("k")[CORE] == b'{"k":1}'
    assert cache.take_pending_overdue(40, 30) == [("k", "default", "k", b'{"k":1}', 10)]
    cache.keep_core("k", b'{"k":2}')  # the newest Pending line's
    cache.set_pending_since("k", 10)
    assert cache.core_kept("k") is True and cache.get("k")[CORE] == b'{"k":2}'
    cache.set_pending_since("k", None)
    assert cache.get("k")[CORE] is None and cache.core_kept("k") is False and cache.pending_tracked() == 1
    # ... and kept when a send replaced it
    cache.set_pending_since("k", 10)
    cache.keep_core("k", b'{"k":3}')
    cache.set_core("k", b'{"k":4}')
    assert cache.core_kept("k") is False
    cache.set_pending_since("k", None)
    assert cache.get("k")[CORE] == b'{"k":4}'
    # put (a whole new entry) clears everything, the kept mark too
    cache.set_pending_since("k", 10)
    cache.keep_core("k", b'{"k":5}')
    cache.put("k", "2", "Pending", "default", "k", b'{"k":6}')
    assert cache.pending_since("k") is None and cache.core_kept("k") is False and cache.get("k")[CORE] == b'{"k":6}'
    cache.set_pending_since("k", None)
    assert cache.get("k")[CORE] == b'{"k":6}'
    cache.set_pending_since("k", 60)
    assert cache.take_pending_overdue(90, 30) == [("k", "default", "k", b'{"k":6}', 60)]  # the mark went too
    # ... and so does every way an entry goes
    cache.observe("DELETED", "k", "3", "Pending", "default", "k")
    cache.observe("DELETED", "u", "3", "Pending", "default", "n")
    assert cache.pending_tracked() == 0 and cache.pending_since("k") is None and len(cache) == 0
    for gone in (lambda: cache.pop("v"), lambda: cache.drop_namespaces(["ns-a"]),
                 lambda: cache.drop_namespaces_except(["default"]), cache.clear):
        cache.put("v", "1", "Pending", "ns-a", "m", None)
        cache.set_pending_since("v", 7)
        cache.keep_core("v", b"{}")
        assert cache.pending_tracked() == 1
        gone()
        assert cache.pending_tracked() == 0 and cache.pending_since("v") is None and cache.core_kept("v") is False
        assert cache.take_pending_overdue(10 ** 9, 0) == []
    # scope_ns, negative values, int64 ends, several pods; to_records() writes a kept core like any core
    cache.clear()
    for i, ns in enumerate(["ns-a", "ns-b", "ns-a", None]):
        cache.put("p%d" % i, "1", "Pending", ns, "n%d" % i, None)
        cache.keep_core("p%d" % i, b'{"i":%d}' % i)
    cache.put("bare", "1", "Pending", "ns-b", "bare", None)
    for uid, since in (("p0", -62135596800), ("p1", 0), ("p2", 253402300799), ("p3", -1), ("bare", 0)):
        cache.set_pending_since(uid, since)
    assert cache.pending_tracked() == 5 and cache.pending_since("p0") == -62135596800
    assert cache.take_pending_overdue(30, 30, "ns-c") == []
    assert cache.take_pending_overdue(30, 30, "ns-b") == [("p1", "ns-b", "n1", b'{"i":1}', 0)]
    assert cache.take_pending_overdue(30, 30, "ns-a") == [("p0", "ns-a", "n0", b'{"i":0}', -62135596800)]
    assert cache.take_pending_overdue(30, 30) == [("p3", None, "n3", b'{"i":3}', -1)]
    assert cache.take_pending_overdue(253402300799 + 30, 30, "ns-a") == [("p2", "ns-a", "n2", b'{"i":2}', 253402300799)]
    cache.keep_core("bare", b"{}")
    assert cache.take_pending_overdue(30, 30) == [("bare", "ns-b", "bare", b"{}", 0)]
    for uid, since in (("p0", 2 ** 63 - 1), ("p1", -2 ** 63)):
        cache.set_pending_since(uid, None)
        cache.keep_core(uid, b"{}")
        cache.set_pending_since(uid, since)
        assert cache.pending_since(uid) == since
    assert [t[0] for t in cache.take_pending_overdue(2 ** 63 - 1, 2 ** 62)] == ["p1"]  # compared without overflow
    records = cache.to_records()
    assert all(len(r) == 6 for r in records) and sorted(r[5] for r in records) == sorted(['{"i":2}', '{"i":3}', "{}", "{}", "{}"])
    fresh = make_pod_cache(native, records)  # after a restart a kept core is an ordinary one
    assert fresh.pending_tracked() == 0 and fresh.pending_since("p0") is None and len(fresh) == 5
    assert not any(fresh.core_kept(u) for u, _ in fresh.items())
    fresh.set_pending_since("p2", 5)
    fresh.set_pending_since("p2", None)
    assert fresh.get("p2")[CORE] == b'{"i":2}'
    cache.load_records(records)  # records over live entries: whole new entries, as put()
    assert cache.pending_tracked() == 0 and cache.take_pending_overdue(2 ** 62, 0) == []
    assert not any(cache.core_kept(u) for u, _ in cache.items())


# ----------------------------------------------------------------------------- a pod's life with sweeps (test 5)

def run_script(s, native, script, cache=None):
    """``script``: ("feed", bytes), ("sweep", now_s[, scope_ns]) and ("look", uid) steps.
    -> (calls, the submitted bytes, counters, control event types, what each
    sweep returned, what each look saw: (pending_since, pending_tracked, has a core, core_kept))."""
    p, rec, m = pipeline(s, native, cache)
    ctrl, swept, looks = [], [], []
    for step in script:
        if step[0] == "feed":
            ctrl += feed(p, native, step[1])
        elif step[0] == "sweep":
            swept.append(p.report_overdue(step[1], 0, *step[2:]))
        else:
            ent = p.cache.get(step[1])
            looks.append((p.cache.pending_since(step[1]), p.cache.pending_tracked(),
                          ent is not None and ent[CORE] is not None, p.cache.core_kept(step[1])))
    return rec.calls, rec.raw, {k: m.c.get(k, 0) for k in COUNTERS}, [c[0] for c in ctrl], swept, looks


def both_scripts(env, ov, script):
    s = settings_for(env, ov)
    py = run_script(s, False, script)
    nat = run_script(s, True, script)
    assert py == nat  # the calls, the bytes, the counters, the sweeps' returns, what each look saw
    return py


def feeds(events, one_read):
    return [("feed", lines(events))] if one_read else [("feed", event_line(t, o)) for t, o in events]


def rvs(calls):
    """(event type, resourceVersion of the payload, pending_seconds of its alert or None)."""
    return [(et, int(core["extra"]["resource_version"]), (core.get("alert") or {}).get("pending_seconds"))
            for _, et, _, _, core in calls]


def created(pod):
    from k8s_watcher_amd.models.findings import pending_since
    since = pending_since(pod)
    assert since is not None
    return since


def check_pod_life():
    f = PodFactory(seed=61, namespaces=["default"])
    p0, q0, d0 = f.new_pod(), f.new_pod(), f.new_pod()
    sched, run_, q_run = f.scheduled(p0), f.running(p0), f.running(q0)
    uid, S = p0["metadata"]["uid"], created(p0)
    assert C1_S <= S <= C1_S + 2 and created(sched) == S  # podgen's BASE_TIME
    phase = merged(RV_EXTRA, {"watcher": {"notify_on": "phase_change"}})
    for one_read in (True, False):
        script = (feeds([("ADDED", with_rv(p0, 1)), ("MODIFIED", with_rv(sched, 2))], one_read)
                  + [("look", uid), ("sweep", S + N - 1), ("sweep", S + N), ("sweep", S + N + 1)]
                  + feeds([("MODIFIED", with_rv(sched, 3))], one_read) + [("look", uid), ("sweep", S + 2 * N)]
                  + feeds([("MODIFIED", with_rv(run_, 4))], one_read) + [("look", uid), ("sweep", S + 3 * N)]
                  # a second pod reaches Running before N; a third is deleted while Pending
                  + feeds([("ADDED", with_rv(q0, 5)), ("MODIFIED", with_rv(q_run, 6)), ("ADDED", with_rv(d0, 7))], one_read)
                  + [("look", d0["metadata"]["uid"])] + feeds([("DELETED", with_rv(d0, 8))], one_read)
                  + [("look", d0["metadata"]["uid"]), ("sweep", S + 10 * N)])
        # production, the critical filter on: nothing of a Pending or Running pod is sent but the alert
        calls, raw, c, ctrl, swept, looks = both_scripts("production", merged(PO(), RV_EXTRA), script)
        assert ctrl == [] and swept == [0, 1, 0, 0, 0, 0]
        assert rvs(calls) == [("MODIFIED", 2, N), ("DELETED", 8, None)]  # the core of the newest Pending line
        assert looks == [(S, 1, True, True), (S, 1, True, True), (None, 0, False, False),
                         (created(d0), 1, True, True), (None, 0, False, False)]
        assert c["events_pending_overdue"] == 1 and c["events_received"] == 8 and c["events_filtered_critical"] == 7
        alert = dict(calls[0][4])
        assert alert.pop("alert") == {"kind": "pending_overdue", "since_unix": S, "pending_seconds": N}
        assert calls[0][:4] == (uid, "MODIFIED", "default", p0["metadata"]["name"]) and alert["status"]["phase"] == "Pending"
        assert list(json.loads(raw[0]))[-1] == "alert"  # spliced in before the closing brace
        assert raw[0].endswith(b',"alert":{"kind":"pending_overdue","since_unix":%d,"pending_seconds":%d}}' % (S, N))
        # ... and the option off: byte-identical notifications and counters, with every alert off and with this one at 0
        for off in (RV_EXTRA, merged(PO(0), RV_EXTRA)):
            o_calls, o_raw, o_c, _, o_swept, o_looks = both_scripts("production", off, script)
            assert o_raw == raw[1:] and o_swept == [0] * 6 and o_c == dict(c, events_pending_overdue=0)
            assert o_looks == [(None, 0, False, False)] * 5  # no core for a pod nothing was sent of
        # staging, notify_on: phase_change: the Pending lines after the first are unchanged and kept
        calls, raw, c, _, swept, looks = both_scripts("staging", merged(PO(), phase), script)
        assert swept == [0, 1, 0, 0, 0, 0]
        assert rvs(calls) == [("ADDED", 1, None), ("MODIFIED", 2, N), ("MODIFIED", 4, None), ("ADDED", 5, None),
                              ("MODIFIED", 6, None), ("ADDED", 7, None), ("DELETED", 8, None)]
        assert looks == [(S, 1, True, True), (S, 1, True, True), (None, 0, True, False),  # Running was sent: its core
                         (created(d0), 1, True, False), (None, 0, False, False)]
        assert c["events_pending_overdue"] == 1 and c["events_unchanged"] == 2
        assert calls[1][4]["alert"] == {"kind": "pending_overdue", "since_unix": S, "pending_seconds": N}
        for off in (phase, merged(PO(0), phase)):
            o_calls, o_raw, o_c, _, o_swept, _ = both_scripts("staging", off, script)
            assert o_raw == raw[:1] + raw[2:] and o_swept == [0] * 6 and o_c == dict(c, events_pending_overdue=0)
    # a Pending pod that begins terminating: the terminating alerts own it, and each kind reports once
    both_on = merged(PO(terminating=True, terminating_overdue_seconds=30), RV_EXTRA)
    from test_termination_overdue import T1_S
    script = (feeds([("ADDED", with_rv(p0, 1))], True) + [("sweep", S + N), ("look", uid)]
              + feeds([("MODIFIED", deleting(sched, 2))], True) + [("look", uid), ("sweep", T1_S + 30), ("sweep", T1_S + 31)])
    calls, _, c, _, swept, looks = both_scripts("production", both_on, script)
    assert swept == [1, 1, 0] and looks == [(S, 1, True, True), (None, 0, True, False)]
    assert [(et, (core.get("alert") or {}).get("kind")) for _, et, _, _, core in calls] == [
        ("MODIFIED", "pending_overdue"), ("MODIFIED", None), ("MODIFIED", "termination_overdue")]
    assert c["events_pending_overdue"] == 1 and c["events_termination_overdue"] == 1 and c["events_terminating"] == 1
    # a line whose core cannot be built leaves none and reports nothing: the pod is reportable once a later line does
    bad = event_line("ADDED", with_rv(p0, 1)).replace(b'"containers":[{', b'"containers":[{"name"},{', 1)
    script = [("feed", bad), ("look", uid), ("sweep", S + N)] + feeds([("MODIFIED", with_rv(sched, 2))], True) + [
        ("look", uid), ("sweep", S + N)]
    ov = merged(PO(), RV_EXTRA, {"watcher": {"validate": "payload"}})
    calls, _, c, ctrl, swept, looks = both_scripts_native_only("production", ov, script)
    assert ctrl == [] and swept == [0, 1] and looks == [(S, 1, False, False), (S, 1, True, True)]
    # every extra field on: the bodies are the same bytes from both engines (both_scripts compares them)
    from k8s_watcher_amd.models.payload import EXTRA_NAMES
    everything = {"watcher": {"payload_extra_fields": list(EXTRA_NAMES)}}
    calls, raw, _, _, swept, _ = both_scripts("production", merged(PO(), everything),
                                              feeds([("ADDED", with_rv(p0, 1))], True) + [("sweep", S + N + 3)])
    assert swept == [1] and raw[-1].endswith(b'"pending_seconds":%d}}' % (N + 3))
    # the log line, with log_events
    for native in (False, True):
        p, rec, _ = pipeline(settings_for("production", merged(PO(), RV_EXTRA)), native)
        p.log_events_setting = True
        seen = []
        p.elog.log = lambda level, msg: seen.append((level, msg))
        feed(p, native, lines([("ADDED", with_rv(p0, 1))]))
        assert p.report_overdue(S + N + 3, 0) == 1
        name = p0["metadata"]["name"]
        assert (20, f"Pod pending overdue: default/{name} - {N + 3}s since creationTimestamp") in seen, (native, seen)


def both_scripts_native_only(env, ov, script):
    """A line only the native light parse accepts (a sub-tree it defers is
    malformed): json.loads rejects it whole, so there is no Python run to
    compare. With the option off the critical filter drops it unreported."""
    s = settings_for(env, ov)
    off = run_script(settings_for(env, merged(ov, PO(0))), True, script)
    assert off[3] == [] and off[0] == []
    return run_script(s, True, script)


def test_pod_life_with_sweeps():
    check_pod_life()


# ----------------------------------------------------------------------------- partitioned against serial (test 6)

PARTITIONS = 16


def pending_batch(seed=7):
    """One batch, every pod's lines interleaved with the others': the fewest
    pods (128 at least: one namespace in five is this shard's and reportable)
    that put one into every one of the 16 partitions. A
    half stay Pending over two to four lines, the others reach Running, are
    deleted while Pending or begin terminating."""
    from k8s_watcher_amd.ops.native import load
    part = load().apply_partition
    f = PodFactory(seed=seed, namespaces=NAMESPACES)
    scripts, parts = [], set()
    while len(scripts) < 128 or len(parts) < PARTITIONS:
        p0 = f.new_pod()
        sched, run_ = f.scheduled(p0), f.running(p0)
        k = len(scripts) % 8
        steps = [("ADDED", p0), ("MODIFIED", sched)]
        steps += {0: [("MODIFIED", sched)], 1: [("MODIFIED", run_)], 2: [], 3: [("MODIFIED", sched), ("MODIFIED", sched)],
                  4: [("DELETED", sched)], 5: [], 6: [("MODIFIED", run_), ("MODIFIED", run_)],
                  7: [("MODIFIED", deleting(sched, 0))]}[k]
        parts.add(part(p0["metadata"]["uid"]))
        scripts.append((p0, steps))
    out, rv = [], 0
    for k in range(4):
        for _, steps in scripts:
            if k < len(steps):
                rv += 1
                out.append(event_line(steps[k][0], with_rv(steps[k][1], rv)))
    return b"".join(out), [p for p, _ in scripts], len(out)


def feed_and_sweep(env, ov, warm, data, partitioned, now_s):
    """``data`` as one batch through the native pipeline (3 decode workers) and
    the native notifier, then one sweep at ``now_s``; -> the sink's alert
    bodies by uid, the other bodies, every cached pod's pending-since and kept
    mark, pending_tracked(), the counters, the growth of apply_stats() over the
    batch and the sweep's return."""
    from k8s_watcher_amd.ops.decode import PyDecoder
    from k8s_watcher_amd.ops.native import load
    from k8s_watcher_amd.parallel.native_notifier import NativeNotifierPool
    from k8s_watcher_amd.testing.stub_sink import StubSink

    async def body():
        sink = StubSink()
        await sink.start()
        s = load_settings(env, overrides=merged(ov, {"clusterapi": {"base_url": sink.url, "health_check_on_start": False}}),
                          environ={})
        m = Metrics()
        pool = NativeNotifierPool(s.clusterapi, m)
        p = EventPipeline(s, PyDecoder(env), pool, m)
        p.log_events_setting = False
        kw = load()
        dpool = kw.DecodePool(3)
        p.attach_native(dpool)
        prev = kw.set_partitioned_apply(partitioned)
        try:
            ctrl = [c[0] for c in p.handle_raw(warm, 1, framed=False)]
            before = kw.apply_stats()
            ctrl += [c[0] for c in p.handle_raw(data, 1, framed=False)]
            after = kw.apply_stats()
        finally:
            kw.set_partitioned_apply(prev)
        stats = {k: after[k] - before[k] for k in after if isinstance(after[k], int)}
        tracked = p.cache.pending_tracked()
        swept = p.report_overdue(now_s, 1)
        assert await pool.drain(20) and ctrl == []
        sent = [{k: v for k, v in x.items() if k != "event_timestamp"} for x in sink.state.payloads()]
        alerts_ = {x["uid"]: json.dumps(x, sort_keys=True) for x in sent if "alert" in x}
        assert len(alerts_) == sum("alert" in x for x in sent) and all(x["event_type"] == "MODIFIED" for x in sent if "alert" in x)
        rest = collections.Counter(json.dumps(x, sort_keys=True) for x in sent if "alert" not in x)
        since = {u: (p.cache.pending_since(u), p.cache.core_kept(u), e[CORE]) for u, e in p.cache.items()}
        counters = {k: v for k, v in m.c.items() if k.startswith(("events_", "bookmarks")) and v}
        assert p.cache.pending_tracked() == tracked
        await pool.close()
        await sink.stop()
        dpool.close()
        return alerts_, rest, since, tracked, counters, stats, swept

    return run(body(), timeout=60)


def check_partitioned_matches_serial():
    from k8s_watcher_amd.ops.native import load
    data, pods, n = pending_batch()
    warm = warm_up()
    assert 128 <= len(pods) <= 200 and 2 * len(pods) <= n <= 4 * len(pods)
    assert {shard_of(ns) for ns in NAMESPACES} == {0, 1}
    mine = [ns for ns in NAMESPACES if shard_of(ns) == 0]
    assert len(mine) >= 2  # one of this shard's namespaces is filtered, another is not
    now_s = C1_S + 10 * N
    sharded = {"watcher": {"shard": {"count": 2, "index": 0}, "namespaces": [ns for ns in NAMESPACES if ns != mine[0]]}}
    for env, ov in (("production", merged(PO(), RV_EXTRA, sharded)),
                    ("staging", merged(PO(terminating=True), RV_EXTRA, sharded, {"watcher": {"notify_on": "phase_change"}}))):
        s_alerts, s_rest, s_since, s_tracked, s_cnt, s_stats, s_swept = feed_and_sweep(env, ov, warm, data, False, now_s)
        p_alerts, p_rest, p_since, p_tracked, p_cnt, p_stats, p_swept = feed_and_sweep(env, ov, warm, data, True, now_s)
        # the partitioned path was taken: one batch, every line of it applied by its partition
        assert s_stats["partitioned_batches"] == 0 and s_stats["serial_batches"] == 1
        assert p_stats["partitioned_batches"] == 1 and p_stats["partitioned_lines"] == n and p_stats["serial_batches"] == 0
        assert p_stats["payload_built"] == s_stats["payload_built"] > 0
        assert p_alerts == s_alerts and p_rest == s_rest and p_since == s_since and p_tracked == s_tracked and p_cnt == s_cnt
        assert p_swept == s_swept == len(s_alerts) == s_cnt["events_pending_overdue"]
        assert s_cnt["events_filtered_namespace"] > 0 and s_cnt["events_other_shard"] > 0
        # the condition: enough reported pods, spread over the store's shards
        part = load().apply_partition
        assert len({part(p["metadata"]["uid"]) for p in pods}) == PARTITIONS
        assert len(s_alerts) >= 8 and len({part(u) for u in s_alerts}) >= 4, (len(s_alerts), {part(u) for u in s_alerts})
        assert s_tracked > len(s_alerts)  # (pods of the namespace the filter drops are tracked and have no core)
        for u, body in s_alerts.items():
            since = s_since[u][0]
            assert json.loads(body)["alert"] == {"kind": "pending_overdue", "since_unix": since, "pending_seconds": now_s - since}
            assert json.loads(body)["extra"]["resource_version"] == json.loads(s_since[u][2])["extra"]["resource_version"]
        # the Python engine: the same reports, values and counters
        p, rec, m = pipeline(settings_for(env, ov), False)
        assert feed(p, False, warm) == [] and feed(p, False, data) == []
        assert p.cache.pending_tracked() == s_tracked
        assert {u: (p.cache.pending_since(u), p.cache.core_kept(u), e[CORE]) for u, e in p.cache.items()} == s_since
        assert p.report_overdue(now_s, 0) == s_swept
        got = {u: json.dumps(dict(core, event_type=et), sort_keys=True) for u, et, _, _, core in rec.calls if "alert" in core}
        assert got == s_alerts
        assert {k: v for k, v in m.c.items() if k.startswith(("events_", "bookmarks")) and v} == s_cnt


def test_partitioned_apply_matches_serial():
    check_partitioned_matches_serial()


# ----------------------------------------------------------------------------- relist and restart (test 7)

def relist(p, native, items, scope=None, notify=True):
    """A LIST of ``items`` reconciled by the engine's own relist; -> control events."""
    from test_native_relist import list_pages, native_relist
    if native:
        return native_relist(p, items, scope, notify=notify)[0]
    evs = p.decoder.decode_list(list_pages(items, 10 ** 6)[0])[2]
    assert all(len(e) == 14 for e in evs)
    return p.reconcile(evs, 0, notify=notify, scope_ns=scope)


def alert_uids(calls):
    return sorted(u for u, _, _, _, core in calls if "alert" in core)


def check_relist(native):
    f = PodFactory(seed=71, namespaces=["default"])
    a, b, c_, d, e = (f.new_pod() for _ in range(5))
    uid = lambda p: p["metadata"]["uid"]  # noqa: E731
    s = settings_for("production", merged(PO(), RV_EXTRA))
    p, rec, m = pipeline(s, native)
    feed(p, native, lines([("ADDED", with_rv(f.running(a), 1)), ("ADDED", with_rv(b, 2)), ("ADDED", with_rv(c_, 3)),
                           ("ADDED", with_rv(f.running(d), 4)), ("ADDED", with_rv(e, 5))]))
    now = created(e) + N
    assert p.cache.pending_tracked() == 3 and p.report_overdue(now, 0) == 3 and alert_uids(rec.calls) == sorted(map(uid, (b, c_, e)))
    del rec.calls[:]
    # the gap (a 410): b moved on Pending (reported already), c is gone while Pending, d moved on, e runs now;
    # a is unchanged
    listed = [with_rv(f.running(a), 1), with_rv(f.scheduled(b), 11), with_rv(f.running(d), 12), with_rv(f.running(e), 13)]
    assert relist(p, native, listed) == []
    # c's DELETED is built from its kept core, the one the alert was built from, not from the cache's summary
    assert [(u, et) for u, et, *_ in rec.calls] == [(uid(c_), "DELETED")]
    gone = rec.calls[0][4]
    assert gone["extra"]["resource_version"] == "3" and gone["status"]["phase"] == "Pending" and "alert" not in gone
    assert p.cache.pending_tracked() == 1 and p.cache.pending_since(uid(b)) == created(b)
    assert p.cache.pending_since(uid(e)) is None and p.cache.get(uid(e))[CORE] is None  # the kept core went with it
    assert json.loads(p.cache.get(uid(b))[CORE])["extra"]["resource_version"] == "11" and p.cache.core_kept(uid(b))
    del rec.calls[:]
    assert p.report_overdue(now + N, 0) == 0 and m.c["events_pending_overdue"] == 3  # b was reported before the gap
    # a restart: the cache rebuilt from its records has the cores (kept ones like any) and no pending-since
    feed(p, native, lines([("ADDED", with_rv(c_, 20))]))
    records = p.cache.to_records()
    assert all(len(r) == 6 for r in records) and sum(r[5] is not None for r in records) == 2
    q, rec2, m2 = pipeline(s, native, make_pod_cache(native, records))
    assert q.cache.pending_tracked() == 0 and q.report_overdue(2 ** 40, 0) == 0
    # ... a relist whose items are all unchanged restores every value, and the sweep reports from the
    # checkpointed cores: the mark did not persist, so b once more
    listed = listed + [with_rv(c_, 20)]
    assert relist(q, native, listed) == [] and rec2.calls == []
    assert q.cache.pending_tracked() == 2 and q.cache.pending_since(uid(b)) == created(b)
    assert q.cache.pending_since(uid(c_)) == created(c_)
    assert q.report_overdue(now + 5, 0) == 2 and alert_uids(rec2.calls) == sorted([uid(b), uid(c_)])
    assert {core["extra"]["resource_version"] for *_, core in rec2.calls} == {"11", "20"}  # the cores as checkpointed
    assert all(core["alert"]["kind"] == "pending_overdue" for *_, core in rec2.calls)
    assert q.report_overdue(now + 6, 0) == 0
    # after the restart b's core counts as an ordinary one: Running clears the value and the core stays
    feed(q, native, lines([("MODIFIED", with_rv(f.running(b), 30))]))
    assert q.cache.pending_since(uid(b)) is None and q.cache.pending_tracked() == 1
    assert json.loads(q.cache.get(uid(b))[CORE])["extra"]["resource_version"] == "11"
    # an unchanged item that is not Pending (cannot happen without a new resourceVersion; the rule all the same)
    q.cache.set_pending_since(uid(d), 5)
    assert relist(q, native, listed) == []
    assert q.cache.pending_since(uid(d)) is None
    # a silent relist (initial_list: skip) tracks nothing, changed items or unchanged
    for cache in (None, make_pod_cache(native, records)):
        r, rec3, _ = pipeline(s, native, cache)
        assert relist(r, native, listed, notify=False) == []
        assert rec3.calls == [] and len(r.cache) == 5 and r.cache.pending_tracked() == 0 and r.report_overdue(2 ** 40, 0) == 0


@pytest.mark.parametrize("native", [True, False], ids=["native-relist", "python-reconcile"])
def test_relist_and_restart(native):
    check_relist(native)


def scoped_pods(seed, ns, n):
    f = PodFactory(seed=seed, namespaces=[ns])
    return f, [f.new_pod() for _ in range(n)]


def check_shared_cache(native):
    """Two scopes on one cache: B is swept while A's relist stands in mid-walk."""
    from test_native_relist import list_pages
    ov = merged(PO(), RV_EXTRA, {"watcher": {"namespace_scope": "server", "namespaces": ["ns-a", "ns-b"]}})
    s = settings_for("production", ov)
    (fa, pods_a), (fb, pods_b) = scoped_pods(91, "ns-a", 90), scoped_pods(92, "ns-b", 12)
    uid = lambda p: p["metadata"]["uid"]  # noqa: E731
    pend_a = {uid(p) for p in pods_a[::3]}  # these stay Pending over A's relist; the others run by then
    pend_b = {uid(p) for p in pods_b[::2]}
    listed_a = [with_rv(fa.scheduled(p) if uid(p) in pend_a else fa.running(p), 500 + i) for i, p in enumerate(pods_a[:-5])]
    now = C1_S + 1000

    def world():
        cache = make_pod_cache(native)
        pa, rec_a, _ = pipeline(s, native, cache)
        pb, rec_b, _ = pipeline(s, native, cache)
        feed(pa, native, lines([("ADDED", with_rv(p, i + 1)) for i, p in enumerate(pods_a)]))
        feed(pb, native, lines([("ADDED", with_rv(p if uid(p) in pend_b else fb.running(p), 200 + i))
                                for i, p in enumerate(pods_b)]))
        assert cache.pending_tracked() == len(pods_a) + len(pend_b) and rec_a.calls == rec_b.calls == []
        return cache, pa, rec_a, pb, rec_b

    def relist_a(pa, between):
        if not native:  # the Python reconcile is one step: the sweep of B comes before it
            between()
            evs = pa.decoder.decode_list(list_pages(listed_a, 10 ** 6)[0])[2]
            return pa.reconcile(evs, 0, scope_ns="ns-a")
        rl = pa.native.relist("ns-a", True)
        ctrl = []
        pages = list_pages(listed_a, 37)
        for k, body in enumerate(pages):
            rl.page(body)
            done = False
            while not done:
                done, c = pa.native_slice(rl.step, 0.0, 0)  # slice budget 0
                ctrl += c
            if k == 0:
                assert len(pages) > 2
                between()  # A's relist stands between two pages of its walk
        done, slices = False, 0
        while not done:
            done, c = pa.native_slice(rl.sweep, 0.0, 0)
            ctrl += c
            slices += 1
            if slices == 1:
                between()  # ... and in its sweep
        assert rl.stats()["deleted"] == 5
        return ctrl

    def state(cache, rec):
        return (sorted((u, et, json.dumps(core, sort_keys=True)) for u, et, _, _, core in rec.calls),
                sorted(map(json.dumps, cache.to_records())), {u: cache.pending_since(u) for u, _ in cache.items()})

    cache0, pa0, rec_a0, _, _ = world()
    assert relist_a(pa0, lambda: None) == []
    unswept = state(cache0, rec_a0)
    assert sorted(et for _, et, *_ in rec_a0.calls) == ["DELETED"] * 5  # the vanished Pending pods, from their kept cores
    assert all(core["status"]["phase"] == "Pending" and int(core["extra"]["resource_version"]) > 85 for *_, core in rec_a0.calls)
    cache, pa, rec_a, pb, rec_b = world()
    sweeps = []
    assert relist_a(pa, lambda: sweeps.append(pb.report_overdue(now, 0, "ns-b"))) == []
    assert sweeps[0] == len(pend_b) and sum(sweeps) == len(pend_b)  # once, whenever it ran again
    assert set(alert_uids(rec_b.calls)) == pend_b and len(rec_b.calls) == len(pend_b)  # only B's pods
    assert state(cache, rec_a) == unswept  # A's relist completed as if nobody had swept
    listed_uids = {uid(p) for p in pods_a[:-5]}
    assert cache.pending_tracked() == len(pend_b) + len(pend_a & listed_uids)
    del rec_a.calls[:]
    assert pa.report_overdue(now, 0, "ns-a") == len(pend_a & listed_uids)
    assert set(alert_uids(rec_a.calls)) == pend_a & listed_uids
    assert all(int(core["extra"]["resource_version"]) >= 500 for *_, core in rec_a.calls)  # the relist's lines' cores
    assert pa.report_overdue(now, 0, "ns-a") == 0 and pb.report_overdue(now, 0, "ns-b") == 0
    assert pa.report_overdue(now, 0, "ns-c") == 0 and pa.report_overdue(now, 0) == 0


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_sweep_between_the_slices_of_another_scopes_relist(native):
    check_shared_cache(native)


# ----------------------------------------------------------------------------- filters

def test_filters():
    f = PodFactory(seed=95, namespaces=["default", "elsewhere"])
    mine, other = f.new_pod(namespace="default"), f.new_pod(namespace="elsewhere")
    events = [("ADDED", with_rv(mine, 1)), ("ADDED", with_rv(other, 2))]
    now = created(other) + N
    # a namespace outside watcher.namespaces: tracked, no core kept, never reported
    ov = merged(PO(), RV_EXTRA, {"watcher": {"namespaces": ["default"]}})
    script = [("feed", lines(events)), ("look", other["metadata"]["uid"]), ("sweep", now), ("sweep", 10 * now)]
    for env, more in (("production", {}), ("staging", {"watcher": {"notify_on": "phase_change"}})):
        calls, _, c, _, swept, looks = both_scripts(env, merged(ov, more), script)
        assert swept == [1, 0] and looks == [(created(other), 2, False, False)]
        assert alert_uids(calls) == [mine["metadata"]["uid"]]
    # a pod of another shard is not even cached
    import zlib
    for index in (0, 1):
        sh = merged(PO(), RV_EXTRA, {"watcher": {"namespaces": [], "shard": {"count": 2, "index": index}}})
        calls, _, c, _, swept, _ = both_scripts("production", sh, [("feed", lines(events)), ("sweep", now)])
        owned = [p for p in (mine, other) if zlib.crc32(p["metadata"]["namespace"].encode()) % 2 == index]
        assert swept == [len(owned)] and c["events_other_shard"] == 2 - len(owned)
        assert alert_uids(calls) == sorted(p["metadata"]["uid"] for p in owned)


# ----------------------------------------------------------------------------- through the native notifier (test 8)

def test_through_the_native_notifier():
    from k8s_watcher_amd.ops.decode import PyDecoder
    from k8s_watcher_amd.parallel.native_notifier import NativeNotifierPool
    from k8s_watcher_amd.testing.stub_sink import StubSink
    f = PodFactory(seed=64, namespaces=["default"])
    p0, q0 = f.new_pod(), f.new_pod()
    S = created(p0)

    async def body():
        sink = StubSink()
        await sink.start()
        s = load_settings("production", environ={}, overrides=merged(PO(), RV_EXTRA, {
            "watcher": {"decode_threads": 0}, "clusterapi": {"base_url": sink.url, "health_check_on_start": False}}))
        m = Metrics()
        pool = NativeNotifierPool(s.clusterapi, m)
        p = EventPipeline(s, PyDecoder("production"), pool, m)
        p.log_events_setting = False
        p.attach_native()
        p.handle_raw(lines([("ADDED", with_rv(p0, 1)), ("MODIFIED", with_rv(f.scheduled(p0), 2)), ("ADDED", with_rv(q0, 3))]),
                     1, framed=False)
        swept = p.report_overdue(S + N + 1, 2)
        # in the same tick, the first pod's DELETED
        p.handle_raw(lines([("DELETED", with_rv(f.scheduled(p0), 4))]), 3, framed=False)
        assert await pool.drain(20)
        got = sink.state.payloads()
        counters = dict(m.c)
        tracked = p.cache.pending_tracked()
        await pool.close()
        await sink.stop()
        return swept, got, counters, tracked

    swept, got, c, tracked = run(body(), timeout=60)
    assert swept == 2 and tracked == 1 and c["events_pending_overdue"] == 2 and c.get("notify_failed", 0) == 0
    mine = [x for x in got if x["uid"] == p0["metadata"]["uid"]]
    assert [(x["event_type"], "alert" in x) for x in mine] == [("MODIFIED", True), ("DELETED", False)]  # in order
    alert = mine[0]
    assert alert["alert"] == {"kind": "pending_overdue", "since_unix": S, "pending_seconds": N + 1}
    assert list(alert)[-3:] == ["alert", "event_timestamp", "event_type"] and alert["extra"]["resource_version"] == "2"
    other = [x for x in got if x["uid"] == q0["metadata"]["uid"]]
    assert [(x["event_type"], "alert" in x) for x in other] == [("MODIFIED", True)]


@pytest.mark.parametrize("engine", ["native", "python"])
def test_end_to_end_service(engine):
    """The only test that reads the wall clock: the service's own 1 s loop."""
    import asyncio
    import time
    from k8s_watcher_amd.engine.service import WatcherService
    from k8s_watcher_amd.kube.kubeconfig import KubeEndpoint
    from k8s_watcher_amd.testing.fake_apiserver import FakeApiServer
    from k8s_watcher_amd.testing.stub_sink import StubSink

    async def body():
        srv = FakeApiServer()
        await srv.start()
        sink = StubSink()
        await sink.start()
        s = load_settings("production", environ={}, overrides=merged(PO(3600), RV_EXTRA, {
            "clusterapi": {"base_url": sink.url}, "watcher": {"engine": engine}}))
        svc = WatcherService(s, endpoint=KubeEndpoint(server=srv.url), metrics=Metrics())
        await svc.start()
        gauge = svc.metrics.gauges["pods_pending_tracked"]
        assert "pods_terminating_tracked" not in svc.metrics.gauges
        f = PodFactory(seed=52, namespaces=["default"])
        pod, young = f.new_pod(), f.new_pod()
        past = time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime(time.time() - 3600))
        pod["metadata"]["creationTimestamp"] = past
        young["metadata"]["creationTimestamp"] = time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime(time.time() - 60))
        srv.create(young)
        srv.create(pod)
        t0 = time.monotonic()
        await sink.state.wait_for(1, timeout=10)  # the alert: the ADDED itself is filtered
        waited = time.monotonic() - t0
        tracked = [gauge()]
        await asyncio.sleep(1.1)  # one more tick: nothing more
        await svc.notifier.drain(5)
        after_a_tick = list(sink.state.payloads())
        srv.delete(pod["metadata"]["namespace"], pod["metadata"]["name"])
        await sink.state.wait_for(2, timeout=10)
        await svc.notifier.drain(5)
        got = sink.state.payloads()
        tracked.append(gauge())
        counters = dict(svc.metrics.c)
        text = svc.metrics.prometheus_text()
        svc.stop()
        await svc.shutdown()
        await sink.stop()
        await srv.stop()
        return pod, past, waited, after_a_tick, got, tracked, counters, text

    pod, past, waited, after_a_tick, got, tracked, c, text = run(body(), timeout=60)
    assert waited < 10
    assert [(x["event_type"], "alert" in x) for x in after_a_tick] == [("MODIFIED", True)]  # exactly one
    assert [(x["event_type"], "alert" in x) for x in got] == [("MODIFIED", True), ("DELETED", False)]
    assert all(x["uid"] == pod["metadata"]["uid"] for x in got)
    alert = got[0]["alert"]
    want = calendar.timegm(datetime.datetime.strptime(past, "%Y-%m-%dT%H:%M:%SZ").timetuple())
    assert alert["kind"] == "pending_overdue" and alert["since_unix"] == want
    assert 3600 <= alert["pending_seconds"] <= 3600 + 15 and got[0]["status"]["phase"] == "Pending"
    assert tracked == [2.0, 1.0]
    assert c["events_pending_overdue"] == 1 and c["events_filtered_critical"] == 2
    assert "pods_pending_tracked 1" in text
    assert [ln for ln in text.splitlines() if "events_pending_overdue" in ln and not ln.startswith("#")][0].endswith(" 1")


def test_metrics():
    from k8s_watcher_amd.metrics import COUNTERS as DECLARED
    assert "events_pending_overdue" in DECLARED and Metrics().c["events_pending_overdue"] == 0
    f = PodFactory(seed=61, namespaces=["default"])
    p0 = f.new_pod()
    s = settings_for("production", PO())
    for native in (False, True):  # the native pipeline adds to the same counter
        p, _, m = pipeline(s, native)
        feed(p, native, lines([("ADDED", with_rv(p0, 1))]))
        assert p.report_overdue(created(p0) + N, 0) == 1 and m.c["events_pending_overdue"] == 1
        assert m.c["events_termination_overdue"] == 0
