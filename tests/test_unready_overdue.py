"""Pods Running but not Ready for N seconds
(``watcher.alerts.unready_overdue_seconds``).

The finding (``models/findings.py`` ``unready_since`` and its native twin in
``ops/csrc/findings.inc``), ``E_UNREADY_SINCE`` from both decoders, the
unready-since, its own reported mark and the kept core in both caches (the
second timer kind that keeps cores), where an event stores them (watch path
serial and partitioned, native relist, Python reconcile, the unchanged items of
a notifying relist), the sweep's third kind in both engines, and the service's
loop. Every sweep but the end-to-end test's takes its clock as an argument.

Every test here but ``test_option_off_is_the_parent_behaviour`` fails without
the option.
"""

import calendar
import collections
import copy
import datetime
import json
import random

import pytest

from conftest import run
from k8s_watcher_amd.engine.pipeline import EventPipeline
from k8s_watcher_amd.metrics import Metrics
from k8s_watcher_amd.ops.cache import CORE, make_pod_cache
from k8s_watcher_amd.ops.decode import E_UID, make_decoder
from k8s_watcher_amd.testing.podgen import PodFactory, event_line
from k8s_watcher_amd.utils.config import ConfigError, load_settings, parse_override
from test_pod_condition_alerts import RV_EXTRA, alerts, escaped, lines, merged, with_rv
from test_terminating_alerts import NAMESPACES, T1, deleting, md, settings_for, shard_of, warm_up
from test_termination_overdue import RawRecorder, feed, mutated_timestamp, valid_timestamp

KEY = "watcher.alerts.unready_overdue_seconds"
N = 300  # the option's value in these tests
C1_S = 1752025888  # podgen's BASE_TIME, 2025-07-09T01:51:28Z
R1 = "2025-07-09T01:52:00Z"  # a transition time, and its seconds since 1970
R1_S = C1_S + 32
E_UNREADY_SINCE = 14
COUNTERS = ("events_received", "events_filtered_critical", "events_filtered_namespace", "events_unchanged",
            "events_other_shard", "events_container_failure", "events_pod_condition", "events_terminating",
            "events_termination_overdue", "events_pending_overdue", "events_unready_overdue", "bookmarks")


def UO(n=N, **kw):
    return alerts(unready_overdue_seconds=n, **kw)


def stamp(seconds):
    return datetime.datetime.fromtimestamp(seconds, datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ")


def unready(f, pod, since_s, rv=None):
    """``pod`` Running with Ready (and ContainersReady) False since ``since_s``."""
    p = f.running(pod)
    for c in p["status"]["conditions"]:
        if c["type"] in ("Ready", "ContainersReady"):
            c.update(status="False", reason="ContainersNotReady", message="containers with unready status: [app]",
                     lastTransitionTime=stamp(since_s))
    return p if rv is None else with_rv(p, rv)


# ----------------------------------------------------------------------------- config (test 1)

def test_config():
    for env in ("development", "staging", "production"):
        assert load_settings(env, environ={}).watcher.unready_overdue_seconds == 0
    w = load_settings("production", environ={}, overrides=UO(45)).watcher
    # it needs no other option, and may stand beside any
    assert (w.unready_overdue_seconds, w.terminating, w.terminating_overdue_seconds, w.pending_overdue_seconds) == (
        45, False, 0, 0)
    w = load_settings("production", environ={}, overrides=UO(45, terminating=True, terminating_overdue_seconds=7,
                                                              pending_overdue_seconds=9)).watcher
    assert (w.unready_overdue_seconds, w.terminating_overdue_seconds, w.pending_overdue_seconds) == (45, 7, 9)
    assert load_settings("staging", environ={}, overrides=parse_override(KEY + "=30")).watcher.unready_overdue_seconds == 30
    assert load_settings("staging", environ={}, overrides=UO("30")).watcher.unready_overdue_seconds == 30
    assert load_settings("staging", environ={}, overrides=UO(" 4000000000 ")).watcher.unready_overdue_seconds == 4000000000
    for bad in (True, False, 1.5, 30.0, [30], {"seconds": 30}, -1, "soon", "-1", "1.5", "", "3e2", "0x10", None):
        with pytest.raises(ConfigError, match=KEY):
            load_settings("staging", environ={}, overrides=UO(bad))


def test_print_config_shows_the_key(capsys):
    from k8s_watcher_amd.utils.config import dump_effective
    dump_effective(load_settings("production", environ={}))
    assert "unready_overdue_seconds: 0" in capsys.readouterr().out
    dump_effective(load_settings("production", environ={}, overrides=UO(45)))
    assert "unready_overdue_seconds: 45" in capsys.readouterr().out


# ----------------------------------------------------------------------------- the corpus (test 2)

TS = ',"deletionTimestamp":"%s"' % T1


def cond(ctype='"Ready"', status='"False"', time='"%s"' % R1, more=""):
    """A condition as raw JSON text; ``time`` None: no lastTransitionTime."""
    return '{"type":%s,"status":%s%s%s}' % (ctype, status, "" if time is None else ',"lastTransitionTime":%s' % time, more)


SCHED = cond('"PodScheduled"', '"True"')
CREADY = cond('"ContainersReady"', '"False"', '"2025-07-09T01:51:40Z"')


def st(phase='"Running"', conds="[%s,%s,%s]" % (SCHED, cond(), CREADY), more=""):
    """A "status" member as raw JSON text; ``conds`` None: no conditions."""
    return '"status":{"phase":%s,"podIP":"10.244.0.7"%s%s}' % (
        phase, "" if conds is None else ',"conditions":%s' % conds, more)


def ready(*a, **kw):
    return st(conds="[%s,%s]" % (SCHED, cond(*a, **kw)))


# (id, the raw "metadata" member(s), the raw "status" member(s) or None, the event type, unready_since of the pod)
CORPUS = [
    ("unready", md(), st(), "MODIFIED", R1_S),
    ("unready-added", md(), st(), "ADDED", R1_S),
    ("unready-deleted-line", md(), st(), "DELETED", R1_S),  # the function's value; a DELETED line is never examined
    ("ready-true", md(), ready(status='"True"'), "MODIFIED", None),
    ("ready-unknown", md(), ready(status='"Unknown"'), "MODIFIED", None),
    ("ready-literal-false", md(), ready(status="false"), "MODIFIED", None),
    ("ready-lower-false", md(), ready(status='"false"'), "MODIFIED", None),
    ("ready-status-null", md(), ready(status="null"), "MODIFIED", None),
    ("ready-status-number", md(), ready(status="0"), "MODIFIED", None),
    ("ready-status-array", md(), ready(status='["False"]'), "MODIFIED", None),
    ("ready-status-trailing-blank", md(), ready(status='"False "'), "MODIFIED", None),
    ("ready-status-missing", md(), st(conds='[{"type":"Ready","lastTransitionTime":"%s"}]' % R1), "MODIFIED", None),
    ("no-ready-element", md(), st(conds="[%s,%s]" % (SCHED, CREADY)), "MODIFIED", None),
    ("empty-conditions", md(), st(conds="[]"), "MODIFIED", None),
    ("only-ready", md(), st(conds="[%s]" % cond()), "MODIFIED", R1_S),
    ("ready-last", md(), st(conds="[%s,%s,%s]" % (SCHED, CREADY, cond())), "MODIFIED", R1_S),
    ("two-ready-first-false", md(), st(conds="[%s,%s]" % (cond(), cond(status='"True"'))), "MODIFIED", R1_S),
    ("two-ready-first-true", md(), st(conds="[%s,%s]" % (cond(status='"True"'), cond())), "MODIFIED", None),
    ("two-ready-first-without-time", md(), st(conds="[%s,%s]" % (cond(time=None), cond())), "MODIFIED", None),
    ("two-ready-first-unknown", md(), st(conds="[%s,%s]" % (cond(status='"Unknown"'), cond())), "MODIFIED", None),
    ("two-ready-both-false", md(), st(conds="[%s,%s]" % (cond(time='"1970-01-01T00:00:07Z"'), cond())), "MODIFIED", 7),
    ("non-object-before", md(), st(conds='["Ready",null,7,[%s],%s]' % (cond(status='"True"'), cond())), "MODIFIED", R1_S),
    ("non-object-only", md(), st(conds='["Ready","False"]'), "MODIFIED", None),
    ("type-number-before", md(), st(conds="[%s,%s]" % (cond("7", '"True"'), cond())), "MODIFIED", R1_S),
    ("type-null-before", md(), st(conds="[%s,%s]" % (cond("null", '"True"'), cond())), "MODIFIED", R1_S),
    ("type-lower-case", md(), ready('"ready"'), "MODIFIED", None),
    ("type-trailing-blank", md(), ready('"Ready "'), "MODIFIED", None),
    ("type-containers-ready", md(), st(conds="[%s]" % CREADY), "MODIFIED", None),
    ("conditions-object", md(), st(conds=cond()), "MODIFIED", None),
    ("conditions-string", md(), st(conds='"Ready=False"'), "MODIFIED", None),
    ("conditions-null", md(), st(conds="null"), "MODIFIED", None),
    ("conditions-number", md(), st(conds="7"), "MODIFIED", None),
    ("conditions-missing", md(), st(conds=None), "MODIFIED", None),
    ("conditions-repeated-last-ready", md(), st(more=',"conditions":[%s]' % cond(status='"True"')), "MODIFIED", None),
    ("conditions-repeated-last-unready", md(), st(conds="[]", more=',"conditions":[%s]' % cond()), "MODIFIED", R1_S),
    ("conditions-repeated-last-null", md(), st(more=',"conditions":null'), "MODIFIED", None),
    ("no-status", md(), None, "MODIFIED", None),
    ("status-null", md(), '"status":null', "MODIFIED", None),
    ("status-array", md(), '"status":["Running"]', "MODIFIED", None),
    ("status-string", md(), '"status":"Running"', "MODIFIED", None),
    ("status-number", md(), '"status":7', "MODIFIED", None),
    ("status-repeated-last-ready", md(), st() + "," + ready(status='"True"'), "MODIFIED", None),
    ("status-repeated-last-unready", md(), ready(status='"True"') + "," + st(), "MODIFIED", R1_S),
    ("status-repeated-last-empty", md(), st() + ',"status":{}', "MODIFIED", None),
    ("phase-pending", md(), st('"Pending"'), "MODIFIED", None),
    ("phase-succeeded-completed", md(), st('"Succeeded"', "[%s]" % cond(more=',"reason":"PodCompleted"')), "MODIFIED", None),
    ("phase-failed", md(), st('"Failed"'), "MODIFIED", None),
    ("phase-unknown", md(), st('"Unknown"'), "MODIFIED", None),
    ("phase-missing", md(), '"status":{"conditions":[%s]}' % cond(), "MODIFIED", None),
    ("phase-null", md(), st("null"), "MODIFIED", None),
    ("phase-number", md(), st("7"), "MODIFIED", None),
    ("phase-lower-case", md(), st('"running"'), "MODIFIED", None),
    ("phase-escaped", md(), st('"R\\u0075nning"'), "MODIFIED", R1_S),
    ("phase-escaped-other", md(), st('"Runnin\\u0067\\u0020"'), "MODIFIED", None),
    ("phase-repeated-last-pending", md(), st(more=',"phase":"Pending"'), "MODIFIED", None),
    ("phase-repeated-last-running", md(), st('"Pending"', more=',"phase":"Running"'), "MODIFIED", R1_S),
    ("terminating", md(TS), st(), "MODIFIED", None),
    ("terminating-any-text", md(',"deletionTimestamp":""'), st(), "MODIFIED", None),
    ("deletion-null", md(',"deletionTimestamp":null'), st(), "MODIFIED", R1_S),
    ("deletion-number", md(',"deletionTimestamp":1752025892'), st(), "MODIFIED", R1_S),
    ("metadata-null", '"metadata":null', st(), "MODIFIED", R1_S),  # not terminating: no metadata says so
    ("time-absent", md(), ready(time=None), "MODIFIED", None),
    ("time-null", md(), ready(time="null"), "MODIFIED", None),
    ("time-number", md(), ready(time=str(R1_S)), "MODIFIED", None),
    ("time-array", md(), ready(time='["%s"]' % R1), "MODIFIED", None),
    ("time-empty", md(), ready(time='""'), "MODIFIED", None),
    ("time-bad-month", md(), ready(time='"2025-13-09T01:52:00Z"'), "MODIFIED", None),
    ("time-second-60", md(), ready(time='"2025-07-09T01:52:60Z"'), "MODIFIED", None),
    ("time-no-zone", md(), ready(time='"2025-07-09T01:52:00"'), "MODIFIED", None),
    ("time-blank-for-t", md(), ready(time='"2025-07-09 01:52:00Z"'), "MODIFIED", None),
    ("time-any-text", md(), ready(time='"soon, été ✓"'), "MODIFIED", None),
    ("time-offset", md(), ready(time='"2025-07-09T10:52:00+09:00"'), "MODIFIED", R1_S),
    ("time-fraction", md(), ready(time='"2025-07-09T01:52:00.75Z"'), "MODIFIED", R1_S),
    ("time-before-1970", md(), ready(time='"1969-12-31T23:59:59Z"'), "MODIFIED", -1),
    ("time-escaped", md(), ready(time='"2025-07-09T01:52:00\\u005a"'), "MODIFIED", R1_S),
    ("time-escaped-other", md(), ready(time='"2025-07-09T01:52:00\\u007a"'), "MODIFIED", None),
    ("time-repeated-last-null", md(), ready(more=',"lastTransitionTime":null'), "MODIFIED", None),
    ("time-repeated-last-string", md(), ready(time="null", more=',"lastTransitionTime":"%s"' % R1), "MODIFIED", R1_S),
    ("time-key-escaped", md(), ready(time=None, more=',"last\\u0054ransitionTime":"%s"' % R1), "MODIFIED", R1_S),
    ("18-bytes-other-key", md(), ready(time=None, more=',"lastTransitionTimf":"%s"' % R1), "MODIFIED", None),
    ("probe-time-is-not-it", md(), ready(time=None, more=',"lastProbeTime":"%s"' % R1), "MODIFIED", None),
    ("type-value-escaped", md(), ready('"\\u0052eady"'), "MODIFIED", R1_S),
    ("type-value-escaped-all", md(), ready('"\\u0052\\u0065\\u0061\\u0064\\u0079"'), "MODIFIED", R1_S),
    ("type-value-escaped-other", md(), ready('"\\u0052eadz"'), "MODIFIED", None),
    ("type-value-escaped-backslash", md(), ready('"\\\\u0052eady"'), "MODIFIED", None),
    ("type-key-escaped", md(), st(conds='[{"t\\u0079pe":"Ready","status":"False","lastTransitionTime":"%s"}]' % R1),
     "MODIFIED", R1_S),
    ("status-value-escaped", md(), ready(status='"\\u0046alse"'), "MODIFIED", R1_S),
    ("status-value-escaped-other", md(), ready(status='"\\u0046alsy"'), "MODIFIED", None),
    ("status-key-escaped", md(), st(conds='[{"type":"Ready","st\\u0061tus":"False","lastTransitionTime":"%s"}]' % R1),
     "MODIFIED", R1_S),
    ("conditions-key-escaped", md(), '"status":{"phase":"Running","c\\u006fnditions":[%s]}' % cond(), "MODIFIED", R1_S),
    ("type-repeated-last-ready", md(), ready(more=',"type":"Ready"', ctype='"Other"'), "MODIFIED", R1_S),
    ("type-repeated-last-other", md(), ready(more=',"type":"Other"'), "MODIFIED", None),
    ("status-repeated-last-true", md(), ready(more=',"status":"True"'), "MODIFIED", None),
    ("false-elsewhere-only", md(), st(conds="[%s,%s]" % (cond(status='"True"'), CREADY)), "MODIFIED", None),
]


def corpus_object(members, status, uid="u-corpus"):
    """The pod as JSON text around the raw metadata and status member(s)."""
    return ('{"kind":"Pod","apiVersion":"v1",%s,"spec":{"nodeName":"mi355x-node-01","containers":[{"name":"c",'
            '"image":"registry.example.com/team/c:v1"}]}%s}'
            % (members.replace("@UID@", uid), "" if status is None else "," + status))


def corpus_line(members, status, etype="MODIFIED", uid="u-corpus"):
    return ('{"type":"%s","object":%s}\n' % (etype, corpus_object(members, status, uid))).encode()


def corpus_pods():
    """The corpus as pod objects (raw JSON text) with the expected unready-since: findings_check's input."""
    return [(corpus_object(members, status), want) for _, members, status, _, want in CORPUS]


@pytest.mark.parametrize("case", CORPUS, ids=[c[0] for c in CORPUS])
def test_finding_table(case):
    from k8s_watcher_amd.models.findings import unready_since
    _, members, status, _, want = case
    got = unready_since(json.loads(corpus_object(members, status)))
    assert got == want and (got is None or type(got) is int)


def test_finding_of_odd_pods():
    from k8s_watcher_amd.models.findings import unready_since
    one = {"type": "Ready", "status": "False", "lastTransitionTime": R1}
    assert unready_since({"status": {"phase": "Running", "conditions": [one]}}) == R1_S
    for pod in ({}, {"status": None}, {"status": {"phase": "Running"}}, {"status": {"phase": "Running", "conditions": (one,)}},
                {"status": {"phase": b"Running", "conditions": [one]}}, {"status": [], "metadata": {}},
                {"status": {"phase": "Running", "conditions": [dict(one, status=False)]}},
                {"status": {"phase": "Running", "conditions": [dict(one, type=b"Ready")]}},
                {"status": {"phase": "Running", "conditions": [one]}, "metadata": {"deletionTimestamp": T1}}):
        assert unready_since(pod) is None, pod


def decoder_for(s, engine="python"):
    w = s.watcher
    return make_decoder(engine, s.environment, w.state_format, w.payload_extra, w.validate,
                        w.container_failures, w.container_failure_reasons, w.pod_conditions, w.pod_condition_rules,
                        w.terminating, w.terminating_overdue_seconds > 0, w.pending_overdue_seconds > 0,
                        w.unready_overdue_seconds > 0)


def pipeline(s, native, cache=None, notifier=None):
    rec, m = RawRecorder(), Metrics()
    p = EventPipeline(s, decoder_for(s), notifier if notifier is not None else rec, m, cache)
    p.log_events_setting = False
    if native:
        p.attach_native()
    return p, rec, m


def expected_cache(events):
    """uid -> unready-since after the decoded ``events`` in order, as the issue states the rule."""
    want = {}
    for ev in events:
        if ev[0] == "DELETED":
            want.pop(ev[E_UID], None)
        elif ev[0] in ("ADDED", "MODIFIED"):
            want[ev[E_UID]] = ev[E_UNREADY_SINCE]
    return want


def same_core(a, b, spelled):
    """Two payload cores are the same bytes; of a line that holds a backslash
    the same JSON value (the native engine copies a string token as the line
    spells it, the Python engine writes it as ``json.dumps`` does)."""
    if a is None or b is None or not spelled:
        return a == b
    return json.loads(a) == json.loads(b)


def check_decoders(data, want_of):
    """``E_UNREADY_SINCE``, ``INVALID`` and the core bytes from both decoders
    (the native one under validate payload and full). -> the Python decoder's events."""
    py = make_decoder("python", "staging", unready=True)
    a = [py.feed(ln)[0] for ln in data]
    for ev, ln in zip(a, data):
        if ev[0] == "INVALID":
            continue
        assert len(ev) == 15 and ev[9:14] == (0, 0, 0, None, None), ln  # the earlier slots, filled as their options' off
        assert ev[E_UNREADY_SINCE] == (None if ev[0] == "DELETED" else want_of(ln)), ln
    for validate in ("payload", "full"):
        nat = make_decoder("native", "staging", validate=validate, unready=True)
        for ea, ln in zip(a, data):
            eb = nat.feed(ln)[0]
            assert ea[0] == eb[0], ln  # INVALID included
            if ea[0] == "INVALID":
                continue
            assert len(eb) == 15 and eb[:7] == ea[:7] and eb[9:] == ea[9:], (validate, ln)
            assert type(eb[E_UNREADY_SINCE]) is type(ea[E_UNREADY_SINCE]), ln
            assert same_core(py.core(ea), nat.core(eb), b"\\" in ln), ln
    return a


def check_pipelines(data, a, overrides=()):
    """The lines as one batch through both fused pipelines, full parse
    (staging) and filter-first (production): the unready-since each stores,
    what is tracked, the notifications' bytes, the INVALID reports."""
    batch = b"".join(data)
    want = expected_cache(a)
    spelled = {e[E_UID] for e, ln in zip(a, data) if b"\\" in ln and e[0] != "INVALID"}
    invalid = [e[0] for e in a if e[0] == "INVALID"]
    for env, ov in (("staging", UO()), ("production", merged(UO(), {"watcher": {"namespaces": []}}))):
        for validate in ("payload", "full"):
            s = settings_for(env, merged(ov, {"watcher": {"validate": validate}}, *overrides))
            got = {}
            for native in (False, True):
                p, rec, m = pipeline(s, native)
                assert [c[0] for c in feed(p, native, batch)] == invalid
                uids = [u for u, _ in p.cache.items()]
                got[native] = ({u: p.cache.unready_since(u) for u in uids}, p.cache.unready_tracked(),
                               {u: p.cache.core_kept(u) for u in uids}, [c[:4] for c in rec.calls],
                               list(zip((c[0] for c in rec.calls), rec.raw)), {u: p.cache.get(u)[CORE] for u in uids})
            assert got[False][:4] == got[True][:4], (env, validate)
            for (u, x), (_, y) in zip(got[False][4], got[True][4]):  # the notifications' bytes
                assert same_core(x, y, u in spelled), (env, validate, u)
            for u, x in got[False][5].items():  # ... and the cached cores', kept or sent
                assert same_core(x, got[True][5][u], u in spelled), (env, validate, u)
            assert got[True][0] == want, (env, validate)
            assert got[True][1] == sum(v is not None for v in want.values())
            if env == "production":  # every tracked pod's line was dropped and its core kept
                assert all(got[True][2][u] for u, v in want.items() if v is not None)
    return want


def check_corpus():
    from k8s_watcher_amd.models.findings import unready_since
    data = [corpus_line(members, status, etype, "c%d" % i) for i, (_, members, status, etype, _) in enumerate(CORPUS)]
    table = {ln: want for ln, (*_, want) in zip(data, CORPUS)}
    for ln, want in table.items():
        assert unready_since(json.loads(ln)["object"]) == want, ln
    a = check_decoders(data, table.__getitem__)
    assert all(e[0] != "INVALID" for e in a)
    want = check_pipelines(data, a)
    assert sum(v is not None for v in want.values()) >= 25 and sum(v is None for v in want.values()) >= 50
    for eng in ("python", "native"):
        d = make_decoder(eng, "staging", terminating=True, overdue=True, pending=True, unready=True)
        evs = [d.feed(ln)[0] for ln in data]
        assert all(len(e) == 15 for e in evs)
        by_id = {c[0]: e for c, e in zip(CORPUS, evs)}
        assert by_id["terminating"][11:] == (1, 1752025892, None, None) and by_id["unready"][11:] == (0, None, None, R1_S)
        assert by_id["phase-pending"][11:13] == (0, None) and by_id["phase-pending"][14] is None


def test_corpus_one_verdict_from_both_engines():
    check_corpus()


def check_option_off():
    """With the option off the tuples are what they were: lengths 9, 13 and 14."""
    data = [corpus_line(members, status, etype, "c%d" % i) for i, (_, members, status, etype, _) in enumerate(CORPUS)]
    for eng in ("python", "native"):
        assert all(len(make_decoder(eng, "staging").feed(ln)[0]) == 9 for ln in data)
        assert all(len(make_decoder(eng, "staging", terminating=True, overdue=True).feed(ln)[0]) == 13 for ln in data)
        assert all(len(make_decoder(eng, "staging", pending=True).feed(ln)[0]) == 14 for ln in data)
    py, nat = make_decoder("python", "staging", pending=True), make_decoder("native", "staging", pending=True)
    for ln in data:
        ea, eb = py.feed(ln)[0], nat.feed(ln)[0]
        assert ea[:7] == eb[:7] and ea[9:] == eb[9:]


# ----------------------------------------------------------------------------- seeded mutations (test 3)

PHASES = ['"Running"'] * 8 + ['"Pending"', '"Succeeded"', '"Failed"', '"Unknown"', '"running"', '"Running "', '""']
STATES = ['"False"'] * 6 + ['"True"', '"True"', '"Unknown"', '"false"', "false", "null", '"False "', "0"]
TYPES = ['"Ready"'] * 5 + ['"ContainersReady"', '"PodScheduled"', '"Initialized"', '"ready"', '"Ready "', "null", "7"]
RETYPED = ["null", "true", "0", "-1.5", "[]", "{}", '["Ready"]', '{"type":"Ready"}', '"Ready"']
BLANKS = ["", "", "", " ", "\t", "  ", "\r"]


def mutated_condition(rng, ws):
    ctype, state = rng.choice(TYPES), rng.choice(STATES)
    if ctype.startswith('"') and rng.random() < 0.2:
        ctype = escaped(rng, json.loads(ctype))
    if state.startswith('"') and rng.random() < 0.2:
        state = escaped(rng, json.loads(state))
    fields = [["type", ctype], ["status", state], ["lastProbeTime", "null"]]
    r = rng.random()
    if r < 0.30:  # one step off the grammar
        fields.append(["lastTransitionTime", mutated_timestamp(rng)])
    elif r < 0.85:
        fields.append(["lastTransitionTime", '"%s"' % valid_timestamp(rng)[0]])
    elif r < 0.93:
        fields.append(["lastTransitionTime", rng.choice(RETYPED + [str(R1_S)])])
    r = rng.random()
    if r < 0.06:
        fields.append([rng.choice(("type", "status", "lastTransitionTime")), rng.choice(TYPES + STATES + ['"%s"' % R1])])
    elif r < 0.12:
        k = rng.randrange(len(fields))
        fields[k][0] = escaped(rng, fields[k][0])[1:-1]
    rng.shuffle(fields)
    return "%s{%s}%s" % (ws(), ",".join('%s"%s"%s:%s%s' % (ws(), k, ws(), ws(), v) for k, v in fields), ws())


def mutated_line(rng, i):
    """A corpus-like line, mutated in the conditions (their number and order,
    each one's type, status and transition time: values, JSON types, escapes,
    repeated keys), the phase, the status, the deletion timestamp and the event
    type; all of it valid JSON."""
    ws = lambda: rng.choice(BLANKS)  # noqa: E731
    phase = rng.choice(PHASES)
    r = rng.random()
    if r < 0.05:
        phase = rng.choice(RETYPED)
    elif r < 0.20:
        phase = escaped(rng, json.loads(phase))
    items = [mutated_condition(rng, ws) for _ in range(rng.choice((0, 1, 1, 2, 3, 3, 4, 5)))]
    if rng.random() < 0.3:  # (a mutated Ready element seldom has all three members right: some that decide first)
        items.insert(0, '{%s"lastTransitionTime":%s"%s","status":"False",%s"type"%s:"Ready"}'
                     % (ws(), ws(), valid_timestamp(rng)[0], ws(), ws()))
    if rng.random() < 0.1:
        items.insert(rng.randrange(len(items) + 1), rng.choice(RETYPED))
    conds = "[%s]" % ",".join(items)
    if rng.random() < 0.05:
        conds = rng.choice(RETYPED)
    fields = [["phase", phase], ["podIP", '"10.244.0.7"'], ["conditions", conds]]
    r = rng.random()
    if r < 0.05:
        fields.append(["conditions", rng.choice(("null", "[]", "[%s]" % mutated_condition(rng, ws)))])
    elif r < 0.08:
        fields.append(["phase", rng.choice(PHASES)])
    elif r < 0.11:
        fields = fields[:2]
    elif r < 0.14:
        fields[2][0] = escaped(rng, "conditions")[1:-1]
    rng.shuffle(fields)
    status = '"status":%s{%s}' % (ws(), ",".join('%s"%s"%s:%s%s' % (ws(), k, ws(), ws(), v) for k, v in fields))
    r = rng.random()
    if r < 0.03:
        status = '"status":%s' % rng.choice(RETYPED)
    elif r < 0.06:
        status = rng.choice(('"status":null,', '"status":{"phase":"Pending"},', st() + ",")) + status
    elif r < 0.09:
        status = status + rng.choice((',"status":null', "," + st(), ',"status":{}'))
    elif r < 0.10:
        status = None
    more = ""
    if rng.random() < 0.10:
        more += ',"deletionTimestamp":%s' % rng.choice(('"%s"' % T1, '""', "null", "17"))
    members = md(more, rv=str(i + 1))
    if rng.random() < 0.02:
        members = rng.choice(('"metadata":null', '"metadata":[]', md() + "," + members))
    etype = "MODIFIED" if rng.random() < 0.85 else rng.choice(("ADDED", "DELETED"))
    return corpus_line(members, status, etype, "u%d" % i)


def fuzz_lines(n=2000, seed=31):
    rng = random.Random(seed)
    return [mutated_line(rng, i) for i in range(n)]


def fuzz_pods(n=200, seed=31):
    """The pod objects (raw JSON text) of the first ``n`` mutated lines: findings_check's input."""
    return [ln[ln.index(b'"object":') + 9:-2].decode() for ln in fuzz_lines(n, seed)]


def check_fuzz():
    from k8s_watcher_amd.models.findings import unready_since
    data = fuzz_lines()
    assert len(data) == 2000
    twin = {ln: unready_since(json.loads(ln)["object"]) for ln in data}
    py = make_decoder("python", "staging", unready=True)
    # the condition on the mutator, by the Python engine alone: enough lines decode, both outcomes are common
    live = [e for e in (py.feed(ln)[0] for ln in data) if e[0] in ("ADDED", "MODIFIED")]
    assert len(live) >= 1500 and sum(e[E_UNREADY_SINCE] is not None for e in live) >= 200
    assert sum(e[E_UNREADY_SINCE] is None for e in live) >= 200
    a = check_decoders(data, twin.__getitem__)
    check_pipelines(data, a)
    check_pipelines(data, a, [{"watcher": {"notify_on": "phase_change"}}])


def test_seeded_mutation_fuzz():
    check_fuzz()


def test_option_off_is_the_parent_behaviour():
    """The one test that passes without the option: tuples and, in
    ``check_pod_life``'s off runs, notifications and counters are unchanged."""
    check_option_off()


# ----------------------------------------------------------------------------- both caches, one API (test 4)

@pytest.mark.parametrize("native", [False, True], ids=["python-cache", "native-cache"])
def test_both_caches_one_api(native):
    cache = make_pod_cache(native)
    cache.set_unready_since("nobody", 5)  # an unknown uid is a no-op
    assert cache.unready_since("nobody") is None and cache.unready_tracked() == 0 and len(cache) == 0
    assert cache.take_unready_overdue(10 ** 9, 0) == []
    cache.observe("ADDED", "u", "1", "Running", "default", "n")
    cache.set_unready_since("u", 100)
    assert cache.unready_since("u") == 100 and cache.unready_tracked() == 1
    assert cache.tracked() == 0 and cache.pending_tracked() == 0 and cache.pending_since("u") is None  # this kind only
    assert cache.take_overdue(10 ** 9, 0) == [] and cache.take_pending_overdue(10 ** 9, 0) == []
    assert cache.take_unready_overdue(1000, 30) == []  # no core: neither returned nor marked
    cache.set_core("u", b'{"a":1}')
    assert cache.take_unready_overdue(129, 30) == []  # the boundary
    assert cache.take_unready_overdue(130, 30) == [("u", "default", "n", b'{"a":1}', 100)]
    assert cache.take_unready_overdue(131, 30) == [] and cache.take_unready_overdue(10 ** 9, 0) == []  # marked
    cache.set_unready_since("u", 50)  # a value keeps the mark, None clears the value and the mark
    assert cache.unready_since("u") == 50 and cache.take_unready_overdue(10 ** 9, 0) == []
    cache.set_unready_since("u", None)
    assert cache.unready_since("u") is None and cache.unready_tracked() == 0 and cache.get("u")[CORE] == b'{"a":1}'
    cache.set_unready_since("u", None)  # twice is fine
    cache.set_unready_since("u", 60)
    assert cache.take_unready_overdue(90, 30) == [("u", "default", "n", b'{"a":1}', 60)]
    # the marks are per kind: reported unready, the pod is still reported by the other two sweeps, once each
    cache.set_deadline("u", 70)
    cache.set_pending_since("u", 80)
    assert (cache.tracked(), cache.pending_tracked(), cache.unready_tracked()) == (1, 1, 1)
    assert cache.take_overdue(100, 30) == [("u", "default", "n", b'{"a":1}', 70)] and cache.take_overdue(100, 30) == []
    assert cache.take_pending_overdue(110, 30) == [("u", "default", "n", b'{"a":1}', 80)]
    cache.set_unready_since("u", None)  # ... and clearing one leaves the others
    assert cache.deadline("u") == 70 and cache.pending_since("u") == 80 and cache.take_pending_overdue(10 ** 9, 0) == []
    cache.set_pending_since("u", None)
    cache.set_deadline("u", None)
    # a kept core goes with the unready timer as with the pending one
    cache.put("k", "1", "Running", "default", "k", None)
    cache.set_unready_since("k", 10)
    cache.keep_core("k", b'{"k":1}')
    assert cache.core_kept("k") is True and cache.take_unready_overdue(40, 30) == [("k", "default", "k", b'{"k":1}', 10)]
    cache.keep_core("k", b'{"k":2}')  # the newest unready line's
    cache.set_unready_since("k", 20)
    assert cache.core_kept("k") is True and cache.get("k")[CORE] == b'{"k":2}'
    cache.set_unready_since("k", None)
    assert cache.get("k")[CORE] is None and cache.core_kept("k") is False and cache.unready_tracked() == 0
    # a Pending -> Running-unready line: clear the pending timer (the old kept core goes), set the unready one, keep
    cache.set_pending_since("k", 5)
    cache.keep_core("k", b'{"pending":1}')
    cache.set_pending_since("k", None)
    assert cache.get("k")[CORE] is None and cache.core_kept("k") is False
    cache.set_unready_since("k", 30)
    cache.keep_core("k", b'{"unready":1}')
    assert (cache.pending_since("k"), cache.unready_since("k"), cache.get("k")[CORE]) == (None, 30, b'{"unready":1}')
    # ... and the reverse
    cache.set_unready_since("k", None)
    assert cache.get("k")[CORE] is None and cache.core_kept("k") is False
    cache.set_pending_since("k", 5)
    cache.keep_core("k", b'{"pending":2}')
    assert (cache.pending_since("k"), cache.unready_since("k"), cache.get("k")[CORE]) == (5, None, b'{"pending":2}')
    # a kept core is held by the kind whose timer stands: clearing the other kind, which has none, leaves it
    cache.set_unready_since("k", None)
    assert cache.get("k")[CORE] == b'{"pending":2}' and cache.core_kept("k") is True
    cache.set_pending_since("k", None)
    assert cache.get("k")[CORE] is None
    # a send replaces a kept core, and the core then stays
    cache.set_unready_since("k", 10)
    cache.keep_core("k", b'{"k":3}')
    cache.set_core("k", b'{"k":4}')
    assert cache.core_kept("k") is False
    cache.set_unready_since("k", None)
    assert cache.get("k")[CORE] == b'{"k":4}'
    # put (a whole new entry) clears everything, the kept mark and the reported mark too
    cache.set_unready_since("k", 10)
    cache.keep_core("k", b'{"k":5}')
    assert len(cache.take_unready_overdue(10 ** 9, 0)) == 1
    cache.put("k", "2", "Running", "default", "k", b'{"k":6}')
    assert cache.unready_since("k") is None and cache.core_kept("k") is False and cache.get("k")[CORE] == b'{"k":6}'
    cache.set_unready_since("k", 60)
    assert cache.take_unready_overdue(90, 30) == [("k", "default", "k", b'{"k":6}', 60)]
    # ... and so does every way an entry goes
    cache.observe("DELETED", "k", "3", "Running", "default", "k")
    cache.observe("DELETED", "u", "3", "Running", "default", "n")
    assert cache.unready_tracked() == 0 and cache.unready_since("k") is None and len(cache) == 0
    for gone in (lambda: cache.pop("v"), lambda: cache.drop_namespaces(["ns-a"]),
                 lambda: cache.drop_namespaces_except(["default"]), cache.clear):
        cache.put("v", "1", "Running", "ns-a", "m", None)
        cache.set_unready_since("v", 7)
        cache.keep_core("v", b"{}")
        assert cache.unready_tracked() == 1
        gone()
        assert cache.unready_tracked() == 0 and cache.unready_since("v") is None and cache.core_kept("v") is False
        assert cache.take_unready_overdue(10 ** 9, 0) == []
    # scope_ns, int64 ends; to_records() writes a kept core like any core and no timer
    for i, ns in enumerate(["ns-a", "ns-b", None]):
        cache.put("p%d" % i, "1", "Running", ns, "n%d" % i, None)
        cache.keep_core("p%d" % i, b'{"i":%d}' % i)
        cache.set_unready_since("p%d" % i, (-2 ** 63, 0, 2 ** 63 - 1)[i])
    assert cache.take_unready_overdue(30, 30, "ns-c") == []
    assert cache.take_unready_overdue(30, 30, "ns-b") == [("p1", "ns-b", "n1", b'{"i":1}', 0)]
    assert [t[0] for t in cache.take_unready_overdue(2 ** 63 - 1, 2 ** 62)] == ["p0"]  # compared without overflow
    records = cache.to_records()
    assert all(len(r) == 6 for r in records) and sorted(r[5] for r in records) == ['{"i":0}', '{"i":1}', '{"i":2}']
    fresh = make_pod_cache(native, records)
    assert fresh.unready_tracked() == 0 and not any(fresh.core_kept(u) for u, _ in fresh.items())


# ----------------------------------------------------------------------------- a pod's life with sweeps (test 5)

def run_script(s, native, script, cache=None):
    """``script``: ("feed", bytes), ("sweep", now_s[, scope_ns]) and ("look", uid) steps.
    -> (calls, the submitted bytes, counters, control event types, what each
    sweep returned, what each look saw: (unready_since, unready_tracked, has a core, core_kept))."""
    p, rec, m = pipeline(s, native, cache)
    ctrl, swept, looks = [], [], []
    for step in script:
        if step[0] == "feed":
            ctrl += feed(p, native, step[1])
        elif step[0] == "sweep":
            swept.append(p.report_overdue(step[1], 0, *step[2:]))
        else:
            ent = p.cache.get(step[1])
            looks.append((p.cache.unready_since(step[1]), p.cache.unready_tracked(),
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
    """(event type, resourceVersion of the payload, unready_seconds of its alert or None)."""
    return [(et, int(core["extra"]["resource_version"]), (core.get("alert") or {}).get("unready_seconds"))
            for _, et, _, _, core in calls]


def check_pod_life():
    f = PodFactory(seed=61, namespaces=["default"])
    p0 = f.new_pod()
    uid, U, U2 = p0["metadata"]["uid"], C1_S + 40, C1_S + 440
    phase = merged(RV_EXTRA, {"watcher": {"notify_on": "phase_change"}})
    gone = deleting(unready(f, p0, U2), 6)
    for one_read in (True, False):
        script = (feeds([("ADDED", with_rv(p0, 1)), ("MODIFIED", unready(f, p0, U, 2))], one_read)
                  + [("look", uid), ("sweep", U + N - 1), ("sweep", U + N), ("sweep", U + N + 1)]
                  # the transition time moves: the mark stays
                  + feeds([("MODIFIED", unready(f, p0, U + 50, 3))], one_read) + [("look", uid), ("sweep", U + 50 + N + 5)]
                  # Ready returns to True, and goes False again: a new period
                  + feeds([("MODIFIED", with_rv(f.running(p0), 4))], one_read) + [("look", uid), ("sweep", U + 3 * N)]
                  + feeds([("MODIFIED", unready(f, p0, U2, 5))], one_read)
                  + [("look", uid), ("sweep", U2 + N - 1), ("sweep", U2 + N)]
                  # deletion begins: the terminating alerts' state; then the pod goes
                  + feeds([("MODIFIED", gone)], one_read) + [("look", uid), ("sweep", U2 + 10 * N)]
                  + feeds([("DELETED", with_rv(gone, 7))], one_read) + [("look", uid), ("sweep", U2 + 20 * N)])
        # production, the critical filter on: nothing of a Pending or Running pod is sent but the alerts
        calls, raw, c, ctrl, swept, looks = both_scripts("production", merged(UO(), RV_EXTRA), script)
        assert ctrl == [] and swept == [0, 1, 0, 0, 0, 0, 1, 0, 0]
        assert rvs(calls) == [("MODIFIED", 2, N), ("MODIFIED", 5, N), ("DELETED", 7, None)]
        assert looks == [(U, 1, True, True), (U + 50, 1, True, True), (None, 0, False, False), (U2, 1, True, True),
                         (None, 0, False, False), (None, 0, False, False)]
        assert c["events_unready_overdue"] == 2 and c["events_received"] == 7 and c["events_filtered_critical"] == 6
        alert = dict(calls[0][4])
        assert alert.pop("alert") == {"kind": "unready_overdue", "since_unix": U, "unready_seconds": N}
        assert calls[0][:4] == (uid, "MODIFIED", "default", p0["metadata"]["name"]) and alert["status"]["phase"] == "Running"
        assert list(json.loads(raw[0]))[-1] == "alert"  # spliced in before the closing brace
        assert raw[0].endswith(b',"alert":{"kind":"unready_overdue","since_unix":%d,"unready_seconds":%d}}' % (U, N))
        # ... and the option off: byte-identical notifications and counters, with every alert off and with this one at 0
        for off in (RV_EXTRA, merged(UO(0), RV_EXTRA)):
            o_calls, o_raw, o_c, _, o_swept, o_looks = both_scripts("production", off, script)
            assert o_raw == raw[2:] and o_swept == [0] * 9 and o_c == dict(c, events_unready_overdue=0)
            assert o_looks == [(None, 0, False, False)] * 6
        # staging, notify_on: phase_change: the Running lines after the first are unchanged and kept
        calls, raw, c, _, swept, looks = both_scripts("staging", merged(UO(), phase), script)
        assert swept == [0, 1, 0, 0, 0, 0, 1, 0, 0]
        assert rvs(calls) == [("ADDED", 1, None), ("MODIFIED", 2, None), ("MODIFIED", 2, N), ("MODIFIED", 5, N),
                              ("DELETED", 7, None)]
        assert looks == [(U, 1, True, False), (U + 50, 1, True, True), (None, 0, False, False), (U2, 1, True, True),
                         (None, 0, False, False), (None, 0, False, False)]
        assert c["events_unready_overdue"] == 2 and c["events_unchanged"] == 4
        for off in (phase, merged(UO(0), phase)):
            o_calls, o_raw, o_c, _, o_swept, _ = both_scripts("staging", off, script)
            assert o_raw == raw[:2] + raw[4:] and o_swept == [0] * 9 and o_c == dict(c, events_unready_overdue=0)
    # every extra field on: the bodies are the same bytes from both engines (both_scripts compares them)
    from k8s_watcher_amd.models.payload import EXTRA_NAMES
    everything = {"watcher": {"payload_extra_fields": list(EXTRA_NAMES)}}
    calls, raw, _, _, swept, _ = both_scripts("production", merged(UO(), everything),
                                              feeds([("ADDED", unready(f, p0, U, 1))], True) + [("sweep", U + N + 3)])
    assert swept == [1] and raw[-1].endswith(b'"unready_seconds":%d}}' % (N + 3))
    # the log line, with log_events
    for native in (False, True):
        p, rec, _ = pipeline(settings_for("production", merged(UO(), RV_EXTRA)), native)
        p.log_events_setting = True
        seen = []
        p.elog.log = lambda level, msg: seen.append((level, msg))
        feed(p, native, lines([("ADDED", unready(f, p0, U, 1))]))
        assert p.report_overdue(U + N + 3, 0) == 1
        name = p0["metadata"]["name"]
        assert (20, f"Pod unready overdue: default/{name} - {N + 3}s since Ready=False") in seen, (native, seen)


def test_pod_life_with_sweeps():
    check_pod_life()


def test_report_overdue_kind_selector():
    """The native sweep's ``pending`` boolean became a kind selector; the old spelling still works."""
    f = PodFactory(seed=61, namespaces=["default"])
    a, b = f.new_pod(), f.new_pod()
    s = settings_for("production", merged(UO(pending_overdue_seconds=N), RV_EXTRA))
    for how in ("positional", "keyword", "kind"):
        p, rec, m = pipeline(s, True)
        feed(p, True, lines([("ADDED", with_rv(a, 1)), ("ADDED", unready(f, b, C1_S + 10, 2))]))
        now = C1_S + 10 * N
        call = {"positional": lambda on: p.native.report_overdue(now, N, None, 0, on),
                "keyword": lambda on: p.native.report_overdue(now, N, None, 0, pending=on),
                "kind": lambda on: p.native.report_overdue(now, N, None, 0, kind=int(on))}[how]
        assert call(False)[0] == 0 and call(True)[0] == 1 and call(True)[0] == 0
        assert p.native.report_overdue(now, N, None, 0, kind=2)[0] == 1
        assert m.c["events_pending_overdue"] == 1 and m.c["events_unready_overdue"] == 1
        with pytest.raises(ValueError):
            p.native.report_overdue(now, N, None, 0, kind=3)


# ----------------------------------------------------------------------------- partitioned against serial (test 6)

PARTITIONS = 16


def unready_batch(seed=7):
    """One batch, every pod's lines interleaved with the others': the fewest
    pods (128 at least: one namespace in five is this shard's and reportable)
    that put one into every one of the 16 partitions. Half run unready over
    two to four lines, the others become Ready, stay Pending, are deleted
    while unready or begin terminating."""
    from k8s_watcher_amd.ops.native import load
    part = load().apply_partition
    f = PodFactory(seed=seed, namespaces=NAMESPACES)
    scripts, parts = [], set()
    while len(scripts) < 128 or len(parts) < PARTITIONS:
        p0 = f.new_pod()
        i = len(scripts)
        bad, bad2, run_ = unready(f, p0, C1_S + 10 + i), unready(f, p0, C1_S + 20 + i), f.running(p0)
        steps = [("ADDED", p0), ("MODIFIED", bad)]
        steps += {0: [("MODIFIED", bad)], 1: [("MODIFIED", run_)], 2: [], 3: [("MODIFIED", bad2), ("MODIFIED", bad2)],
                  4: [("DELETED", bad)], 5: [("MODIFIED", run_), ("MODIFIED", bad2)], 6: [("MODIFIED", f.scheduled(p0))],
                  7: [("MODIFIED", deleting(bad, 0))]}[i % 8]
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
    bodies by uid, the other bodies, every cached pod's unready-since, kept
    mark and core, unready_tracked(), the counters, the growth of apply_stats()
    over the batch and the sweep's return."""
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
        tracked = p.cache.unready_tracked()
        swept = p.report_overdue(now_s, 1)
        assert await pool.drain(20) and ctrl == []
        sent = [{k: v for k, v in x.items() if k != "event_timestamp"} for x in sink.state.payloads()]
        alerts_ = {x["uid"]: json.dumps(x, sort_keys=True) for x in sent if "alert" in x}
        assert len(alerts_) == sum("alert" in x for x in sent) and all(x["event_type"] == "MODIFIED" for x in sent if "alert" in x)
        rest = collections.Counter(json.dumps(x, sort_keys=True) for x in sent if "alert" not in x)
        since = {u: (p.cache.unready_since(u), p.cache.core_kept(u), e[CORE]) for u, e in p.cache.items()}
        counters = {k: v for k, v in m.c.items() if k.startswith(("events_", "bookmarks")) and v}
        assert p.cache.unready_tracked() == tracked
        await pool.close()
        await sink.stop()
        dpool.close()
        return alerts_, rest, since, tracked, counters, stats, swept

    return run(body(), timeout=60)


def check_partitioned_matches_serial():
    from k8s_watcher_amd.ops.native import load
    data, pods, n = unready_batch()
    warm = warm_up()
    assert 128 <= len(pods) <= 200 and 2 * len(pods) <= n <= 4 * len(pods)
    assert {shard_of(ns) for ns in NAMESPACES} == {0, 1}
    mine = [ns for ns in NAMESPACES if shard_of(ns) == 0]
    assert len(mine) >= 2  # one of this shard's namespaces is filtered, another is not
    now_s = C1_S + 10 * N
    sharded = {"watcher": {"shard": {"count": 2, "index": 0}, "namespaces": [ns for ns in NAMESPACES if ns != mine[0]]}}
    for env, ov in (("production", merged(UO(), RV_EXTRA, sharded)),
                    ("staging", merged(UO(terminating=True, pending_overdue_seconds=4000000000), RV_EXTRA, sharded,
                                       {"watcher": {"notify_on": "phase_change"}}))):
        s_alerts, s_rest, s_since, s_tracked, s_cnt, s_stats, s_swept = feed_and_sweep(env, ov, warm, data, False, now_s)
        p_alerts, p_rest, p_since, p_tracked, p_cnt, p_stats, p_swept = feed_and_sweep(env, ov, warm, data, True, now_s)
        # the partitioned path was taken: one batch, every line of it applied by its partition
        assert s_stats["partitioned_batches"] == 0 and s_stats["serial_batches"] == 1
        assert p_stats["partitioned_batches"] == 1 and p_stats["partitioned_lines"] == n and p_stats["serial_batches"] == 0
        assert p_stats["payload_built"] == s_stats["payload_built"] > 0
        assert p_alerts == s_alerts and p_rest == s_rest and p_since == s_since and p_tracked == s_tracked and p_cnt == s_cnt
        assert p_swept == s_swept == len(s_alerts) == s_cnt["events_unready_overdue"]
        assert s_cnt["events_filtered_namespace"] > 0 and s_cnt["events_other_shard"] > 0
        # the condition: every store shard is filled, enough reported pods, spread over the shards
        part = load().apply_partition
        assert len({part(p["metadata"]["uid"]) for p in pods}) == PARTITIONS
        assert len(s_alerts) >= 8 and len({part(u) for u in s_alerts}) >= 4, (len(s_alerts), {part(u) for u in s_alerts})
        assert s_tracked > len(s_alerts)  # (pods of the namespace the filter drops are tracked and have no core)
        for u, body in s_alerts.items():
            since = s_since[u][0]
            assert json.loads(body)["alert"] == {"kind": "unready_overdue", "since_unix": since, "unready_seconds": now_s - since}
            assert json.loads(body)["extra"]["resource_version"] == json.loads(s_since[u][2])["extra"]["resource_version"]
        # the Python engine: the same reports, values and counters
        p, rec, m = pipeline(settings_for(env, ov), False)
        assert feed(p, False, warm) == [] and feed(p, False, data) == []
        assert p.cache.unready_tracked() == s_tracked
        assert {u: (p.cache.unready_since(u), p.cache.core_kept(u), e[CORE]) for u, e in p.cache.items()} == s_since
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
    assert all(len(e) == 15 for e in evs)
    return p.reconcile(evs, 0, notify=notify, scope_ns=scope)


def alert_uids(calls):
    return sorted(u for u, _, _, _, core in calls if "alert" in core)


def check_relist(native):
    f = PodFactory(seed=71, namespaces=["default"])
    a, b, c_, d, e = (f.new_pod() for _ in range(5))
    uid = lambda p: p["metadata"]["uid"]  # noqa: E731
    U = C1_S + 30
    s = settings_for("production", merged(UO(), RV_EXTRA))
    p, rec, m = pipeline(s, native)
    feed(p, native, lines([("ADDED", with_rv(f.running(a), 1)), ("ADDED", unready(f, b, U, 2)), ("ADDED", unready(f, c_, U, 3)),
                           ("ADDED", with_rv(d, 4)), ("ADDED", unready(f, e, U, 5))]))
    now = U + N
    assert p.cache.unready_tracked() == 3 and p.report_overdue(now, 0) == 3 and alert_uids(rec.calls) == sorted(map(uid, (b, c_, e)))
    del rec.calls[:]
    # the gap (a 410): b is still unready (reported already), c is gone while unready, d runs unready now, e is
    # Ready; a is unchanged
    listed = [with_rv(f.running(a), 1), unready(f, b, U, 11), unready(f, d, U + 5, 12), with_rv(f.running(e), 13)]
    assert relist(p, native, listed) == []
    # c's DELETED is built from its kept core, the one the alert was built from, not from the cache's summary
    assert [(u, et) for u, et, *_ in rec.calls] == [(uid(c_), "DELETED")]
    gone = rec.calls[0][4]
    assert gone["extra"]["resource_version"] == "3" and gone["status"]["phase"] == "Running" and "alert" not in gone
    assert [c["status"] for c in gone["status"]["conditions"] if c["type"] == "Ready"] == ["False"]
    assert p.cache.unready_tracked() == 2 and p.cache.unready_since(uid(b)) == U and p.cache.unready_since(uid(d)) == U + 5
    assert p.cache.unready_since(uid(e)) is None and p.cache.get(uid(e))[CORE] is None  # the kept core went with it
    assert json.loads(p.cache.get(uid(b))[CORE])["extra"]["resource_version"] == "11" and p.cache.core_kept(uid(b))
    del rec.calls[:]
    assert p.report_overdue(now + N, 0) == 1 and alert_uids(rec.calls) == [uid(d)]  # b was reported before the gap
    assert m.c["events_unready_overdue"] == 4
    # a restart: the cache rebuilt from its records has the cores (kept ones like any) and no unready-since
    records = p.cache.to_records()
    assert all(len(r) == 6 for r in records) and sum(r[5] is not None for r in records) == 2
    q, rec2, m2 = pipeline(s, native, make_pod_cache(native, records))
    assert q.cache.unready_tracked() == 0 and q.report_overdue(2 ** 40, 0) == 0
    # ... a relist whose items are all unchanged restores every value, and the sweep reports from the
    # checkpointed cores: the marks did not persist
    assert relist(q, native, listed) == [] and rec2.calls == []
    assert q.cache.unready_tracked() == 2 and q.cache.unready_since(uid(b)) == U and q.cache.unready_since(uid(d)) == U + 5
    assert q.report_overdue(now + 5, 0) == 2 and alert_uids(rec2.calls) == sorted([uid(b), uid(d)])
    assert {core["extra"]["resource_version"] for *_, core in rec2.calls} == {"11", "12"}
    assert all(core["alert"]["kind"] == "unready_overdue" for *_, core in rec2.calls)
    assert q.report_overdue(now + 6, 0) == 0
    # after the restart b's core counts as an ordinary one: Ready clears the value and the core stays
    feed(q, native, lines([("MODIFIED", with_rv(f.running(b), 30))]))
    assert q.cache.unready_since(uid(b)) is None and q.cache.unready_tracked() == 1
    assert json.loads(q.cache.get(uid(b))[CORE])["extra"]["resource_version"] == "11"
    # an unchanged item that is not unready (cannot happen without a new resourceVersion; the rule all the same)
    q.cache.set_unready_since(uid(a), 5)
    assert relist(q, native, [x for x in listed if uid(x) != uid(b)] + [with_rv(f.running(b), 30)]) == []
    assert q.cache.unready_since(uid(a)) is None
    # a silent relist (initial_list: skip) tracks nothing, changed items or unchanged
    for cache in (None, make_pod_cache(native, records)):
        r, rec3, _ = pipeline(s, native, cache)
        assert relist(r, native, listed, notify=False) == []
        assert rec3.calls == [] and len(r.cache) == 4 and r.cache.unready_tracked() == 0 and r.report_overdue(2 ** 40, 0) == 0


@pytest.mark.parametrize("native", [True, False], ids=["native-relist", "python-reconcile"])
def test_relist_and_restart(native):
    check_relist(native)


def check_shared_cache(native):
    """Two scopes on one cache: B is swept while A's relist stands in mid-walk."""
    from test_native_relist import list_pages
    ov = merged(UO(), RV_EXTRA, {"watcher": {"namespace_scope": "server", "namespaces": ["ns-a", "ns-b"]}})
    s = settings_for("production", ov)
    fa, fb = PodFactory(seed=91, namespaces=["ns-a"]), PodFactory(seed=92, namespaces=["ns-b"])
    pods_a, pods_b = [fa.new_pod() for _ in range(90)], [fb.new_pod() for _ in range(12)]
    uid = lambda p: p["metadata"]["uid"]  # noqa: E731
    U = C1_S + 30
    bad_a = {uid(p) for p in pods_a[::3]}  # these stay unready over A's relist; the others are Ready by then
    bad_b = {uid(p) for p in pods_b[::2]}
    listed_a = [unready(fa, p, U, 500 + i) if uid(p) in bad_a else with_rv(fa.running(p), 500 + i)
                for i, p in enumerate(pods_a[:-5])]
    now = U + 1000

    def world():
        cache = make_pod_cache(native)
        pa, rec_a, _ = pipeline(s, native, cache)
        pb, rec_b, _ = pipeline(s, native, cache)
        feed(pa, native, lines([("ADDED", unready(fa, p, U, i + 1)) for i, p in enumerate(pods_a)]))
        feed(pb, native, lines([("ADDED", unready(fb, p, U, 200 + i) if uid(p) in bad_b else with_rv(fb.running(p), 200 + i))
                                for i, p in enumerate(pods_b)]))
        assert cache.unready_tracked() == len(pods_a) + len(bad_b) and rec_a.calls == rec_b.calls == []
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
                sorted(map(json.dumps, cache.to_records())), {u: cache.unready_since(u) for u, _ in cache.items()})

    cache0, pa0, rec_a0, _, _ = world()
    assert relist_a(pa0, lambda: None) == []
    unswept = state(cache0, rec_a0)
    assert sorted(et for _, et, *_ in rec_a0.calls) == ["DELETED"] * 5  # the vanished unready pods, from their kept cores
    assert all(core["status"]["phase"] == "Running" and int(core["extra"]["resource_version"]) > 85 for *_, core in rec_a0.calls)
    cache, pa, rec_a, pb, rec_b = world()
    sweeps = []
    assert relist_a(pa, lambda: sweeps.append(pb.report_overdue(now, 0, "ns-b"))) == []
    assert sweeps[0] == len(bad_b) and sum(sweeps) == len(bad_b)  # once, whenever it ran again
    assert set(alert_uids(rec_b.calls)) == bad_b and len(rec_b.calls) == len(bad_b)  # only B's pods
    assert state(cache, rec_a) == unswept  # A's relist completed as if nobody had swept
    listed_uids = {uid(p) for p in pods_a[:-5]}
    assert cache.unready_tracked() == len(bad_b) + len(bad_a & listed_uids)
    del rec_a.calls[:]
    assert pa.report_overdue(now, 0, "ns-a") == len(bad_a & listed_uids)
    assert set(alert_uids(rec_a.calls)) == bad_a & listed_uids
    assert all(int(core["extra"]["resource_version"]) >= 500 for *_, core in rec_a.calls)  # the relist's lines' cores
    assert pa.report_overdue(now, 0, "ns-a") == 0 and pb.report_overdue(now, 0, "ns-b") == 0
    assert pa.report_overdue(now, 0, "ns-c") == 0 and pa.report_overdue(now, 0) == 0


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_sweep_between_the_slices_of_another_scopes_relist(native):
    check_shared_cache(native)


# ----------------------------------------------------------------------------- every alert on together (test 8)

def test_all_alerts_on_together():
    from test_termination_overdue import T1_S
    f = PodFactory(seed=61, namespaces=["default"])
    p0 = f.new_pod()
    uid, U = p0["metadata"]["uid"], C1_S + 2 * N
    everything = merged(UO(N, pending_overdue_seconds=N, terminating=True, terminating_overdue_seconds=30,
                           container_failures=True, pod_conditions=True), RV_EXTRA)
    bad = unready(f, p0, U)
    script = (feeds([("ADDED", with_rv(p0, 1)), ("MODIFIED", with_rv(f.scheduled(p0), 2))], True)
              + [("look", uid), ("sweep", C1_S + N + 2), ("sweep", C1_S + N + 3)]
              # Pending -> Running and unready in one line: the pending timer and its kept core go, this line's is kept
              + feeds([("MODIFIED", with_rv(bad, 3))], True) + [("look", uid), ("sweep", U + N - 1), ("sweep", U + N)]
              # ... back to Pending (an odd server; the rule all the same), and unready again: each period reports
              + feeds([("MODIFIED", with_rv(f.scheduled(p0), 4))], True) + [("look", uid), ("sweep", U + 2 * N)]
              + feeds([("MODIFIED", with_rv(bad, 5))], True) + [("look", uid), ("sweep", U + 2 * N)]
              + feeds([("MODIFIED", deleting(bad, 6))], True) + [("look", uid), ("sweep", T1_S + 30), ("sweep", T1_S + 10 * N)])
    for env, ov in (("production", everything), ("staging", merged(everything, {"watcher": {"notify_on": "phase_change"}}))):
        calls, _, c, ctrl, swept, looks = both_scripts(env, ov, script)
        kinds = [(et, int(core["extra"]["resource_version"]), (core.get("alert") or {}).get("kind"))
                 for _, et, _, _, core in calls if env == "production" or "alert" in core or et == "DELETED"]
        # (each period of either kind reports once: a mark goes with its timer)
        want = [("MODIFIED", 2, "pending_overdue"), ("MODIFIED", 3, "unready_overdue"), ("MODIFIED", 4, "pending_overdue"),
                ("MODIFIED", 5, "unready_overdue"), ("MODIFIED", 6, "termination_overdue")]
        if env == "production":  # (the terminating alert itself, let through the critical filter)
            want.insert(4, ("MODIFIED", 6, None))
        assert ctrl == [] and kinds == want, (env, kinds)
        assert swept == [1, 0, 0, 1, 1, 1, 1, 0], (env, swept)
        assert c["events_pending_overdue"] == 2
        assert looks[0][0] is None and looks[1][:2] == (U, 1) and looks[2][:2] == (None, 0) and looks[3][:2] == (U, 1)
        assert looks[4][:2] == (None, 0)
        assert c["events_unready_overdue"] == 2 and c["events_termination_overdue"] == 1 and c["events_terminating"] == 1


# ----------------------------------------------------------------------------- filters and the initial list (test 9)

def test_filters():
    f = PodFactory(seed=95, namespaces=["default", "elsewhere"])
    mine, other = f.new_pod(namespace="default"), f.new_pod(namespace="elsewhere")
    U = C1_S + 20
    events = [("ADDED", unready(f, mine, U, 1)), ("ADDED", unready(f, other, U, 2))]
    now = U + N
    # a namespace outside watcher.namespaces: tracked, no core kept, never reported
    ov = merged(UO(), RV_EXTRA, {"watcher": {"namespaces": ["default"]}})
    script = [("feed", lines(events)), ("look", other["metadata"]["uid"]), ("sweep", now), ("sweep", 10 * now)]
    for env, more in (("production", {}), ("staging", {"watcher": {"notify_on": "phase_change"}})):
        calls, _, c, _, swept, looks = both_scripts(env, merged(ov, more), script)
        assert swept == [1, 0] and looks == [(U, 2, False, False)]
        assert alert_uids(calls) == [mine["metadata"]["uid"]]
    # a pod of another shard is not even cached
    import zlib
    for index in (0, 1):
        sh = merged(UO(), RV_EXTRA, {"watcher": {"namespaces": [], "shard": {"count": 2, "index": index}}})
        calls, _, c, _, swept, _ = both_scripts("production", sh, [("feed", lines(events)), ("sweep", now)])
        owned = [p for p in (mine, other) if zlib.crc32(p["metadata"]["namespace"].encode()) % 2 == index]
        assert swept == [len(owned)] and c["events_other_shard"] == 2 - len(owned)
        assert alert_uids(calls) == sorted(p["metadata"]["uid"] for p in owned)


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_initial_list_skip(native):
    """A silent first LIST tracks nothing; the first watch line of the pod does."""
    f = PodFactory(seed=96, namespaces=["default"])
    a = f.new_pod()
    U = C1_S + 20
    s = settings_for("production", merged(UO(), RV_EXTRA, {"watcher": {"initial_list": "skip"}}))
    p, rec, m = pipeline(s, native)
    assert relist(p, native, [unready(f, a, U, 1)], notify=False) == []
    assert len(p.cache) == 1 and p.cache.unready_tracked() == 0 and p.report_overdue(U + 10 * N, 0) == 0 and rec.calls == []
    feed(p, native, lines([("MODIFIED", unready(f, a, U, 2))]))
    assert p.cache.unready_tracked() == 1 and p.report_overdue(U + N, 0) == 1 and alert_uids(rec.calls) == [a["metadata"]["uid"]]


# ----------------------------------------------------------------------------- through the native notifier (test 10)

def test_through_the_native_notifier():
    from k8s_watcher_amd.ops.decode import PyDecoder
    from k8s_watcher_amd.parallel.native_notifier import NativeNotifierPool
    from k8s_watcher_amd.testing.stub_sink import StubSink
    f = PodFactory(seed=64, namespaces=["default"])
    p0, q0 = f.new_pod(), f.new_pod()
    U = C1_S + 20

    async def body():
        sink = StubSink()
        await sink.start()
        s = load_settings("production", environ={}, overrides=merged(UO(), RV_EXTRA, {
            "watcher": {"decode_threads": 0}, "clusterapi": {"base_url": sink.url, "health_check_on_start": False}}))
        m = Metrics()
        pool = NativeNotifierPool(s.clusterapi, m)
        p = EventPipeline(s, PyDecoder("production"), pool, m)
        p.log_events_setting = False
        p.attach_native()
        p.handle_raw(lines([("ADDED", with_rv(p0, 1)), ("MODIFIED", unready(f, p0, U, 2)), ("ADDED", unready(f, q0, U, 3))]),
                     1, framed=False)
        swept = p.report_overdue(U + N + 1, 2)
        # in the same tick, the first pod's DELETED
        p.handle_raw(lines([("DELETED", unready(f, p0, U, 4))]), 3, framed=False)
        assert await pool.drain(20)
        got = sink.state.payloads()
        counters = dict(m.c)
        tracked = p.cache.unready_tracked()
        await pool.close()
        await sink.stop()
        return swept, got, counters, tracked

    swept, got, c, tracked = run(body(), timeout=60)
    assert swept == 2 and tracked == 1 and c["events_unready_overdue"] == 2 and c.get("notify_failed", 0) == 0
    mine = [x for x in got if x["uid"] == p0["metadata"]["uid"]]
    assert [(x["event_type"], "alert" in x) for x in mine] == [("MODIFIED", True), ("DELETED", False)]  # in order
    alert = mine[0]
    assert alert["alert"] == {"kind": "unready_overdue", "since_unix": U, "unready_seconds": N + 1}
    assert list(alert)[-3:] == ["alert", "event_timestamp", "event_type"] and alert["extra"]["resource_version"] == "2"
    other = [x for x in got if x["uid"] == q0["metadata"]["uid"]]
    assert [(x["event_type"], "alert" in x) for x in other] == [("MODIFIED", True)]


# ----------------------------------------------------------------------------- end to end (test 11)

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
        s = load_settings("production", environ={}, overrides=merged(UO(3600), RV_EXTRA, {
            "clusterapi": {"base_url": sink.url}, "watcher": {"engine": engine}}))
        svc = WatcherService(s, endpoint=KubeEndpoint(server=srv.url), metrics=Metrics())
        await svc.start()
        gauge = svc.metrics.gauges["pods_unready_tracked"]
        assert "pods_terminating_tracked" not in svc.metrics.gauges and "pods_pending_tracked" not in svc.metrics.gauges
        f = PodFactory(seed=52, namespaces=["default"])
        past = int(time.time()) - 3600
        pod, young, fine = unready(f, f.new_pod(), past), unready(f, f.new_pod(), past + 3540), f.running(f.new_pod())
        for x in (young, fine, pod):
            srv.create(x)
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
    assert alert["kind"] == "unready_overdue" and alert["since_unix"] == past
    assert 3600 <= alert["unready_seconds"] <= 3600 + 15 and got[0]["status"]["phase"] == "Running"
    assert tracked == [2.0, 1.0]
    assert c["events_unready_overdue"] == 1 and c["events_filtered_critical"] == 3
    assert "pods_unready_tracked 1" in text
    assert [ln for ln in text.splitlines() if "events_unready_overdue" in ln and not ln.startswith("#")][0].endswith(" 1")


# ----------------------------------------------------------------------------- metrics (test 12)

def test_metrics():
    from k8s_watcher_amd.metrics import COUNTERS as DECLARED
    assert "events_unready_overdue" in DECLARED and Metrics().c["events_unready_overdue"] == 0
    f = PodFactory(seed=61, namespaces=["default"])
    p0 = f.new_pod()
    U = C1_S + 20
    s = settings_for("production", UO())
    for native in (False, True):  # the native pipeline adds to the same counter
        p, _, m = pipeline(s, native)
        feed(p, native, lines([("ADDED", unready(f, p0, U, 1))]))
        assert p.cache.unready_tracked() == 1
        assert p.report_overdue(U + N, 0) == 1 and m.c["events_unready_overdue"] == 1
        assert m.c["events_termination_overdue"] == 0 and m.c["events_pending_overdue"] == 0
