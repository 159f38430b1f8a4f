"""Pods still terminating past their deletion deadline
(``watcher.alerts.terminating_overdue_seconds``).

The deadline grammar (``models/findings.py`` ``deletion_deadline`` and
``ops/csrc/findings.inc``), ``E_DEADLINE`` from both decoders, the deadline and
the reported mark in both caches, where an event stores the deadline (watch
path serial and partitioned, native relist, Python reconcile, the unchanged
items of a notifying relist), the sweep (``EventPipeline.report_overdue``) in
both engines, and what drives it. Every sweep but the end-to-end test's takes
its clock as an argument.
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
from k8s_watcher_amd.ops.cache import make_pod_cache
from k8s_watcher_amd.ops.decode import E_DEADLINE, make_decoder
from k8s_watcher_amd.testing.podgen import PodFactory, event_line
from k8s_watcher_amd.utils.config import ConfigError, load_settings, parse_override
from test_pod_condition_alerts import RV_EXTRA, Recorder, alerts, escaped, lines, merged, with_rv
from test_terminating_alerts import (COUNTERS as TERM_COUNTERS, T1, T2, corpus_line, corpus_object, deleting,
                                     md, settings_for, terminating_batch, warm_up)

KEY = "watcher.alerts.terminating_overdue_seconds"
N = 30  # the option's value in these tests
T1_S = 1752025892  # T1 and T2 (30 s earlier) as the issue pins them
T2_S = T1_S - 30
T3 = "2025-07-09T02:51:32Z"  # an hour after T1
COUNTERS = TERM_COUNTERS + ("events_termination_overdue",)


def OV(n=N, **kw):
    return alerts(terminating=True, terminating_overdue_seconds=n, **kw)


# ----------------------------------------------------------------------------- config (test 1)

def test_config():
    for env in ("development", "staging", "production"):
        assert load_settings(env, environ={}).watcher.terminating_overdue_seconds == 0
    w = load_settings("production", environ={}, overrides=OV(45)).watcher
    assert w.terminating_overdue_seconds == 45 and w.terminating is True
    ov = merged(parse_override("watcher.alerts.terminating=true"), parse_override(KEY + "=30"))
    assert load_settings("staging", environ={}, overrides=ov).watcher.terminating_overdue_seconds == 30
    assert load_settings("staging", environ={}, overrides=OV("30")).watcher.terminating_overdue_seconds == 30
    for bad in (True, False, 1.5, 30.0, [30], {"seconds": 30}, -1, "soon", "-1", "1.5", "", None):
        with pytest.raises(ConfigError, match=KEY):
            load_settings("staging", environ={}, overrides=OV(bad))
    # above 0 it needs the terminating alert, and says so with both keys
    for ov in (alerts(terminating_overdue_seconds=30), alerts(terminating=False, terminating_overdue_seconds=1)):
        with pytest.raises(ConfigError, match=KEY) as exc:
            load_settings("production", environ={}, overrides=ov)
        assert "watcher.alerts.terminating:" in str(exc.value) or "watcher.alerts.terminating " in str(exc.value)
    assert load_settings("production", environ={}, overrides=alerts(terminating_overdue_seconds=0)).watcher.terminating is False
    # no key for the check period
    from k8s_watcher_amd.engine.scopes import OVERDUE_CHECK_SECONDS
    assert OVERDUE_CHECK_SECONDS == 1.0


def test_print_config_shows_the_key(capsys):
    from k8s_watcher_amd.utils.config import dump_effective
    dump_effective(load_settings("production", environ={}))
    assert "terminating_overdue_seconds: 0" in capsys.readouterr().out
    dump_effective(load_settings("production", environ={}, overrides=OV(45)))
    assert "terminating_overdue_seconds: 45" in capsys.readouterr().out


# ----------------------------------------------------------------------------- the deadline (test 2)

PINNED = [
    ("1970-01-01T00:00:00Z", 0),
    ("1969-12-31T23:59:59Z", -1),
    ("2000-02-29T12:00:00Z", 951825600),
    ("2025-07-09T01:51:32Z", 1752025892),
    ("2025-07-09T10:51:32+09:00", 1752025892),
    ("2024-12-31T23:59:59-05:30", 1735709399),
    ("2100-02-28T23:59:59Z", 4107542399),
    ("2100-03-01T00:00:00Z", 4107542400),
    ("9999-12-31T23:59:59Z", 253402300799),
    ("0001-01-01T00:00:00Z", -62135596800),
    # fractions are dropped, offsets reach 23:59 either way
    ("2025-07-09T01:51:32.9Z", 1752025892),
    ("2025-07-09T01:51:32.123456789Z", 1752025892),
    ("1969-12-31T23:59:59.999999999Z", -1),
    ("2025-07-09T01:51:32+23:59", 1752025892 - 86340),
    ("2025-07-09T01:51:32-23:59", 1752025892 + 86340),
    ("2025-07-09T01:51:32+00:00", 1752025892),
    ("2025-07-09T01:51:32-00:00", 1752025892),
]
NO_DEADLINE = [
    "2100-02-29T00:00:00Z", "2025-13-01T00:00:00Z", "2025-07-09T24:00:00Z", "2025-07-09T01:51:60Z",
    "2025-07-09t01:51:32z", "2025-07-09T01:51:32", "2025-07-09T01:51:32+0900", "2025-07-09T01:51:32.Z",
    "0000-01-01T00:00:00Z",
    # the rest of the grammar's edges
    "", "Z", "2025-07-09", "2025-07-09T01:51:32z", "2025-07-09t01:51:32Z", " 2025-07-09T01:51:32Z",
    "2025-07-09T01:51:32Z ", "2025-07-09T01:51:32Z\n", "2025-07-09 01:51:32Z", "2025-00-09T01:51:32Z",
    "2025-07-00T01:51:32Z", "2025-07-32T01:51:32Z", "2025-06-31T01:51:32Z", "2023-02-29T01:51:32Z",
    "1900-02-29T01:51:32Z", "2025-07-09T01:60:32Z", "2025-07-09T01:51:32.1234567890Z", "2025-07-09T01:51:32+24:00",
    "2025-07-09T01:51:32+09:60", "2025-07-09T01:51:32+9:00", "2025-07-09T01:51:32+09:00Z", "2025-07-09T01:51:32ZZ",
    "2025-07-09T01:51:32,5Z", "+2025-07-09T01:51:32Z", "02025-07-09T01:51:32Z", "2025-7-09T01:51:32Z",
    "２025-07-09T01:51:32Z", "2025-07-09T01:51:3２Z", "2025-07-09T01:51:32 Z", "2025-07-09T01:51:32.٣Z",
    "2025-07-09T01:51:32\\u005a", "2025-07-09T01:51:32\x00Z",
]
# raw JSON spellings with escapes: the deadline is the decoded text's
SPELLED = [
    ('"2025-07-09T01:51:32\\u005a"', T1_S), ('"2025-07-09T01:51:32\\u005A"', T1_S),
    ('"\\u0032025-07-09\\u005401:51:32Z"', T1_S), ('"2025-07-09T01:51:32\\u002b09:00"', T1_S - 32400),
    ('"2025-07-09T01:51:32\\u007a"', None), ('"2025-07-09T01\\/51:32Z"', None), ('"2025-07-09T01:51:32Z\\n"', None),
    ('"2025-07-09T01:51:32\\uff3a"', None), ('"\\ud83d\\ude002025-07-09T01:51:32Z"', None),
    ('"2025-07-09T01:51:32\\\\u005a"', None),
]


def pod_with(text):
    return {"metadata": {"uid": "u", "deletionTimestamp": text}, "status": {"phase": "Running"}}


def reference_seconds(y, mo, d, h, mi, s, offset_s):
    """``datetime``'s answer (naive arithmetic, so that year 1 and 9999 with an offset stay in range)."""
    delta = datetime.datetime(y, mo, d, h, mi, s) - datetime.datetime(1970, 1, 1)
    return delta.days * 86400 + delta.seconds - offset_s


def valid_timestamp(rng):
    """-> (text, seconds by datetime): any year 1-9999, any offset, a fraction of 0-9 digits."""
    y, mo = rng.randint(1, 9999), rng.randint(1, 12)
    d = rng.randint(1, calendar.monthrange(y, mo)[1])
    h, mi, s = rng.randint(0, 23), rng.randint(0, 59), rng.randint(0, 59)
    frac = "".join(rng.choice("0123456789") for _ in range(rng.randint(0, 9)))
    offset, zone = 0, "Z"
    if rng.random() < 0.6:
        oh, om, sign = rng.randint(0, 23), rng.randint(0, 59), rng.choice("+-")
        offset = (oh * 3600 + om * 60) * (1 if sign == "+" else -1)
        zone = "%s%02d:%02d" % (sign, oh, om)
    text = "%04d-%02d-%02dT%02d:%02d:%02d%s%s" % (y, mo, d, h, mi, s, "." + frac if frac else "", zone)
    return text, reference_seconds(y, mo, d, h, mi, s, offset)


def test_deadline_table():
    from k8s_watcher_amd.models.findings import deletion_deadline
    for text, want in PINNED:
        assert deletion_deadline(pod_with(text)) == want, text
    for text in NO_DEADLINE:
        assert deletion_deadline(pod_with(text)) is None, text
    for raw, want in SPELLED:
        assert deletion_deadline(pod_with(json.loads(raw))) == want, raw
    # not terminating: no deadline, whatever else is there
    for pod in ({}, None, [], {"metadata": None}, {"metadata": {"deletionTimestamp": None}},
                {"metadata": {"deletionTimestamp": 1752025892}}, {"metadata": {"deletionTimestamp": [T1]}},
                {"metadata": [T1]}, {"metadata": {"creationTimestamp": T1}}):
        assert deletion_deadline(pod) is None, pod
    rng = random.Random(2025)
    for _ in range(500):
        text, want = valid_timestamp(rng)
        assert deletion_deadline(pod_with(text)) == want, text


FULLWIDTH = "０１２３４５６７８９"


def mutated_timestamp(rng):
    """A valid timestamp after one mutation, as a raw JSON string token."""
    text, _ = valid_timestamp(rng)
    kind = rng.randrange(11)
    digits = [i for i, ch in enumerate(text) if ch.isdigit()]
    if kind == 0:  # a digit replaced by a letter or a full-width digit
        i = rng.choice(digits)
        text = text[:i] + rng.choice(("x", "O", "l", FULLWIDTH[int(text[i])])) + text[i + 1:]
    elif kind == 1:  # a character dropped
        i = rng.randrange(len(text))
        text = text[:i] + text[i + 1:]
    elif kind == 2:  # ... or doubled
        i = rng.randrange(len(text))
        text = text[:i] + text[i] + text[i:]
    elif kind == 3:  # lower case
        text = text.replace("T", "t") if rng.random() < 0.5 or not text.endswith("Z") else text[:-1] + "z"
    elif kind == 4:  # a field pushed out of its range
        at, val = rng.choice(((0, "0000"), (5, "13"), (5, "00"), (8, "32"), (8, "00"), (11, "24"), (14, "60"), (17, "60"),
                              (17, "61"), (-5, "24"), (-2, "60")))
        if at >= 0 or not text.endswith("Z"):
            at = at if at >= 0 else len(text) + at
            text = text[:at] + val + text[at + len(val):]
        else:
            text = text[:17] + "60" + text[19:]
    elif kind == 5:  # a leap day: there in a leap year only
        text = text[:5] + "02-29" + text[10:]
    elif kind == 6:  # a fraction of ten digits
        text = text[:19] + "." + "".join(rng.choice("0123456789") for _ in range(10)) + text[19:].lstrip(".0123456789")
    elif kind == 7:  # separators swapped
        a, b = rng.choice((("-", ":"), (":", "-"), ("T", " "), (":", "."), ("T", "-")))
        text = text.replace(a, b, rng.choice((1, 2)))
    elif kind == 8:  # the fraction replaced by another of 1-9 digits: still valid
        text = (text[:19] + "." + "".join(rng.choice("0123456789") for _ in range(rng.randint(1, 9)))
                + text[19:].lstrip(".0123456789"))
    # (kinds 9 and 10: left valid; below, any of them may be spelled with \uXXXX escapes)
    if kind >= 9 or rng.random() < 0.3:
        return escaped(rng, text)
    return json.dumps(text, ensure_ascii=False)


def timestamp_lines(n=2000, seed=23):
    """The tables above and ``n`` seeded mutations as watch lines of Running pods u0, u1, ...
    -> [(line bytes, uid, event type)]."""
    raws = [json.dumps(t, ensure_ascii=False) for t, _ in PINNED] + [json.dumps(t, ensure_ascii=False) for t in NO_DEADLINE]
    raws += [raw for raw, _ in SPELLED]
    rng = random.Random(seed)
    raws += [mutated_timestamp(rng) for _ in range(n)]
    out = []
    for i, raw in enumerate(raws):
        etype = "DELETED" if i % 97 == 96 else "ADDED" if i % 5 == 0 else "MODIFIED"
        uid = "u%d" % i
        out.append((corpus_line(md(',"deletionTimestamp":%s' % raw, rv=str(i + 1)), etype, uid), uid, etype))
    return out


def fuzz_pods(n=200, seed=23):
    """The pod objects (raw JSON text) of the first ``n`` mutated lines: findings_check's input."""
    skip = len(PINNED) + len(NO_DEADLINE) + len(SPELLED)
    return [ln[ln.index(b'"object":') + 9:-2].decode() for ln, _, _ in timestamp_lines(n, seed)[skip:]]


def timestamp_corpus():
    """The pinned tables as pod objects (raw JSON text) with the expected deadline."""
    raws = [(json.dumps(t, ensure_ascii=False), want) for t, want in PINNED]
    raws += [(json.dumps(t, ensure_ascii=False), None) for t in NO_DEADLINE] + list(SPELLED)
    return [(corpus_object(md(',"deletionTimestamp":%s' % raw)), want) for raw, want in raws]


def decoder_for(s, engine="python"):
    w = s.watcher
    return make_decoder(engine, s.environment, w.state_format, w.payload_extra, w.validate,
                        w.container_failures, w.container_failure_reasons, w.pod_conditions, w.pod_condition_rules,
                        w.terminating, w.terminating_overdue_seconds > 0)


def pipeline(s, native, cache=None, notifier=None):
    rec, m = Recorder(), Metrics()
    p = EventPipeline(s, decoder_for(s), notifier if notifier is not None else rec, m, cache)
    p.log_events_setting = False
    if native:
        p.attach_native()
    return p, rec, m


def feed(p, native, data):
    return p.handle_raw(data, 0, framed=False) if native else p.handle_batch(p.decoder.feed(data), 0)


def check_deadlines():
    """``E_DEADLINE`` from both decoders (the native one under validate payload
    and full) and the deadline both fused pipelines store (full parse and
    filter-first) on the tables and 2,000 mutated timestamps: all the Python
    function's."""
    from k8s_watcher_amd.models.findings import deletion_deadline
    data = timestamp_lines()
    n_tables = len(PINNED) + len(NO_DEADLINE) + len(SPELLED)
    assert len(data) == 2000 + n_tables
    want = {}
    for ln, uid, etype in data:
        want[uid] = deletion_deadline(json.loads(ln)["object"])
    # the condition on the seed, by the Python function alone
    mutated = [want[uid] for _, uid, _ in data[n_tables:]]
    assert sum(d is not None for d in mutated) >= 300 and sum(d is None for d in mutated) >= 300
    for (text, w), (_, uid, _) in zip(PINNED, data):
        assert want[uid] == w, text
    py = make_decoder("python", "staging", terminating=True, overdue=True)
    a = [py.feed(ln)[0] for ln, _, _ in data]
    for ev, (ln, uid, etype) in zip(a, data):
        assert ev[0] == etype and len(ev) == 13, ln
        assert ev[E_DEADLINE] == (None if etype == "DELETED" else want[uid]), ln
        assert ev[E_DEADLINE] is None or (type(ev[E_DEADLINE]) is int and ev[11] == 1), ln
    for validate in ("payload", "full"):
        nat = make_decoder("native", "staging", validate=validate, terminating=True, overdue=True)
        for ea, (ln, _, _) in zip(a, data):
            eb = nat.feed(ln)[0]
            assert len(eb) == 13 and eb[:7] == ea[:7] and eb[9:] == ea[9:], (validate, ln)
            assert type(eb[E_DEADLINE]) is type(ea[E_DEADLINE]), ln
    # with the option off the tuples are what they were
    for eng in ("python", "native"):
        d = make_decoder(eng, "staging", terminating=True)
        assert all(len(d.feed(ln)[0]) == 12 for ln, _, _ in data[:40])
        d = make_decoder(eng, "staging", terminating=False, overdue=True)  # nothing without the terminating alert
        assert all(len(d.feed(ln)[0]) == 9 for ln, _, _ in data[:40])
    # the fused pipelines: staging parses every line in full, production filter-first
    batch = b"".join(ln for ln, _, _ in data)
    live = {uid for _, uid, etype in data if etype != "DELETED"}
    for env, ov in (("staging", OV()), ("production", merged(OV(), {"watcher": {"namespaces": []}}))):
        for validate in ("payload", "full"):
            s = settings_for(env, merged(ov, {"watcher": {"validate": validate}}))
            got = {}
            for native in (False, True):
                p, rec, m = pipeline(s, native)
                assert feed(p, native, batch) == []
                got[native] = ({uid: p.cache.deadline(uid) for _, uid, _ in data}, p.cache.tracked(), len(rec.calls))
                assert set(u for u, _ in p.cache.items()) == live
            assert got[False] == got[True], (env, validate)
            assert got[True][0] == {uid: (want[uid] if uid in live else None) for _, uid, _ in data}, (env, validate)
            assert got[True][1] == sum(want[uid] is not None for uid in live)


def test_deadlines_one_verdict_from_both_engines():
    check_deadlines()


# ----------------------------------------------------------------------------- both caches, one API (test 3)

@pytest.mark.parametrize("native", [False, True], ids=["python-cache", "native-cache"])
def test_both_caches_one_api(native):
    cache = make_pod_cache(native)
    # an unknown uid is a no-op
    cache.set_deadline("nobody", 5)
    assert cache.deadline("nobody") is None and cache.tracked() == 0 and len(cache) == 0
    assert cache.take_overdue(10 ** 9, 0) == []
    cache.observe("ADDED", "u", "1", "Running", "default", "n")
    assert cache.deadline("u") is None and cache.tracked() == 0
    cache.set_deadline("u", 100)
    assert cache.deadline("u") == 100 and cache.tracked() == 1
    # no core: neither returned nor marked; a later core makes it reportable
    assert cache.take_overdue(1000, 30) == []
    cache.set_core("u", b'{"a":1}')
    # the boundary: now - d == after fires, one second earlier does not
    assert cache.take_overdue(129, 30) == []
    assert cache.take_overdue(130, 30) == [("u", "default", "n", b'{"a":1}', 100)]
    assert cache.take_overdue(131, 30) == [] and cache.take_overdue(10 ** 9, 0) == []  # marked
    # a value keeps the mark (a deadline that moves does not re-alert), None clears deadline and mark
    cache.set_deadline("u", 50)
    assert cache.deadline("u") == 50 and cache.take_overdue(10 ** 9, 0) == []
    cache.set_deadline("u", None)
    assert cache.deadline("u") is None and cache.tracked() == 0
    cache.set_deadline("u", None)  # twice is fine
    cache.set_deadline("u", 60)
    assert cache.take_overdue(89, 30) == [] and cache.take_overdue(90, 30) == [("u", "default", "n", b'{"a":1}', 60)]
    # put (a whole new entry) clears both
    cache.put("u", "2", "Running", "default", "n", b'{"b":2}')
    assert cache.deadline("u") is None and cache.tracked() == 0
    cache.set_deadline("u", 60)
    assert cache.take_overdue(90, 30) == [("u", "default", "n", b'{"b":2}', 60)]
    # ... and so does every way an entry goes
    cache.observe("DELETED", "u", "3", "Running", "default", "n")
    assert cache.tracked() == 0 and cache.deadline("u") is None
    for gone in (lambda: cache.pop("v"), lambda: cache.drop_namespaces(["ns-a"]),
                 lambda: cache.drop_namespaces_except(["default"]), cache.clear):
        cache.put("v", "1", "Running", "ns-a", "m", b"{}")
        cache.set_deadline("v", 7)
        assert cache.tracked() == 1
        gone()
        assert cache.tracked() == 0 and cache.deadline("v") is None and cache.take_overdue(10 ** 9, 0) == []
    # scope_ns, negative deadlines, int64 ends, several pods; to_records() knows nothing of any of it
    cache.clear()
    for i, ns in enumerate(["ns-a", "ns-b", "ns-a", None]):
        cache.put("p%d" % i, "1", "Running", ns, "n%d" % i, b'{"i":%d}' % i)
    cache.put("bare", "1", "Running", "ns-b", "bare", None)
    for uid, due in (("p0", -62135596800), ("p1", 0), ("p2", 253402300799), ("p3", -1), ("bare", 0)):
        cache.set_deadline(uid, due)
    records = sorted(cache.to_records())
    assert cache.tracked() == 5 and cache.deadline("p0") == -62135596800 and cache.deadline("p2") == 253402300799
    assert cache.take_overdue(30, 30, "ns-c") == []
    assert cache.take_overdue(30, 30, "ns-b") == [("p1", "ns-b", "n1", b'{"i":1}', 0)]
    assert sorted(cache.take_overdue(30, 30, "ns-a")) == [("p0", "ns-a", "n0", b'{"i":0}', -62135596800)]
    assert cache.take_overdue(30, 30) == [("p3", None, "n3", b'{"i":3}', -1)]
    assert cache.take_overdue(253402300799 + 30, 30, "ns-a") == [("p2", "ns-a", "n2", b'{"i":2}', 253402300799)]
    cache.set_core("bare", b"{}")
    assert cache.take_overdue(30, 30) == [("bare", "ns-b", "bare", b"{}", 0)]
    for uid, due in (("p0", 2 ** 63 - 1), ("p1", -2 ** 63)):
        cache.set_deadline(uid, None)
        cache.set_deadline(uid, due)
        assert cache.deadline(uid) == due
    assert [t[0] for t in cache.take_overdue(2 ** 63 - 1, 2 ** 62)] == ["p1"]
    assert cache.tracked() == 5
    assert sorted(r[:5] for r in cache.to_records()) == sorted(r[:5] for r in records)
    assert all(len(r) == 6 for r in cache.to_records())
    fresh = make_pod_cache(native, cache.to_records())
    assert fresh.tracked() == 0 and fresh.deadline("p0") is None and len(fresh) == 5
    cache.load_records(cache.to_records())  # records over live entries: whole new entries, as put()
    assert cache.tracked() == 0 and cache.take_overdue(2 ** 62, 0) == []


# ----------------------------------------------------------------------------- a pod's life with sweeps (test 4)

class RawRecorder(Recorder):
    """Keeps the submitted bytes too."""

    def __init__(self):
        super().__init__()
        self.raw = []

    def submit(self, uid, et, ns, name, core, read_ns, ts):
        super().submit(uid, et, ns, name, core, read_ns, ts)
        self.raw.append(bytes(core))


def run_script(s, native, script, cache=None):
    """``script``: ("feed", bytes) and ("sweep", now_s[, scope_ns]) steps.
    -> (calls, the submitted bytes, counters, control event types, what each sweep returned)."""
    rec = RawRecorder()
    p, _, m = pipeline(s, native, cache, rec)
    ctrl, swept = [], []
    for step in script:
        if step[0] == "feed":
            ctrl += feed(p, native, step[1])
        else:
            swept.append(p.report_overdue(step[1], 0, *step[2:]))
    return rec.calls, rec.raw, {k: m.c.get(k, 0) for k in COUNTERS}, [c[0] for c in ctrl], swept, p.cache.tracked()


def both_scripts(env, ov, script):
    s = settings_for(env, ov)
    py = run_script(s, False, script)
    nat = run_script(s, True, script)
    assert py == nat  # the calls, the bytes, the counters, the sweeps' returns, what is tracked
    return py


def feeds(events, one_read):
    return [("feed", lines(events))] if one_read else [("feed", event_line(t, o)) for t, o in events]


def rvs(calls):
    """(event type, resourceVersion of the payload, overdue_seconds of its alert or None)."""
    return [(et, int(core["extra"]["resource_version"]), (core.get("alert") or {}).get("overdue_seconds"))
            for _, et, _, _, core in calls]


def pod_life(seed=61):
    f = PodFactory(seed=seed, namespaces=["default"])
    p0 = f.new_pod()
    return p0, f.running(p0)


def check_pod_life():
    p0, run_ = pod_life()
    begin = [("ADDED", with_rv(p0, 1)), ("MODIFIED", with_rv(run_, 2)), ("MODIFIED", deleting(run_, 3))]
    phase = merged(RV_EXTRA, {"watcher": {"notify_on": "phase_change"}})
    for one_read in (True, False):
        script = (feeds(begin, one_read) + [("sweep", T1_S + N - 1), ("sweep", T1_S + N), ("sweep", T1_S + N + 1)]
                  + feeds([("MODIFIED", deleting(run_, 4, finalizers=("example.com/a",)))], one_read)  # a finalizer goes
                  + [("sweep", T1_S + 2 * N)] + feeds([("DELETED", deleting(run_, 6, finalizers=None))], one_read)
                  + [("sweep", T1_S + 3 * N)])
        # production, the critical filter on
        calls, raw, c, ctrl, swept, tracked = both_scripts("production", merged(OV(), RV_EXTRA), script)
        assert ctrl == [] and swept == [0, 1, 0, 0, 0] and tracked == 0
        assert rvs(calls) == [("MODIFIED", 3, None), ("MODIFIED", 3, N), ("DELETED", 6, None)]
        assert c["events_termination_overdue"] == 1 and c["events_terminating"] == 1
        assert c["events_received"] == 5 and c["events_filtered_critical"] == 3  # the sweep receives nothing
        term, alert = calls[0][4], calls[1][4]
        assert alert.pop("alert") == {"kind": "termination_overdue", "deadline_unix": T1_S, "overdue_seconds": N}
        assert alert == term and calls[1][:4] == calls[0][:4]  # the cached core, the member apart
        assert list(json.loads(raw[1]))[-1] == "alert"  # spliced in before the closing brace
        assert raw[1] == raw[0][:-1] + (b',"alert":{"kind":"termination_overdue","deadline_unix":%d,'
                                        b'"overdue_seconds":%d}}' % (T1_S, N))
        # staging, notify_on: phase_change
        calls, _, c, _, swept, _ = both_scripts("staging", merged(OV(), phase), script)
        assert swept == [0, 1, 0, 0, 0]
        assert rvs(calls) == [("ADDED", 1, None), ("MODIFIED", 2, None), ("MODIFIED", 3, None), ("MODIFIED", 3, N),
                              ("DELETED", 6, None)]
        assert c["events_termination_overdue"] == 1 and c["events_terminating"] == 1 and c["events_unchanged"] == 1
        # the option off: today's notifications, the sweep does nothing
        for env, ov, want in (("production", RV_EXTRA, [("MODIFIED", 3, None), ("DELETED", 6, None)]),
                              ("staging", phase, [("ADDED", 1, None), ("MODIFIED", 2, None), ("MODIFIED", 3, None),
                                                  ("DELETED", 6, None)])):
            calls, _, c, _, swept, tracked = both_scripts(env, merged(alerts(terminating=True), ov), script)
            assert rvs(calls) == want and swept == [0] * 5 and tracked == 0 and c["events_termination_overdue"] == 0
        # the timestamp goes and comes back: a second alert
        again = (feeds(begin, one_read) + [("sweep", T1_S + N)] + feeds([("MODIFIED", with_rv(run_, 4))], one_read)
                 + [("sweep", T1_S + N + 1)] + feeds([("MODIFIED", deleting(run_, 5, ts=T3))], one_read)
                 + [("sweep", T1_S + 3600 + N - 1), ("sweep", T1_S + 3600 + N + 7), ("sweep", T1_S + 7200)])
        calls, _, c, _, swept, tracked = both_scripts("production", merged(OV(), RV_EXTRA), again)
        assert swept == [1, 0, 0, 1, 0] and tracked == 1
        assert rvs(calls) == [("MODIFIED", 3, None), ("MODIFIED", 3, N), ("MODIFIED", 5, None), ("MODIFIED", 5, N + 7)]
        assert [core["alert"]["deadline_unix"] for *_, core in calls if "alert" in core] == [T1_S, T1_S + 3600]
        assert c["events_termination_overdue"] == 2 and c["events_terminating"] == 2
        # a forced delete moves the deadline after the alert: none (earlier or later)
        forced = (feeds(begin, one_read) + [("sweep", T1_S + N)]
                  + feeds([("MODIFIED", deleting(run_, 4, ts=T2, grace=0))], one_read) + [("sweep", T1_S + N + 1)]
                  + feeds([("MODIFIED", deleting(run_, 5, ts=T3))], one_read) + [("sweep", T1_S + 7200)])
        calls, _, c, _, swept, tracked = both_scripts("production", merged(OV(), RV_EXTRA), forced)
        assert swept == [1, 0, 0] and tracked == 1 and c["events_termination_overdue"] == 1
        assert rvs(calls) == [("MODIFIED", 3, None), ("MODIFIED", 3, N)]
        # ... but before the alert the moved deadline is the one that counts
        moved = (feeds(begin + [("MODIFIED", deleting(run_, 4, ts=T2, grace=0))], one_read)
                 + [("sweep", T2_S + N - 1), ("sweep", T2_S + N)])
        calls, _, _, _, swept, _ = both_scripts("production", merged(OV(), RV_EXTRA), moved)
        assert swept == [0, 1] and calls[-1][4]["alert"] == {"kind": "termination_overdue", "deadline_unix": T2_S,
                                                             "overdue_seconds": N}
        # a timestamp of another shape: terminating, reported as such, never overdue
        odd = feeds(begin[:2] + [("MODIFIED", deleting(run_, 3, ts="2025-07-09T01:51:32"))], one_read) + [("sweep", 2 ** 62)]
        calls, _, c, _, swept, tracked = both_scripts("production", merged(OV(), RV_EXTRA), odd)
        assert swept == [0] and tracked == 0 and rvs(calls) == [("MODIFIED", 3, None)] and c["events_terminating"] == 1
    # every extra field on: the bodies are the same bytes from both engines (both_scripts compares them)
    from k8s_watcher_amd.models.payload import EXTRA_NAMES
    everything = {"watcher": {"payload_extra_fields": list(EXTRA_NAMES)}}
    script = feeds(begin, True) + [("sweep", T1_S + N + 3)]
    calls, raw, _, _, swept, _ = both_scripts("production", merged(OV(), everything), script)
    assert swept == [1] and calls[-1][4]["extra"]["termination"]["deletion_timestamp"] == T1
    assert calls[-1][4]["alert"]["overdue_seconds"] == N + 3 and raw[-1].endswith(b'"overdue_seconds":33}}')
    # the log line, with log_events
    for native in (False, True):
        s = settings_for("production", merged(OV(), RV_EXTRA))
        p, rec, _ = pipeline(s, native)
        p.log_events_setting = True
        seen = []
        p.elog.log = lambda level, msg: seen.append((level, msg))
        feed(p, native, lines(begin))
        assert p.report_overdue(T1_S + N + 3, 0) == 1
        name = run_["metadata"]["name"]
        assert (20, f"Pod termination overdue: default/{name} - {N + 3}s past deletionTimestamp") in seen, (native, seen)


def test_pod_life_with_sweeps():
    check_pod_life()


# ----------------------------------------------------------------------------- partitioned against serial (test 5)

def feed_and_sweep(env, ov, warm, data, partitioned, now_s):
    """``data`` as one batch through the native pipeline (3 decode workers) and
    the native notifier, then one sweep at ``now_s``; -> the sink's alert
    bodies by uid, the other bodies, every cached pod's deadline, tracked(),
    the counters, the apply's probe and the sweep's return."""
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
            kw.probe(True)
            ctrl += [c[0] for c in p.handle_raw(data, 1, framed=False)]
        finally:
            probe = kw.probe(False)
            kw.set_partitioned_apply(prev)
        tracked = p.cache.tracked()
        swept = p.report_overdue(now_s, 1)
        assert await pool.drain(20) and ctrl == []
        sent = [{k: v for k, v in x.items() if k != "event_timestamp"} for x in sink.state.payloads()]
        alerts_ = {x["uid"]: json.dumps(x, sort_keys=True) for x in sent if "alert" in x}
        assert len(alerts_) == sum("alert" in x for x in sent) and all(x["event_type"] == "MODIFIED" for x in sent if "alert" in x)
        rest = collections.Counter(json.dumps(x, sort_keys=True) for x in sent if "alert" not in x)
        deadlines = {u: p.cache.deadline(u) for u, _ in p.cache.items()}
        counters = {k: v for k, v in m.c.items() if k.startswith(("events_", "bookmarks")) and v}
        assert p.cache.tracked() == tracked
        await pool.close()
        await sink.stop()
        dpool.close()
        return alerts_, rest, deadlines, tracked, counters, probe, swept

    return run(body(), timeout=60)


def check_partitioned_matches_serial():
    from k8s_watcher_amd.ops.native import load
    data, pod_ns, n = terminating_batch()
    warm = warm_up()
    now_s = T1_S + N
    ov = merged(OV(), RV_EXTRA)
    s_alerts, s_rest, s_due, s_tracked, s_cnt, s_probe, s_swept = feed_and_sweep("production", ov, warm, data, False, now_s)
    p_alerts, p_rest, p_due, p_tracked, p_cnt, p_probe, p_swept = feed_and_sweep("production", ov, warm, data, True, now_s)
    assert s_probe.get("partitioned_batches", 0) == 0
    assert p_probe["partitioned_batches"] == 1 and p_probe["lines"] == n and p_probe["tail_serial_lines"] == 0
    assert p_alerts == s_alerts and p_rest == s_rest and p_due == s_due and p_tracked == s_tracked and p_cnt == s_cnt
    assert p_swept == s_swept == len(s_alerts) == s_cnt["events_termination_overdue"]
    # the condition: enough reported pods, spread over the store's shards
    part = load().apply_partition
    assert len(s_alerts) >= 8 and len({part(u) for u in s_alerts}) >= 4, (len(s_alerts), {part(u) for u in s_alerts})
    assert s_tracked > len(s_alerts)  # (pods of namespaces the filter drops are tracked and have no core)
    assert set(s_due.values()) >= {None, T1_S, T2_S}
    for u, body in s_alerts.items():
        a = json.loads(body)["alert"]
        assert a == {"kind": "termination_overdue", "deadline_unix": s_due[u], "overdue_seconds": now_s - s_due[u]}
    # the Python engine: the same reports, deadlines and counters
    s = settings_for("production", ov)
    rec = RawRecorder()
    p, _, m = pipeline(s, False, None, rec)
    assert feed(p, False, warm) == [] and feed(p, False, data) == []
    assert p.cache.tracked() == s_tracked and {u: p.cache.deadline(u) for u, _ in p.cache.items()} == s_due
    assert p.report_overdue(now_s, 0) == s_swept
    got = {u: json.dumps(dict(core, event_type=et), sort_keys=True) for u, et, _, _, core in rec.calls if "alert" in core}
    assert got == s_alerts
    assert {k: v for k, v in m.c.items() if k.startswith(("events_", "bookmarks")) and v} == s_cnt


def test_partitioned_apply_matches_serial():
    check_partitioned_matches_serial()


# ----------------------------------------------------------------------------- relist and restart (test 6)

def relist(p, native, items, scope=None, notify=True):
    """A LIST of ``items`` reconciled by the engine's own relist; -> control events."""
    from test_native_relist import list_pages, native_relist
    if native:
        return native_relist(p, items, scope, notify=notify)[0]
    evs = p.decoder.decode_list(list_pages(items, 10 ** 6)[0])[2]
    assert all(len(e) == 13 for e in evs)
    return p.reconcile(evs, 0, notify=notify, scope_ns=scope)


def alert_uids(calls):
    return sorted(u for u, _, _, _, core in calls if "alert" in core)


def check_relist(native):
    f = PodFactory(seed=71, namespaces=["default"])
    a, b, c_, d, e = (f.running(f.new_pod()) for _ in range(5))
    uid = lambda p: p["metadata"]["uid"]  # noqa: E731
    s = settings_for("production", merged(OV(), RV_EXTRA))
    p, rec, m = pipeline(s, native)
    feed(p, native, lines([("ADDED", with_rv(a, 1)), ("ADDED", deleting(b, 2)), ("ADDED", with_rv(c_, 3)),
                           ("ADDED", with_rv(d, 4)), ("ADDED", deleting(e, 5))]))
    assert p.cache.tracked() == 2 and p.report_overdue(T1_S + N, 0) == 2
    del rec.calls[:]
    # the gap (a 410): a's deletion began, b moved on terminating (reported already), c is gone, d moved on,
    # e's timestamp went away
    listed = [deleting(a, 10), deleting(b, 11, finalizers=("example.com/a",)), with_rv(d, 12), with_rv(e, 13)]
    assert relist(p, native, listed) == []
    assert sorted((u, et) for u, et, *_ in rec.calls) == sorted([(uid(a), "MODIFIED"), (uid(c_), "DELETED")])
    assert p.cache.tracked() == 2 and p.cache.deadline(uid(a)) == T1_S and p.cache.deadline(uid(e)) is None
    del rec.calls[:]
    assert p.report_overdue(T1_S + N - 1, 0) == 0
    assert p.report_overdue(T1_S + N, 0) == 1 and alert_uids(rec.calls) == [uid(a)]  # b was reported before the gap
    assert rec.calls[0][4]["extra"]["resource_version"] == "10" and m.c["events_termination_overdue"] == 3
    # a restart: the cache rebuilt from its records has the cores and no deadline
    records = p.cache.to_records()
    assert all(len(r) == 6 for r in records)
    q, rec2, m2 = pipeline(s, native, make_pod_cache(native, records))
    assert q.cache.tracked() == 0 and q.report_overdue(2 ** 40, 0) == 0
    # ... a relist whose items are all unchanged restores every deadline, and the sweep reports from the
    # checkpointed cores: the mark did not persist, so a and b once more
    assert relist(q, native, listed) == [] and rec2.calls == []
    assert q.cache.tracked() == 2 and q.cache.deadline(uid(a)) == T1_S and q.cache.deadline(uid(b)) == T1_S
    assert q.report_overdue(T1_S + N + 5, 0) == 2 and alert_uids(rec2.calls) == sorted([uid(a), uid(b)])
    assert {core["extra"]["resource_version"] for *_, core in rec2.calls} == {"10", "2"}  # the cores as checkpointed
    assert all(core["alert"]["overdue_seconds"] == N + 5 for *_, core in rec2.calls)
    assert q.report_overdue(T1_S + N + 6, 0) == 0
    # an unchanged item whose timestamp is gone (cannot happen without a new resourceVersion; the rule all the same)
    q.cache.set_deadline(uid(d), 5)
    assert relist(q, native, listed) == [] and q.cache.deadline(uid(d)) is None and q.cache.tracked() == 2
    # a silent relist (initial_list: skip) tracks nothing, changed items or unchanged
    for cache in (None, make_pod_cache(native, records)):
        r, rec3, _ = pipeline(s, native, cache)
        assert relist(r, native, listed, notify=False) == []
        assert rec3.calls == [] and len(r.cache) == 4 and r.cache.tracked() == 0 and r.report_overdue(2 ** 40, 0) == 0


@pytest.mark.parametrize("native", [True, False], ids=["native-relist", "python-reconcile"])
def test_relist_and_restart(native):
    check_relist(native)


def scoped_pods(seed, ns, n):
    f = PodFactory(seed=seed, namespaces=[ns])
    return [f.running(f.new_pod()) for _ in range(n)]


def check_shared_cache(native):
    """Two scopes on one cache: B is swept while A's relist stands in mid-walk."""
    from test_native_relist import list_pages
    ov = merged(OV(), RV_EXTRA, {"watcher": {"namespace_scope": "server", "namespaces": ["ns-a", "ns-b"]}})
    s = settings_for("production", ov)
    pods_a, pods_b = scoped_pods(91, "ns-a", 90), scoped_pods(92, "ns-b", 12)
    uid = lambda p: p["metadata"]["uid"]  # noqa: E731
    term_a = {uid(p) for p in pods_a[::3]}
    term_b = {uid(p) for p in pods_b[::2]}
    listed_a = [deleting(p, 500 + i) if uid(p) in term_a else with_rv(p, 500 + i) for i, p in enumerate(pods_a[:-5])]

    def world():
        cache = make_pod_cache(native)
        pa, rec_a, _ = pipeline(s, native, cache)
        pb, rec_b, _ = pipeline(s, native, cache)
        feed(pa, native, lines([("ADDED", with_rv(p, i + 1)) for i, p in enumerate(pods_a)]))
        feed(pb, native, lines([("ADDED", deleting(p, 200 + i) if uid(p) in term_b else with_rv(p, 200 + i))
                                for i, p in enumerate(pods_b)]))
        assert cache.tracked() == len(term_b) and len(rec_b.calls) == len(term_b)
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
                sorted(map(json.dumps, cache.to_records())), {u: cache.deadline(u) for u, _ in cache.items()})

    cache0, pa0, rec_a0, _, _ = world()
    assert relist_a(pa0, lambda: None) == []
    unswept = state(cache0, rec_a0)
    cache, pa, rec_a, pb, rec_b = world()
    del rec_b.calls[:]
    sweeps = []
    assert relist_a(pa, lambda: sweeps.append(pb.report_overdue(T1_S + N, 0, "ns-b"))) == []
    assert sweeps[0] == len(term_b) and sum(sweeps) == len(term_b)  # once, whenever it ran again
    assert set(alert_uids(rec_b.calls)) == term_b and len(rec_b.calls) == len(term_b)  # only B's pods
    assert state(cache, rec_a) == unswept  # A's relist completed as if nobody had swept
    listed_uids = {uid(p) for p in pods_a[:-5]}
    assert cache.tracked() == len(term_b) + len(term_a & listed_uids)
    del rec_a.calls[:]
    assert pa.report_overdue(T1_S + N, 0, "ns-a") == len(term_a & listed_uids)
    assert set(alert_uids(rec_a.calls)) == term_a & listed_uids
    assert pa.report_overdue(T1_S + N, 0, "ns-a") == 0 and pb.report_overdue(T1_S + N, 0, "ns-b") == 0
    assert pa.report_overdue(T1_S + N, 0, "ns-c") == 0 and pa.report_overdue(T1_S + N, 0) == 0


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_sweep_between_the_slices_of_another_scopes_relist(native):
    check_shared_cache(native)


# ----------------------------------------------------------------------------- filters (test 7)

def test_filters():
    f = PodFactory(seed=95, namespaces=["default", "elsewhere"])
    mine, other = f.running(f.new_pod(namespace="default")), f.running(f.new_pod(namespace="elsewhere"))
    events = [("ADDED", with_rv(mine, 1)), ("ADDED", with_rv(other, 2)),
              ("MODIFIED", deleting(mine, 3)), ("MODIFIED", deleting(other, 4))]
    # a namespace outside watcher.namespaces: tracked, never notified, so never reported
    ov = merged(OV(), RV_EXTRA, {"watcher": {"namespaces": ["default"]}})
    calls, _, c, _, swept, tracked = both_scripts("production", ov, [("feed", lines(events)), ("sweep", T1_S + N),
                                                                     ("sweep", T1_S + 10 * N)])
    assert swept == [1, 0] and tracked == 2 and c["events_filtered_namespace"] == 1
    assert alert_uids(calls) == [mine["metadata"]["uid"]]
    # a pod of another shard is not even cached
    import zlib
    for index in (0, 1):
        sh = merged(OV(), RV_EXTRA, {"watcher": {"namespaces": [], "shard": {"count": 2, "index": index}}})
        calls, _, c, _, swept, tracked = both_scripts("production", sh, [("feed", lines(events)), ("sweep", T1_S + N)])
        owned = [p for p in (mine, other) if zlib.crc32(p["metadata"]["namespace"].encode()) % 2 == index]
        assert swept == [len(owned)] and tracked == len(owned) and c["events_other_shard"] == 2 * (2 - len(owned))
        assert alert_uids(calls) == sorted(p["metadata"]["uid"] for p in owned)
    # primed by initial_list: skip: nothing to report from until an event left a core
    s = settings_for("production", merged(OV(), RV_EXTRA))
    for native in (False, True):
        p, rec, _ = pipeline(s, native)
        assert relist(p, native, [deleting(mine, 3)], notify=False) == []
        assert p.cache.tracked() == 0 and p.report_overdue(T1_S + N, 0) == 0 and rec.calls == []
        feed(p, native, lines([("MODIFIED", deleting(mine, 4, finalizers=()))]))  # the alert that deletion began
        assert p.cache.tracked() == 1 and [et for _, et, *_ in rec.calls] == ["MODIFIED"]
        assert p.report_overdue(T1_S + N, 0) == 1 and rvs(rec.calls) == [("MODIFIED", 4, None), ("MODIFIED", 4, N)]


# ----------------------------------------------------------------------------- through the native notifier (test 8)

def test_through_the_native_notifier():
    from k8s_watcher_amd.ops.decode import PyDecoder
    from k8s_watcher_amd.parallel.native_notifier import NativeNotifierPool
    from k8s_watcher_amd.testing.stub_sink import StubSink
    p0, run_ = pod_life(seed=64)
    q0, run2 = pod_life(seed=65)

    async def body():
        sink = StubSink()
        await sink.start()
        s = load_settings("production", environ={}, overrides=merged(OV(), RV_EXTRA, {
            "watcher": {"decode_threads": 0}, "clusterapi": {"base_url": sink.url, "health_check_on_start": False}}))
        m = Metrics()
        pool = NativeNotifierPool(s.clusterapi, m)
        p = EventPipeline(s, PyDecoder("production"), pool, m)
        p.log_events_setting = False
        p.attach_native()
        p.handle_raw(lines([("ADDED", with_rv(p0, 1)), ("MODIFIED", deleting(run_, 2)), ("ADDED", deleting(run2, 3))]),
                     1, framed=False)
        swept = p.report_overdue(T1_S + N, 2)
        # in the same tick, the first pod's DELETED
        p.handle_raw(lines([("DELETED", deleting(run_, 4, finalizers=None))]), 3, framed=False)
        assert await pool.drain(20)
        got = sink.state.payloads()
        counters = dict(m.c)
        tracked = p.cache.tracked()
        await pool.close()
        await sink.stop()
        return swept, got, counters, tracked

    swept, got, c, tracked = run(body(), timeout=60)
    assert swept == 2 and tracked == 1 and c["events_termination_overdue"] == 2 and c.get("notify_failed", 0) == 0
    uid = run_["metadata"]["uid"]
    mine = [x for x in got if x["uid"] == uid]
    assert [(x["event_type"], "alert" in x) for x in mine] == [("MODIFIED", False), ("MODIFIED", True), ("DELETED", False)]
    alert = mine[1]
    assert alert["alert"] == {"kind": "termination_overdue", "deadline_unix": T1_S, "overdue_seconds": N}
    assert list(alert)[-3:] == ["alert", "event_timestamp", "event_type"] and alert["extra"]["resource_version"] == "2"
    assert {k: v for k, v in alert.items() if k not in ("alert", "event_timestamp")} == {
        k: v for k, v in mine[0].items() if k != "event_timestamp"}
    other = [x for x in got if x["uid"] == run2["metadata"]["uid"]]
    assert [(x["event_type"], "alert" in x) for x in other] == [("ADDED", False), ("MODIFIED", True)]


# ----------------------------------------------------------------------------- end to end (test 9)

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
        s = load_settings("production", environ={}, overrides=merged(OV(1), RV_EXTRA, {
            "clusterapi": {"base_url": sink.url}, "watcher": {"engine": engine}}))
        svc = WatcherService(s, endpoint=KubeEndpoint(server=srv.url), metrics=Metrics())
        await svc.start()
        gauge = svc.metrics.gauges["pods_terminating_tracked"]
        f = PodFactory(seed=52, namespaces=["default"])
        pod = f.running(f.new_pod())
        srv.create(pod)
        past = time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime(time.time() - 3600))
        srv.update(deleting(pod, 0, ts=past))
        t0 = time.monotonic()
        await sink.state.wait_for(2, timeout=10)  # deletion began, and the overdue alert
        waited = time.monotonic() - t0
        tracked = [gauge()]
        await asyncio.sleep(3)
        await svc.notifier.drain(5)
        after_3s = list(sink.state.payloads())
        srv.delete(pod["metadata"]["namespace"], pod["metadata"]["name"])
        await sink.state.wait_for(3, timeout=10)
        await svc.notifier.drain(5)
        got = sink.state.payloads()
        tracked.append(gauge())
        counters = dict(svc.metrics.c)
        text = svc.metrics.prometheus_text()
        svc.stop()
        await svc.shutdown()
        await sink.stop()
        await srv.stop()
        return pod, past, waited, after_3s, got, tracked, counters, text

    pod, past, waited, after_3s, got, tracked, c, text = run(body(), timeout=60)
    assert waited < 10
    assert [(x["event_type"], "alert" in x) for x in after_3s] == [("MODIFIED", False), ("MODIFIED", True)]  # exactly one
    assert [(x["event_type"], "alert" in x) for x in got] == [("MODIFIED", False), ("MODIFIED", True), ("DELETED", False)]
    assert all(x["uid"] == pod["metadata"]["uid"] for x in got)
    alert = got[1]["alert"]
    want = calendar.timegm(datetime.datetime.strptime(past, "%Y-%m-%dT%H:%M:%SZ").timetuple())
    assert alert["kind"] == "termination_overdue" and alert["deadline_unix"] == want
    assert 3600 <= alert["overdue_seconds"] <= 3600 + 15
    assert tracked == [1.0, 0.0]
    assert c["events_termination_overdue"] == 1 and c["events_terminating"] == 1
    assert "pods_terminating_tracked 0" in text


# ----------------------------------------------------------------------------- the counter and the gauge (test 10)

def test_metrics():
    from k8s_watcher_amd.metrics import COUNTERS as DECLARED
    assert "events_termination_overdue" in DECLARED and Metrics().c["events_termination_overdue"] == 0
    p0, run_ = pod_life()
    s = settings_for("production", OV())
    for native in (False, True):  # the native pipeline adds to the same counter
        p, _, m = pipeline(s, native)
        feed(p, native, lines([("ADDED", with_rv(p0, 1)), ("MODIFIED", deleting(run_, 2))]))
        assert p.report_overdue(T1_S + N, 0) == 1 and m.c["events_termination_overdue"] == 1
        text = m.prometheus_text()  # the body of /metrics
        assert [ln for ln in text.splitlines() if "events_termination_overdue" in ln and not ln.startswith("#")][0].endswith(" 1")


def test_the_driver_skips_scopes_that_are_not_ready():
    """``Reflector.check_overdue``: the scope's namespace or the whole cache;
    nothing before the first sync, during a relist or after stop()."""
    import asyncio
    from k8s_watcher_amd.engine.reflector import Reflector
    from k8s_watcher_amd.engine.scopes import ScopeSet

    class Pipe:
        native = None

        def __init__(self):
            self.seen = []

        def report_overdue(self, now_s, read_ns, scope_ns=None):
            self.seen.append((now_s, scope_ns))
            return 3

    async def body():
        s = settings_for("production", OV())
        out = []
        for ns in (None, "ns-a"):
            pipe = Pipe()
            r = Reflector(None, s, None, pipe, Metrics(), namespace=ns)
            assert r.check_overdue(100) == 0 and pipe.seen == []  # not yet synced
            r.synced.set()
            assert r.check_overdue(101) == 3 and pipe.seen == [(101, ns)]
            r._syncing = True  # in mid-relist
            assert r.check_overdue(102) == 0
            r._syncing = False
            assert r.check_overdue(103) == 3
            out.append((r, pipe))
        # the loop: every live scope, each tick, by the clock it is given; a non-leader has none
        import logging
        import k8s_watcher_amd.engine.scopes as scopes_mod
        stop = asyncio.Event()
        ss = ScopeSet(s.watcher, Metrics(), logging.getLogger("test"), stop, lambda: None, lambda: None, None, None)
        ss.reflectors = lambda: [r for r, _ in out]
        period, scopes_mod.OVERDUE_CHECK_SECONDS = scopes_mod.OVERDUE_CHECK_SECONDS, 0.001
        try:
            ticks = iter([500.9, 501.2])

            def clock():
                try:
                    return next(ticks)
                except StopIteration:
                    stop.set()
                    return 502.0
            await asyncio.wait_for(ss.overdue_loop(clock), 5)
        finally:
            scopes_mod.OVERDUE_CHECK_SECONDS = period
        assert [p.seen[2:] for _, p in out] == [[(500, None), (501, None), (502, None)],
                                                [(500, "ns-a"), (501, "ns-a"), (502, "ns-a")]]
        out[0][0].stop()
        assert out[0][0].check_overdue(104) == 0

    run(body(), timeout=10)
