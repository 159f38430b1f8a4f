"""Pods whose graceful deletion has begun through the critical filter (``watcher.alerts.terminating``).

The rule (``models/findings.py`` ``terminating`` and ``ops/csrc/findings.inc``:
``metadata`` is an object whose ``deletionTimestamp`` is a string), its 1-or-0
signature and the filter rule in both engines — the watch path (serial and
partitioned apply), the native relist, the Python reconcile — the payload
extra field ``termination`` (mask bit 8) and the counter.
"""

import collections
import json
import random
import zlib

import pytest

from k8s_watcher_amd.engine.pipeline import EventPipeline
from k8s_watcher_amd.metrics import Metrics
from k8s_watcher_amd.ops.decode import make_decoder
from k8s_watcher_amd.testing.podgen import PodFactory, event_line
from k8s_watcher_amd.utils.config import ConfigError, load_settings, parse_override
from test_pod_condition_alerts import RV_EXTRA, Recorder, alerts, escaped, lines, merged, sent_rvs, with_rv

ON = alerts(terminating=True)
ALL_ON = alerts(terminating=True, pod_conditions=True, container_failures=True)
TERM_BIT = 1 << 8
TERM_EXTRA = {"watcher": {"payload_extra_fields": ["termination"]}}
COUNTERS = ("events_received", "events_filtered_critical", "events_filtered_namespace", "events_unchanged",
            "events_other_shard", "events_container_failure", "events_pod_condition", "events_terminating", "bookmarks")
T1 = "2025-07-09T01:51:32Z"
T2 = "2025-07-09T01:51:02Z"


# ----------------------------------------------------------------------------- config (test 1)

def test_config():
    from k8s_watcher_amd.models.payload import EXTRA_NAMES, extra_mask
    for env in ("development", "staging", "production"):
        assert load_settings(env, environ={}).watcher.terminating is False
    w = load_settings("production", environ={}, overrides=ON).watcher
    assert w.terminating is True and w.critical_events_only is True
    assert w.pod_conditions is False and w.container_failures is False  # independent of the other two
    w = load_settings("staging", environ={}, overrides=parse_override("watcher.alerts.terminating=true")).watcher
    assert w.terminating is True
    for bad in ("perhaps", [True], {"on": True}):
        with pytest.raises(ConfigError, match="watcher.alerts.terminating"):
            load_settings("staging", environ={}, overrides=alerts(terminating=bad))
    assert EXTRA_NAMES.index("termination") == 8 == EXTRA_NAMES.index("pod_condition_alerts") + 1
    assert extra_mask(["termination"]) == TERM_BIT == 256
    w = load_settings("staging", environ={}, overrides=TERM_EXTRA).watcher
    assert w.payload_extra == TERM_BIT and w.terminating is False  # the field does not need the option
    with pytest.raises(ConfigError, match="watcher.payload_extra_fields"):
        load_settings("staging", environ={}, overrides={"watcher": {"payload_extra_fields": ["terminations"]}})


def test_print_config_shows_the_key(capsys):
    from k8s_watcher_amd.utils.config import dump_effective
    dump_effective(load_settings("production", environ={}))
    assert "terminating: false" in capsys.readouterr().out
    dump_effective(load_settings("production", environ={}, overrides=ON))
    assert "terminating: true" in capsys.readouterr().out


# ----------------------------------------------------------------------------- the corpus (test 2)

def md(more="", uid="@UID@", rv="7"):
    """A "metadata" member as raw JSON text, `more` spliced in untouched after the identity fields."""
    return '"metadata":{"uid":"%s","name":"p","namespace":"default","resourceVersion":"%s"%s}' % (uid, rv, more)


TS = ',"deletionTimestamp":"%s"' % T1

# (id, the raw "metadata" member(s) of the pod, the event type, terminating?)
CORPUS = [
    ("absent", md(), "MODIFIED", False),
    ("string", md(TS), "MODIFIED", True),
    ("string-with-the-rest", md(TS + ',"deletionGracePeriodSeconds":30,"finalizers":["example.com/a","example.com/b"]'),
     "MODIFIED", True),
    ("string-of-any-text", md(',"deletionTimestamp":"soon, été ✓"'), "MODIFIED", True),
    ("empty-string", md(',"deletionTimestamp":""'), "MODIFIED", True),
    ("null", md(',"deletionTimestamp":null'), "MODIFIED", False),
    ("number", md(',"deletionTimestamp":1752025892'), "MODIFIED", False),
    ("true", md(',"deletionTimestamp":true'), "MODIFIED", False),
    ("object", md(',"deletionTimestamp":{"time":"%s"}' % T1), "MODIFIED", False),
    ("array", md(',"deletionTimestamp":["%s"]' % T1), "MODIFIED", False),
    ("escaped-key", md(',"deletion\\u0054imestamp":"%s"' % T1), "MODIFIED", True),
    ("escaped-keys-of-the-rest", md(TS + ',"deletionGr\\u0061cePeriodSeconds":5,"fin\\u0061lizers":["x"]'),
     "MODIFIED", True),
    ("repeated-string-then-null", md(TS + ',"deletionTimestamp":null'), "MODIFIED", False),
    ("repeated-null-then-string", md(',"deletionTimestamp":null' + TS), "MODIFIED", True),
    ("repeated-the-rest", md(TS + ',"finalizers":["a"],"deletionGracePeriodSeconds":30,"finalizers":null,'
                             '"deletionGracePeriodSeconds":0'), "MODIFIED", True),
    # keys of the right length and other text
    ("creation-timestamp-alone", md(',"creationTimestamp":"%s"' % T1), "MODIFIED", False),
    ("17-bytes-other-key", md(',"deletionTimestamq":"%s"' % T1), "MODIFIED", False),
    ("10-bytes-not-finalizers", md(TS + ',"finalizerz":["example.com/a"]'), "MODIFIED", True),
    ("26-bytes-not-grace-period", md(TS + ',"deletionGracePeriodSecondz":30'), "MODIFIED", True),
    # the whole object
    ("metadata-array", '"metadata":["deletionTimestamp","%s"]' % T1, "MODIFIED", False),
    ("metadata-repeated-last-without", md(TS) + "," + md(), "MODIFIED", False),
    ("metadata-repeated-last-with", md() + "," + md(TS), "MODIFIED", True),
    ("metadata-repeated-last-null", md(TS) + ',"metadata":null', "MODIFIED", False),
    ("metadata-repeated-last-array", md(TS) + ',"metadata":[]', "MODIFIED", False),
    ("deleted-line-with-it", md(TS + ',"deletionGracePeriodSeconds":0'), "DELETED", True),
    ("added-line-with-it", md(TS), "ADDED", True),
]


def corpus_object(members, uid="u-corpus"):
    """The pod as JSON text around the raw metadata member(s)."""
    return ('{"kind":"Pod","apiVersion":"v1",%s,"spec":{"nodeName":"mi355x-node-01","containers":[{"name":"c",'
            '"image":"registry.example.com/team/c:v1"}]},"status":{"phase":"Running","podIP":"10.244.0.7"}}'
            % members.replace("@UID@", uid))


def corpus_line(members, etype="MODIFIED", uid="u-corpus"):
    return ('{"type":"%s","object":%s}\n' % (etype, corpus_object(members, uid))).encode()


def want_termination(pod):
    """The extra field from the decoded object, written out here again: raw values, null when absent."""
    m = pod.get("metadata")
    m = m if isinstance(m, dict) else {}
    return {"deletion_timestamp": m.get("deletionTimestamp"), "grace_period_seconds": m.get("deletionGracePeriodSeconds"),
            "finalizers": m.get("finalizers")}


@pytest.mark.parametrize("case", CORPUS, ids=[c[0] for c in CORPUS])
def test_finding_table(case):
    from k8s_watcher_amd.models.findings import terminating, terminating_signature
    _, members, _, want = case
    pod = json.loads(corpus_object(members))
    assert terminating(pod) is want and terminating_signature(pod) == int(want)


def test_finding_of_odd_pods():
    from k8s_watcher_amd.models.findings import terminating
    for pod in ({}, None, [], "x", {"metadata": None}, {"metadata": []}, {"metadata": {"deletionTimestamp": None}}):
        assert terminating(pod) is False


def settings_for(env, ov):
    return load_settings(env, overrides=merged({"watcher": {"decode_threads": 0}}, ov), environ={})


def decoder_for(s, engine="python"):
    w = s.watcher
    return make_decoder(engine, s.environment, w.state_format, w.payload_extra, w.validate,
                        w.container_failures, w.container_failure_reasons, w.pod_conditions, w.pod_condition_rules,
                        w.terminating)


def pipeline(s, native):
    rec, m = Recorder(), Metrics()
    p = EventPipeline(s, decoder_for(s), rec, m)
    p.log_events_setting = False
    if native:
        p.attach_native()
    return p, rec, m


def feed(p, native, data):
    return p.handle_raw(data, 0, framed=False) if native else p.handle_batch(p.decoder.feed(data), 0)


def run_engine(s, native, pieces):
    """Feed the pieces (bytes, one batch each); -> (calls, counters, control event types)."""
    p, rec, m = pipeline(s, native)
    ctrl = []
    for data in pieces:
        ctrl += feed(p, native, data)
    return rec.calls, {k: m.c.get(k, 0) for k in COUNTERS}, [c[0] for c in ctrl]


def both(env, ov, pieces):
    s = settings_for(env, ov)
    py = run_engine(s, False, pieces)
    nat = run_engine(s, True, pieces)
    assert py == nat
    return py


REPR_ODD_STATE = ('{"metadata":{"uid":"u-repr","name":"p","namespace":"default","resourceVersion":"3",'
                  '"deletionTimestamp":"%s","deletionGracePeriodSeconds":30,"finalizers":["example.com/a"]},'
                  '"status":{"phase":"Running","containerStatuses":[{"name":"c","ready":false,"restartCount":1,'
                  '"state":{"terminated":{"exitCode":1.5}}}]}}' % T1)


def check_corpus():
    """One verdict from both engines on the finding, the core bytes and INVALID:
    both decoders (the native one under validate payload and full) and the
    fused pipeline (the full parse and filter-first)."""
    from k8s_watcher_amd.models.findings import terminating
    from k8s_watcher_amd.models.payload import EXTRA_NAMES
    py = make_decoder("python", "staging", extra=TERM_BIT, terminating=True)
    for validate in ("payload", "full"):
        nat = make_decoder("native", "staging", extra=TERM_BIT, validate=validate, terminating=True)
        for name, members, etype, want in CORPUS:
            pod = json.loads(corpus_object(members))
            assert terminating(pod) is want, name
            line = corpus_line(members, etype)
            a, b = py.feed(line)[0], nat.feed(line)[0]
            assert a[0] == b[0] == etype, (name, validate)  # none is INVALID, in either engine
            assert len(a) == len(b) == 12 and a[9] == b[9] == 0 and a[10] == b[10] == 0, (name, validate)
            # the finding: DELETED never carries the signature
            assert a[11] == b[11] == (int(want) if etype != "DELETED" else 0), (name, validate)
            ca, cb = py.core(a), nat.core(b)
            assert ca == cb, (name, validate)  # byte-identical
            assert json.loads(cb)["extra"] == {"termination": want_termination(pod)}, (name, validate)
            assert (json.loads(cb)["extra"]["termination"]["deletion_timestamp"] is not None) >= want, name
    # the copied spans are checked like the other copied spans: a malformed one makes the line INVALID
    for bad in (',"finalizers":[tru]', ',"deletionGracePeriodSeconds":3o', TS[:-1] + '\\x"'):
        line = corpus_line(md(bad))
        with pytest.raises(ValueError):
            json.loads(line)
        assert py.feed(line)[0][0] == "INVALID", bad
        for validate in ("payload", "full"):
            nat = make_decoder("native", "staging", extra=TERM_BIT, validate=validate, terminating=True)
            assert nat.feed(line)[0][0] == "INVALID", (bad, validate)
        for native in (False, True):
            calls, _, ctrl = run_engine(settings_for("staging", merged(ON, TERM_EXTRA)), native, [line])
            assert calls == [] and ctrl == ["INVALID"], (bad, native)
    # all nine bits, a mask above 255 through every hand-off, and the eight older bits keep their meaning
    line = corpus_line(md(TS + ',"deletionGracePeriodSeconds":30,"finalizers":["example.com/a"]'))
    term = {"deletion_timestamp": T1, "grace_period_seconds": 30, "finalizers": ["example.com/a"]}
    for mask, keys in ((0b111111111, list(EXTRA_NAMES)), (0b11111111, list(EXTRA_NAMES[:8])),
                       (0b100010000, ["resource_version", "termination"])):
        cores = []
        for eng in ("python", "native"):
            d = make_decoder(eng, "staging", extra=mask)
            ev = d.feed(line)[0]
            cores.append(d.core(ev))
            extra = json.loads(cores[-1])["extra"]
            assert len(ev) == 9 and list(extra) == keys and extra.get("termination", term) == term, (eng, mask)
        names = [EXTRA_NAMES[i] for i in range(len(EXTRA_NAMES)) if mask >> i & 1]
        calls, _, _ = both("staging", {"watcher": {"payload_extra_fields": names}}, [line])
        assert cores[0] == cores[1] and [core for *_, core in calls] == [json.loads(cores[0])]
    # a pod known only from the cache has none of the three
    for eng in ("python", "native"):
        d = make_decoder(eng, "staging", extra=TERM_BIT)
        assert json.loads(d.core_from_summary("u", "default", "n", "Running"))["extra"] == {
            "termination": {"deletion_timestamp": None, "grace_period_seconds": None, "finalizers": None}}
    # state_format python_repr: the native rendering and the Python fallback (a state the native one leaves to it)
    for obj in (corpus_object(md(TS)), REPR_ODD_STATE):
        line = ('{"type":"MODIFIED","object":%s}\n' % obj).encode()
        a, b = (make_decoder(eng, "staging", "python_repr", extra=TERM_BIT, terminating=True) for eng in ("python", "native"))
        ea, eb = a.feed(line)[0], b.feed(line)[0]
        assert ea[0] == eb[0] == "MODIFIED" and ea[11] == eb[11] == 1
        assert a.core(ea) == b.core(eb) and json.loads(b.core(eb))["extra"]["termination"]["deletion_timestamp"] == T1
        ov = merged(ON, TERM_EXTRA, {"watcher": {"state_format": "python_repr"}})
        calls, c, ctrl = both("production", ov, [line])
        assert ctrl == [] and len(calls) == 1 and c["events_terminating"] == 1
        assert calls[0][4]["extra"]["termination"]["deletion_timestamp"] == T1
    # the fused pipeline: the full parse without a filter, filter-first with the critical filter
    data = b"".join(corpus_line(members, etype, uid="u%d" % n) for n, (_, members, etype, _) in enumerate(CORPUS))
    pods = [json.loads(corpus_object(members, "u%d" % n)) for n, (_, members, _, _) in enumerate(CORPUS)]
    for env, ov in (("staging", {}), ("staging", ON), ("production", alerts(critical_events_only=False))):
        calls, c, ctrl = both(env, merged(ov, TERM_EXTRA), [data])
        assert ctrl == [] and c["events_terminating"] == 0
        # (production filters namespaces: a pod whose metadata is no object has none)
        kept = [p for p in pods if env == "staging" or isinstance(p["metadata"], dict)]
        assert len(kept) in (len(pods), len(pods) - 3)
        assert [core["extra"]["termination"] for *_, core in calls] == [want_termination(p) for p in kept]
    calls, c, ctrl = both("production", merged(ON, TERM_EXTRA), [data])
    sent = [n for n, (_, _, etype, want) in enumerate(CORPUS) if want or etype == "DELETED"]
    assert ctrl == [] and [core["extra"]["termination"] for *_, core in calls] == [want_termination(pods[n]) for n in sent]
    assert [et for _, et, *_ in calls] == [CORPUS[n][2] for n in sent]
    assert c["events_terminating"] == sum(want and etype != "DELETED" for _, _, etype, want in CORPUS)
    assert c["events_filtered_critical"] == len(CORPUS) - len(sent)


def test_corpus_one_verdict_from_both_engines():
    check_corpus()


def test_both_caches_swap_terminating():
    from k8s_watcher_amd.ops.cache import make_pod_cache
    for native in (False, True):
        cache = make_pod_cache(native)
        assert cache.swap_terminating("nobody", 1) == 0 and len(cache) == 0
        cache.observe("ADDED", "u", "1", "Running", "default", "n")
        assert cache.swap_terminating("u", 0) == 0
        assert cache.swap_terminating("u", 1) == 0
        assert cache.swap_failure("u", 3) == 0 and cache.swap_condition("u", 5) == 0  # each its own field
        assert cache.swap_terminating("u", 1) == 1
        assert cache.swap_failure("u", 0) == 3 and cache.swap_condition("u", 0) == 5
        assert cache.swap_terminating("u", 0) == 1
        assert cache.get("u")[:5] == ["1", "Running", "default", "n", None]
        assert cache.to_records() == [["u", "1", "Running", "default", "n", None]]  # never persisted
        cache.swap_terminating("u", 1)
        cache.put("u", "2", "Running", "default", "n", None)  # a whole new entry
        assert cache.swap_terminating("u", 0) == 0


# ----------------------------------------------------------------------------- a pod's life (test 3)

def deleting(pod, rv, ts=T1, grace=30, finalizers=("example.com/a", "example.com/b")):
    p = with_rv(pod, rv)
    p["metadata"]["deletionTimestamp"] = ts
    p["metadata"]["deletionGracePeriodSeconds"] = grace
    if finalizers is not None:
        p["metadata"]["finalizers"] = list(finalizers)
    return p


def life(seed=61, ns="default"):
    f = PodFactory(seed=seed, namespaces=[ns])
    p0 = f.new_pod()
    run_ = f.running(p0)
    return [
        ("ADDED", with_rv(p0, 1)),
        ("MODIFIED", with_rv(run_, 2)),
        ("MODIFIED", deleting(run_, 3)),
        ("MODIFIED", deleting(run_, 4, finalizers=("example.com/a",))),  # a finalizer went
        ("MODIFIED", deleting(run_, 5, ts=T2, grace=0, finalizers=("example.com/a",))),  # a forced delete
        ("DELETED", deleting(run_, 6, ts=T2, grace=0, finalizers=None)),
    ]


def check_pod_life():
    events = life()
    assert [o["status"]["phase"] for _, o in events] == ["Pending"] + ["Running"] * 5
    for pieces in ([lines(events)], [event_line(t, o) for t, o in events]):  # one read, and one read per event
        # production, the critical filter on: when deletion begins, and the DELETED
        calls, c, ctrl = both("production", merged(ON, RV_EXTRA), pieces)
        assert ctrl == []
        assert sent_rvs(calls) == [("MODIFIED", 3), ("DELETED", 6)]
        assert c["events_terminating"] == 1 and c["events_filtered_critical"] == 4
        assert c["events_received"] == 6 and c["events_unchanged"] == 0
        assert c["events_container_failure"] == 0 and c["events_pod_condition"] == 0
        assert "termination" not in json.dumps(calls)
        # ... and the payload can say what is left to wait for
        calls, _, _ = both("production", merged(ON, TERM_EXTRA), pieces)
        assert [core["extra"]["termination"] for *_, core in calls] == [
            {"deletion_timestamp": T1, "grace_period_seconds": 30, "finalizers": ["example.com/a", "example.com/b"]},
            {"deletion_timestamp": T2, "grace_period_seconds": 0, "finalizers": None}]
        # the option off: what today's code sends
        calls, c, _ = both("production", RV_EXTRA, pieces)
        assert sent_rvs(calls) == [("DELETED", 6)]
        assert c["events_terminating"] == 0 and c["events_filtered_critical"] == 5
        # notify_on: phase_change in staging: ADDED and the phase change as today, and the one alert
        phase = merged(RV_EXTRA, {"watcher": {"notify_on": "phase_change"}})
        off, c_off, _ = both("staging", phase, pieces)
        assert sent_rvs(off) == [("ADDED", 1), ("MODIFIED", 2), ("DELETED", 6)]
        assert c_off["events_unchanged"] == 3 and c_off["events_terminating"] == 0
        on, c_on, _ = both("staging", merged(ON, phase), pieces)
        assert sent_rvs(on) == [("ADDED", 1), ("MODIFIED", 2), ("MODIFIED", 3), ("DELETED", 6)]
        assert c_on["events_unchanged"] == 2 and c_on["events_terminating"] == 1
        assert c_on["events_filtered_critical"] == 0


def test_pod_life_both_engines():
    check_pod_life()


def test_option_off_is_today():
    """With the option off tuples, payloads and counters are what they were;
    with it on the two older slots are there and 0."""
    s = settings_for("production", {})
    py = run_engine(s, False, [lines(life())])
    assert py == run_engine(s, True, [lines(life())])
    calls, c, _ = py
    assert [et for _, et, *_ in calls] == ["DELETED"] and "extra" not in calls[0][4]
    assert c["events_terminating"] == 0 and c["events_filtered_critical"] == 5
    for eng in ("python", "native"):
        assert all(len(e) == 9 for e in decoder_for(s, eng).feed(lines(life())))
        assert all(len(e) == 10 for e in decoder_for(settings_for("production", alerts(container_failures=True)), eng)
                   .feed(lines(life())))
        assert all(len(e) == 11 for e in decoder_for(settings_for("production", alerts(pod_conditions=True)), eng)
                   .feed(lines(life())))
        ev = decoder_for(settings_for("production", ON), eng).feed(lines(life()))
        assert all(len(e) == 12 and e[9] == 0 and e[10] == 0 for e in ev)
        assert [e[11] for e in ev] == [0, 0, 1, 1, 1, 0]


def test_the_timestamp_going_away_is_silent_and_a_new_deletion_alerts_again():
    f = PodFactory(seed=62, namespaces=["default"])
    run_ = f.running(f.new_pod())
    events = [("ADDED", with_rv(run_, 1)), ("MODIFIED", deleting(run_, 2)), ("MODIFIED", with_rv(run_, 3)),
              ("MODIFIED", deleting(run_, 4)), ("MODIFIED", deleting(run_, 5, ts=T2))]
    calls, c, _ = both("production", merged(ON, RV_EXTRA), [lines(events)])
    assert sent_rvs(calls) == [("MODIFIED", 2), ("MODIFIED", 4)]
    assert c["events_terminating"] == 2 and c["events_filtered_critical"] == 3


def test_native_decoder_through_handle_batch_over_the_native_cache():
    """What the native engine's WatchList path and reconcile run on: the native
    decoder's tuples through handle_batch, the signature in the native cache."""
    from k8s_watcher_amd.ops.cache import make_pod_cache
    s = settings_for("production", merged(ON, RV_EXTRA))
    want = run_engine(s, False, [lines(life())])
    rec, m = Recorder(), Metrics()
    dec = decoder_for(s, "native")
    p = EventPipeline(s, dec, rec, m, make_pod_cache(True))
    p.log_events_setting = False
    assert p.handle_batch(dec.feed(lines(life())), 0) == []
    assert (rec.calls, {k: m.c.get(k, 0) for k in COUNTERS}) == want[:2]


# ----------------------------------------------------------------------------- seen first while terminating (test 4)

def test_seen_first_while_terminating():
    f = PodFactory(seed=63, namespaces=["default"])
    run_ = f.running(f.new_pod())
    events = [("ADDED", deleting(run_, 1)), ("MODIFIED", deleting(run_, 2, finalizers=()))]
    for pieces in ([lines(events)], [event_line(t, o) for t, o in events]):
        calls, c, ctrl = both("production", merged(ON, RV_EXTRA), pieces)
        assert ctrl == [] and sent_rvs(calls) == [("ADDED", 1)]
        assert c["events_terminating"] == 1 and c["events_filtered_critical"] == 1
    calls, c, _ = both("production", RV_EXTRA, [lines(events)])
    assert calls == [] and c["events_terminating"] == 0 and c["events_filtered_critical"] == 2


# ----------------------------------------------------------------------------- partitioned apply (test 5)

PARTITIONS = 16
NAMESPACES = ["default", "kube-system", "production", "batch", "monitoring"]
SHARDS = 2


def shard_of(ns):
    return zlib.crc32(ns.encode()) % SHARDS


def terminating_batch(seed=7):
    """One batch, every pod's lines interleaved with the others': the fewest
    pods (64 at least) that put a pod with five or six lines into every one of
    the 16 partitions. Every other pod becomes terminating in this batch, the
    one that added it: deletion begins, a finalizer goes, the delete is forced,
    DELETED; every sixth is first seen terminating; the others move on without."""
    from k8s_watcher_amd.ops.native import load
    part = load().apply_partition
    rng = random.Random(seed)
    f = PodFactory(seed=seed, namespaces=NAMESPACES)
    scripts, long_parts = [], set()
    while len(scripts) < 64 or len(long_parts) < PARTITIONS:
        p0 = f.new_pod()
        run_ = f.running(p0)
        k = len(scripts) % 6
        if k in (0, 2, 4):
            steps = [("ADDED", lambda rv, p=p0: with_rv(p, rv)),
                     ("MODIFIED", lambda rv, p=run_: with_rv(p, rv)),
                     ("MODIFIED", lambda rv, p=run_: deleting(p, rv)),
                     ("MODIFIED", lambda rv, p=run_: deleting(p, rv, finalizers=("example.com/a",))),
                     ("MODIFIED", lambda rv, p=run_: deleting(p, rv, ts=T2, grace=0, finalizers=())),
                     ("DELETED", lambda rv, p=run_: deleting(p, rv, ts=T2, grace=0, finalizers=None))]
        elif k == 1:
            steps = [("ADDED", lambda rv, p=run_: deleting(p, rv)),
                     ("MODIFIED", lambda rv, p=run_: deleting(p, rv, finalizers=())),
                     ("MODIFIED", lambda rv, p=run_: with_rv(p, rv)),  # the timestamp went: nothing
                     ("MODIFIED", lambda rv, p=run_: deleting(p, rv, ts=T2)),  # ... and deletion began again
                     ("MODIFIED", lambda rv, p=run_: deleting(p, rv, ts=T2, grace=0)),
                     ("DELETED", lambda rv, p=run_: deleting(p, rv, ts=T2, grace=0))]
        else:
            steps = [("ADDED", lambda rv, p=p0: with_rv(p, rv)),
                     ("MODIFIED", lambda rv, p=run_: with_rv(p, rv)),
                     ("MODIFIED", lambda rv, p=run_: with_rv(p, rv)),
                     ("MODIFIED", lambda rv, p=run_: with_rv(p, rv)),
                     ("MODIFIED", lambda rv, p=run_: with_rv(p, rv)),
                     ("DELETED", lambda rv, p=run_: with_rv(p, rv))]
        steps = steps[:rng.choice((4, 5, 6))]
        if len(steps) >= 5:
            long_parts.add(part(p0["metadata"]["uid"]))
        scripts.append((p0["metadata"]["namespace"], steps))
    out, rv = [], 0
    for k in range(6):
        for _, steps in scripts:
            if k < len(steps):
                rv += 1
                et, make = steps[k]
                out.append(event_line(et, make(rv)))
    return b"".join(out), [ns for ns, _ in scripts], len(out)


def warm_up():
    f = PodFactory(seed=8, namespaces=NAMESPACES)
    out = []
    for ns in f.namespaces:
        p0 = f.new_pod(namespace=ns)
        out += [("ADDED", with_rv(p0, 1)), ("MODIFIED", with_rv(f.running(p0), 2))]
    return lines(out)


def feed_one_batch(env, ov, warm, data, partitioned):
    """`data` as one batch through the native pipeline and the native notifier,
    after `warm` (too few lines to be partitioned) taught the cache the
    namespaces and phases; -> what the sink got, the cache with each pod's
    terminating signature, the counters, the resume point, the control events
    and the apply's probe."""
    from conftest import run
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
        assert await pool.drain(20)
        got = [(x["uid"], x["event_type"], json.dumps(x, sort_keys=True)) for x in
               ({k: v for k, v in sent.items() if k != "event_timestamp"} for sent in sink.state.payloads())]
        cache = {u: [e[0], e[1], e[2], e[3], json.loads(e[4]) if e[4] else None] for u, e in p.cache.items()}
        for u, e in cache.items():  # read last: the swap writes what it read back
            sig = p.cache.swap_terminating(u, 0)
            p.cache.swap_terminating(u, sig)
            e.append(sig)
        counters = {k: v for k, v in m.c.items() if k.startswith(("events_", "bookmarks"))}
        rv = p.native.last_rv()
        await pool.close()
        await sink.stop()
        dpool.close()
        return got, cache, counters, rv, ctrl, probe

    return run(body(), timeout=60)


def check_partitioned_matches_serial():
    from test_partitioned_apply import per_uid
    data, pod_ns, n = terminating_batch()
    warm = warm_up()
    n_pods = len(pod_ns)
    assert 64 <= n_pods <= 160 and 4 * n_pods <= n <= 6 * n_pods
    # production filters namespaces; the sharded run owns some of the namespaces and not others
    assert {shard_of(ns) for ns in NAMESPACES} == {0, 1} and "batch" in pod_ns
    mine = [ns for ns in NAMESPACES if shard_of(ns) == 0]
    assert len(mine) >= 2  # one of this shard's namespaces is filtered, another is not
    sharded = merged(ON, TERM_EXTRA, {"watcher": {"notify_on": "phase_change", "shard": {"count": SHARDS, "index": 0},
                                                  "namespaces": [ns for ns in NAMESPACES if ns != mine[0]]}})
    for env, ov in (("production", merged(ON, TERM_EXTRA)), ("staging", sharded), ("production", ALL_ON)):
        s_got, s_cache, s_cnt, s_rv, s_ctrl, s_probe = feed_one_batch(env, ov, warm, data, partitioned=False)
        p_got, p_cache, p_cnt, p_rv, p_ctrl, p_probe = feed_one_batch(env, ov, warm, data, partitioned=True)
        assert s_probe.get("partitioned_batches", 0) == 0
        # one partitioned batch, every line of it applied by its partition
        assert p_probe["partitioned_batches"] == 1 and p_probe["lines"] == n and p_probe["tail_serial_lines"] == 0
        assert collections.Counter(p_got) == collections.Counter(s_got)  # the bodies, byte for byte but the time
        assert per_uid(p_got) == per_uid(s_got)  # per pod in stream order
        assert p_cache == s_cache and p_cnt == s_cnt and p_rv == s_rv and p_ctrl == s_ctrl == []
        assert any(e[5] == 1 for e in s_cache.values()) and any(e[5] == 0 for e in s_cache.values())
        assert s_cnt["events_terminating"] >= n_pods // 8
        assert s_cnt["events_filtered_namespace"] > 0
        if env == "staging":
            assert s_cnt["events_other_shard"] > 0 and s_cnt["events_unchanged"] > 0
        # and the serial native apply is the Python engine's verdict
        calls, c, _ = run_engine(settings_for(env, ov), False, [warm, data])
        assert per_uid([(u, et, json.dumps(core, sort_keys=True)) for u, et, _, _, core in calls]) == per_uid(
            [(u, et, json.dumps({k: v for k, v in json.loads(b).items() if k != "event_type"}, sort_keys=True))
             for u, et, b in s_got])
        assert {k: v for k, v in s_cnt.items() if k in COUNTERS and v} == {k: v for k, v in c.items() if v}


def test_partitioned_apply_matches_serial_with_terminating():
    check_partitioned_matches_serial()


# ----------------------------------------------------------------------------- relist (test 6)

def check_relist(native):
    from test_native_relist import list_pages, native_relist
    f = PodFactory(seed=71, namespaces=["default"])
    a, b, c_, d = (f.running(f.new_pod()) for _ in range(4))
    uid = lambda p: p["metadata"]["uid"]  # noqa: E731
    s = settings_for("production", merged(ON, RV_EXTRA))
    p, rec, m = pipeline(s, native)
    watch = lines([("ADDED", with_rv(a, 1)), ("ADDED", deleting(b, 2)), ("ADDED", with_rv(c_, 3)), ("ADDED", with_rv(d, 4))])
    feed(p, native, watch)
    assert [(u, et) for u, et, *_ in rec.calls] == [(uid(b), "ADDED")]
    del rec.calls[:]
    # the gap (a 410): a's deletion began, b is terminating as before with one finalizer less, c is gone,
    # d only moved on
    listed = [deleting(a, 10), deleting(b, 11, finalizers=("example.com/a",)), with_rv(d, 12)]
    if native:
        ctrl, stats = native_relist(p, listed, None)
        assert stats["modified"] == 3 and stats["deleted"] == 1
    else:
        _, _, evs = p.decoder.decode_list(list_pages(listed, 10 ** 6)[0])
        assert all(len(e) == 12 for e in evs) and [e[11] for e in evs] == [1, 1, 0]
        ctrl = p.reconcile(evs, 0)
    assert ctrl == []
    # one alert, no repeat, one synthesised DELETED
    assert sorted((u, et) for u, et, *_ in rec.calls) == sorted([(uid(a), "MODIFIED"), (uid(c_), "DELETED")])
    assert m.c["events_terminating"] == 2 and m.c["events_filtered_critical"] == 5
    assert [core["extra"]["resource_version"] for u, et, _, _, core in rec.calls if et == "MODIFIED"] == ["10"]
    # a silent relist (initial_list: skip) leaves no signature: the pod is reported at its next event
    q, rec2, _ = pipeline(s, native)
    if native:
        native_relist(q, listed, None, notify=False)
    else:
        q.reconcile(q.decoder.decode_list(list_pages(listed, 10 ** 6)[0])[2], 0, notify=False)
    assert rec2.calls == [] and len(q.cache) == 3
    feed(q, native, lines([("MODIFIED", deleting(b, 20, finalizers=()))]))
    assert [(u, et) for u, et, *_ in rec2.calls] == [(uid(b), "MODIFIED")]


@pytest.mark.parametrize("native", [True, False], ids=["native-relist", "python-reconcile"])
def test_relist(native):
    check_relist(native)


# ----------------------------------------------------------------------------- all three options on (test 7)

def test_all_three_options_on():
    from test_container_failures import CLB, UP, died, set_status
    from test_pod_condition_alerts import disrupted
    f = PodFactory(seed=81, namespaces=["default"])
    run_ = f.running(f.new_pod())
    crash = set_status(run_, 0, CLB, 1, died(1, "Error"))
    crash2 = set_status(run_, 0, CLB, 2, died(1, "Error"))
    events = [("ADDED", set_status(run_, 1, UP)),
              ("MODIFIED", deleting(disrupted(crash, 0), 2)),    # new on all three sides: sent once, counted in each
              ("MODIFIED", deleting(disrupted(crash, 0), 3)),    # none is new
              ("MODIFIED", deleting(disrupted(crash2, 0), 4)),   # only the container findings changed
              ("MODIFIED", disrupted(crash2, 5)),                # the timestamp went: nothing
              ("MODIFIED", deleting(disrupted(crash2, 0), 6)),   # ... and came back: only that signature is new
              ("MODIFIED", deleting(with_rv(crash2, 0), 7)),     # the condition went: nothing
              ("MODIFIED", deleting(disrupted(crash2, 0), 8))]   # ... and came back: only the condition signature
    for pieces in ([lines(events)], [event_line(t, o) for t, o in events]):
        calls, c, _ = both("production", merged(ALL_ON, RV_EXTRA), pieces)
        assert sent_rvs(calls) == [("MODIFIED", 2), ("MODIFIED", 4), ("MODIFIED", 6), ("MODIFIED", 8)]
        assert c["events_container_failure"] == 2 and c["events_pod_condition"] == 2 and c["events_terminating"] == 2
        assert c["events_filtered_critical"] == 4
    # each option alone sees its own side only
    calls, c, _ = both("production", merged(ON, RV_EXTRA), [lines(events)])
    assert sent_rvs(calls) == [("MODIFIED", 2), ("MODIFIED", 6)]
    assert (c["events_container_failure"], c["events_pod_condition"], c["events_terminating"]) == (0, 0, 2)
    calls, c, _ = both("production", merged(alerts(pod_conditions=True), RV_EXTRA), [lines(events)])
    assert sent_rvs(calls) == [("MODIFIED", 2), ("MODIFIED", 8)]
    assert (c["events_container_failure"], c["events_pod_condition"], c["events_terminating"]) == (0, 2, 0)
    calls, c, _ = both("production", merged(alerts(container_failures=True), RV_EXTRA), [lines(events)])
    assert sent_rvs(calls) == [("MODIFIED", 2), ("MODIFIED", 4)]
    assert (c["events_container_failure"], c["events_pod_condition"], c["events_terminating"]) == (2, 0, 0)
    # two of the three: an event new on those two sides is counted in both, and not in the third
    calls, c, _ = both("production", merged(alerts(terminating=True, container_failures=True), RV_EXTRA), [lines(events)])
    assert sent_rvs(calls) == [("MODIFIED", 2), ("MODIFIED", 4), ("MODIFIED", 6)]
    assert (c["events_container_failure"], c["events_pod_condition"], c["events_terminating"]) == (2, 0, 2)


# ----------------------------------------------------------------------------- seeded mutation fuzz (test 8)

KEYS = ("deletionTimestamp", "deletionGracePeriodSeconds", "finalizers")
# spelled as json.dumps spells them, so that a copied value is the same bytes in both engines
VALUES = {
    "deletionTimestamp": ['"%s"' % T1, '"%s"' % T2, '""', '"not a time"', '"été ✓"'],
    "deletionGracePeriodSeconds": ["30", "0", "-1", "3600"],
    "finalizers": ['["example.com/a"]', '["example.com/a","kubernetes"]', "[]"],
}
RETYPED = ["null", "true", "false", "0", "-15", "[]", "{}", '["%s"]' % T1, '{"deletionTimestamp":"%s"}' % T1, '"x"']
NEAR_KEYS = ["creationTimestamp", "deletionTimestamq", "finalizerz", "deletionGracePeriodSecondz", "deletiontimestamp",
             "deletionTimestamps"]
BLANKS = ["", "", "", " ", "\t", "  ", "\r"]


def mutated_metadata(rng, uid, rv):
    """A metadata object as raw JSON text, the three keys mutated in type,
    order, repetition, escaping and whitespace; all of it valid JSON."""
    pairs = [["uid", '"%s"' % uid], ["name", '"p-%s"' % uid], ["namespace", '"default"'], ["resourceVersion", '"%d"' % rv],
             ["creationTimestamp", '"%s"' % T1]]
    for k in KEYS:
        if rng.random() < (0.6 if k == "deletionTimestamp" else 0.5):
            pairs.append([k, rng.choice(VALUES[k])])
    for _ in range(rng.randrange(5)):
        k = rng.choice(KEYS)
        m = rng.randrange(7)
        if m == 0:    # drop the field
            pairs = [p for p in pairs if p[0] != k]
        elif m == 1:  # repeat it, the last value another one of its type
            pairs.append([k, rng.choice(VALUES[k])])
        elif m == 2:  # repeat it, the last value of another type
            pairs.append([k, rng.choice(RETYPED)])
        elif m == 3:  # retype it where it stands
            pairs = [[a, rng.choice(RETYPED)] if a == k else [a, b] for a, b in pairs]
        elif m == 4:  # escape characters of its key
            pairs = [[escaped(rng, a)[1:-1], b] if a == k else [a, b] for a, b in pairs]
        elif m == 5:  # a key that only looks like it
            pairs.append([rng.choice(NEAR_KEYS), rng.choice(VALUES[k] + RETYPED)])
        else:         # reorder the fields
            rng.shuffle(pairs)
    ws = lambda: rng.choice(BLANKS)  # noqa: E731
    body = ",".join('%s"%s"%s:%s%s%s' % (ws(), a, ws(), ws(), b, ws()) for a, b in pairs)
    text = "{%s}" % body
    r = rng.random()
    if r < 0.03:   # metadata of another type
        return rng.choice(RETYPED)
    if r < 0.08:   # metadata repeated: this one is the last
        return '{"deletionTimestamp":"%s"},"metadata":%s' % (T1, text)
    return text


def fuzz_lines(n=2000, seed=11):
    rng = random.Random(seed)
    out = []
    for i in range(n):
        etype = "MODIFIED" if rng.random() < 0.9 else rng.choice(("ADDED", "DELETED"))
        out.append(corpus_line('"metadata":%s' % mutated_metadata(rng, "u%d" % i, i + 1), etype))
    return out


def test_seeded_mutation_fuzz():
    from k8s_watcher_amd.models.findings import terminating
    data = fuzz_lines()
    assert len(data) == 2000
    py = make_decoder("python", "staging", extra=TERM_BIT, terminating=True)
    a = [py.feed(ln)[0] for ln in data]
    # the condition: the Python engine alone decodes them as pod events, and both verdicts are well represented
    decoded = [(ln, e) for ln, e in zip(data, a) if e[0] in ("ADDED", "MODIFIED", "DELETED")]
    live = [e for _, e in decoded if e[0] != "DELETED"]
    assert len(decoded) >= 1000, len(decoded)
    assert sum(e[11] == 1 for e in live) >= 300 and sum(e[11] == 0 for e in live) >= 300
    for ln, e in decoded:
        pod = json.loads(ln)["object"]
        assert e[11] == (int(terminating(pod)) if e[0] != "DELETED" else 0), ln
        assert json.loads(py.core(e))["extra"]["termination"] == want_termination(pod), ln
    for validate in ("payload", "full"):
        nat = make_decoder("native", "staging", extra=TERM_BIT, validate=validate, terminating=True)
        for ln, ea in zip(data, a):
            eb = nat.feed(ln)[0]
            assert ea[0] == eb[0], ln  # INVALID included
            if ea[0] == "INVALID":
                continue
            assert len(eb) == 12 and ea[11] == eb[11], ln
            assert py.core(ea) == nat.core(eb), ln  # byte-identical
    # the same lines through the fused pipelines: one sequence of notifications and counters
    for env in ("production", "staging"):
        calls, c, ctrl = both(env, merged(ON, TERM_EXTRA), [b"".join(data)])
        assert ctrl == [t for t in (e[0] for e in a) if t == "INVALID"] and c["events_received"] == len(decoded)
    assert c["events_terminating"] == 0 and len(calls) == len(decoded)  # staging: nothing is filtered to begin with
    # under the critical filter (every pod is Running), against the rule written out again here: an
    # event is an alert when it is terminating and the pod's last event was not
    calls, c, _ = both("production", merged(ON, TERM_EXTRA, {"watcher": {"namespaces": []}}), [b"".join(data)])
    state, alerts_, deleted = {}, 0, 0
    for _, e in decoded:
        if e[0] == "DELETED":
            state.pop(e[1], None)
            deleted += 1
        else:
            alerts_ += e[11] == 1 and state.get(e[1], 0) == 0
            state[e[1]] = e[11]
    assert alerts_ >= 300 and c["events_terminating"] == alerts_ == len(calls) - deleted


# ----------------------------------------------------------------------------- the counter (test 9)

def test_metric_is_declared_and_exported():
    from k8s_watcher_amd.metrics import COUNTERS as DECLARED
    assert "events_terminating" in DECLARED and Metrics().c["events_terminating"] == 0
    m = Metrics()
    s = settings_for("production", ON)
    p = EventPipeline(s, decoder_for(s), Recorder(), m)
    p.log_events_setting = False
    p.handle_batch(p.decoder.feed(lines(life())), 0)
    text = m.prometheus_text()  # the body of /metrics
    assert [ln for ln in text.splitlines() if "events_terminating" in ln and not ln.startswith("#")][0].endswith(" 1")
    # the native pipeline adds to the same counter
    m2 = Metrics()
    p = EventPipeline(s, decoder_for(s), Recorder(), m2)
    p.log_events_setting = False
    p.attach_native()
    p.handle_raw(lines(life()), 0, framed=False)
    assert m2.c["events_terminating"] == 1
