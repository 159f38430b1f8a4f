"""Container failures through the critical filter (``watcher.alerts.container_failures``).

The findings (``models/findings.py`` and ``ops/csrc/findings.inc``: one verdict
on every pod), the failure signature and the filter rule in both engines — the
watch path (serial and partitioned apply), the native relist, the Python
reconcile — the payload extra field ``container_failures``, the configuration
keys, and one run end to end against the fake API server.
"""

import collections
import copy
import json

import pytest
from hypothesis import HealthCheck, given
from hypothesis import settings as hyp_settings
from hypothesis import strategies as st

from conftest import run
from k8s_watcher_amd.engine.pipeline import EventPipeline
from k8s_watcher_amd.metrics import Metrics
from k8s_watcher_amd.ops.decode import make_decoder
from k8s_watcher_amd.testing.podgen import PodFactory, event_line
from k8s_watcher_amd.utils.config import ConfigError, load_settings, parse_override

ON = {"watcher": {"alerts": {"container_failures": True}}}
FAILURES_BIT = 0b1000000


def merged(*dicts):
    out = {}
    for d in dicts:
        for k, v in d.items():
            out[k] = merged(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else copy.deepcopy(v)
    return out


# ----------------------------------------------------------------------------- the corpus (tests 1 and 6)

def fnd(container, kind, reason=None, exit_code=None, restart_count=None, init=False):
    return {"container": container, "init": init, "kind": kind, "reason": reason, "exit_code": exit_code,
            "restart_count": restart_count}


def cs(name='"app"', rc="0", state="{}", last="{}"):
    """One containerStatuses element as raw JSON text (the values are raw tokens)."""
    return '{"name":%s,"ready":false,"restartCount":%s,"state":%s,"lastState":%s,"image":"i"}' % (name, rc, state, last)


WAIT_CLB = '{"waiting":{"reason":"CrashLoopBackOff","message":"back-off 10s"}}'
TERM = '{"terminated":{"exitCode":%s,"reason":%s}}'
RUNNING = '{"running":{"startedAt":"2025-07-09T01:51:32Z"}}'

# (id, raw initContainerStatuses or None, raw containerStatuses or None, expected findings)
CORPUS = [
    ("healthy", None, "[%s]" % cs(state=RUNNING), []),
    ("waiting", None, "[%s]" % cs(state=WAIT_CLB), [fnd("app", "waiting", "CrashLoopBackOff", None, 0)]),
    ("terminated", None, "[%s]" % cs(state=TERM % (2, '"Error"')), [fnd("app", "terminated", "Error", 2, 0)]),
    ("terminated-negative", None, "[%s]" % cs(state=TERM % (-3, "null")), [fnd("app", "terminated", None, -3, 0)]),
    ("restarted", None, "[%s]" % cs(rc="3", state=RUNNING, last=TERM % (137, '"OOMKilled"')),
     [fnd("app", "restarted", "OOMKilled", 137, 3)]),
    ("waiting+restarted", None, "[%s]" % cs(rc="1", state=WAIT_CLB, last=TERM % (1, '"Error"')),
     [fnd("app", "waiting", "CrashLoopBackOff", None, 1), fnd("app", "restarted", "Error", 1, 1)]),
    ("init", "[%s]" % cs(name='"setup"', state='{"waiting":{"reason":"ImagePullBackOff"}}'),
     "[%s]" % cs(state='{"waiting":{"reason":"PodInitializing"}}'),
     [fnd("setup", "waiting", "ImagePullBackOff", None, 0, init=True)]),
    ("init-then-main", "[%s]" % cs(name='"setup"', rc="2", state=RUNNING, last=TERM % (1, '"Error"')),
     "[%s,%s]" % (cs(state=RUNNING), cs(name='"side"', state='{"waiting":{"reason":"ErrImagePull"}}')),
     [fnd("setup", "restarted", "Error", 1, 2, init=True), fnd("side", "waiting", "ErrImagePull", None, 0)]),
    ("reason-outside-set", None, "[%s]" % cs(state='{"waiting":{"reason":"ContainerCreating"}}'), []),
    ("waiting-outside-set-and-terminated", None,
     "[%s]" % cs(state='{"waiting":{"reason":"Other"},"terminated":{"exitCode":1}}'),
     [fnd("app", "terminated", None, 1, 0)]),
    ("waiting-wins-over-terminated", None,
     "[%s]" % cs(state='{"terminated":{"exitCode":1},"waiting":{"reason":"RunContainerError"}}'),
     [fnd("app", "waiting", "RunContainerError", None, 0)]),
    ("exit-0", None, "[%s]" % cs(rc="1", state=TERM % (0, '"Completed"'), last=TERM % (0, '"Completed"')), []),
    ("exit-minus-0", None, "[%s]" % cs(rc="1", state=TERM % ("-0", "null"), last=TERM % ("-0", "null")), []),
    ("exit-true", None, "[%s]" % cs(rc="1", state=TERM % ("true", "null"), last=TERM % ("true", "null")), []),
    ("exit-float", None, "[%s]" % cs(rc="1", state=TERM % ("1.0", "null"), last=TERM % ("1.0", "null")), []),
    ("exit-exponent", None, "[%s]" % cs(rc="1", state=TERM % ("1e2", "null"), last=TERM % ("1e2", "null")), []),
    ("exit-string", None, "[%s]" % cs(rc="1", state=TERM % ('"1"', "null"), last=TERM % ('"1"', "null")), []),
    ("exit-null", None, "[%s]" % cs(rc="1", state=TERM % ("null", "null"), last=TERM % ("null", "null")), []),
    ("restart-count-true", None, "[%s]" % cs(rc="true", state=RUNNING, last=TERM % (1, "null")), []),
    ("restart-count-float", None, "[%s]" % cs(rc="1.0", state=RUNNING, last=TERM % (1, "null")), []),
    ("restart-count-string", None, "[%s]" % cs(rc='"2"', state=RUNNING, last=TERM % (1, "null")), []),
    ("restart-count-negative", None, "[%s]" % cs(rc="-1", state=RUNNING, last=TERM % (1, "null")), []),
    ("restart-count-0", None, "[%s]" % cs(rc="0", state=RUNNING, last=TERM % (1, "null")), []),
    ("restart-count-wrong-type-in-finding", None, "[%s]" % cs(rc="1.5", state=WAIT_CLB),
     [fnd("app", "waiting", "CrashLoopBackOff", None, None)]),
    ("restart-count-minus-0-in-finding", None, "[%s]" % cs(rc="-0", state=WAIT_CLB),
     [fnd("app", "waiting", "CrashLoopBackOff", None, 0)]),
    ("reason-number", None, "[%s]" % cs(state='{"waiting":{"reason":5}}'), []),
    ("reason-of-terminated-not-a-string", None, "[%s]" % cs(state=TERM % (1, "[1]")),
     [fnd("app", "terminated", None, 1, 0)]),
    ("state-string", None, "[%s]" % cs(state='"CrashLoopBackOff"'), []),
    ("state-array", None, "[%s]" % cs(state="[%s]" % WAIT_CLB), []),
    ("waiting-array", None, "[%s]" % cs(state='{"waiting":["CrashLoopBackOff"]}'), []),
    ("terminated-string", None, "[%s]" % cs(state='{"terminated":"1"}'), []),
    ("last-state-array", None, "[%s]" % cs(rc="2", state=RUNNING, last="[%s]" % (TERM % (1, "null"))), []),
    ("name-number", None, "[%s]" % cs(name="7", state=WAIT_CLB), [fnd(None, "waiting", "CrashLoopBackOff", None, 0)]),
    ("elements-not-objects", None, '["x",null,[%s],7,%s]' % (cs(state=WAIT_CLB), cs(name='"b"', state=WAIT_CLB)),
     [fnd("b", "waiting", "CrashLoopBackOff", None, 0)]),
    ("statuses-object", '{"a":%s}' % cs(state=WAIT_CLB), '{"a":%s}' % cs(state=WAIT_CLB), []),
    ("statuses-string-and-null", '"x"', "null", []),
    ("duplicate-state-last-healthy", None,
     '[{"name":"app","restartCount":0,"state":%s,"state":%s}]' % (WAIT_CLB, RUNNING), []),
    ("duplicate-state-last-failing", None,
     '[{"name":"app","restartCount":0,"state":%s,"state":%s}]' % (RUNNING, WAIT_CLB),
     [fnd("app", "waiting", "CrashLoopBackOff", None, 0)]),
    ("duplicate-reason", None, "[%s]" % cs(state='{"waiting":{"reason":"CrashLoopBackOff","reason":"Fine"}}'), []),
    ("duplicate-restart-count", None,
     '[{"name":"app","restartCount":0,"restartCount":4,"state":%s,"lastState":%s}]' % (RUNNING, TERM % (9, "null")),
     [fnd("app", "restarted", None, 9, 4)]),
    ("escaped-reason", None, "[%s]" % cs(state='{"waiting":{"reason":"Crash\\u004coopBack\\u004Fff"}}'),
     [fnd("app", "waiting", "CrashLoopBackOff", None, 0)]),
    ("escaped-keys", None,
     '[{"n\\u0061me":"app","restartCount":0,"st\\u0061te":{"w\\u0061iting":{"re\\u0061son":"ErrImagePull"}}}]',
     [fnd("app", "waiting", "ErrImagePull", None, 0)]),
    ("no-arrays", None, None, []),
]


def corpus_pod(init_raw, cs_raw, uid="u-corpus", rv="7", phase="Running"):
    """The pod as JSON text, the raw status arrays spliced in untouched."""
    f = PodFactory(seed=3, namespaces=["default"])
    pod = f.running(f.new_pod())
    pod["metadata"].update(uid=uid, resourceVersion=rv)
    st_ = pod["status"]
    st_["phase"] = phase
    st_.pop("containerStatuses", None)
    if cs_raw is not None:
        st_["containerStatuses"] = "@CS@"
    if init_raw is not None:
        st_["initContainerStatuses"] = "@INIT@"
    text = json.dumps(pod, separators=(",", ":"), ensure_ascii=False)
    return text.replace('"@CS@"', cs_raw or "").replace('"@INIT@"', init_raw or "")


def corpus_line(init_raw, cs_raw, etype="MODIFIED", **kw):
    return ('{"type":"%s","object":%s}\n' % (etype, corpus_pod(init_raw, cs_raw, **kw))).encode()


@pytest.mark.parametrize("case", CORPUS, ids=[c[0] for c in CORPUS])
def test_findings_table(case):
    from k8s_watcher_amd.models.findings import container_findings, failure_signature
    _, init_raw, cs_raw, want = case
    pod = json.loads(corpus_pod(init_raw, cs_raw))
    got = container_findings(pod)
    assert got == want
    assert all(type(f["exit_code"]) in (int, type(None)) and type(f["restart_count"]) in (int, type(None))
               for f in got)
    assert (failure_signature(got) == 0) == (not want)


def test_findings_odd_pods_and_custom_reasons():
    from k8s_watcher_amd.models.findings import container_findings
    for pod in ({}, {"status": None}, {"status": []}, {"status": {"containerStatuses": None}}):
        assert container_findings(pod) == []
    pod = json.loads(corpus_pod(None, "[%s]" % cs(state='{"waiting":{"reason":"ContainerCreating"}}')))
    assert container_findings(pod, ["ContainerCreating"]) == [fnd("app", "waiting", "ContainerCreating", None, 0)]
    pod = json.loads(corpus_pod(None, "[%s]" % cs(state=WAIT_CLB)))
    assert container_findings(pod, ["ContainerCreating"]) == []
    # ephemeral containers are not looked at
    pod["status"]["ephemeralContainerStatuses"] = pod["status"]["containerStatuses"]
    pod["status"]["containerStatuses"] = []
    assert container_findings(pod) == []


# ----------------------------------------------------------------------------- both engines over one stream

class Recorder:
    def __init__(self):
        self.calls = []

    def submit(self, uid, et, ns, name, core, read_ns, ts):
        self.calls.append((uid, et, ns, name, json.loads(core)))

    def flush(self):
        pass


COUNTERS = ("events_received", "events_filtered_critical", "events_filtered_namespace", "events_unchanged",
            "events_other_shard", "events_container_failure", "bookmarks")


def settings_for(env, ov):
    return load_settings(env, overrides=merged({"watcher": {"decode_threads": 0}}, ov), environ={})


def decoder_for(s, engine="python"):
    w = s.watcher
    kw = {}
    if getattr(w, "container_failures", False):  # (the option-off guard also runs where the option does not exist)
        kw = {"failures": True, "failure_reasons": w.container_failure_reasons}
    return make_decoder(engine, s.environment, w.state_format, w.payload_extra, w.validate, **kw)


def pipeline(s, native):
    rec, m = Recorder(), Metrics()
    p = EventPipeline(s, decoder_for(s), rec, m)
    p.log_events_setting = False
    if native:
        p.attach_native()
    return p, rec, m


def run_engine(s, native, pieces):
    """Feed the pieces (bytes, one batch each); -> (calls, counters, control event types)."""
    p, rec, m = pipeline(s, native)
    ctrl = []
    for data in pieces:
        if native:
            ctrl += p.handle_raw(data, 0, framed=False)
        else:
            ctrl += p.handle_batch(p.decoder.feed(data), 0)
    return rec.calls, {k: m.c.get(k, 0) for k in COUNTERS}, [c[0] for c in ctrl]


def both(env, ov, pieces):
    s = settings_for(env, ov)
    py = run_engine(s, False, pieces)
    nat = run_engine(s, True, pieces)
    assert py == nat
    return py


def set_status(pod, rv, state, rc=0, last=None, phase=None):
    p = copy.deepcopy(pod)
    p["metadata"]["resourceVersion"] = str(rv)
    c = p["status"]["containerStatuses"][0]
    c["state"] = state
    c["restartCount"] = rc
    c["lastState"] = last or {}
    c["ready"] = "running" in state
    if phase:
        p["status"]["phase"] = phase
    return p


CLB = {"waiting": {"reason": "CrashLoopBackOff", "message": "back-off 10s restarting failed container"}}
UP = {"running": {"startedAt": "2025-07-09T01:55:00Z"}}


def died(code, reason):
    return {"terminated": {"exitCode": code, "reason": reason, "startedAt": "2025-07-09T01:51:32Z",
                           "finishedAt": "2025-07-09T01:52:00Z", "containerID": "containerd://0"}}


def life(seed=21, ns="default"):
    """One pod's life (test 2): (type, pod) in order."""
    f = PodFactory(seed=seed, namespaces=[ns])
    p0 = f.new_pod()
    p0["metadata"]["resourceVersion"] = "1"
    run_ = f.running(p0)
    return [
        ("ADDED", p0),
        ("MODIFIED", set_status(run_, 2, UP)),
        ("MODIFIED", set_status(run_, 3, CLB, 1, died(1, "Error"))),
        ("MODIFIED", set_status(run_, 4, CLB, 1, died(1, "Error"))),
        ("MODIFIED", set_status(run_, 5, UP, 2, died(137, "OOMKilled"))),
        ("MODIFIED", set_status(run_, 6, CLB, 2, died(137, "OOMKilled"))),
        ("DELETED", set_status(run_, 7, CLB, 2, died(137, "OOMKilled"))),
    ]


def lines(events):
    return b"".join(event_line(t, o) for t, o in events)


def check_pod_life(env="production"):
    events = life()
    calls, c, ctrl = both(env, ON, [lines(events)])
    assert ctrl == []
    assert [et for _, et, *_ in calls] == ["MODIFIED", "MODIFIED", "MODIFIED", "DELETED"]
    assert all("extra" not in core for *_, core in calls)
    # exactly the third, fifth, sixth and seventh events, in that order
    sent = [events[i][1] for i in (2, 4, 5, 6)]
    assert [core["status"]["container_statuses"][0]["state"] for *_, core in calls] == \
        [p["status"]["containerStatuses"][0]["state"] for p in sent]
    assert [core["status"]["container_statuses"][0]["restart_count"] for *_, core in calls] == [1, 2, 2, 2]
    assert c["events_container_failure"] == 3
    assert c["events_filtered_critical"] == 3  # the first two and the unchanged-signature fourth
    assert c["events_received"] == 7 and c["events_unchanged"] == 0


def test_pod_life_production_both_engines():
    check_pod_life()


def test_pod_life_one_event_per_read():
    """The same life, one read per event: the signature lives in the cache, not in the batch."""
    events = life()
    calls, c, _ = both("production", ON, [event_line(t, o) for t, o in events])
    assert [et for _, et, *_ in calls] == ["MODIFIED", "MODIFIED", "MODIFIED", "DELETED"]
    assert c["events_container_failure"] == 3 and c["events_filtered_critical"] == 3


def test_native_decoder_through_handle_batch_over_the_native_cache():
    """What the native engine's WatchList path and reconcile run on: the native
    decoder's tuples through handle_batch, the signature in the native cache."""
    from k8s_watcher_amd.ops.cache import make_pod_cache
    s = settings_for("production", ON)
    want = run_engine(s, False, [lines(life())])
    rec, m = Recorder(), Metrics()
    dec = decoder_for(s, "native")
    p = EventPipeline(s, dec, rec, m, make_pod_cache(True))
    p.log_events_setting = False
    events = dec.feed(lines(life()))
    assert [len(e) for e in events] == [10] * 7
    assert p.handle_batch(events, 0) == []
    assert (rec.calls, {k: m.c.get(k, 0) for k in COUNTERS}) == want[:2]


def test_recovery_is_silent_and_a_relapse_alerts_again():
    f = PodFactory(seed=22, namespaces=["default"])
    run_ = f.running(f.new_pod())
    events = [("ADDED", set_status(run_, 1, UP)),
              ("MODIFIED", set_status(run_, 2, CLB, 1, died(1, "Error"))),
              ("MODIFIED", set_status(run_, 3, UP, 0)),   # findings empty: nothing sent, the signature back to 0
              ("MODIFIED", set_status(run_, 4, CLB, 1, died(1, "Error")))]  # the same findings as before: alerts again
    calls, c, _ = both("production", ON, [lines(events)])
    assert [(et, core["status"]["container_statuses"][0]["restart_count"]) for _, et, _, _, core in calls] == \
        [("MODIFIED", 1), ("MODIFIED", 1)]
    assert c["events_container_failure"] == 2 and c["events_filtered_critical"] == 2


def test_pending_pod_with_init_container_in_image_pull_back_off():
    f = PodFactory(seed=23, namespaces=["default"])
    pend = f.scheduled(f.new_pod())
    pend["status"]["initContainerStatuses"] = [
        {"name": "fetch", "state": {"waiting": {"reason": "ImagePullBackOff", "message": "Back-off pulling image"}},
         "lastState": {}, "ready": False, "restartCount": 0, "image": "registry.example.com/none:v0", "imageID": ""}]
    for c_ in pend["status"]["containerStatuses"]:
        c_["state"] = {"waiting": {"reason": "PodInitializing"}}
    events = []
    for rv in (1, 2, 3):
        p = copy.deepcopy(pend)
        p["metadata"]["resourceVersion"] = str(rv)
        events.append(("ADDED" if rv == 1 else "MODIFIED", p))
    calls, c, _ = both("production", ON, [lines(events)])
    assert [(et, core["status"]["phase"]) for _, et, _, _, core in calls] == [("ADDED", "Pending")]
    assert c["events_container_failure"] == 1 and c["events_filtered_critical"] == 2


def test_staging_phase_change():
    f = PodFactory(seed=24, namespaces=["default"])
    run_ = f.running(f.new_pod())
    events = [("ADDED", set_status(run_, 1, UP)),
              ("MODIFIED", set_status(run_, 2, CLB, 1, died(1, "Error"))),   # same phase, new findings: sent
              ("MODIFIED", set_status(run_, 3, CLB, 1, died(1, "Error"))),   # unchanged findings
              ("MODIFIED", set_status(run_, 4, UP, 1, died(1, "Error")))]    # waiting gone: other findings, sent
    ov = merged(ON, {"watcher": {"notify_on": "phase_change"}})
    calls, c, _ = both("staging", ov, [lines(events)])
    assert [(et, core["status"]["container_statuses"][0]["restart_count"]) for _, et, _, _, core in calls] == \
        [("ADDED", 0), ("MODIFIED", 1), ("MODIFIED", 1)]
    assert c["events_unchanged"] == 1 and c["events_container_failure"] == 2 and c["events_filtered_critical"] == 0
    # without the option the phase alone decides
    calls, c, _ = both("staging", {"watcher": {"notify_on": "phase_change"}}, [lines(events)])
    assert [et for _, et, *_ in calls] == ["ADDED"] and c["events_unchanged"] == 3


def test_option_off_is_today():
    """The guard: with the option off (and no extra bit) nothing changes — this passes without the feature too."""
    s = settings_for("production", {})
    py = run_engine(s, False, [lines(life())])
    nat = run_engine(s, True, [lines(life())])
    assert py == nat
    calls, c, _ = py
    assert [et for _, et, *_ in calls] == ["DELETED"]
    assert "container_failures" not in json.dumps(calls)
    assert c["events_container_failure"] == 0 and c["events_filtered_critical"] == 6
    ev = decoder_for(s).feed(lines(life()))
    assert all(len(e) == 9 for e in ev)
    ev = decoder_for(s, "native").feed(lines(life()))
    assert all(len(e) == 9 for e in ev)


def test_custom_reasons_reach_both_engines():
    f = PodFactory(seed=25, namespaces=["default"])
    run_ = f.running(f.new_pod())
    events = [("ADDED", set_status(run_, 1, {"waiting": {"reason": "ContainerCreating"}}, phase="Pending")),
              ("MODIFIED", set_status(run_, 2, {"waiting": {"reason": "CrashLoopBackOff"}}))]
    ov = merged(ON, {"watcher": {"alerts": {"container_failure_reasons": ["ContainerCreating"]}}})
    calls, c, _ = both("production", ov, [lines(events)])
    assert [et for _, et, *_ in calls] == ["ADDED"] and c["events_container_failure"] == 1


# ----------------------------------------------------------------------------- the extra field (test 6)

def check_extra_field():
    from k8s_watcher_amd.models.payload import EXTRA_FIELDS, extra_mask
    assert EXTRA_FIELDS.index("container_failures") == 6 and extra_mask(["container_failures"]) == FAILURES_BIT
    for mask in (FAILURES_BIT, 0b1111111):
        py = make_decoder("python", "staging", extra=mask)
        nat = make_decoder("native", "staging", extra=mask)
        for name, init_raw, cs_raw, want in CORPUS:
            for etype in ("MODIFIED", "DELETED"):
                line = corpus_line(init_raw, cs_raw, etype)
                a, b = py.feed(line)[0], nat.feed(line)[0]
                assert a[0] == b[0] == etype and len(a) == len(b) == 9, name
                ca, cb = py.core(a), nat.core(b)
                assert json.loads(ca) == json.loads(cb), name
                if event_line(etype, json.loads(line)["object"]) == line:
                    # byte for byte where the input is spelled as json.dumps spells it (the base payload
                    # copies raw tokens: an escape, a repeated key, -0 or 1e2 is copied as written)
                    assert ca == cb, name
                extra = json.loads(cb)["extra"]
                assert extra["container_failures"] == want, name
                assert list(extra) == [n for i, n in enumerate(EXTRA_FIELDS) if mask >> i & 1]
    # the six older bits keep their meaning
    d = make_decoder("native", "staging", extra=0b111111)
    extra = json.loads(d.core(d.feed(corpus_line(None, "[%s]" % cs(state=WAIT_CLB)))[0]))["extra"]
    assert list(extra) == ["pod_ip", "host_ip", "start_time", "qos_class", "resource_version", "owner_references"]
    # a pod known only from the cache
    for eng in ("python", "native"):
        core = make_decoder(eng, "staging", extra=FAILURES_BIT).core_from_summary("u", "default", "n", "Running")
        assert json.loads(core)["extra"] == {"container_failures": []}


def test_extra_field_both_decoders():
    check_extra_field()


def test_extra_field_through_the_pipelines():
    """The fused pipeline emits it too (light and full parse), with the filter option on or off."""
    data = b"".join(corpus_line(i, c, "ADDED" if n == 0 else "MODIFIED", uid="u%d" % n, rv=str(n + 1))
                    for n, (_, i, c, _) in enumerate(CORPUS))
    want = [w for *_, w in CORPUS]
    for env, ov in (("staging", {}), ("production", {"watcher": {"alerts": {"critical_events_only": False}}}),
                    ("staging", ON)):
        ov = merged(ov, {"watcher": {"payload_extra_fields": ["container_failures"]}})
        calls, _, ctrl = both(env, ov, [data])
        assert ctrl == [] and [core["extra"]["container_failures"] for *_, core in calls] == want


def test_signatures_agree_across_spellings():
    """Two spellings of one findings list are one signature, in each decoder."""
    plain = corpus_line(None, "[%s]" % cs(rc="0", state=WAIT_CLB))
    escaped = corpus_line(None, "[%s]" % cs(rc="-0", state='{"waiting":{"reason":"Crash\\u004coopBackOff"}}'))
    other = corpus_line(None, "[%s]" % cs(rc="1", state=WAIT_CLB))
    healthy = corpus_line(None, "[%s]" % cs(state=RUNNING))
    for eng in ("python", "native"):
        d = make_decoder(eng, "production", failures=True)
        sig = [d.feed(x)[0][9] for x in (plain, escaped, other, healthy)]
        assert sig[0] == sig[1] != 0 and sig[2] not in (0, sig[0]) and sig[3] == 0
        assert d.feed(corpus_line(None, "[%s]" % cs(state=WAIT_CLB), "DELETED"))[0][9] == 0
        _, _, items = d.decode_list(('{"metadata":{"resourceVersion":"5"},"items":[%s]}'
                                     % corpus_pod(None, "[%s]" % cs(state=WAIT_CLB))).encode())
        assert items[0][9] == sig[0]


def test_both_caches_swap_failure():
    from k8s_watcher_amd.ops.cache import make_pod_cache
    for native in (False, True):
        cache = make_pod_cache(native)
        assert cache.swap_failure("nobody", 5) == 0 and len(cache) == 0
        cache.observe("ADDED", "u", "1", "Running", "default", "n")
        assert cache.swap_failure("u", 0) == 0
        assert cache.swap_failure("u", 2 ** 64 - 1) == 0
        assert cache.swap_failure("u", 7) == 2 ** 64 - 1
        assert cache.swap_failure("u", 0) == 7
        assert cache.get("u")[:5] == ["1", "Running", "default", "n", None]
        assert [r[:5] for r in cache.to_records()] == [["u", "1", "Running", "default", "n"]]  # never persisted
        assert all(len(r) == 6 for r in cache.to_records())
        cache.swap_failure("u", 9)
        cache.put("u", "2", "Running", "default", "n", None)  # a whole new entry
        assert cache.swap_failure("u", 0) == 0


# ----------------------------------------------------------------------------- fuzz (test 7)

REASON_WORDS = ["CrashLoopBackOff", "ErrImagePull", "ImagePullBackOff", "ContainerCreating", "Error", "OOMKilled", ""]
leaf = st.one_of(st.none(), st.booleans(), st.integers(-2, 3), st.sampled_from([0.0, 1.0, 2.5, 1e2]),
                 st.sampled_from(REASON_WORDS))
KEYS = ["name", "restartCount", "state", "lastState", "waiting", "terminated", "running", "reason", "exitCode"]
junk = st.recursive(leaf, lambda ch: st.one_of(st.lists(ch, max_size=2),
                                               st.dictionaries(st.sampled_from(KEYS), ch, max_size=3)), max_leaves=6)


def some_keys(**kw):
    return st.fixed_dictionaries({}, optional=kw)


waiting_s = st.one_of(some_keys(reason=leaf, message=leaf), junk)
terminated_s = st.one_of(some_keys(exitCode=leaf, reason=leaf), junk)
state_s = st.one_of(some_keys(waiting=waiting_s, terminated=terminated_s, running=st.just({})), junk)
status_s = st.one_of(some_keys(name=st.one_of(st.sampled_from(["app", "side"]), leaf), restartCount=leaf,
                               state=state_s, lastState=state_s), junk)
array_s = st.one_of(st.lists(status_s, max_size=3), st.none(), junk)
event_s = st.tuples(st.integers(0, 3), st.sampled_from(["ADDED", "MODIFIED", "MODIFIED", "MODIFIED", "DELETED"]),
                    st.sampled_from(["Pending", "Running", "Running", "Failed"]), array_s, array_s, st.booleans())
FUZZ_PROFILES = [("production", {}), ("staging", {"watcher": {"notify_on": "phase_change"}})]
_fuzz_settings = {}


def fuzz_settings(i):
    if i not in _fuzz_settings:
        env, ov = FUZZ_PROFILES[i]
        _fuzz_settings[i] = settings_for(env, merged(ON, ov, {"watcher": {
            "payload_extra_fields": ["container_failures"]}}))
    return _fuzz_settings[i]


@hyp_settings(max_examples=400, deadline=None, database=None, derandomize=True,
              suppress_health_check=list(HealthCheck))
@given(st.integers(0, len(FUZZ_PROFILES) - 1), st.lists(event_s, min_size=1, max_size=6))
def test_fuzz_both_engines_agree(profile, events):
    f = PodFactory(seed=31, namespaces=["default"])
    base = [f.running(f.new_pod()) for _ in range(4)]
    out = []
    for rv, (i, etype, phase, init, css, with_init) in enumerate(events, 1):
        p = copy.deepcopy(base[i])
        p["metadata"]["resourceVersion"] = str(rv)
        p["status"]["phase"] = phase
        p["status"]["containerStatuses"] = css
        if with_init:
            p["status"]["initContainerStatuses"] = init
        out.append(event_line(etype, p))
    s = fuzz_settings(profile)
    py = run_engine(s, False, [b"".join(out)])
    nat = run_engine(s, True, [b"".join(out)])
    assert py == nat  # the same notification sequence, cores and counters


# ----------------------------------------------------------------------------- partitioned apply (test 8)

def failing_batch(n_pods=64, rounds=31, seed=5):
    """~2,000 lines over 64 pods: healthy, failing and repeated signatures mixed."""
    import random
    rng = random.Random(seed)
    f = PodFactory(seed=seed, namespaces=["default", "kube-system", "production", "batch", "monitoring"])
    pods = [f.running(f.new_pod()) for _ in range(n_pods)]
    shapes = [(UP, 0, None), (CLB, 1, died(1, "Error")), (CLB, 2, died(1, "Error")), (UP, 2, died(137, "OOMKilled")),
              ({"waiting": {"reason": "ImagePullBackOff"}}, 0, None), (died(3, "Error"), 0, None)]
    rv = 0
    out = []
    for p in pods:
        rv += 1
        out.append(event_line("ADDED", set_status(p, rv, UP)))
    last = [0] * n_pods
    for _ in range(rounds):
        for i, p in enumerate(pods):
            rv += 1
            k = last[i] if rng.random() < 0.4 else rng.randrange(len(shapes))  # 40%: the same signature again
            last[i] = k
            state, rc, prev = shapes[k]
            out.append(event_line("MODIFIED", set_status(p, rv, state, rc, prev)))
    return b"".join(out), len(out)


def check_partitioned_matches_serial():
    from test_partitioned_apply import feed, per_uid
    data, n = failing_batch()
    assert 1900 <= n <= 2100
    for env, ov in (("production", ON), ("staging", merged(ON, {"watcher": {"notify_on": "phase_change"}}))):
        s_got, s_cache, s_cnt, s_rv, s_ctrl, s_probe, _ = feed(env, ov, data, partitioned=False, piece=1 << 20)
        p_got, p_cache, p_cnt, p_rv, p_ctrl, p_probe, parts = feed(env, ov, data, partitioned=True, piece=1 << 20)
        assert s_probe.get("partitioned_batches", 0) == 0
        assert p_probe["partitioned_batches"] > 0 and parts > 0
        assert collections.Counter(p_got) == collections.Counter(s_got)
        assert per_uid(p_got) == per_uid(s_got)
        assert p_cache == s_cache and p_cnt == s_cnt and p_rv == s_rv and p_ctrl == s_ctrl == []
        assert s_cnt["events_container_failure"] > 100
        # and the serial native apply is the Python engine's verdict
        calls, c, _ = run_engine(settings_for(env, ov), False, [data])
        assert per_uid([(u, et, core["status"]["phase"]) for u, et, _, _, core in calls]) == per_uid(s_got)
        assert {k: v for k, v in s_cnt.items() if k in COUNTERS and v} == {k: v for k, v in c.items() if v}


def test_partitioned_apply_matches_serial_with_failures():
    check_partitioned_matches_serial()


# ----------------------------------------------------------------------------- relist after a 410 (test 9)

@pytest.mark.parametrize("native", [True, False], ids=["native-relist", "python-reconcile"])
def test_relist_after_410(native):
    from test_native_relist import list_pages, native_relist
    f = PodFactory(seed=41, namespaces=["default"])
    a, b, c_ = (f.running(f.new_pod()) for _ in range(3))
    s = settings_for("production", ON)
    p, rec, m = pipeline(s, native)
    watch = lines([("ADDED", set_status(a, 1, UP)), ("ADDED", set_status(b, 2, CLB, 1, died(1, "Error"))),
                   ("ADDED", set_status(c_, 3, UP))])
    if native:
        p.handle_raw(watch, 0, framed=False)
    else:
        p.handle_batch(p.decoder.feed(watch), 0)
    assert [(u, et) for u, et, *_ in rec.calls] == [(b["metadata"]["uid"], "ADDED")]
    del rec.calls[:]
    # the gap: a began failing, b's resourceVersion moved with the same findings, c only moved on
    listed = [set_status(a, 10, CLB, 1, died(1, "Error")), set_status(b, 11, CLB, 1, died(1, "Error")),
              set_status(c_, 12, UP)]
    if native:
        ctrl, stats = native_relist(p, listed, None)
        assert stats["modified"] == 3
    else:
        _, _, evs = p.decoder.decode_list(list_pages(listed, 10 ** 6)[0])
        ctrl = p.reconcile(evs, 0)
    assert ctrl == []
    assert [(u, et) for u, et, *_ in rec.calls] == [(a["metadata"]["uid"], "MODIFIED")]
    assert m.c["events_container_failure"] == 2 and m.c["events_filtered_critical"] == 4
    # a silent relist (initial_list: skip) leaves no signature: the pod is reported at its next event
    q, rec2, m2 = pipeline(s, native)
    if native:
        native_relist(q, listed, None, notify=False)
    else:
        q.reconcile(q.decoder.decode_list(list_pages(listed, 10 ** 6)[0])[2], 0, notify=False)
    assert rec2.calls == [] and len(q.cache) == 3
    again = lines([("MODIFIED", set_status(b, 20, CLB, 1, died(1, "Error")))])
    if native:
        q.handle_raw(again, 0, framed=False)
    else:
        q.handle_batch(q.decoder.feed(again), 0)
    assert [(u, et) for u, et, *_ in rec2.calls] == [(b["metadata"]["uid"], "MODIFIED")]


# ----------------------------------------------------------------------------- end to end (test 10)

def test_end_to_end_service():
    from k8s_watcher_amd.engine.service import WatcherService
    from k8s_watcher_amd.kube.kubeconfig import KubeEndpoint
    from k8s_watcher_amd.testing.fake_apiserver import FakeApiServer
    from k8s_watcher_amd.testing.stub_sink import StubSink

    async def body():
        srv = FakeApiServer()
        await srv.start()
        sink = StubSink()
        await sink.start()
        s = load_settings("production", environ={}, overrides=merged(ON, {
            "clusterapi": {"base_url": sink.url},
            "watcher": {"engine": "native", "payload_extra_fields": ["container_failures"]}}))
        svc = WatcherService(s, endpoint=KubeEndpoint(server=srv.url), metrics=Metrics())
        await svc.start()
        f = PodFactory(seed=51, namespaces=["default"])
        pod = f.running(f.new_pod())
        srv.create(set_status(pod, 0, UP))
        srv.update(set_status(pod, 0, CLB, 1, died(1, "Error")))
        await sink.state.wait_for(1, timeout=20)
        srv.update(set_status(pod, 0, CLB, 1, died(1, "Error")))   # nothing new
        srv.update(set_status(pod, 0, CLB, 2, died(1, "Error")))   # crashed again
        await sink.state.wait_for(2, timeout=20)
        await svc.notifier.drain(5)
        got = sink.state.payloads()
        counters = dict(svc.metrics.c)
        svc.stop()
        await svc.shutdown()
        await sink.stop()
        await srv.stop()
        return pod, got, counters

    pod, got, c = run(body(), timeout=60)
    name = pod["status"]["containerStatuses"][0]["name"]
    assert [(p["event_type"], p["uid"]) for p in got] == [("MODIFIED", pod["metadata"]["uid"])] * 2
    assert [p["extra"]["container_failures"] for p in got] == [
        [fnd(name, "waiting", "CrashLoopBackOff", None, rc), fnd(name, "restarted", "Error", 1, rc)] for rc in (1, 2)]
    assert c["events_container_failure"] == 2 and c["events_filtered_critical"] == 2


# ----------------------------------------------------------------------------- configuration (test 11)

def test_config_keys():
    from k8s_watcher_amd.models.findings import DEFAULT_FAILURE_REASONS
    for env in ("development", "staging", "production"):
        w = load_settings(env, environ={}).watcher
        assert w.container_failures is False
        assert w.container_failure_reasons == list(DEFAULT_FAILURE_REASONS) == [
            "CrashLoopBackOff", "ImagePullBackOff", "ErrImagePull", "ErrImageNeverPull", "InvalidImageName",
            "CreateContainerConfigError", "CreateContainerError", "RunContainerError"]
    w = load_settings("production", environ={},
                      overrides=parse_override("watcher.alerts.container_failures=true")).watcher
    assert w.container_failures is True and w.critical_events_only is True
    ov = merged(parse_override("watcher.alerts.container_failures=true"),
                parse_override("watcher.alerts.container_failure_reasons=[OOMish, CrashLoopBackOff]"))
    w = load_settings("staging", environ={}, overrides=ov).watcher
    assert w.container_failure_reasons == ["OOMish", "CrashLoopBackOff"]
    with pytest.raises(ConfigError):
        load_settings("staging", environ={}, overrides=merged(ON, {"watcher": {"alerts": {
            "container_failure_reasons": []}}}))
    # an empty list only matters once the option is on
    assert load_settings("staging", environ={}, overrides={"watcher": {"alerts": {
        "container_failure_reasons": []}}}).watcher.container_failure_reasons == []
    for bad in ("CrashLoopBackOff", [1], [""]):
        with pytest.raises(ConfigError):
            load_settings("staging", environ={}, overrides={"watcher": {"alerts": {
                "container_failure_reasons": bad}}})
    with pytest.raises(ConfigError):
        load_settings("staging", environ={}, overrides={"watcher": {"alerts": {"container_failures": "perhaps"}}})


def test_print_config_shows_the_keys(capsys):
    from k8s_watcher_amd.utils.config import dump_effective
    s = load_settings("production", environ={}, overrides=parse_override("watcher.alerts.container_failures=true"))
    dump_effective(s)
    out = capsys.readouterr().out
    assert "container_failures: true" in out and "container_failure_reasons:" in out and "CrashLoopBackOff" in out


def test_metric_is_declared():
    from k8s_watcher_amd.metrics import COUNTERS as DECLARED
    assert "events_container_failure" in DECLARED and Metrics().c["events_container_failure"] == 0
