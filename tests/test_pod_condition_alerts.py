"""Unschedulable and disrupted pods through the critical filter (``watcher.alerts.pod_conditions``).

The rules (``watcher.alerts.pod_condition_rules``), the condition findings
(``models/findings.py`` and ``ops/csrc/findings.inc``: one verdict on every
pod), their signature and the filter rule in both engines — the watch path
(serial and partitioned apply), the native relist, the Python reconcile — the
payload extra field ``pod_condition_alerts`` and the counter.
"""

import collections
import copy
import json
import random

import pytest

from k8s_watcher_amd.engine.pipeline import EventPipeline
from k8s_watcher_amd.metrics import Metrics
from k8s_watcher_amd.ops.decode import make_decoder
from k8s_watcher_amd.testing.podgen import PodFactory, event_line
from k8s_watcher_amd.utils.config import ConfigError, load_settings, parse_override

ON = {"watcher": {"alerts": {"pod_conditions": True}}}
BOTH_ON = {"watcher": {"alerts": {"pod_conditions": True, "container_failures": True}}}
CONDITIONS_BIT = 0b10000000
DEFAULT_RULES = ["PodScheduled=False:Unschedulable", "PodScheduled=False:SchedulerError", "DisruptionTarget=True"]


def merged(*dicts):
    out = {}
    for d in dicts:
        for k, v in d.items():
            out[k] = merged(out[k], v) if isinstance(v, dict) and isinstance(out.get(k), dict) else copy.deepcopy(v)
    return out


# ----------------------------------------------------------------------------- the rules (test 1)

def alerts(**kw):
    return {"watcher": {"alerts": kw}}


def test_rules():
    from k8s_watcher_amd.models.findings import DEFAULT_CONDITION_RULES, condition_rules, parse_condition_rule
    for env in ("development", "staging", "production"):
        w = load_settings(env, environ={}).watcher
        assert w.pod_conditions is False
        assert w.pod_condition_rules == list(DEFAULT_CONDITION_RULES) == DEFAULT_RULES
    assert condition_rules(None) == (("PodScheduled", "False", "Unschedulable"),
                                     ("PodScheduled", "False", "SchedulerError"), ("DisruptionTarget", "True", None))
    # split at the first "=", the rest at the first ":": a ":" (or "=") further on belongs to the reason
    assert parse_condition_rule("Ready=False:a:b=c") == ("Ready", "False", "a:b=c")
    assert parse_condition_rule("X=Y=Z") == ("X", "Y=Z", None)
    w = load_settings("production", environ={}, overrides=merged(ON, alerts(
        pod_condition_rules=["Ready=False:a:b"]))).watcher
    assert w.pod_conditions is True and w.critical_events_only is True and w.pod_condition_rules == ["Ready=False:a:b"]
    w = load_settings("staging", environ={}, overrides=parse_override("watcher.alerts.pod_conditions=true")).watcher
    assert w.pod_conditions is True
    many = ["T%d=True" % i for i in range(33)]
    assert len(load_settings("staging", environ={}, overrides=alerts(
        pod_condition_rules=many[:32])).watcher.pod_condition_rules) == 32
    for bad in (["PodScheduled"], ["=False"], ["PodScheduled="], ["PodScheduled=False:"], many, [5], "Ready=False"):
        for on in (False, True):
            with pytest.raises(ConfigError, match="watcher.alerts.pod_condition_rules"):
                load_settings("staging", environ={}, overrides=alerts(pod_conditions=on, pod_condition_rules=bad))
    with pytest.raises(ConfigError, match="watcher.alerts.pod_condition_rules"):
        load_settings("staging", environ={}, overrides=alerts(pod_conditions=True, pod_condition_rules=[]))
    # an empty list only matters once the option is on
    assert load_settings("staging", environ={}, overrides=alerts(pod_condition_rules=[])).watcher.pod_condition_rules == []
    with pytest.raises(ConfigError, match="watcher.alerts.pod_conditions"):
        load_settings("staging", environ={}, overrides=alerts(pod_conditions="perhaps"))


def test_print_config_shows_the_keys(capsys):
    from k8s_watcher_amd.utils.config import dump_effective
    dump_effective(load_settings("production", environ={}, overrides=ON))
    out = capsys.readouterr().out
    assert "pod_conditions: true" in out and "pod_condition_rules:" in out and "DisruptionTarget=True" in out


# ----------------------------------------------------------------------------- the corpus (test 2)

MSG = '"0/16 nodes are available: 16 Insufficient amd.com/gpu."'
T0 = '"2025-07-09T01:51:32Z"'


def cond(type_='"PodScheduled"', status='"False"', reason='"Unschedulable"', message=MSG, ltt=T0):
    """One conditions element as raw JSON text (the values are raw tokens; None leaves the key out)."""
    parts = [("type", type_), ("status", status), ("reason", reason), ("message", message),
             ("lastProbeTime", "null"), ("lastTransitionTime", ltt)]
    return "{%s}" % ",".join('"%s":%s' % (k, v) for k, v in parts if v is not None)


def cf(type_, status, reason=None):
    return {"type": type_, "status": status, "reason": reason}


UNSCHED = cf("PodScheduled", "False", "Unschedulable")
DISRUPT = cf("DisruptionTarget", "True", "PreemptionByScheduler")
C_UNSCHED = cond()
C_DISRUPT = cond('"DisruptionTarget"', '"True"', '"PreemptionByScheduler"', '"preempting"')
C_FINE = cond(status='"True"', reason=None, message=None)


def status_of(cond_raw):
    return '{"phase":"Pending","conditions":%s,"qosClass":"Burstable"}' % cond_raw


# (id, raw status object, expected findings)
CORPUS = [(name, status_of(raw), want) for name, raw, want in [
    ("healthy", "[%s]" % C_FINE, []),
    ("unschedulable", "[%s]" % C_UNSCHED, [UNSCHED]),
    ("scheduler-error", "[%s]" % cond(reason='"SchedulerError"'), [cf("PodScheduled", "False", "SchedulerError")]),
    ("disruption-target", "[%s,%s]" % (C_FINE, C_DISRUPT), [DISRUPT]),
    ("wildcard-without-reason", "[%s]" % cond('"DisruptionTarget"', '"True"', None), [cf("DisruptionTarget", "True")]),
    ("wildcard-reason-number", "[%s]" % cond('"DisruptionTarget"', '"True"', "5"), [cf("DisruptionTarget", "True")]),
    ("wildcard-reason-empty", "[%s]" % cond('"DisruptionTarget"', '"True"', '""'), [cf("DisruptionTarget", "True", "")]),
    ("reason-outside-rules", "[%s]" % cond(reason='"Other"'), []),
    ("reason-missing", "[%s]" % cond(reason=None), []),
    ("reason-prefix", "[%s]" % cond(reason='"Unschedulable2"'), []),
    ("conditions-null", "null", []),
    ("conditions-string", '"PodScheduled=False"', []),
    ("conditions-object", '{"a":%s}' % C_UNSCHED, []),
    ("conditions-empty", "[]", []),
    ("elements-not-objects", '[7,[%s],"x",null,1.5,%s]' % (C_UNSCHED, C_UNSCHED), [UNSCHED]),
    ("type-number", "[%s]" % cond(type_="7"), []),
    ("type-true", "[%s]" % cond(type_="true"), []),
    ("type-null", "[%s]" % cond(type_="null"), []),
    ("type-missing", "[%s]" % cond(type_=None), []),
    ("status-number", "[%s]" % cond(status="0"), []),
    ("status-false-literal", "[%s]" % cond(status="false"), []),
    ("status-null", "[%s]" % cond(status="null"), []),
    ("status-lowercase", "[%s]" % cond(status='"false"'), []),
    ("reason-true", "[%s]" % cond(reason="true"), []),
    ("reason-null", "[%s]" % cond(reason="null"), []),
    ("reason-array", "[%s]" % cond(reason='["Unschedulable"]'), []),
    ("escaped-type", "[%s]" % cond(type_='"PodSched\\u0075led"'), [UNSCHED]),
    ("escaped-status-and-reason", "[%s]" % cond(status='"F\\u0061lse"', reason='"Un\\u0073chedulable"'), [UNSCHED]),
    ("escaped-keys", '[{"t\\u0079pe":"PodScheduled","st\\u0061tus":"False","re\\u0061son":"Unschedulable"}]', [UNSCHED]),
    ("escape-that-is-no-match", "[%s]" % cond(reason='"Unschedulable\\n"'), []),
    ("repeated-reason-last-matches",
     '[{"type":"PodScheduled","status":"False","reason":"Other","reason":"Unschedulable"}]', [UNSCHED]),
    ("repeated-reason-last-misses",
     '[{"type":"PodScheduled","status":"False","reason":"Unschedulable","reason":"Other"}]', []),
    ("repeated-type", '[{"type":"Ready","status":"False","reason":"Unschedulable","type":"PodScheduled"}]', [UNSCHED]),
    ("message-a", "[%s]" % cond(message='"0/16 nodes are available"', ltt='"2025-07-09T01:00:00Z"'), [UNSCHED]),
    ("message-b", "[%s]" % cond(message='"0/16 nodes: 15 Insufficient amd.com/gpu, 1 tainted"',
                                ltt='"2025-07-09T02:00:00Z"'), [UNSCHED]),
    ("two-in-order", "[%s,%s]" % (C_UNSCHED, C_DISRUPT), [UNSCHED, DISRUPT]),
    ("two-reversed", "[%s,%s]" % (C_DISRUPT, C_UNSCHED), [DISRUPT, UNSCHED]),
    ("same-twice", "[%s,%s]" % (C_UNSCHED, C_UNSCHED), [UNSCHED, UNSCHED]),
]] + [
    ("repeated-conditions-last-healthy",
     '{"phase":"Pending","conditions":[%s],"conditions":[%s]}' % (C_UNSCHED, C_FINE), []),
    ("repeated-conditions-last-matching",
     '{"phase":"Pending","conditions":[%s],"conditions":[%s]}' % (C_FINE, C_UNSCHED), [UNSCHED]),
    ("repeated-conditions-last-null", '{"phase":"Pending","conditions":[%s],"conditions":null}' % C_UNSCHED, []),
    ("repeated-status-last-healthy", '%s,"status":%s' % (status_of("[%s]" % C_UNSCHED), status_of("[%s]" % C_FINE)), []),
    ("repeated-status-last-matching", '%s,"status":%s' % (status_of("[%s]" % C_FINE), status_of("[%s]" % C_UNSCHED)),
     [UNSCHED]),
    ("repeated-status-last-without-conditions", '%s,"status":{"phase":"Pending"}' % status_of("[%s]" % C_UNSCHED), []),
    ("status-null", "null", []),
    ("no-conditions", '{"phase":"Pending"}', []),
]

# the array cut short inside its second element, in a line whose brackets still balance
TRUNCATED = status_of('[%s,{"type":"Ready","status"}]' % C_UNSCHED)


def corpus_pod(status_raw, uid="u-corpus", rv="7"):
    """The pod as JSON text, the raw status spliced in untouched."""
    f = PodFactory(seed=3, namespaces=["default"])
    pod = f.new_pod()
    pod["metadata"].update(uid=uid, resourceVersion=rv)
    pod["status"] = "@STATUS@"
    return json.dumps(pod, separators=(",", ":"), ensure_ascii=False).replace('"@STATUS@"', status_raw)


def corpus_line(status_raw, etype="MODIFIED", **kw):
    return ('{"type":"%s","object":%s}\n' % (etype, corpus_pod(status_raw, **kw))).encode()


@pytest.mark.parametrize("case", CORPUS, ids=[c[0] for c in CORPUS])
def test_findings_table(case):
    from k8s_watcher_amd.models.findings import condition_findings, condition_signature
    _, status_raw, want = case
    got = condition_findings(json.loads(corpus_pod(status_raw)))
    assert got == want
    assert (condition_signature(got) == 0) == (not want)


def test_findings_odd_pods_and_custom_rules():
    from k8s_watcher_amd.models.findings import condition_findings
    for pod in ({}, None, [], {"status": None}, {"status": []}, {"status": {"conditions": None}}):
        assert condition_findings(pod) == []
    pod = json.loads(corpus_pod(status_of("[%s,%s]" % (C_UNSCHED, cond('"Ready"', '"False"', '"ContainersNotReady"')))))
    assert condition_findings(pod, ["Ready=False"]) == [cf("Ready", "False", "ContainersNotReady")]
    assert condition_findings(pod, ["Ready=False:Other"]) == []
    assert condition_findings(pod, []) == []
    # a finding never carries the message or the times
    assert all(set(f) == {"type", "status", "reason"} for f in condition_findings(pod))


class Recorder:
    def __init__(self):
        self.calls = []

    def submit(self, uid, et, ns, name, core, read_ns, ts):
        self.calls.append((uid, et, ns, name, json.loads(core)))

    def flush(self):
        pass


COUNTERS = ("events_received", "events_filtered_critical", "events_filtered_namespace", "events_unchanged",
            "events_other_shard", "events_container_failure", "events_pod_condition", "bookmarks")


def settings_for(env, ov):
    return load_settings(env, overrides=merged({"watcher": {"decode_threads": 0}}, ov), environ={})


def decoder_for(s, engine="python"):
    w = s.watcher
    return make_decoder(engine, s.environment, w.state_format, w.payload_extra, w.validate,
                        w.container_failures, w.container_failure_reasons, w.pod_conditions, w.pod_condition_rules)


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


def check_corpus():
    """One verdict from both engines: the Python function, both decoders' extra
    field and signature, and the fused pipeline (filter-first and full parse)."""
    from k8s_watcher_amd.models.findings import condition_findings
    from k8s_watcher_amd.models.payload import EXTRA_FIELDS, extra_mask
    assert EXTRA_FIELDS.index("pod_condition_alerts") == 7 == EXTRA_FIELDS.index("container_failures") + 1
    assert extra_mask(["pod_condition_alerts"]) == CONDITIONS_BIT
    py = make_decoder("python", "staging", extra=CONDITIONS_BIT, conditions=True)
    nat = make_decoder("native", "staging", extra=CONDITIONS_BIT, conditions=True)
    sigs = {"python": [], "native": []}
    for name, status_raw, want in CORPUS:
        assert condition_findings(json.loads(corpus_pod(status_raw))) == want, name
        for etype in ("MODIFIED", "DELETED"):
            line = corpus_line(status_raw, etype)
            a, b = py.feed(line)[0], nat.feed(line)[0]
            assert a[0] == b[0] == etype and len(a) == len(b) == 11 and a[9] == b[9] == 0, name
            ca, cb = json.loads(py.core(a)), json.loads(nat.core(b))
            assert ca == cb and cb["extra"] == {"pod_condition_alerts": want}, name
            if etype == "DELETED":
                assert a[10] == b[10] == 0, name
            else:
                sigs["python"].append(a[10])
                sigs["native"].append(b[10])
    # a signature is 0 for no findings, and equal exactly when the findings are
    for eng, sig in sigs.items():
        for i, (ni, _, wi) in enumerate(CORPUS):
            assert (sig[i] == 0) == (not wi) and 0 <= sig[i] < 2 ** 64, (eng, ni)
            for j, (nj, _, wj) in enumerate(CORPUS):
                assert (sig[i] == sig[j]) == (wi == wj), (eng, ni, nj)
    names = [c[0] for c in CORPUS]
    for eng, sig in sigs.items():
        assert sig[names.index("message-a")] == sig[names.index("message-b")] == sig[names.index("unschedulable")] != 0
        assert sig[names.index("two-in-order")] != sig[names.index("two-reversed")]
    # all eight bits, and the seven older ones keep their meaning
    for mask, keys in ((0b11111111, list(EXTRA_FIELDS)), (0b1111111, list(EXTRA_FIELDS[:7]))):
        for eng in ("python", "native"):
            d = make_decoder(eng, "staging", extra=mask)
            ev = d.feed(corpus_line(status_of("[%s]" % C_UNSCHED)))[0]
            extra = json.loads(d.core(ev))["extra"]
            assert len(ev) == 9 and list(extra) == keys, (eng, mask)
            assert extra.get("pod_condition_alerts", [UNSCHED]) == [UNSCHED]
    # custom rules reach the extra field with the filter option off; a pod known only from the cache has none
    for eng in ("python", "native"):
        d = make_decoder(eng, "staging", extra=CONDITIONS_BIT, condition_rules=["PodScheduled=True"])
        assert json.loads(d.core(d.feed(corpus_line(status_of("[%s]" % C_FINE)))[0]))["extra"] == {
            "pod_condition_alerts": [cf("PodScheduled", "True")]}
        assert json.loads(d.core_from_summary("u", "default", "n", "Pending"))["extra"] == {"pod_condition_alerts": []}
    # the fused pipeline: filter-first with the option on, the full parse without it
    data = b"".join(corpus_line(st_, "ADDED" if n == 0 else "MODIFIED", uid="u%d" % n, rv=str(n + 1))
                    for n, (_, st_, _) in enumerate(CORPUS))
    for env, ov in (("staging", {}), ("staging", ON), ("production", alerts(critical_events_only=False))):
        ov = merged(ov, {"watcher": {"payload_extra_fields": ["pod_condition_alerts"]}})
        calls, _, ctrl = both(env, ov, [data])
        assert ctrl == [] and [core["extra"]["pod_condition_alerts"] for *_, core in calls] == [w for *_, w in CORPUS]
    # the truncated array: json.loads refuses the line, and so does the native engine in every parse
    line = corpus_line(TRUNCATED)
    with pytest.raises(ValueError):
        json.loads(line)
    for mask in (0, CONDITIONS_BIT):
        for on in (False, True):
            assert [d.feed(line)[0][0] for d in (make_decoder(e, "staging", extra=mask, conditions=on)
                                                 for e in ("python", "native"))] == ["INVALID", "INVALID"]
    for ov in ({}, ON, merged(ON, {"watcher": {"payload_extra_fields": ["pod_condition_alerts"]}})):
        s = settings_for("staging", ov)
        for native in (False, True):
            calls, _, ctrl = run_engine(s, native, [line])
            assert calls == [] and ctrl == ["INVALID"], (ov, native)


def test_corpus_one_verdict_from_both_engines():
    check_corpus()


def test_both_caches_swap_condition():
    from k8s_watcher_amd.ops.cache import make_pod_cache
    for native in (False, True):
        cache = make_pod_cache(native)
        assert cache.swap_condition("nobody", 5) == 0 and len(cache) == 0
        cache.observe("ADDED", "u", "1", "Pending", "default", "n")
        assert cache.swap_condition("u", 0) == 0
        assert cache.swap_condition("u", 2 ** 64 - 1) == 0
        assert cache.swap_failure("u", 3) == 0  # its own field: the two do not see each other
        assert cache.swap_condition("u", 7) == 2 ** 64 - 1
        assert cache.swap_failure("u", 0) == 3
        assert cache.swap_condition("u", 0) == 7
        assert cache.get("u")[:5] == ["1", "Pending", "default", "n", None]
        assert cache.to_records() == [["u", "1", "Pending", "default", "n", None]]  # never persisted
        cache.swap_condition("u", 9)
        cache.put("u", "2", "Pending", "default", "n", None)  # a whole new entry
        assert cache.swap_condition("u", 0) == 0


# ----------------------------------------------------------------------------- a pod's life (test 3)

def with_rv(pod, rv):
    p = copy.deepcopy(pod)
    p["metadata"]["resourceVersion"] = str(rv)
    return p


def pending(pod, rv, reason, message):
    p = with_rv(pod, rv)
    p["status"] = {"phase": "Pending", "qosClass": "Burstable", "conditions": [
        {"type": "PodScheduled", "status": "False", "lastProbeTime": None,
         "lastTransitionTime": "2025-07-09T01:%02d:00Z" % rv, "reason": reason, "message": message}]}
    return p


def disrupted(pod, rv):
    p = with_rv(pod, rv)
    p["status"]["conditions"].append(
        {"type": "DisruptionTarget", "status": "True", "lastProbeTime": None, "lastTransitionTime": "2025-07-09T02:00:00Z",
         "reason": "PreemptionByScheduler", "message": "default-scheduler: preempting to accommodate a higher priority pod"})
    return p


def life(seed=61, ns="default"):
    f = PodFactory(seed=seed, namespaces=[ns])
    p0 = f.new_pod()
    sched = f.scheduled(p0)
    run_ = f.running(sched)
    return [
        ("ADDED", pending(p0, 1, "Unschedulable", "0/16 nodes are available: 16 Insufficient amd.com/gpu.")),
        ("MODIFIED", pending(p0, 2, "Unschedulable", "0/16 nodes are available: 15 Insufficient amd.com/gpu, 1 tainted.")),
        ("MODIFIED", pending(p0, 3, "SchedulerError", "binding rejected: timeout")),
        ("MODIFIED", with_rv(sched, 4)),
        ("MODIFIED", with_rv(run_, 5)),
        ("MODIFIED", disrupted(run_, 6)),
        ("MODIFIED", disrupted(run_, 7)),
        ("DELETED", disrupted(run_, 8)),
    ]


def lines(events):
    return b"".join(event_line(t, o) for t, o in events)


RV_EXTRA = {"watcher": {"payload_extra_fields": ["resource_version"]}}  # says which event a notification is


def sent_rvs(calls):
    return [(et, int(core["extra"]["resource_version"])) for _, et, _, _, core in calls]


def check_pod_life():
    events = life()
    for pieces in ([lines(events)], [event_line(t, o) for t, o in events]):  # one read, and one read per event
        # production, the critical filter on
        calls, c, ctrl = both("production", merged(ON, RV_EXTRA), pieces)
        assert ctrl == []
        assert sent_rvs(calls) == [("ADDED", 1), ("MODIFIED", 3), ("MODIFIED", 6), ("DELETED", 8)]
        assert c["events_pod_condition"] == 3 and c["events_filtered_critical"] == 4
        assert c["events_received"] == 8 and c["events_unchanged"] == 0 and c["events_container_failure"] == 0
        assert "pod_condition_alerts" not in json.dumps(calls)
        # the option off: the phase alone decides
        calls, c, _ = both("production", RV_EXTRA, pieces)
        assert sent_rvs(calls) == [("DELETED", 8)]
        assert c["events_pod_condition"] == 0 and c["events_filtered_critical"] == 7
        # notify_on: phase_change without the critical filter: the phase changes as today, the condition events too
        phase = merged(RV_EXTRA, {"watcher": {"notify_on": "phase_change"}})
        off, c_off, _ = both("staging", phase, pieces)
        assert sent_rvs(off) == [("ADDED", 1), ("MODIFIED", 5), ("DELETED", 8)]
        assert c_off["events_unchanged"] == 5 and c_off["events_pod_condition"] == 0
        on, c_on, _ = both("staging", merged(ON, phase), pieces)
        assert sent_rvs(on) == [("ADDED", 1), ("MODIFIED", 3), ("MODIFIED", 5), ("MODIFIED", 6), ("DELETED", 8)]
        assert [x for x in on if x in off] == off
        assert c_on["events_unchanged"] == 3 and c_on["events_pod_condition"] == 2
        assert c_on["events_filtered_critical"] == 0


def test_pod_life_both_engines():
    check_pod_life()


def test_recovery_is_silent_and_a_relapse_alerts_again():
    f = PodFactory(seed=62, namespaces=["default"])
    p0 = f.new_pod()
    sched = f.scheduled(p0)
    events = [("ADDED", pending(p0, 1, "Unschedulable", "a")), ("MODIFIED", with_rv(sched, 2)),
              ("MODIFIED", pending(p0, 3, "Unschedulable", "b")), ("MODIFIED", pending(p0, 4, "Unschedulable", "c"))]
    calls, c, _ = both("production", merged(ON, RV_EXTRA), [lines(events)])
    assert sent_rvs(calls) == [("ADDED", 1), ("MODIFIED", 3)]
    assert c["events_pod_condition"] == 2 and c["events_filtered_critical"] == 2


def test_option_off_is_today():
    """The guard: with both options off, tuples, payloads and counters are what they were."""
    s = settings_for("production", {})
    py = run_engine(s, False, [lines(life())])
    nat = run_engine(s, True, [lines(life())])
    assert py == nat
    calls, c, _ = py
    assert [et for _, et, *_ in calls] == ["DELETED"] and "extra" not in calls[0][4]
    assert c["events_pod_condition"] == 0 and c["events_filtered_critical"] == 7
    for eng in ("python", "native"):
        assert all(len(e) == 9 for e in decoder_for(s, eng).feed(lines(life())))
        only_failures = settings_for("production", alerts(container_failures=True))
        assert all(len(e) == 10 for e in decoder_for(only_failures, eng).feed(lines(life())))
        ev = decoder_for(settings_for("production", ON), eng).feed(lines(life()))
        assert all(len(e) == 11 and e[9] == 0 for e in ev) and [e[10] != 0 for e in ev] == [
            True, True, True, False, False, True, True, False]
        assert ev[0][10] == ev[1][10] != ev[2][10] and ev[5][10] == ev[6][10]


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


# ----------------------------------------------------------------------------- partitioned apply (test 4)

PARTITIONS = 16


def conditions_batch(seed=7):
    """One batch, every pod's lines interleaved with the others': the fewest
    pods (64 at least) that put a pod with five or six lines into every one of
    the 16 partitions; every third pod goes unschedulable -> another message ->
    another reason -> scheduled, the others move on without a finding."""
    from k8s_watcher_amd.ops.native import load
    part = load().apply_partition
    rng = random.Random(seed)
    f = PodFactory(seed=seed, namespaces=["default", "kube-system", "production", "batch", "monitoring"])
    scripts, long_parts = [], set()
    while len(scripts) < 64 or len(long_parts) < PARTITIONS:
        p0 = f.new_pod()
        sched = f.scheduled(p0)
        run_ = f.running(sched)
        if len(scripts) % 3 == 0:
            steps = [("ADDED", lambda rv, p=p0: pending(p, rv, "Unschedulable", "0/16 nodes are available")),
                     ("MODIFIED", lambda rv, p=p0: pending(p, rv, "Unschedulable", "0/16 nodes: 1 tainted")),
                     ("MODIFIED", lambda rv, p=p0: pending(p, rv, "SchedulerError", "binding rejected")),
                     ("MODIFIED", lambda rv, p=sched: with_rv(p, rv)),
                     ("MODIFIED", lambda rv, p=run_: with_rv(p, rv)),
                     ("MODIFIED", lambda rv, p=run_: disrupted(p, rv))]
        else:
            steps = [("ADDED", lambda rv, p=p0: with_rv(p, rv)),
                     ("MODIFIED", lambda rv, p=sched: with_rv(p, rv)),
                     ("MODIFIED", lambda rv, p=run_: with_rv(p, rv)),
                     ("MODIFIED", lambda rv, p=run_: disrupted(p, rv)),
                     ("MODIFIED", lambda rv, p=run_: disrupted(p, rv)),
                     ("DELETED", lambda rv, p=run_: disrupted(p, rv))]
        steps = steps[:rng.choice((4, 5, 6))]
        if len(steps) >= 5:
            long_parts.add(part(p0["metadata"]["uid"]))
        scripts.append(steps)
    out, rv = [], 0
    for k in range(6):
        for steps in scripts:
            if k < len(steps):
                rv += 1
                et, make = steps[k]
                out.append(event_line(et, make(rv)))
    return b"".join(out), len(scripts), len(out)


def feed_one_batch(env, ov, warm, data, partitioned, keep=lambda body: body["status"]["phase"]):
    """As test_partitioned_apply.feed, but `data` is one batch, fed after
    `warm`: a few lines (too few to be partitioned) that teach the cache the
    namespaces and phases, which a partition leaves to the serial path.
    `keep`: what a notification's body is compared by, after uid and type."""
    from conftest import run
    from k8s_watcher_amd.parallel.native_notifier import NativeNotifierPool
    from k8s_watcher_amd.ops.decode import PyDecoder
    from k8s_watcher_amd.ops.native import load
    from k8s_watcher_amd.testing.stub_sink import StubSink

    async def body():
        sink = StubSink()
        await sink.start()
        s = load_settings(env, overrides=dict(ov, clusterapi={"base_url": sink.url, "health_check_on_start": False}),
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
        got = [(x["uid"], x["event_type"], keep(x)) for x in sink.state.payloads()]
        cache = {u: [e[0], e[1], e[2], e[3], json.loads(e[4]) if e[4] else None] for u, e in p.cache.items()}
        counters = {k: v for k, v in m.c.items() if k.startswith(("events_", "bookmarks"))}
        rv = p.native.last_rv()
        await pool.close()
        await sink.stop()
        dpool.close()
        return got, cache, counters, rv, ctrl, probe

    return run(body(), timeout=60)


def warm_up():
    f = PodFactory(seed=8, namespaces=["default", "kube-system", "production", "batch", "monitoring"])
    out = []
    for ns in f.namespaces:
        p0 = f.new_pod(namespace=ns)
        out += [("ADDED", with_rv(p0, 1)), ("MODIFIED", with_rv(f.running(p0), 2))]
    return lines(out)


def check_partitioned_matches_serial():
    from test_partitioned_apply import per_uid
    data, n_pods, n = conditions_batch()
    warm = warm_up()
    assert 64 <= n_pods <= 160 and 4 * n_pods <= n <= 6 * n_pods
    for env, ov in (("production", ON), ("staging", merged(ON, {"watcher": {"notify_on": "phase_change"}})),
                    ("production", BOTH_ON)):
        s_got, s_cache, s_cnt, s_rv, s_ctrl, s_probe = feed_one_batch(env, ov, warm, data, partitioned=False)
        p_got, p_cache, p_cnt, p_rv, p_ctrl, p_probe = feed_one_batch(env, ov, warm, data, partitioned=True)
        assert s_probe.get("partitioned_batches", 0) == 0
        # one partitioned batch, every line of it applied by its partition
        assert p_probe["partitioned_batches"] == 1 and p_probe["lines"] == n and p_probe["tail_serial_lines"] == 0
        assert collections.Counter(p_got) == collections.Counter(s_got)
        assert per_uid(p_got) == per_uid(s_got)  # per pod in stream order
        assert p_cache == s_cache and p_cnt == s_cnt and p_rv == s_rv and p_ctrl == s_ctrl == []
        assert s_cnt["events_pod_condition"] >= n_pods // 3
        # and the serial native apply is the Python engine's verdict
        calls, c, _ = run_engine(settings_for(env, ov), False, [warm, data])
        assert per_uid([(u, et, core["status"]["phase"]) for u, et, _, _, core in calls]) == per_uid(s_got)
        assert {k: v for k, v in s_cnt.items() if k in COUNTERS and v} == {k: v for k, v in c.items() if v}


def test_partitioned_apply_matches_serial_with_conditions():
    check_partitioned_matches_serial()


# ----------------------------------------------------------------------------- relist (test 5)

def check_relist(native):
    from test_native_relist import list_pages, native_relist
    f = PodFactory(seed=71, namespaces=["default"])
    a0, b0, c0 = (f.new_pod() for _ in range(3))
    a, b, c_ = (f.running(p) for p in (a0, b0, c0))
    s = settings_for("production", ON)
    p, rec, m = pipeline(s, native)
    watch = lines([("ADDED", with_rv(a, 1)), ("ADDED", pending(b0, 2, "Unschedulable", "0/16 nodes")),
                   ("ADDED", with_rv(c_, 3))])
    if native:
        p.handle_raw(watch, 0, framed=False)
    else:
        p.handle_batch(p.decoder.feed(watch), 0)
    assert [(u, et) for u, et, *_ in rec.calls] == [(b0["metadata"]["uid"], "ADDED")]
    del rec.calls[:]
    # the gap: a became unschedulable (recreated elsewhere, say), b's resourceVersion moved with the same
    # findings and another message, c only moved on
    listed = [pending(a0, 10, "Unschedulable", "0/16 nodes"), pending(b0, 11, "Unschedulable", "0/16 nodes: 1 tainted"),
              with_rv(c_, 12)]
    if native:
        ctrl, stats = native_relist(p, listed, None)
        assert stats["modified"] == 3
    else:
        _, _, evs = p.decoder.decode_list(list_pages(listed, 10 ** 6)[0])
        assert all(len(e) == 11 for e in evs)
        ctrl = p.reconcile(evs, 0)
    assert ctrl == []
    assert [(u, et) for u, et, *_ in rec.calls] == [(a0["metadata"]["uid"], "MODIFIED")]
    assert m.c["events_pod_condition"] == 2 and m.c["events_filtered_critical"] == 4
    # a silent relist (initial_list: skip) leaves no signature: the pod is reported at its next event
    q, rec2, _ = pipeline(s, native)
    if native:
        native_relist(q, listed, None, notify=False)
    else:
        q.reconcile(q.decoder.decode_list(list_pages(listed, 10 ** 6)[0])[2], 0, notify=False)
    assert rec2.calls == [] and len(q.cache) == 3
    again = lines([("MODIFIED", pending(b0, 20, "Unschedulable", "0/16 nodes"))])
    if native:
        q.handle_raw(again, 0, framed=False)
    else:
        q.handle_batch(q.decoder.feed(again), 0)
    assert [(u, et) for u, et, *_ in rec2.calls] == [(b0["metadata"]["uid"], "MODIFIED")]


@pytest.mark.parametrize("native", [True, False], ids=["native-relist", "python-reconcile"])
def test_relist(native):
    check_relist(native)


# ----------------------------------------------------------------------------- both options on (test 6)

def test_both_options_on():
    from test_container_failures import CLB, UP, died, set_status
    f = PodFactory(seed=81, namespaces=["default"])
    run_ = f.running(f.new_pod())
    crash = set_status(run_, 0, CLB, 1, died(1, "Error"))
    crash2 = set_status(run_, 0, CLB, 2, died(1, "Error"))
    events = [("ADDED", set_status(run_, 1, UP)),
              ("MODIFIED", disrupted(crash, 2)),    # new on both sides: sent once, counted in both
              ("MODIFIED", disrupted(crash, 3)),    # neither is new
              ("MODIFIED", disrupted(crash2, 4)),   # only the container findings changed
              ("MODIFIED", with_rv(crash2, 5)),     # the condition went: nothing
              ("MODIFIED", disrupted(crash2, 6)),   # ... and came back: only the condition signature is new
              ("MODIFIED", disrupted(set_status(run_, 0, UP), 7))]  # the containers recovered: nothing
    for pieces in ([lines(events)], [event_line(t, o) for t, o in events]):
        calls, c, _ = both("production", merged(BOTH_ON, RV_EXTRA), pieces)
        assert sent_rvs(calls) == [("MODIFIED", 2), ("MODIFIED", 4), ("MODIFIED", 6)]
        assert c["events_container_failure"] == 2 and c["events_pod_condition"] == 2
        assert c["events_filtered_critical"] == 4
    # each option alone sees its own side only
    calls, c, _ = both("production", merged(ON, RV_EXTRA), [lines(events)])
    assert sent_rvs(calls) == [("MODIFIED", 2), ("MODIFIED", 6)]
    assert c["events_container_failure"] == 0 and c["events_pod_condition"] == 2
    calls, c, _ = both("production", merged(alerts(container_failures=True), RV_EXTRA), [lines(events)])
    assert sent_rvs(calls) == [("MODIFIED", 2), ("MODIFIED", 4)]
    assert c["events_container_failure"] == 2 and c["events_pod_condition"] == 0


# ----------------------------------------------------------------------------- seeded mutation fuzz (test 7)

FUZZ_RULES = DEFAULT_RULES + ["Ready=False", "ContainersReady=False:ContainersNotReady", "Odd=Trüe:réason \"q\""]
TYPES = ["PodScheduled", "DisruptionTarget", "Ready", "ContainersReady", "Initialized", "Odd", "podscheduled"]
STATUSES = ["True", "False", "Unknown", "false", "Trüe"]
REASONS = ["Unschedulable", "SchedulerError", "PreemptionByScheduler", "ContainersNotReady", "réason \"q\"", "", "x"]
RETYPED = ["null", "true", "false", "0", "-1.5", "[]", "{}", '["False"]', '{"reason":"Unschedulable"}']


def escaped(rng, text):
    """A JSON spelling of the string with some characters written as \\uXXXX."""
    out = []
    for ch in text:
        if rng.random() < 0.3 and ord(ch) < 0x10000:
            out.append("\\u%04x" % ord(ch))
        else:
            out.append(json.dumps(ch, ensure_ascii=False)[1:-1])
    return '"%s"' % "".join(out)


def mutated_conditions(rng, conditions):
    """The conditions as raw JSON text after a few mutations, all of them valid JSON."""
    elems = []
    for cnd in conditions:
        pairs = [[k, json.dumps(v, ensure_ascii=False)] for k, v in cnd.items()]
        for _ in range(rng.randrange(4)):
            k = rng.choice(("type", "status", "reason"))
            m = rng.randrange(7)
            if m == 0:    # drop the field
                pairs = [p for p in pairs if p[0] != k]
            elif m == 1:  # duplicate it, the last value another one
                pairs.append([k, json.dumps(rng.choice({"type": TYPES, "status": STATUSES, "reason": REASONS}[k]),
                                            ensure_ascii=False)])
            elif m == 2:  # retype it
                pairs = [[a, rng.choice(RETYPED)] if a == k else [a, b] for a, b in pairs]
            elif m == 3:  # escape characters of its value
                pairs = [[a, escaped(rng, json.loads(b))] if a == k and b.startswith('"') else [a, b] for a, b in pairs]
            elif m == 4:  # escape characters of its key
                pairs = [[escaped(rng, a)[1:-1], b] if a == k else [a, b] for a, b in pairs]
            elif m == 5:  # another value
                choice = {"type": TYPES, "status": STATUSES, "reason": REASONS}[k]
                pairs = [[a, json.dumps(rng.choice(choice), ensure_ascii=False)] if a == k else [a, b] for a, b in pairs]
            else:         # reorder the fields
                rng.shuffle(pairs)
        elems.append("{%s}" % ",".join('"%s":%s' % (a, b) for a, b in pairs))
    for _ in range(rng.randrange(3)):
        m = rng.randrange(4)
        if m == 0 and elems:
            elems.insert(rng.randrange(len(elems) + 1), rng.choice(elems))  # duplicate an element
        elif m == 1:
            elems.insert(rng.randrange(len(elems) + 1), rng.choice(RETYPED))  # an element that is no object
        elif m == 2 and elems:
            del elems[rng.randrange(len(elems))]
        else:
            rng.shuffle(elems)
    text = "[%s]" % ",".join(elems)
    return rng.choice(RETYPED) if rng.random() < 0.03 else text


def fuzz_lines(n=2000, seed=11):
    rng = random.Random(seed)
    f = PodFactory(seed=seed, namespaces=["default", "batch"])
    out = []
    for i in range(n):
        p0 = f.new_pod()
        pod = (pending(p0, i + 1, rng.choice(REASONS[:3]), "0/16 nodes are available"), f.scheduled(p0),
               f.running(p0), disrupted(f.running(p0), i + 1))[i % 4]
        raw = mutated_conditions(rng, pod["status"]["conditions"])
        pod["status"]["conditions"] = "@COND@"
        text = json.dumps(pod, separators=(",", ":"), ensure_ascii=False).replace('"@COND@"', raw)
        out.append(('{"type":"MODIFIED","object":%s}\n' % text).encode())
    return out


def test_seeded_mutation_fuzz():
    from k8s_watcher_amd.models.findings import condition_findings, condition_rules
    rules = condition_rules(FUZZ_RULES)
    data = fuzz_lines()
    assert len(data) == 2000
    py = make_decoder("python", "staging", extra=CONDITIONS_BIT, conditions=True, condition_rules=FUZZ_RULES)
    nat = make_decoder("native", "staging", extra=CONDITIONS_BIT, conditions=True, condition_rules=FUZZ_RULES)
    a = [py.feed(ln)[0] for ln in data]
    # the mutations keep the lines valid JSON: checked against the Python engine alone, before anything relies on it
    py_invalid = sum(e[0] == "INVALID" for e in a)
    assert py_invalid < 0.10 * len(data), py_invalid
    b = [nat.feed(ln)[0] for ln in data]
    both_invalid = matched = 0
    sig_of = {}
    for ln, ea, eb in zip(data, a, b):
        if eb[0] == "INVALID":
            assert ea[0] == "INVALID", ln
            both_invalid += 1
            continue
        assert ea[0] == eb[0] == "MODIFIED", ln
        want = condition_findings(json.loads(ln)["object"], rules)
        got = json.loads(nat.core(eb))["extra"]["pod_condition_alerts"]
        assert got == want == json.loads(py.core(ea))["extra"]["pod_condition_alerts"], ln
        assert (eb[10] == 0) == (not want) == (ea[10] == 0), ln
        key = json.dumps(want)
        assert sig_of.setdefault(key, eb[10]) == eb[10], ln  # equal findings, equal signature
        matched += bool(want)
    assert both_invalid < 0.10 * len(data)
    assert len(set(sig_of.values())) == len(sig_of)  # other findings, another signature
    assert matched > 400 and len(sig_of) > 30  # the fuzz does reach the rules
    # the same lines through the fused pipelines, filter-first: one sequence of notifications and counters
    ov = merged(ON, alerts(pod_condition_rules=FUZZ_RULES), {"watcher": {"payload_extra_fields": ["pod_condition_alerts"]}})
    for env in ("production", "staging"):
        calls, c, ctrl = both(env, ov, [b"".join(data)])
        assert ctrl == [] and c["events_received"] == 2000
    assert c["events_pod_condition"] == 0 and len(calls) == 2000  # staging: nothing is filtered to begin with


# ----------------------------------------------------------------------------- the counter (test 8)

def test_metric_is_declared_and_exported():
    from k8s_watcher_amd.metrics import COUNTERS as DECLARED
    assert "events_pod_condition" in DECLARED and Metrics().c["events_pod_condition"] == 0
    m = Metrics()
    s = settings_for("production", ON)
    p = EventPipeline(s, decoder_for(s), Recorder(), m)
    p.log_events_setting = False
    p.handle_batch(p.decoder.feed(lines(life())), 0)
    text = m.prometheus_text()  # the body of /metrics
    assert "events_pod_condition" in text
    assert [ln for ln in text.splitlines() if "events_pod_condition" in ln and not ln.startswith("#")][0].endswith(" 3")
