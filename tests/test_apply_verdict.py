"""One apply verdict from three engines: the Python engine, the native serial
apply (``apply_line``) and the native partitioned apply (``apply_par`` and the
loop thread's tail), ops/csrc/engine.inc.

One stream holds every situation the filters tell apart — phases, both alert
signatures through new / repeated / changed / cleared, deletes, foreign
namespaces and shards — plus a counted set of lines only the serial path
takes. It runs under a pairwise-covering set of the filter options; serial
and partitioned must agree on notifications, cache, counters, control events
and the resume point, and the Python engine on notifications and counters.
"""

import collections
import itertools
import json
import zlib

import pytest

from k8s_watcher_amd.testing.podgen import PodFactory, event_line
from test_container_failures import CLB, UP, died, set_status
from test_partitioned_apply import per_uid
from test_pod_condition_alerts import (COUNTERS, disrupted, feed_one_batch, merged, pending, run_engine, settings_for,
                                       with_rv)

ENV = "production"  # the critical filter exists there alone; every option below is set explicitly
WARM_NS = ["default", "kube-system", "production", "batch", "monitoring"]
NS_SET = ["default", "production", "monitoring"]  # watcher.namespaces, when set: batch and kube-system are outside
SHARDS = 2
NONE_UID = "\0<none>"  # the key a pod without metadata.uid is cached under (podcache.inc)
EXTRA = {"watcher": {"payload_extra_fields": ["resource_version", "container_failures", "pod_condition_alerts"]}}


def crc(text):
    return zlib.crc32(text.encode()) % SHARDS


MINE = crc("default")  # this watcher's shard index: the one "default" falls in


def named(prefix):
    """The first prefix-N that falls in this watcher's shard, as a namespace and as a uid alike."""
    return next(t for t in ("%s-%d" % (prefix, i) for i in range(64)) if crc(t) == MINE)


# ----------------------------------------------------------------------------- the options

OPTIONS = collections.OrderedDict([
    ("critical", (True, False)),
    ("notify_on", ("phase_change", "all")),
    ("namespaces", ("set", "none")),
    ("shard", ("namespace", "uid", "none")),
    ("alerts", ("both", "failures", "conditions", "none")),
])
ALL_ON = (True, "phase_change", "set", "namespace", "both")


def pairs_of(cfg):
    return {((i, a), (j, b)) for (i, a), (j, b) in itertools.combinations(enumerate(cfg), 2)}


def covering_configs():
    """ALL_ON first, then greedily the configuration that covers the most
    pairs of option values not yet seen together, until none is left."""
    product = list(itertools.product(*OPTIONS.values()))
    todo = set().union(*(pairs_of(c) for c in product))
    out = [ALL_ON]
    todo -= pairs_of(ALL_ON)
    while todo:
        best = max(product, key=lambda c: len(pairs_of(c) & todo))  # max keeps the first of equals: deterministic
        out.append(best)
        todo -= pairs_of(best)
    return out


CONFIGS = covering_configs()


def overrides(cfg):
    critical, notify_on, namespaces, shard, alerts = cfg
    w = {"notify_on": notify_on, "namespaces": NS_SET if namespaces == "set" else [],
         "alerts": {"critical_events_only": critical, "container_failures": alerts in ("both", "failures"),
                    "pod_conditions": alerts in ("both", "conditions")}}
    if shard != "none":
        w["shard"] = {"count": SHARDS, "index": MINE, "key": shard}
    return merged(EXTRA, {"watcher": w})


def test_configurations_cover_every_pair():
    assert CONFIGS[0] == ALL_ON and len(CONFIGS) == len(set(CONFIGS)) <= 24
    seen = set().union(*(pairs_of(c) for c in CONFIGS))
    keys = list(OPTIONS.values())
    for i, j in itertools.combinations(range(len(keys)), 2):
        for a in keys[i]:
            for b in keys[j]:
                assert ((i, a), (j, b)) in seen, (i, a, j, b)
    s = settings_for(ENV, overrides(ALL_ON)).watcher
    assert s.critical_events_only and s.notify_on == "phase_change" and s.namespaces == NS_SET
    assert s.container_failures and s.pod_conditions


# ----------------------------------------------------------------------------- the stream

def no_status(pod, rv):
    p = with_rv(pod, rv)
    del p["status"]
    return p


def phase(pod, rv, ph):
    p = with_rv(pod, rv)
    p["status"]["phase"] = ph
    return p


def scripts_for(f, ns, far_ns):
    """Per-pod scripts, a list of (type, rv -> pod) each, for pods in `ns`
    (two of them in `far_ns`, outside watcher.namespaces). Between them: every
    situation the filters tell apart on a line a partition can take."""
    def pod(namespace=ns):
        p0 = f.new_pod(namespace=namespace)
        return p0, f.scheduled(p0), f.running(p0)

    out = []
    p0, sched, run_ = pod()  # phases: ADDED non-terminal, same phase, new phase, no status, terminal, DELETED known
    out.append([("ADDED", lambda rv, p=p0: with_rv(p, rv)), ("MODIFIED", lambda rv, p=sched: with_rv(p, rv)),
                ("MODIFIED", lambda rv, p=run_: with_rv(p, rv)), ("MODIFIED", lambda rv, p=run_: no_status(p, rv)),
                ("MODIFIED", lambda rv, p=run_: phase(p, rv, "Succeeded")),
                ("DELETED", lambda rv, p=run_: phase(p, rv, "Succeeded"))])
    p0, sched, run_ = pod()  # ADDED with a terminal phase
    out.append([("ADDED", lambda rv, p=run_: phase(p, rv, "Failed")), ("MODIFIED", lambda rv, p=run_: phase(p, rv, "Failed")),
                ("DELETED", lambda rv, p=run_: phase(p, rv, "Failed"))])
    p0, sched, run_ = pod()  # a failure signature: new, repeated, changed, cleared, and the same findings again (new: the clear was kept)
    out.append([("ADDED", lambda rv, p=run_: set_status(p, rv, UP)),
                ("MODIFIED", lambda rv, p=run_: set_status(p, rv, CLB, 1, died(1, "Error"))),
                ("MODIFIED", lambda rv, p=run_: set_status(p, rv, CLB, 1, died(1, "Error"))),
                ("MODIFIED", lambda rv, p=run_: set_status(p, rv, UP, 2, died(137, "OOMKilled"))),
                ("MODIFIED", lambda rv, p=run_: set_status(p, rv, UP)),
                ("MODIFIED", lambda rv, p=run_: set_status(p, rv, UP, 2, died(137, "OOMKilled")))])
    p0, sched, run_ = pod()  # a condition signature: new (on ADDED), repeated, changed, cleared, the same again, another
    out.append([("ADDED", lambda rv, p=p0: pending(p, rv, "Unschedulable", "0/16 nodes are available")),
                ("MODIFIED", lambda rv, p=p0: pending(p, rv, "Unschedulable", "0/16 nodes: 1 tainted")),
                ("MODIFIED", lambda rv, p=p0: pending(p, rv, "SchedulerError", "binding rejected")),
                ("MODIFIED", lambda rv, p=sched: with_rv(p, rv)),
                ("MODIFIED", lambda rv, p=run_: with_rv(p, rv)),
                ("MODIFIED", lambda rv, p=p0: pending(p, rv, "SchedulerError", "binding rejected again")),
                ("MODIFIED", lambda rv, p=run_: disrupted(p, rv))])
    p0, sched, run_ = pod()  # both signatures new on one line, neither, one, the other, DELETED with findings
    crash, crash2 = set_status(run_, 0, CLB, 1, died(1, "Error")), set_status(run_, 0, CLB, 2, died(1, "Error"))
    out.append([("ADDED", lambda rv, p=run_: set_status(p, rv, UP)), ("MODIFIED", lambda rv, p=crash: disrupted(p, rv)),
                ("MODIFIED", lambda rv, p=crash: disrupted(p, rv)), ("MODIFIED", lambda rv, p=crash2: disrupted(p, rv)),
                ("MODIFIED", lambda rv, p=crash2: with_rv(p, rv)), ("MODIFIED", lambda rv, p=crash2: disrupted(p, rv)),
                ("DELETED", lambda rv, p=crash2: disrupted(p, rv))])
    p0, sched, run_ = pod()  # DELETED of a pod never seen
    out.append([("DELETED", lambda rv, p=run_: with_rv(p, rv))])
    p0, sched, run_ = pod(far_ns)  # a pod outside watcher.namespaces
    out.append([("ADDED", lambda rv, p=p0: with_rv(p, rv)), ("MODIFIED", lambda rv, p=run_: with_rv(p, rv)),
                ("MODIFIED", lambda rv, p=run_: phase(p, rv, "Failed")), ("DELETED", lambda rv, p=run_: phase(p, rv, "Failed"))])
    p0, sched, run_ = pod(far_ns)  # outside watcher.namespaces AND a new signature: namespace-filtered, no alert
    out.append([("ADDED", lambda rv, p=run_: set_status(p, rv, UP)),
                ("MODIFIED", lambda rv, p=run_: disrupted(set_status(p, 0, CLB, 1, died(1, "Error")), rv)),
                ("MODIFIED", lambda rv, p=run_: pending(p, rv, "Unschedulable", "evicted and waiting"))])
    return out


def serial_only_lines():
    """(kind, bytes): "serial" lines no partition takes, "bail" lines a
    partition stops at, "plain" lines that belong with them. The pods of the
    bail lines are in this watcher's shard whichever key it shards by."""
    f = PodFactory(seed=17, namespaces=["default"])
    out = []
    nouid = f.running(f.new_pod())
    del nouid["metadata"]["uid"]  # cached under NONE_UID: a partition takes it (shard_of its hash)
    out.append(("plain", None, event_line("ADDED", phase(nouid, 7001, "Failed"))))
    out.append(("plain", None, event_line("DELETED", phase(nouid, 7002, "Failed"))))
    esc = f.running(f.new_pod())
    esc["metadata"]["uid"] = "esc@-uid"
    for i, et in enumerate(("ADDED", "MODIFIED")):  # the uid written with an escape
        raw = event_line(et, phase(esc, 7010 + i, "Failed" if i else "Running")).replace(b"esc@-uid", b"esc\\u0041-uid")
        out.append(("serial", "escA-uid", raw))
    late_ns = named("late-ns")  # a namespace first seen mid-batch: its first line and all that follow in its partition
    late = f.running(f.new_pod(namespace=late_ns))
    late["metadata"]["uid"] = named("late-uid")
    out.append(("bail", late["metadata"]["uid"], event_line("ADDED", with_rv(late, 7020))))
    out.append(("plain", late["metadata"]["uid"], event_line("MODIFIED", phase(late, 7021, "Succeeded"))))
    out.append(("serial", None, b'{"type":"BOOKMARK","object":{"kind":"Pod","metadata":{"resourceVersion":"7030"}}}\n'))
    out.append(("serial", None, b'{"type":"ERROR","object":{"kind":"Status","code":500,"message":"boom"}}\n'))
    out.append(("serial", None, b"\xff\xfe these are not json\n"))
    # filter fields valid (an ADDED in a terminal phase, in "default", in this shard: every filter
    # keeps it), containerStatuses malformed: the cache is updated, INVALID reported, nothing sent
    bad = phase(f.running(f.new_pod(namespace="default")), 7040, "Failed")
    bad["metadata"]["uid"] = named("bad-cs")
    bad["status"]["containerStatuses"] = "@CS@"
    raw = event_line("ADDED", bad).replace(b'"@CS@"', b'[{"name" "app"}]')
    out.append(("bail", bad["metadata"]["uid"], raw))
    return out, bad["metadata"], late_ns


def build_stream():
    from k8s_watcher_amd.ops.native import load
    part = load().apply_partition
    f = PodFactory(seed=23, namespaces=WARM_NS)
    scripts = []
    for rep in range(8):  # every script in several namespaces and partitions
        scripts += scripts_for(f, WARM_NS[rep % len(WARM_NS)], ("batch", "kube-system")[rep % 2])
    rows, rv = [], 100
    for k in range(max(len(s) for s in scripts)):
        for s in scripts:
            if k < len(s):
                rv += 1
                et, make = s[k]
                pod = make(rv)
                rows.append(("plain", pod["metadata"]["uid"], event_line(et, pod)))
    special, bad_meta, late_ns = serial_only_lines()
    step = len(rows) // (len(special) + 2)  # spread over the batch, in their own order
    for i, row in enumerate(special):
        rows.insert((i + 1) * step + i, row)
    # the fallback rule: a partition stops at the first line it cannot take, and the loop
    # thread applies that line and every later one of the same partition, with the lines no
    # partition takes at all
    expect_serial, stopped = 0, set()
    for kind, uid, _ in rows:
        p = None if kind == "serial" else part(NONE_UID if uid is None else uid)
        if kind == "bail":
            stopped.add(p)
        if p is None or p in stopped:
            expect_serial += 1
    n_special = sum(kind != "plain" for kind, _, _ in special)
    return b"".join(r[2] for r in rows), len(rows), expect_serial, n_special, bad_meta, late_ns


def warm_lines():
    """Twelve lines, too few to be partitioned: a pod in each namespace, its
    uid in this watcher's shard (a line of another shard teaches the cache
    nothing), through Pending and Running, and the two terminal phases."""
    f = PodFactory(seed=9, namespaces=WARM_NS)
    out = []
    for ns in WARM_NS:
        p0 = f.new_pod(namespace=ns)
        p0["metadata"]["uid"] = named("warm-" + ns)
        out += [event_line("ADDED", with_rv(p0, 1)), event_line("MODIFIED", with_rv(f.running(p0), 2))]
    run_ = f.running(f.new_pod(namespace="default"))
    run_["metadata"]["uid"] = named("warm-terminal")
    out += [event_line("ADDED", phase(run_, 3, "Succeeded")), event_line("MODIFIED", phase(run_, 4, "Failed"))]
    return b"".join(out)


STREAM = {}


def the_stream():
    if not STREAM:
        STREAM["v"] = (warm_lines(),) + build_stream()
    return STREAM["v"]


def test_the_stream_is_what_the_test_needs():
    warm, data, n, expect_serial, n_special, bad_meta, late_ns = the_stream()
    assert warm.count(b"\n") < 24 and 200 <= n <= 600
    assert late_ns not in WARM_NS and crc(late_ns) == MINE and crc(bad_meta["uid"]) == MINE
    assert n_special == 7 and n_special <= expect_serial < n // 4  # the fallback adds a partition's rest, not the batch


# ----------------------------------------------------------------------------- the three engines

def alert_fields(body):
    x = body["extra"]
    return (int(x["resource_version"]), json.dumps(x["container_failures"], sort_keys=True),
            json.dumps(x["pod_condition_alerts"], sort_keys=True))


def feed_native(ov, warm, data, partitioned):
    return feed_one_batch(ENV, ov, warm, data, partitioned, keep=lambda x: (x["status"]["phase"],) + alert_fields(x))


@pytest.mark.parametrize("cfg", CONFIGS, ids=["-".join(str(v) for v in c) for c in CONFIGS])
def test_three_engines_one_verdict(cfg):
    warm, data, n, expect_serial, n_special, bad_meta, late_ns = the_stream()
    ov = overrides(cfg)
    critical, notify_on, namespaces, shard, alerts = cfg
    s_got, s_cache, s_cnt, s_rv, s_ctrl, s_probe = feed_native(ov, warm, data, partitioned=False)
    p_got, p_cache, p_cnt, p_rv, p_ctrl, p_probe = feed_native(ov, warm, data, partitioned=True)
    # the partitioned run was one: one batch, and only the lines the fallback rule names went serial
    assert s_probe.get("partitioned_batches", 0) == 0
    assert p_probe["partitioned_batches"] == 1 and p_probe["lines"] == n
    assert p_probe["tail_serial_lines"] == expect_serial
    # serial and partitioned: every item
    assert collections.Counter(p_got) == collections.Counter(s_got)
    assert per_uid(p_got) == per_uid(s_got)
    assert p_cache == s_cache
    assert p_cnt == s_cnt
    assert p_ctrl == s_ctrl and sorted(s_ctrl) == ["ERROR", "INVALID", "INVALID"]
    assert p_rv == s_rv and s_rv
    # the malformed line: cached with its resourceVersion and phase, without a core, never sent
    assert s_cache[bad_meta["uid"]] == ["7040", "Failed", "default", bad_meta["name"], None]
    assert bad_meta["uid"] not in per_uid(s_got)
    # the Python engine: notifications and counters
    calls, c, py_ctrl = run_engine(settings_for(ENV, ov), False, [warm, data])
    py_got = [(core["uid"], et, (core["status"]["phase"],) + alert_fields(core)) for _, et, _, _, core in calls]
    assert per_uid(py_got) == per_uid(s_got)
    # (the malformed line is one event to the native engine, whose filter fields it could read;
    # json.loads refuses the whole line before the Python engine counts anything)
    assert {k: v for k, v in s_cnt.items() if k in COUNTERS and v} == {
        k: v + (k == "events_received") for k, v in c.items() if v}
    assert sorted(py_ctrl) == sorted(s_ctrl)
    # the stream reached what it was built for
    assert c["bookmarks"] == 1 and len(s_got) > 0
    assert (c["events_filtered_critical"] > 0) == critical
    assert (c["events_unchanged"] > 0) == (notify_on == "phase_change")
    assert (c["events_filtered_namespace"] > 0) == (namespaces == "set")
    assert (c["events_other_shard"] > 0) == (shard != "none")
    filtering = critical or notify_on == "phase_change"  # an alert is counted when only its signature let the event pass
    assert (c["events_container_failure"] > 0) == (alerts in ("both", "failures") and filtering)
    assert (c["events_pod_condition"] > 0) == (alerts in ("both", "conditions") and filtering)
    if namespaces == "set":  # wrong namespace and a new signature: filtered, not an alert
        assert calls and all(ns in NS_SET for _, _, ns, _, _ in calls)
