"""The payload pre-filter (ops/csrc/engine.inc, ``payload_prefiltered``):
decode builds no payload for an event the critical filter keeps but the
namespace filter or the shard rule will drop. Nothing observable may move:
with the pre-filter on and off the native engine submits the same bodies,
returns the same control tuples and counts the same — on the partitioned
path, on the serial path with a decode pool and with no pool at all — and
agrees with the Python engine. Only ``_kwcore.apply_stats()`` tells the two
apart (``payload_built`` / ``payload_prefiltered``).
"""

import collections
import copy
import json
import zlib

import pytest

from conftest import run
from k8s_watcher_amd.engine.pipeline import EventPipeline
from k8s_watcher_amd.metrics import Metrics
from k8s_watcher_amd.ops.decode import PyDecoder
from k8s_watcher_amd.ops.native import load
from k8s_watcher_amd.parallel.native_notifier import NativeNotifierPool
from k8s_watcher_amd.testing.podgen import PodFactory, event_line
from k8s_watcher_amd.testing.stub_sink import StubSink
from k8s_watcher_amd.utils.config import load_settings

ENV = "production"  # the critical filter is on there
ALLOWED = ["default", "payments"]  # with the dropped two: one namespace in each of the four shards
DROPPED = ["batch", "kube-system"]
NAMESPACES = ALLOWED + DROPPED
SHARDS = 4
TERMINAL = ("Failed", "Succeeded")


def with_rv(pod, rv, phase=None):
    p = copy.deepcopy(pod)
    p["metadata"]["resourceVersion"] = str(rv)
    if phase is not None:
        p["status"]["phase"] = phase
    return p


def escaped(line: bytes, ns: str) -> bytes:
    """The line with its namespace's first letter written as a \\u escape."""
    plain = b'"namespace":"%s"' % ns.encode()
    assert line.count(plain) == 1
    return line.replace(plain, b'"namespace":"\\u%04x%s"' % (ord(ns[0]), ns[1:].encode()))


def build_corpus():
    """-> (warm, data, rows). `warm`: a few lines (too few for the decode
    pool) that teach the cache every namespace and phase, so the partitions
    of `data` take its lines themselves. `rows`: what the filters see of every
    line of both, in order: (type, namespace | None, uid | None, critical_kept,
    namespace_escaped)."""
    f = PodFactory(seed=31, namespaces=NAMESPACES)
    rows, warm, data = [], [], []
    rv = [100]

    def put(out, etype, pod, esc=False):
        rv[0] += 1
        pod = with_rv(pod, rv[0])
        md = pod["metadata"]
        line = event_line(etype, pod)
        if esc:
            line = escaped(line, md["namespace"])
        status = pod.get("status")
        kept = etype == "DELETED" or status is None or status.get("phase") in TERMINAL
        rows.append((etype, md.get("namespace"), md.get("uid"), kept, esc))
        out.append(line)

    for ns in NAMESPACES:  # Pending, Running and both terminal phases; every namespace
        p = f.new_pod(namespace=ns)
        put(warm, "ADDED", p)
        put(warm, "MODIFIED", f.running(f.scheduled(p)))
    p = f.running(f.new_pod(namespace="default"))
    put(warm, "ADDED", with_rv(p, 0, "Succeeded"))
    put(warm, "MODIFIED", with_rv(p, 0, "Failed"))
    assert len(warm) < 24

    lives = []
    for i in range(36):  # whole lives, nine per namespace: ADDED, 3 x MODIFIED (the last terminal), DELETED
        lives.append(f.lifecycle(NAMESPACES[i % 4], failed=i % 3 == 0))
    for k in range(5):
        for life in lives:
            put(data, *life[k])
    two = f.lifecycle("batch", failed=True) + f.lifecycle("default", failed=False)
    for etype, pod in two:  # two pods' events back to back: several events of one pod in one batch
        put(data, etype, pod)
    for ns in ("default", "batch"):  # no uid: cached under one key, DELETED as well
        p = f.terminated(f.running(f.new_pod(namespace=ns)), failed=True)
        del p["metadata"]["uid"]
        put(data, "ADDED", p)
        put(data, "DELETED", p)
    p = f.terminated(f.running(f.new_pod(namespace="default")))
    del p["metadata"]["namespace"]  # no namespace: never allowed, and not for the pre-filter to say
    put(data, "ADDED", p)
    put(data, "DELETED", p)
    for ns in ("payments", "kube-system"):  # escaped spellings of an allowed and of a dropped namespace
        p = f.running(f.new_pod(namespace=ns))
        put(data, "ADDED", p, esc=True)
        put(data, "MODIFIED", f.terminated(p, failed=True), esc=True)
        put(data, "DELETED", f.terminated(p, failed=True), esc=True)
    bookmark = b'{"type":"BOOKMARK","object":{"kind":"Pod","metadata":{"resourceVersion":"777"}}}\n'
    data.insert(len(data) // 2, bookmark)
    rows.insert(len(warm) + len(data) // 2, ("BOOKMARK", None, None, False, False))
    return b"".join(warm), b"".join(data), rows


CORPUS = {}


def corpus():
    if not CORPUS:
        CORPUS["v"] = build_corpus()
    return CORPUS["v"]


def test_the_corpus_is_what_the_tests_need():
    warm, data, rows = corpus()
    assert 180 <= data.count(b"\n") <= 260 and len(rows) == (warm + data).count(b"\n")
    kinds = collections.Counter(r[0] for r in rows)
    assert set(kinds) == {"ADDED", "MODIFIED", "DELETED", "BOOKMARK"}
    assert {r[1] for r in rows} == set(NAMESPACES) | {None}
    assert any(r[2] is None and r[0] != "BOOKMARK" for r in rows)
    assert {r[1] for r in rows if r[4]} == {"payments", "kube-system"} and b'"\\u0070ayments"' in data
    assert any(r[3] for r in rows) and any(not r[3] and r[0] != "BOOKMARK" for r in rows)
    for key in ("namespace", "uid"):  # every shard gets lines of its own, whichever key
        assert {shard_of(r, key) for r in rows if r[0] != "BOOKMARK"} == set(range(SHARDS))


def shard_of(row, key):
    text = row[2] if key == "uid" else row[1]
    return zlib.crc32((text or "").encode()) % SHARDS


def expected_payloads(rows, namespaces, shard):
    """(built, prefiltered): what decode does about the payloads of the lines
    the critical filter keeps. The pre-filter decides from plain text only:
    an escaped namespace is built, whatever it spells."""
    built = pre = 0
    for row in rows:
        etype, ns, uid, kept, esc = row
        if not kept:
            continue
        drop = bool(namespaces) and ns is not None and not esc and ns not in namespaces
        if shard is not None:
            key, index = shard
            if not (esc and key == "namespace") and shard_of(row, key) != index:
                drop = True
        if drop:
            pre += 1
        else:
            built += 1
    return built, pre


def overrides(namespaces=ALLOWED, shard=None, threads=0):
    w = {"namespaces": list(namespaces), "decode_threads": threads}
    if shard is not None:
        w["shard"] = {"count": SHARDS, "index": shard[1], "key": shard[0]}
    return {"watcher": w}


class Recorder:
    def __init__(self):
        self.calls = []

    def submit(self, uid, et, ns, name, core, read_ns, ts):
        self.calls.append((uid, et, ns, name, bytes(core)))

    def flush(self):
        pass


class Switch:
    """``_kwcore.set_payload_prefilter`` for one run; -> the counters' growth."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.kw = load()
        self.prev = self.kw.set_payload_prefilter(self.on)
        self.before = self.kw.apply_stats()
        return self

    def __exit__(self, *exc):
        after = self.kw.apply_stats()
        self.kw.set_payload_prefilter(self.prev)
        self.stats = {k: after[k] - self.before[k] for k in after}


def run_python(ov, pieces):
    s = load_settings(ENV, overrides=ov, environ={})
    rec, m = Recorder(), Metrics()
    p = EventPipeline(s, PyDecoder(ENV), rec, m)
    p.log_events_setting = False
    ctrl = []
    for data in pieces:
        ctrl += p.handle_batch(p.decoder.feed(data), 0)
    return rec.calls, ctrl, dict(m.c)


def run_serial(ov, pieces, prefilter, workers=0):
    """The native engine handing its submits back to Python: the serial apply,
    on the calling thread alone (workers 0) or behind a decode pool.
    -> (calls with the core's bytes, control tuples, Metrics.c, apply_stats growth)"""
    s = load_settings(ENV, overrides=ov, environ={})
    rec, m = Recorder(), Metrics()
    p = EventPipeline(s, PyDecoder(ENV), rec, m)
    p.log_events_setting = False
    dpool = load().DecodePool(workers) if workers else None
    with Switch(prefilter) as sw:
        p.attach_native(dpool)
        assert p.native.decode_threads() == workers
        ctrl = []
        for data in pieces:
            ctrl += p.handle_raw(data, 0, framed=False)
    if dpool is not None:
        dpool.close()
    return rec.calls, ctrl, dict(m.c), sw.stats, p


def body_key(body: bytes):
    x = json.loads(body)
    x.pop("event_timestamp")  # stamped at submit: the one field that differs from run to run
    return json.dumps(x, sort_keys=True)


def run_partitioned(ov, warm, data, prefilter):
    """The native engine submitting to its native notifier, `data` as one
    partitioned batch. -> (bodies as the sink got them, per pod in order;
    control tuples; Metrics.c; apply_stats growth)"""
    async def body():
        sink = StubSink()
        await sink.start()
        s = load_settings(ENV, overrides=dict(ov, clusterapi={"base_url": sink.url, "health_check_on_start": False}),
                          environ={})
        m = Metrics()
        pool = NativeNotifierPool(s.clusterapi, m)
        p = EventPipeline(s, PyDecoder(ENV), pool, m)
        p.log_events_setting = False
        dpool = load().DecodePool(3)
        with Switch(prefilter) as sw:
            p.attach_native(dpool)
            ctrl = p.handle_raw(warm, 1, framed=False)
            ctrl += p.handle_raw(data, 1, framed=False)
        assert await pool.drain(20)
        got = collections.defaultdict(list)
        for _, b in sink.state.received:
            got[json.loads(b)["uid"]].append(body_key(b))
        counters = {k: v for k, v in m.c.items() if k.startswith(("events_", "bookmarks"))}
        await pool.close()
        await sink.stop()
        dpool.close()
        return dict(got), ctrl, counters, sw.stats

    return run(body(), timeout=60)


def per_uid(calls):
    out = collections.defaultdict(list)
    for uid, et, ns, name, core in calls:
        x = json.loads(core)
        x["event_type"] = et
        out[uid].append(json.dumps(x, sort_keys=True))
    return dict(out)


SHARDINGS = [None] + [(key, i) for key in ("namespace", "uid") for i in range(SHARDS)]
SHARD_IDS = ["unsharded"] + ["%s-%d" % s for s in SHARDINGS[1:]]
RUNS = {}


def serial_runs(shard):
    """Each configuration's four serial runs, made once: (prefilter, workers) -> run_serial's."""
    if shard not in RUNS:
        warm, data, rows = corpus()
        RUNS[shard] = {(on, workers): run_serial(overrides(shard=shard), [warm, data], on, workers)[:4]
                       for on in (True, False) for workers in (0, 3)}
    return RUNS[shard]


@pytest.mark.parametrize("shard", SHARDINGS, ids=SHARD_IDS)
def test_on_and_off_submit_the_same(shard):
    """Bodies byte for byte and in order, control tuples and Metrics.c: the
    same with the pre-filter on and off, with no pool and behind one (the
    batch is over PARALLEL_MIN_LINES and, handing its submits to Python, under
    no partition) — and the Python engine's."""
    warm, data, rows = corpus()
    runs = serial_runs(shard)
    base_calls, base_ctrl, base_c, _ = runs[(False, 0)]
    assert base_ctrl == [] and base_c["bookmarks"] == 1
    for key, (calls, ctrl, c, _) in runs.items():
        assert calls == base_calls and ctrl == base_ctrl and c == base_c, key
    py_calls, py_ctrl, py_c = run_python(overrides(shard=shard), [warm, data])
    assert py_ctrl == base_ctrl and py_c == base_c
    assert [(u, et, ns, nm, json.loads(core)) for u, et, ns, nm, core in py_calls] == [
        (u, et, ns, nm, json.loads(core)) for u, et, ns, nm, core in base_calls]
    # the corpus did what it is for: sends, both filters at work, the escaped allowed namespace sent
    # (sharded by namespace, a shard has the allowed namespaces or the dropped ones)
    if shard is None or shard[0] == "uid":
        assert base_calls and base_c["events_filtered_namespace"] > 0
    else:
        assert bool(base_calls) == (shard[1] in (2, 3)) == (base_c.get("events_filtered_namespace", 0) == 0)
    assert (base_c.get("events_other_shard", 0) > 0) == (shard is not None)
    if shard is None:
        sent_ns = {ns for _, _, ns, _, _ in base_calls}
        assert sent_ns == set(ALLOWED) and any(b'"\\u0070ayments"' in core for *_, core in base_calls)


@pytest.mark.parametrize("shard", SHARDINGS, ids=SHARD_IDS)
def test_partitioned_on_and_off_submit_the_same(shard):
    """One read of over 24 lines to a native notifier: the partitioned path."""
    warm, data, rows = corpus()
    ov = overrides(shard=shard, threads=3)
    kw = load()
    on_got, on_ctrl, on_c, on_stats = run_partitioned(ov, warm, data, True)
    off_got, off_ctrl, off_c, off_stats = run_partitioned(ov, warm, data, False)
    for stats in (on_stats, off_stats):
        # (a sharded watcher learns no namespace from another shard's warm-up lines: a partition
        # stops at the first line of a namespace never seen and leaves its rest to the loop)
        assert stats["partitioned_batches"] == 1 and stats["partitioned_lines"] > (150 if shard is None else 24)
    assert on_got == off_got and on_ctrl == off_ctrl == [] and on_c == off_c
    base_calls, _, base_c, _ = serial_runs(shard)[(False, 0)]
    assert on_got == per_uid(base_calls)
    assert on_c == {k: v for k, v in base_c.items() if k.startswith(("events_", "bookmarks"))}
    built, pre = expected_payloads(rows, ALLOWED, shard)
    assert (on_stats["payload_built"], on_stats["payload_prefiltered"]) == (built, pre)
    assert (off_stats["payload_built"], off_stats["payload_prefiltered"]) == (built + pre, 0)
    assert kw.set_payload_prefilter(True) is True  # the default, and left as found


def test_the_shards_sends_are_the_unsharded_runs_once_each():
    base = collections.Counter(serial_runs(None)[(True, 0)][0])
    assert base
    for key in ("namespace", "uid"):
        union = collections.Counter()
        for i in range(SHARDS):
            mine = collections.Counter(serial_runs((key, i))[(True, 3)][0])
            assert mine or key == "namespace", (key, i)  # (two of the four namespaces are dropped ones)
            union += mine
        assert union == base, key


@pytest.mark.parametrize("workers", [0, 3])
def test_counters(workers):
    warm, data, rows = corpus()
    for shard in (None, ("namespace", 1), ("uid", 2)):
        built, pre = expected_payloads(rows, ALLOWED, shard)
        assert built > 0 and pre > 0
        on, off = (serial_runs(shard)[(flag, workers)][3] for flag in (True, False))
        assert (on["payload_built"], on["payload_prefiltered"]) == (built, pre), shard
        assert (off["payload_built"], off["payload_prefiltered"]) == (built + pre, 0), shard
    # the escaped namespaces are built, the dropped one's too: two critical-kept lines of each
    plain_only = [r for r in rows if not r[4]]
    assert expected_payloads(rows, ALLOWED, None)[0] - expected_payloads(plain_only, ALLOWED, None)[0] == 4
    # no namespace filter and one shard: nothing for the pre-filter to say
    kept = sum(r[3] for r in rows)
    stats = run_serial(overrides(namespaces=[]), [warm, data], True, workers)[3]
    assert (stats["payload_built"], stats["payload_prefiltered"]) == (kept, 0)


# ----------------------------------------------------------------------------- a malformed payload

def malformed_line(f, ns, rv, what):
    """An ADDED in a terminal phase whose filter fields are fine and whose
    payload sub-tree is not JSON: the light parse takes the line."""
    p = with_rv(f.running(f.new_pod(namespace=ns)), rv, "Failed")
    if what == "spec":
        p["spec"]["containers"] = "@BAD@"
    else:
        p["status"][what] = "@BAD@"
    line = event_line("ADDED", p)
    assert line.count(b'"@BAD@"') == 1
    return p["metadata"], line.replace(b'"@BAD@"', b'[{"name" "app"}]')


@pytest.mark.parametrize("what", ["spec", "conditions", "containerStatuses"])
@pytest.mark.parametrize("prefilter", [True, False], ids=["on", "off"])
@pytest.mark.parametrize("path", ["threads0", "pool", "partitioned"])
def test_malformed_payload_subtree(what, prefilter, path):
    """In a dropped namespace the line is no INVALID: it is namespace-filtered
    and the cache takes its resourceVersion and phase. In an allowed one it is
    reported, nothing is sent, and the cache takes them all the same. (The
    parent commit does exactly this; the pre-filter must not move it.)"""
    warm, _, _ = corpus()
    f = PodFactory(seed=77, namespaces=NAMESPACES)
    out_md, out_line = malformed_line(f, "batch", 9001, what)
    in_md, in_line = malformed_line(f, "default", 9002, what)
    filler = [event_line("ADDED", with_rv(f.running(f.new_pod(namespace=NAMESPACES[i % 4])), 9100 + i))
              for i in range(30 if path == "partitioned" else 8)]
    data = b"".join(filler[:4] + [out_line, in_line] + filler[4:])
    if path == "partitioned":
        got, ctrl, c, stats = run_partitioned(overrides(threads=3), warm, data, prefilter)
        assert stats["partitioned_batches"] == 1
        sent = set(got)
    else:
        calls, ctrl, c, stats, p = run_serial(overrides(), [warm, data], prefilter, 3 if path == "pool" else 0)
        sent = {u for u, *_ in calls}
        cache = dict(p.cache.items())
        for md in (out_md, in_md):
            assert list(cache[md["uid"]][:4]) == [md["resourceVersion"], "Failed", md["namespace"], md["name"]]
            assert not cache[md["uid"]][4]
    assert [t[0] for t in ctrl] == ["INVALID"] and in_md["name"].encode() in ctrl[0][8].encode()
    assert out_md["uid"] not in sent and in_md["uid"] not in sent
    n_warm = warm.count(b"\n")
    assert c["events_received"] == n_warm + len(filler) + 2
    assert c["events_filtered_namespace"] == 1  # the dropped one: counted, not reported
    assert stats["payload_prefiltered"] == (1 if prefilter else 0)


# ----------------------------------------------------------------------------- the serial path while workers decode

@pytest.mark.parametrize("n_lines", [6, 12, 23])
def test_first_seen_namespace_while_workers_decode(n_lines):
    """6-23 lines take the decode pool and not the partitions: the loop
    applies line by line — interning a namespace it has never seen — while the
    workers decode the lines after it, of dropped namespaces. A worker that
    read the cache's namespace table there would race with that intern; the
    output is what no pool at all gives."""
    f = PodFactory(seed=55, namespaces=NAMESPACES)
    first = with_rv(f.terminated(f.running(f.new_pod(namespace="default"))), 1)
    lines = [event_line("ADDED", first)]  # an allowed namespace, first seen here: no warm-up
    for i in range(n_lines - 1):
        ns = ("batch", "kube-system", "never-configured-%d" % i)[i % 3]  # dropped ones, first seen as well
        pod = f.terminated(f.running(f.new_pod(namespace=ns)), failed=i % 2 == 0)
        lines.append(event_line("MODIFIED" if i % 4 else "DELETED", with_rv(pod, 2 + i)))
    data = b"".join(lines)
    base = run_serial(overrides(), [data], True, 0)
    for _ in range(5):  # a race shows on some runs only; each is a few milliseconds
        pooled = run_serial(overrides(), [data], True, 3)
        assert pooled[:4] == base[:4]
        assert pooled[3]["serial_batches"] == 1 and pooled[3]["partitioned_batches"] == 0
    assert len(base[0]) == 1 and base[2]["events_filtered_namespace"] == n_lines - 1
    assert (base[3]["payload_built"], base[3]["payload_prefiltered"]) == (1, n_lines - 1)
    assert run_serial(overrides(), [data], False, 3)[:3] == base[:3]


# ----------------------------------------------------------------------------- relist

def test_relist_changed_items_of_a_dropped_namespace():
    """A LIST page whose changed items are all in a dropped namespace: pass 2
    builds no payload, nothing is sent, each is counted as namespace-filtered
    and the cache holds the new resourceVersions."""
    f = PodFactory(seed=91, namespaces=NAMESPACES)
    pods = [f.running(f.new_pod(namespace="batch")) for _ in range(20)]
    known = b"".join(event_line("ADDED", with_rv(p, 100 + i)) for i, p in enumerate(pods[:10]))
    # ten known ones changed (terminal now: the critical filter keeps them), ten new
    items = [with_rv(f.terminated(p, failed=i % 2 == 0), 500 + i) for i, p in enumerate(pods)]
    page = json.dumps({"kind": "PodList", "apiVersion": "v1", "metadata": {"resourceVersion": "999"}, "items": items},
                      separators=(",", ":")).encode()
    results = {}
    for prefilter in (True, False):
        for workers in (0, 3):
            s = load_settings(ENV, overrides=overrides(), environ={})
            rec, m = Recorder(), Metrics()
            p = EventPipeline(s, PyDecoder(ENV), rec, m)
            p.log_events_setting = False
            dpool = load().DecodePool(workers) if workers else None
            with Switch(prefilter) as sw:
                p.attach_native(dpool)
                assert p.handle_raw(known, 0, framed=False) == []
                before = dict(m.c)
                rl = p.native.relist(None, True)
                rl.page(page)
                done, ctrl = False, []
                while not done:
                    done, c = p.native_slice(rl.step, 1e6, 0)
                    ctrl += c
            if dpool is not None:
                dpool.close()
            assert ctrl == [] and rec.calls == []
            assert rl.stats()["modified"] == 10 and rl.stats()["added"] == 10
            assert m.c["events_filtered_namespace"] - before.get("events_filtered_namespace", 0) == 20
            cache = dict(p.cache.items())
            for it in items:
                md = it["metadata"]
                assert list(cache[md["uid"]][:4]) == [md["resourceVersion"], it["status"]["phase"], "batch", md["name"]]
            assert sw.stats["payload_prefiltered"] == (20 if prefilter else 0)
            assert sw.stats["payload_built"] == (0 if prefilter else 20)
            results[(prefilter, workers)] = (dict(m.c), sorted((u, list(e[:4])) for u, e in cache.items()))
    assert len({json.dumps(v, sort_keys=True) for v in results.values()}) == 1
