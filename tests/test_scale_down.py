"""Scaling the sharded StatefulSet down, and in its rolling order: whole
services against a fake API server and a stub clusterapi, sharing one
hand-over directory (engine/handover.py, parallel/shard.py). A removed
ordinal never starts under the new count; what it wrote as it shut down — a
parting record per namespace, then its manifest — is what its namespaces' new
owners start from, without waiting out ``handover_wait_seconds``. The
protocol's unit tests are in test_parting.py."""

import asyncio
import collections
import json
import os
import time

from conftest import run
from k8s_watcher_amd.parallel.shard import shard_of
from k8s_watcher_amd.testing.fake_apiserver import FakeApiServer
from k8s_watcher_amd.testing.podgen import PodFactory
from k8s_watcher_amd.testing.stub_sink import StubSink
from k8s_watcher_amd.utils.config import load_settings

SYNC_BOUND = 5.0  # a namespace is watched by its new owner this long after that owner's start(), at the latest
WAIT = 20.0       # shard.handover_wait_seconds: what a new owner without a record sits through


def _shard_settings(sink, i, count, hdir, ck=None, assignment="hash", wait=WAIT, retry_delay=None, engine="native"):
    cl = {"base_url": sink.url, "health_check_on_start": False}
    if retry_delay is not None:
        cl["retry"] = {"delay_seconds": retry_delay, "max_attempts": 1000, "max_delay_seconds": retry_delay}
    w = {"namespace_scope": "discover", "engine": engine,
         "shard": {"count": count, "index": i, "assignment": assignment, "handover_dir": hdir,
                   "handover_wait_seconds": wait},
         "retry": {"delay_seconds": 0.05, "max_attempts": 0}}
    if ck:
        w["checkpoint"] = {"path": ck, "interval_seconds": 3600}
    return load_settings("staging", overrides={"clusterapi": cl, "watcher": w})


def _moves(old_count, new_count, per=2):
    """``{(old owner, new owner): [namespaces]}`` with ``per`` namespaces for
    every way a namespace can go between the two counts (``hash``
    assignment): twelve namespaces between two and three shards."""
    out = collections.defaultdict(list)
    for n in (f"ns-{i}" for i in range(400)):
        key = (shard_of(n, old_count), shard_of(n, new_count))
        if len(out[key]) < per:
            out[key].append(n)
    assert len(out) == old_count * new_count and all(len(v) == per for v in out.values())
    return dict(out)


class World:
    """The API server, the sink and the shards of one test."""

    def __init__(self, tmp_path, nss, engine="native", pods_per_namespace=4, seed=31):
        self.tmp, self.nss, self.engine = tmp_path, list(nss), engine
        self.hdir = str(tmp_path / "handover")
        self.per, self.seed = pods_per_namespace, seed
        self.running = []
        self.want = collections.Counter()  # (uid, event type) the sink is to hold, each exactly once

    async def open(self):
        from k8s_watcher_amd.kube.kubeconfig import KubeEndpoint
        self.srv = FakeApiServer(namespaces=self.nss)
        await self.srv.start()
        self.sink = StubSink()
        await self.sink.start()
        self.ep = KubeEndpoint(server=self.srv.url)
        self.f = PodFactory(seed=self.seed, namespaces=self.nss)
        self.pods = [self.create(ns) for ns in self.nss for _ in range(self.per)]
        return self

    async def close(self):
        for svc in list(self.running):
            await self.stop(svc)
        await self.sink.stop()
        await self.srv.stop()

    # -- the cluster
    def of(self, ns, skip=0):
        return [p for p in self.pods if p["metadata"]["namespace"] == ns][skip]

    def create(self, ns):
        pod = self.srv.create(self.f.running(self.f.new_pod(namespace=ns)))
        self.want[(pod["metadata"]["uid"], "ADDED")] += 1
        return pod

    def modify(self, pod):
        self.srv.update(self.f.terminated(pod))
        self.want[(pod["metadata"]["uid"], "MODIFIED")] += 1

    def delete(self, pod):
        self.srv.delete(pod["metadata"]["namespace"], pod["metadata"]["name"])
        self.pods.remove(pod)
        self.want[(pod["metadata"]["uid"], "DELETED")] += 1

    def got(self):
        return collections.Counter((p["uid"], p["event_type"]) for p in self.sink.state.payloads())

    async def delivered(self, timeout=10.0):
        """Everything wanted has arrived (or ``timeout`` passed), and what follows it had its time."""
        end = time.monotonic() + timeout
        while self.sink.state.count < sum(self.want.values()) and time.monotonic() < end:
            await asyncio.sleep(0.02)
        await asyncio.sleep(0.4)

    # -- the shards
    def shard(self, i, count, **kw):
        from k8s_watcher_amd.engine.service import WatcherService
        from k8s_watcher_amd.metrics import Metrics
        svc = WatcherService(_shard_settings(self.sink, i, count, self.hdir, str(self.tmp / f"ck{i}.bin"),
                                             engine=self.engine, **kw), endpoint=self.ep, metrics=Metrics())
        svc.index, svc.count = i, count
        return svc

    def owned(self, svc):
        return [n for n in self.nss if shard_of(n, svc.count) == svc.index]

    async def start(self, svc, limit=SYNC_BOUND + 1.0):
        """Start ``svc``; the seconds from then until every namespace it owns has
        a synced watch on it, or None if some had none after ``limit``."""
        t0 = time.monotonic()
        self.running.append(svc)
        await svc.start()
        while time.monotonic() - t0 < limit:
            if all(any(r.namespace == n and r.synced.is_set() for r in svc.reflectors) for n in self.owned(svc)):
                return time.monotonic() - t0
            await asyncio.sleep(0.02)
        return None

    async def stop(self, svc, drain=5.0):
        self.running.remove(svc)
        if drain >= 1:
            await svc.notifier.drain(drain)
        svc.stop()
        await svc.shutdown(drain_timeout=drain)

    def owners(self):
        return {r.namespace: svc.index for svc in self.running for r in svc.reflectors}

    def counted(self, name):
        return sum(svc.metrics.c.get(name, 0) for svc in self.running)

    def manifest(self, i):
        try:
            with open(os.path.join(self.hdir, f"shard-{i}.parted.json")) as f:
                return json.load(f)
        except OSError:
            return {}

    def records_left(self):
        return sorted(x for x in os.listdir(self.hdir) if x.endswith((".parting.json", ".handover.json")))


async def _three_to_two(w, owed=False):
    """Three shards sync and shut down gracefully; while all are down a pod of
    one of shard 2's namespaces is deleted and one of another is modified; two
    shards start under count 2. With ``owed``, clusterapi answers 503 to a
    MODIFIED of a third pod of shard 2's as it goes down, and its drain is cut
    short. Returns what (a) asserts of it."""
    held = [n for n in w.nss if shard_of(n, 3) == 2]
    assert len(held) >= 3
    old = [w.shard(i, 3, retry_delay=30 if i == 2 and owed else None) for i in range(3)]
    for svc in old:
        assert await w.start(svc) is not None
    await w.delivered()
    assert w.got() == w.want
    late = w.of(held[2])
    if owed:
        w.sink.state.down = True
        w.modify(late)
        for _ in range(500):
            if old[2].metrics.c["notify_retried"] >= 1:
                break
            await asyncio.sleep(0.01)
        await w.stop(old[2], drain=0.2)  # not drained: the MODIFIED is in its checkpoint and its parting record
        w.sink.state.down = False
    for svc in list(w.running):
        await w.stop(svc)
    listed = {i: w.manifest(i).get("namespaces") for i in range(3)}
    w.delete(w.of(held[0]))
    w.modify(w.of(held[1]))
    new = [w.shard(i, 2) for i in range(2)]
    first = asyncio.ensure_future(w.start(new[1]))
    await asyncio.sleep(0.3)
    took = [await w.start(new[0]), await first]
    await w.delivered(timeout=10 if None not in took else 2)
    return {"held": held, "listed": listed, "took": took, "new": new, "late": late}


def _three_to_two_problems(w, res):
    held, problems = res["held"], []
    if w.got() != w.want:
        extra, missing = w.got() - w.want, w.want - w.got()
        problems.append(f"sink: {sum(extra.values())} notification(s) too many {sorted(extra.items())[:4]}, "
                        f"{sum(missing.values())} missing {sorted(missing.items())[:4]}")
    for i, secs in enumerate(res["took"]):
        if secs is None or secs >= SYNC_BOUND:
            problems.append(f"shard {i} of 2: its namespaces not all watched {SYNC_BOUND:g}s after its start ({secs})")
    if w.counted("shard_handover_timeouts") != 0:
        problems.append(f"shard_handover_timeouts == {w.counted('shard_handover_timeouts')}")
    if w.counted("shard_partings_in") != len(held):
        problems.append(f"shard_partings_in == {w.counted('shard_partings_in')}, shard 2 held {len(held)}")
    if w.counted("shard_parting_missing") != 0:
        problems.append(f"shard_parting_missing == {w.counted('shard_parting_missing')}")
    if res["listed"][2] != sorted(held):
        problems.append(f"shard 2's manifest lists {res['listed'][2]}, it held {sorted(held)}")
    if w.records_left():
        problems.append(f"records left in the directory: {w.records_left()}")
    if w.owners() != {n: shard_of(n, 2) for n in w.nss}:
        problems.append(f"owners: {w.owners()}")
    return problems


def _twelve():
    return sorted(n for names in _moves(3, 2).values() for n in names)


def test_three_to_two_hands_the_removed_shards_namespaces_over(tmp_path, engine="native"):
    """(a) No live pod is re-ADDED, the deletion and the change made while every
    shard was down arrive exactly once, and nothing waits for a record that
    cannot come: every namespace is watched by its new owner within
    ``SYNC_BOUND`` of that owner's start, with ``handover_wait_seconds`` at 20."""
    async def body():
        w = await World(tmp_path, _twelve(), engine=engine).open()
        try:
            return _three_to_two_problems(w, await _three_to_two(w))
        finally:
            await w.close()

    assert run(body(), timeout=120) == []


def test_three_to_two_carries_the_removed_shards_owed_notification(tmp_path):
    """(b) The MODIFIED clusterapi refused while shard 2 went down arrives once,
    from the namespace's new owner, before that owner's own notification for
    the same pod."""
    async def body():
        w = await World(tmp_path, _twelve()).open()
        try:
            res = await _three_to_two(w, owed=True)
            problems = _three_to_two_problems(w, res)
            uid = res["late"]["metadata"]["uid"]
            w.delete(res["late"])
            await w.delivered()
            mine = [(p["event_type"], p["status"]["phase"]) for p in w.sink.state.payloads() if p["uid"] == uid]
            resent = [svc.metrics.c["checkpoint_owed_resent"] for svc in res["new"]]
            return problems, mine, resent, shard_of(res["late"]["metadata"]["namespace"], 2), w.got() == w.want
        finally:
            await w.close()

    problems, mine, resent, dst, exact = run(body(), timeout=120)
    assert problems == []
    assert mine == [("ADDED", "Running"), ("MODIFIED", "Succeeded"), ("DELETED", "Succeeded")], mine
    assert resent[dst] == 1 and sum(resent) == 1 and exact


def test_three_to_two_and_back_discards_the_returning_shards_checkpoint(tmp_path):
    """(e) Ordinal 2 comes back under count 3 with the checkpoint of before it
    was removed, an owed MODIFIED in it: what other shards took over meanwhile
    is not its to say any more. Nothing of it is sent again."""
    async def body():
        w = await World(tmp_path, _twelve()).open()
        try:
            res = await _three_to_two(w, owed=True)
            problems = _three_to_two_problems(w, res)
            w.modify(w.of(res["held"][0]))  # its interim owner reports it; ordinal 2's checkpoint knows the pod as it was
            await w.delivered()
            for svc in list(w.running):
                await w.stop(svc)
            back = [w.shard(i, 3) for i in range(3)]
            starts = [asyncio.ensure_future(w.start(back[2]))]  # with its gains still to come from 0 and 1
            await asyncio.sleep(0.3)
            starts += [asyncio.ensure_future(w.start(svc)) for svc in back[:2]]  # each gains from the other
            took = await asyncio.gather(*starts)
            w.delete(w.of(res["held"][1], skip=1))
            await w.delivered()
            return (problems, took, w.got() == w.want, (w.got() - w.want, w.want - w.got()), w.owners(),
                    back[2].metrics.c["checkpoint_owed_resent"], w.counted("shard_handover_timeouts"),
                    w.records_left(), os.path.exists(os.path.join(w.hdir, "shard-2.parted.json")))
        finally:
            await w.close()

    problems, took, exact, diff, owners, resent, timeouts, left, manifest = run(body(), timeout=120)
    assert problems == []
    assert exact, diff
    assert None not in took and resent == 0 and timeouts == 0
    assert owners == {n: shard_of(n, 3) for n in _twelve()}
    assert left == [] and not manifest


def test_rolling_two_to_three_in_the_statefulsets_order(tmp_path):
    """(c) A rolling update from two shards to three: the new ordinal 2 starts
    while 0 and 1 still run under count 2, then 1 is replaced, then 0. Pods
    come, change and go in the namespaces that move, between the steps."""
    moves = _moves(2, 3)
    nss = sorted(n for names in moves.values() for n in names)

    async def body():
        w = await World(tmp_path, nss, pods_per_namespace=3).open()
        try:
            old = [w.shard(i, 2) for i in range(2)]
            for svc in old:
                assert await w.start(svc) is not None
            await w.delivered()
            new2 = w.shard(2, 3)
            await w.start(new2, limit=0.5)  # everything it owns is another's until that one restarts
            w.create(moves[(0, 2)][0])      # reported by the old owners, still watching
            w.modify(w.of(moves[(1, 2)][0]))
            await w.delivered()
            assert w.got() == w.want
            await w.stop(old[1])
            w.delete(w.of(moves[(1, 2)][0], skip=1))  # nobody watches: new 2's reconcile, after new 1's record
            w.create(moves[(1, 0)][0])                  # ... new 0's, two steps on
            w.modify(w.of(moves[(1, 1)][0]))            # ... new 1's resumed watch
            new1 = w.shard(1, 3)
            await w.start(new1, limit=0.5)
            w.modify(w.of(moves[(0, 1)][0]))  # old 0 still has it
            w.delete(w.of(moves[(1, 0)][1]))  # nobody has: handed to 0, which is still the old one
            await asyncio.sleep(0.5)  # what a running shard has to say of these, it says now
            await w.stop(old[0])
            w.delete(w.of(moves[(0, 1)][0], skip=1))
            w.delete(w.of(moves[(0, 2)][0]))
            w.modify(w.of(moves[(0, 0)][0]))
            new0 = w.shard(0, 3)
            took = await w.start(new0)
            for svc in (new1, new2):
                for _ in range(300):
                    if all(any(r.namespace == n and r.synced.is_set() for r in svc.reflectors) for n in w.owned(svc)):
                        break
                    await asyncio.sleep(0.02)
            w.modify(w.of(moves[(0, 2)][1]))  # the new layout, live
            w.create(moves[(1, 0)][1])
            await w.delivered()
            return (took, w.got() == w.want, (w.got() - w.want, w.want - w.got()), w.owners(),
                    w.counted("shard_handover_timeouts"), w.records_left())
        finally:
            await w.close()

    took, exact, diff, owners, timeouts, left = run(body(), timeout=120)
    assert exact, diff
    assert took is not None and timeouts == 0
    assert owners == {n: shard_of(n, 3) for n in nss}
    assert left == []


def test_rolling_three_to_two(tmp_path):
    """(d) Ordinal 2 stops for good, then 1 is replaced while 0 still runs under
    count 3, then 0. A pod goes in a namespace moving 2→1 and one in a
    namespace moving 1→0, each while nobody watched it."""
    moves = _moves(3, 2)
    nss = _twelve()

    async def body():
        w = await World(tmp_path, nss, pods_per_namespace=3).open()
        try:
            old = [w.shard(i, 3) for i in range(3)]
            for svc in old:
                assert await w.start(svc) is not None
            await w.delivered()
            await w.stop(old[2])
            w.delete(w.of(moves[(2, 1)][0]))
            await w.stop(old[1])
            new1 = w.shard(1, 2)
            await w.start(new1, limit=0.5)  # 0→1 namespaces wait for old 0's restart
            parted = new1.metrics.c.get("shard_partings_in", 0)
            w.delete(w.of(moves[(1, 0)][0]))  # handed to shard 0 by new 1; old 0 does not take it
            w.modify(w.of(moves[(0, 1)][0]))  # old 0 still watches
            await asyncio.sleep(0.5)  # what a running shard has to say of these, it says now
            await w.stop(old[0])
            new0 = w.shard(0, 2)
            took = await w.start(new0)
            for _ in range(300):
                if all(any(r.namespace == n and r.synced.is_set() for r in new1.reflectors) for n in w.owned(new1)):
                    break
                await asyncio.sleep(0.02)
            await w.delivered()
            return (took, parted, w.got() == w.want, (w.got() - w.want, w.want - w.got()), w.owners(),
                    w.counted("shard_handover_timeouts"), w.counted("shard_partings_in"), w.records_left())
        finally:
            await w.close()

    took, parted, exact, diff, owners, timeouts, partings, left = run(body(), timeout=120)
    assert exact, diff
    assert took is not None and took < SYNC_BOUND and timeouts == 0
    assert parted == len(moves[(2, 1)]) and partings == len(moves[(2, 1)]) + len(moves[(2, 0)])
    assert owners == {n: shard_of(n, 2) for n in nss}
    assert left == []
