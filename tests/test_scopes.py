"""The watch scopes on their own (engine/scopes.py ``ScopeSet``): fake
reflectors, a recording hand-over, a Python pod cache and a logger outside the
tree, with no API server and no native extension. The end-to-end cases, whole
services against a fake API server, are in test_sharding.py, test_scale_down.py
and test_reflector.py.

Two shards with ``assignment: balanced`` and the namespaces below give every
kind of move: with ``{ns-a, ns-e}`` shard 0 owns ns-e and shard 1 ns-a; once
ns-b appears, shard 1 owns it and ns-a moves to shard 0
(:func:`test_the_layout_these_cases_stand_on` holds that true)."""

import asyncio
import logging
import time

from conftest import run
from k8s_watcher_amd.engine.scopes import ScopeSet
from k8s_watcher_amd.metrics import Metrics
from k8s_watcher_amd.ops.cache import make_pod_cache
from k8s_watcher_amd.parallel.shard import owner_of
from k8s_watcher_amd.utils.config import ShardSettings, WatcherSettings

BEFORE = {"ns-a", "ns-e"}
AFTER = {"ns-a", "ns-b", "ns-e"}
DRAIN = 0.2  # namespace_drain_seconds
INVALID_LINE = ("INVALID", None, None, None, None, None, False, None, "bad json")


class FakeReflector:
    """What a ScopeSet touches of a reflector: ``run()`` waits for ``stop()``
    (and raises ``fail`` then, or at once with ``fail_now``)."""

    def __init__(self, rig, namespace, resource_version, primed):
        self.rig, self.namespace, self.resource_version, self.primed = rig, namespace, resource_version, primed
        self.pipeline = rig.pipeline
        self.synced = asyncio.Event()
        self.stopped = asyncio.Event()
        self.stops, self.paused, self.deletes, self.controls = 0, [], 0, []
        self.fail = self.fail_now = None

    async def run(self):
        if self.fail_now is not None:
            raise self.fail_now
        try:
            await self.stopped.wait()
        except asyncio.CancelledError:
            if self.fail is None:
                raise
        if self.fail is not None:
            raise self.fail

    def stop(self):
        self.stops += 1
        self.stopped.set()

    def set_paused(self, paused):
        self.paused.append(paused)

    def notify_cached_deleted(self):
        self.deletes += 1
        for ev in self.pipeline.delete_scope(self.namespace, time.monotonic_ns()):
            self._handle_control(ev)

    def _handle_control(self, ev):
        self.controls.append(ev)


class FakePipeline:
    """``delete_scope`` drops the namespace's pods from the rig's cache (the
    real one notifies them DELETED first) and returns the rig's control events."""

    def __init__(self, rig):
        self.rig = rig
        self.deleted = []

    def delete_scope(self, ns, now_ns):
        self.deleted.append(ns)
        self.rig.cache.drop_namespaces({ns})
        return list(self.rig.controls)


class FakeHandover:
    def __init__(self):
        self.calls = []  # ("begin_gain", ns) | ("cancel_gain", ns) | ("begin_out", ns, dst) | ("cancel_out", ns)
        self.gains = set()

    def begin_gain(self, ns):
        self.calls.append(("begin_gain", ns))
        self.gains.add(ns)

    def cancel_gain(self, ns):
        self.calls.append(("cancel_gain", ns))
        had = ns in self.gains
        self.gains.discard(ns)
        return had

    def begin_out(self, ns, dst):
        self.calls.append(("begin_out", ns, dst))

    def cancel_out(self, ns):
        self.calls.append(("cancel_out", ns))
        return False

    def gaining(self):
        return set(self.gains)


class FakeNamespaceWatcher:
    def __init__(self, names, on_change):
        self.names, self.on_change = set(names), on_change
        self.synced = asyncio.Event()
        self.stopped = asyncio.Event()

    async def run(self):
        self.synced.set()
        await self.stopped.wait()

    def stop(self):
        self.stopped.set()


class Rig:
    """A ScopeSet over fakes; build it inside the running loop."""

    def __init__(self, hdir="", index=0, count=2, drain=DRAIN):
        shard = ShardSettings(count=count, index=index, assignment="balanced", handover_dir=str(hdir or ""))
        self.watcher = WatcherSettings(namespace_scope="discover", namespace_drain_seconds=drain, shard=shard)
        self.metrics = Metrics()
        self.cache = make_pod_cache(False)
        self.stop = asyncio.Event()
        self.handover = FakeHandover()
        self.pipeline = FakePipeline(self)
        self.controls = []  # what delete_scope returns: control events
        self.made = []  # every reflector ever built, in order
        self.next_fail = self.next_fail_now = None
        self.messages = []
        self.log = logging.Logger("test.scopes")  # not in the logging tree: nothing else hears it
        handler = logging.Handler()
        handler.emit = lambda rec: self.messages.append((rec.levelname, rec.getMessage()))
        self.log.addHandler(handler)
        self.drain_timers = []  # [handle, fired] of every drain timer ever scheduled
        self._count_drain_timers()
        self.nsw = None
        self.build()

    # ---- the seams: everything the cases do to the class under test
    def build(self):
        self.scopes = ScopeSet(self.watcher, self.metrics, self.log, self.stop, cache=lambda: self.cache,
                               handover=lambda: self.handover, make_reflector=self._make_reflector,
                               make_namespace_watcher=self._make_namespace_watcher)

    async def begin(self, names, gains=(), live=True, saved_rvs=None):
        """Start-up as the service does it: resolve, start every scope, go live."""
        self.names0 = set(names)
        self.scopes.saved_rvs = saved_rvs or {}
        scopes = await self.scopes.resolve()
        await self.scopes.start_all(scopes, set(gains))
        if live:
            self.go_live()
        return scopes

    def go_live(self):
        self.scopes.go_live()

    def change(self, names):
        """The namespace watch saw the set become ``names``."""
        self.nsw.names = set(names)
        self.nsw.on_change(set(names))

    def start(self, ns, primed=True):
        return self.scopes.start(ns, primed=primed)

    def stop_scope(self, ns, handover_to=None):
        self.scopes.stop_scope(ns, handover_to)

    def saturated(self, flag):
        self.scopes.set_saturated(flag)

    def reflectors(self):
        return self.scopes.reflectors()

    def failure(self):
        return self.scopes.failure

    def restart_reconcile(self, scopes):
        self.scopes.reconcile_cache(scopes, lambda ns: self.pipeline.delete_scope(ns, time.monotonic_ns()))

    def tasks(self):
        return self.scopes.tasks()

    def stop_all(self):
        self.scopes.stop()

    # ---- fakes' factories
    def _make_namespace_watcher(self, on_change):
        self.nsw = FakeNamespaceWatcher(self.names0, on_change)
        return self.nsw

    def _make_reflector(self, ns, resource_version, primed):
        r = FakeReflector(self, ns, resource_version, primed)
        r.fail, r.fail_now = self.next_fail, self.next_fail_now
        self.next_fail = self.next_fail_now = None
        self.made.append(r)
        return r

    def _count_drain_timers(self):
        loop = asyncio.get_running_loop()
        call_later = loop.call_later

        def counting(delay, cb, *args):
            if getattr(cb, "__name__", "") != "_retire":
                return call_later(delay, cb, *args)
            entry = [None, False]

            def fire(*a):
                entry[1] = True
                cb(*a)

            entry[0] = call_later(delay, fire, *args)
            self.drain_timers.append(entry)
            return entry[0]

        loop.call_later = counting

    # ---- helpers
    def pending_drain_timers(self):
        return sum(1 for h, fired in self.drain_timers if not fired and not h.cancelled())

    def fill(self, ns, n):
        for i in range(n):
            self.cache.put(f"{ns}-u{i}", str(100 + i), "Running", ns, f"pod-{i}", b'{"phase":"Running"}')

    def cached(self, ns):
        return self.cache.count_namespace(ns)

    def watching(self):
        return [r.namespace for r in self.reflectors()]

    def of(self, ns):
        found = [r for r in self.reflectors() if r.namespace == ns]
        assert len(found) == 1, (ns, self.watching())
        return found[0]

    def logged(self, level, text):
        return sum(1 for lv, msg in self.messages if lv == level and msg == text)

    async def until(self, cond, timeout=2.0):
        end = time.monotonic() + timeout
        while not cond():
            assert time.monotonic() < end, (self.handover.calls, self.messages)
            await asyncio.sleep(0.01)

    async def end(self):
        self.stop.set()
        self.stop_all()
        for t in self.tasks():
            t.cancel()
        await asyncio.sleep(0)


def test_the_layout_these_cases_stand_on():
    assert owner_of("ns-e", BEFORE, 2, "balanced") == 0 and owner_of("ns-a", BEFORE, 2, "balanced") == 1
    assert [owner_of(ns, AFTER, 2, "balanced") for ns in ("ns-a", "ns-b", "ns-e")] == [0, 1, 0]


# ---------------------------------------------------------------- start-up
def test_a_change_before_the_set_is_live_waits_for_the_replay(tmp_path):
    async def body():
        rig = Rig(tmp_path, index=1)
        assert await rig.begin(BEFORE, live=False) == ["ns-a"]
        first = rig.of("ns-a")
        rig.change(AFTER)  # seen while the first scopes were starting
        assert rig.watching() == ["ns-a"] and first.stops == 0 and rig.handover.calls == []
        assert rig.metrics.c["scopes_started"] == 0 and rig.metrics.c["scopes_stopped"] == 0
        rig.go_live()
        assert rig.watching() == ["ns-b"] and first.stops == 1
        assert rig.metrics.c["scopes_started"] == 1 and rig.metrics.c["scopes_stopped"] == 1
        await rig.end()

    run(body(), timeout=10)


def test_start_up_resumes_each_scope_from_its_own_point_and_waits_for_gains(tmp_path):
    async def body():
        rig = Rig(tmp_path, count=1)
        await rig.begin(BEFORE, gains={"ns-e"}, saved_rvs={"ns-a": "41"})
        assert rig.watching() == ["ns-a"] and rig.handover.calls == [("begin_gain", "ns-e")]
        r = rig.of("ns-a")
        assert (r.resource_version, r.primed) == ("41", True)
        await rig.end()

    run(body(), timeout=10)


# ---------------------------------------------------------------- the namespace-change decision
def test_a_new_owned_namespace_starts_primed(tmp_path):
    async def body():
        rig = Rig(tmp_path, index=1)
        await rig.begin(BEFORE)
        assert rig.of("ns-a").primed is False  # nothing was saved: the first scopes announce what they list
        rig.change(AFTER)
        r = rig.of("ns-b")
        assert r.primed is True and r.resource_version is None
        assert rig.metrics.c["scopes_started"] == 1
        assert rig.logged("INFO", "Watching namespace ns-b (new or now owned by shard 1)") == 1
        assert ("begin_gain", "ns-b") not in rig.handover.calls  # it was nobody's before
        await rig.end()

    run(body(), timeout=10)


def test_a_namespace_of_another_shard_is_gained_through_its_record(tmp_path):
    async def body():
        rig = Rig(tmp_path, index=0)
        await rig.begin(BEFORE)
        rig.change(AFTER)
        assert rig.handover.calls == [("cancel_out", "ns-a"), ("begin_gain", "ns-a")]
        assert rig.watching() == ["ns-e"]  # no watch of ns-a before its record is in
        assert rig.metrics.c["scopes_started"] == 1
        assert rig.logged("INFO", "Watching namespace ns-a (new or now owned by shard 0)") == 1
        await rig.end()

    run(body(), timeout=10)


def test_without_a_handover_directory_a_gained_namespace_starts_at_once():
    async def body():
        rig = Rig("", index=0)
        await rig.begin(BEFORE)
        rig.change(AFTER)
        assert rig.watching() == ["ns-e", "ns-a"] and rig.of("ns-a").primed is True
        assert ("begin_gain", "ns-a") not in rig.handover.calls
        await rig.end()

    run(body(), timeout=10)


def test_a_namespace_that_moves_away_is_handed_over_with_its_pods_still_cached(tmp_path):
    async def body():
        rig = Rig(tmp_path, index=1)
        await rig.begin(BEFORE)
        rig.fill("ns-a", 3)
        gone = rig.of("ns-a")
        rig.change(AFTER)
        assert gone.stops == 1 and "ns-a" not in rig.watching()
        assert ("begin_out", "ns-a", 0) in rig.handover.calls
        assert rig.cached("ns-a") == 3
        assert rig.metrics.c["scopes_stopped"] == 1
        assert rig.logged("INFO", "Stopped watching namespace ns-a (owned by another shard)") == 1
        await asyncio.sleep(0)
        assert rig.failure().done() is False  # stopped on purpose
        await rig.end()

    run(body(), timeout=10)


def test_without_a_handover_directory_a_namespace_that_moves_away_is_forgotten():
    async def body():
        rig = Rig("", index=1)
        await rig.begin(BEFORE)
        rig.fill("ns-a", 3)
        rig.fill("ns-b", 2)
        rig.change(AFTER)
        assert "ns-a" not in rig.watching() and not [c for c in rig.handover.calls if c[0] == "begin_out"]
        assert rig.cached("ns-a") == 0 and rig.cached("ns-b") == 2
        assert rig.metrics.c["scopes_stopped"] == 1
        await rig.end()

    run(body(), timeout=10)


def test_a_namespace_that_comes_back_before_its_record_went_out():
    """``cancel_out`` first, then a primed start. (With a hand-over directory
    the start waits for a record instead, as for any namespace that was
    another shard's under the previous set: the next case.)"""
    async def body():
        rig = Rig("", index=1)
        await rig.begin(BEFORE)
        rig.change(AFTER)
        del rig.handover.calls[:]
        rig.change(BEFORE)
        assert rig.handover.calls[0] == ("cancel_out", "ns-a")
        assert rig.watching() == ["ns-a"] and rig.of("ns-a").primed is True
        assert rig.made[-1] is rig.of("ns-a") and len(rig.made) == 3  # ns-a, ns-b, ns-a again
        await rig.end()

    run(body(), timeout=10)


def test_a_namespace_that_comes_back_with_a_handover_directory(tmp_path):
    async def body():
        rig = Rig(tmp_path, index=1)
        await rig.begin(BEFORE)
        rig.change(AFTER)
        del rig.handover.calls[:]
        rig.change(BEFORE)
        assert rig.handover.calls[:2] == [("cancel_out", "ns-a"), ("begin_gain", "ns-a")]
        assert rig.watching() == []  # ns-b stopped (deleted, nothing cached), ns-a waits for a record
        await rig.end()

    run(body(), timeout=10)


# ---------------------------------------------------------------- a deleted namespace drains
def test_a_deleted_namespace_keeps_its_watch_until_its_pods_are_gone():
    async def body():
        rig = Rig("", count=1, drain=5.0)
        await rig.begin(BEFORE)
        rig.fill("ns-a", 2)
        r = rig.of("ns-a")
        rig.change({"ns-e"})
        await asyncio.sleep(0.08)  # a step or two of the drain
        assert r.stops == 0 and rig.watching() == ["ns-a", "ns-e"]
        rig.cache.drop_namespaces({"ns-a"})  # its pods' DELETED events came
        t0 = time.monotonic()
        await rig.until(lambda: r.stops == 1)
        assert time.monotonic() - t0 < 0.5  # within a few 50 ms steps, long before the drain limit
        assert rig.watching() == ["ns-e"] and r.deletes == 0
        assert rig.metrics.c["namespace_deleted_synthesized"] == 0 and rig.metrics.c["scopes_stopped"] == 1
        assert rig.logged("INFO", "Stopped watching namespace ns-a (deleted)") == 1
        await rig.end()

    run(body(), timeout=10)


def test_pods_left_after_the_drain_limit_are_notified_deleted_by_the_reflector():
    async def body():
        rig = Rig("", count=1)
        await rig.begin(BEFORE)
        rig.fill("ns-a", 3)
        rig.fill("ns-e", 2)
        rig.controls = [INVALID_LINE]
        r = rig.of("ns-a")
        t0 = time.monotonic()
        rig.change({"ns-e"})
        await rig.until(lambda: r.stops == 1)
        assert DRAIN - 0.01 <= time.monotonic() - t0 < DRAIN + 0.3  # (timers may fire a clock tick early)
        assert rig.pipeline.deleted == ["ns-a"]
        assert r.controls == [INVALID_LINE]  # the reflector's to count and log, as a watch line's
        assert not [m for _, m in rig.messages if "undecodable cached entry" in m]
        assert rig.metrics.c["namespace_deleted_synthesized"] == 3 and rig.metrics.c["scopes_stopped"] == 1
        assert rig.logged("WARNING", "Namespace ns-a deleted: 3 pod(s) without a DELETED event after 0.2s; "
                                     "notifying them as DELETED from the cache") == 1
        assert rig.logged("INFO", "Stopped watching namespace ns-a (deleted)") == 1
        assert rig.cached("ns-e") == 2 and rig.watching() == ["ns-e"]
        assert r.deletes == 1  # through the reflector's one method for it
        await rig.end()

    run(body(), timeout=10)


def test_a_namespace_recreated_inside_the_window_keeps_its_watch():
    async def body():
        rig = Rig("", count=1)
        await rig.begin(BEFORE)
        rig.fill("ns-a", 2)
        r = rig.of("ns-a")
        rig.change({"ns-e"})
        assert rig.pending_drain_timers() == 1
        rig.change({"ns-e", "ns-x"})  # an unrelated change while ns-a drains
        assert rig.pending_drain_timers() == 1  # its timer is running: no second one
        await asyncio.sleep(0.07)
        assert rig.pending_drain_timers() == 1
        rig.change({"ns-a", "ns-e", "ns-x"})  # created again
        assert rig.pending_drain_timers() == 0
        made = len(rig.drain_timers)
        await asyncio.sleep(DRAIN + 0.1)
        assert len(rig.drain_timers) == made and rig.pending_drain_timers() == 0
        assert rig.of("ns-a") is r and r.stops == 0 and r.deletes == 0
        assert rig.cached("ns-a") == 2
        assert rig.metrics.c["namespace_deleted_synthesized"] == 0 and rig.metrics.c["scopes_stopped"] == 0
        assert rig.metrics.c["scopes_started"] == 1  # ns-x
        await rig.end()

    run(body(), timeout=10)


def test_a_namespace_deleted_while_still_being_gained(tmp_path):
    async def body():
        rig = Rig(tmp_path, count=1)
        await rig.begin(BEFORE, gains={"ns-a"})
        assert rig.handover.calls == [("begin_gain", "ns-a")] and rig.watching() == ["ns-e"]
        rig.fill("ns-a", 1)
        rig.change({"ns-e"})
        assert rig.handover.calls[1:] == [("cancel_gain", "ns-a")] and rig.handover.gaining() == set()
        assert rig.drain_timers == [] and rig.metrics.c["scopes_stopped"] == 0
        await rig.end()

    run(body(), timeout=10)


# ---------------------------------------------------------------- one scope
def test_a_scope_that_fails_fails_the_set_and_one_stopped_on_purpose_does_not():
    async def body():
        rig = Rig("", count=1)
        await rig.begin(BEFORE)
        stopped = rig.of("ns-a")
        stopped.fail = RuntimeError("after its stop")
        rig.stop_scope("ns-a")
        await asyncio.sleep(0.02)
        assert rig.failure().done() is False and rig.watching() == ["ns-e"]
        boom = RuntimeError("watch failed for good")
        rig.next_fail_now = boom
        rig.start("ns-x")
        await rig.until(lambda: rig.failure().done())
        assert rig.failure().exception() is boom
        await rig.end()

    run(body(), timeout=10)


def test_nothing_fails_the_set_after_the_stop_event():
    async def body():
        rig = Rig("", count=1)
        await rig.begin(BEFORE)
        rig.of("ns-a").fail = RuntimeError("while stopping")
        rig.stop.set()
        rig.of("ns-a").stop()
        await asyncio.sleep(0.02)
        assert rig.failure().done() is False
        rig.change({"ns-e"})  # and no decision is taken any more
        assert rig.watching() == ["ns-a", "ns-e"] and rig.drain_timers == []
        await rig.end()

    run(body(), timeout=10)


def test_saturation_pauses_every_scope_and_new_ones_start_paused():
    async def body():
        rig = Rig("", count=1)
        await rig.begin(BEFORE)
        rig.saturated(True)
        assert [r.paused for r in rig.reflectors()] == [[True], [True]]
        late = rig.start("ns-x")
        assert late.paused == [True]
        rig.saturated(False)
        assert [r.paused[-1] for r in rig.reflectors()] == [False, False, False]
        assert rig.start("ns-y").paused == []
        await rig.end()

    run(body(), timeout=10)


# ---------------------------------------------------------------- a restart with a checkpoint
def test_restart_notifies_the_pods_of_namespaces_deleted_meanwhile():
    async def body():
        rig = Rig("", count=1)
        rig.fill("ns-a", 2)
        rig.fill("ns-e", 1)
        rig.fill("ns-gone", 2)
        rig.controls = [INVALID_LINE]
        await rig.begin(BEFORE, live=False)
        rig.restart_reconcile(["ns-a"])  # ns-e exists but is no longer this shard's
        assert rig.pipeline.deleted == ["ns-gone"]
        assert rig.metrics.c["namespace_deleted_synthesized"] == 2
        assert rig.logged("WARNING", "Namespace ns-gone was deleted while the watcher was down: notifying its "
                                     "2 cached pod(s) as DELETED") == 1
        assert rig.logged("WARNING", "Skipping undecodable cached entry (INVALID): bad json") == 1
        assert rig.metrics.c["events_invalid"] == 0 and all(r.controls == [] for r in rig.made)
        assert (rig.cached("ns-a"), rig.cached("ns-e"), rig.cached("ns-gone")) == (2, 0, 0)
        await rig.end()

    run(body(), timeout=10)
