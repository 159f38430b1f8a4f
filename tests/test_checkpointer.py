"""When the checkpoint is cut and written (engine/checkpoint.py
``Checkpointer``), on its own: a pod cache of three pods, fake reflectors and a
temporary path, with no API server and no service. The module's
``write_native`` is wrapped so that a write can be held on its executor thread.

The ordering cases pin what ``WatcherService`` did while it owned this code:
the first two were run against it as it was (``service.write_native`` wrapped
the same way) before the move, and passed there."""

import asyncio
import logging
import os
import threading

from conftest import run
from k8s_watcher_amd.engine import checkpoint as checkpoint_mod
from k8s_watcher_amd.engine.checkpoint import Checkpointer, load_checkpoint
from k8s_watcher_amd.metrics import Metrics
from k8s_watcher_amd.ops.cache import make_pod_cache
from k8s_watcher_amd.utils.config import CheckpointSettings

REAL_WRITE_NATIVE = checkpoint_mod.write_native
GAUGES = ["checkpoint_bytes", "checkpoint_owed", "checkpoint_pods", "checkpoint_stall_ms", "checkpoint_write_ms",
          "checkpoint_written_at"]


class FakeReflector:
    def __init__(self, scope, rv):
        self.scope, self.rv, self.paused = scope, rv, []

    def set_paused(self, paused):
        self.paused.append(paused)


class FakeNotifier:
    """No ``core``: with clusterapi enabled that means format 1."""

    def __init__(self, drains=True, saturated=False, reflectors=()):
        self.drains, self.saturated, self.reflectors = drains, saturated, reflectors
        self.seen_paused = []  # every reflector's last ``set_paused`` when ``drain`` was called

    async def drain(self, timeout):
        self.seen_paused.append([r.paused[-1] for r in self.reflectors])
        return self.drains


class HeldWrites:
    """``write_native`` with a gate in it: ``calls`` lists ("start" | "end",
    the cut's resume point) in the order the executor threads got there."""

    def __init__(self, real):
        self.real = real
        self.calls = []
        self.open = threading.Event()
        self.open.set()
        self.fail = None

    def __call__(self, snap, path, scopes, meta=None):
        self.calls.append(("start", scopes["*"]))
        try:
            assert self.open.wait(10)
            if self.fail is not None:
                fail, self.fail = self.fail, None
                raise fail
            return self.real(snap, path, scopes, meta)
        finally:
            self.calls.append(("end", scopes["*"]))

    async def entered(self, n=1):
        for _ in range(2000):
            if sum(1 for kind, _ in self.calls if kind == "start") >= n:
                return
            await asyncio.sleep(0.001)
        raise AssertionError(self.calls)


class Rig:
    def __init__(self, tmp_path, monkeypatch, native=True, path=True, notifier=None, interval=3600.0):
        self.path = str(tmp_path / "ck.bin") if path else None
        self.metrics = Metrics()
        self.cache = make_pod_cache(native)
        for i in range(3):
            self.put(i)
        self.reflector = FakeReflector("*", "1")
        self.notifier = notifier
        if notifier is not None:
            notifier.reflectors = [self.reflector]
        self.messages = []
        self.log = logging.Logger("test.checkpointer")  # not in the logging tree: nothing else hears it
        handler = logging.Handler()
        handler.emit = lambda rec: self.messages.append((rec.levelname, rec.getMessage()))
        self.log.addHandler(handler)
        self.writes = HeldWrites(REAL_WRITE_NATIVE)
        monkeypatch.setattr(checkpoint_mod, "write_native", self.writes)
        self.ck = Checkpointer(CheckpointSettings(path=self.path, interval_seconds=interval), native, True,
                               self.metrics, self.log, cache=lambda: self.cache, notifier=lambda: self.notifier,
                               reflectors=lambda: [self.reflector])

    def put(self, i):
        self.cache.put(f"uid-{i}", str(10 + i), "Running", "ns-a" if i % 2 else "ns-b", f"pod-{i}", b'{"phase":"Running"}')

    def move_on(self, rv):
        """What a later cut differs in: the resume point and one more pod."""
        self.reflector.rv = rv
        self.put(len(self.cache))

    def on_disk(self, native=True):
        scopes, cache, meta, owed = load_checkpoint(self.path, native_cache=native)
        return scopes, len(cache)

    def written(self):
        return self.metrics.c["checkpoints_written"]


async def _let_run(n=10):
    for _ in range(n):
        await asyncio.sleep(0)


def test_two_writes_issued_together_land_one_after_the_other_in_cut_order(tmp_path, monkeypatch):
    async def body():
        rig = Rig(tmp_path, monkeypatch)
        rig.writes.open.clear()
        both = [asyncio.ensure_future(rig.ck.now()), asyncio.ensure_future(rig.ck.now())]
        await rig.writes.entered()
        await _let_run()
        assert rig.writes.calls == [("start", "1")]  # the second has not cut, let alone begun to write
        rig.move_on("2")
        rig.writes.open.set()
        assert await asyncio.gather(*both) == [True, True]
        assert rig.writes.calls == [("start", "1"), ("end", "1"), ("start", "2"), ("end", "2")]
        assert rig.on_disk() == ({"*": "2"}, 4) and rig.written() == 2

    run(body(), timeout=20)


def test_final_cut_waits_for_a_periodic_write_whose_task_was_cancelled(tmp_path, monkeypatch):
    async def body():
        rig = Rig(tmp_path, monkeypatch, interval=0.001)
        rig.writes.open.clear()
        periodic = asyncio.ensure_future(rig.ck.loop())
        await rig.writes.entered()
        periodic.cancel()  # as shutdown does; the write goes on, on its thread
        await asyncio.gather(periodic, return_exceptions=True)
        rig.move_on("2")
        cuts = []
        final = asyncio.ensure_future(rig.ck.final_cut(lambda snap=None: cuts.append(snap)))
        await _let_run()
        assert not final.done() and cuts == [] and rig.writes.calls == [("start", "1")]
        rig.writes.open.set()
        await final
        assert rig.writes.calls == [("start", "1"), ("end", "1"), ("start", "2"), ("end", "2")]
        assert rig.on_disk() == ({"*": "2"}, 4)
        assert len(cuts) == 1 and cuts[0].stats()["entries"] == 4
        # both files landed; the one whose task was cancelled before it saw that is not counted
        assert rig.written() == 1
        assert rig.messages == []

    run(body(), timeout=20)


def test_final_cut_reports_a_failed_write_in_flight_and_still_writes(tmp_path, monkeypatch):
    async def body():
        rig = Rig(tmp_path, monkeypatch)
        rig.writes.open.clear()
        rig.writes.fail = OSError(28, "No space left on device")
        first = asyncio.ensure_future(rig.ck.now())
        await rig.writes.entered()
        first.cancel()
        await asyncio.gather(first, return_exceptions=True)
        rig.move_on("2")
        final = asyncio.ensure_future(rig.ck.final_cut())
        await _let_run()
        rig.writes.open.set()
        await final
        assert [m for m in rig.messages if m[0] == "WARNING"] == [
            ("WARNING", "Checkpoint write in progress at shutdown failed: [Errno 28] No space left on device")]
        assert rig.on_disk() == ({"*": "2"}, 4) and rig.written() == 1

    run(body(), timeout=20)


def test_without_a_path_nothing_is_written_but_the_final_cut_is_still_a_cut(tmp_path, monkeypatch):
    async def body():
        rig = Rig(tmp_path, monkeypatch, path=False)
        assert await rig.ck.now() is False
        cuts = []
        await rig.ck.final_cut(lambda snap=None: cuts.append(snap))
        assert len(cuts) == 1 and cuts[0].owed() == [] and cuts[0].stats()["entries"] == 3
        await rig.ck.final_cut()  # and without at_cut, nothing at all
        assert rig.writes.calls == [] and rig.written() == 0 and os.listdir(tmp_path) == []
        assert rig.ck.last is None

    run(body(), timeout=20)


def test_format_1_pauses_the_readers_drains_saves_and_resumes(tmp_path, monkeypatch):
    async def body():
        for saturated in (False, True):
            rig = Rig(tmp_path, monkeypatch, native=False, notifier=FakeNotifier(saturated=saturated))
            assert not rig.ck.consistent()
            assert await rig.ck.now(drain_timeout=1.0) is True
            assert rig.notifier.seen_paused == [[True]]  # drained with the readers paused
            assert rig.reflector.paused == [True, saturated]  # and resumed to what the notifier says
            assert rig.on_disk(native=False) == ({"*": "1"}, 3) and rig.written() == 1
            os.unlink(rig.path)

        rig = Rig(tmp_path, monkeypatch, native=False, notifier=FakeNotifier(drains=False))
        assert await rig.ck.now(drain_timeout=1.0) is False
        assert rig.reflector.paused == [True, False] and rig.notifier.seen_paused == [[True]]
        assert os.listdir(tmp_path) == [] and rig.written() == 0

        cuts = []
        await rig.ck.final_cut(lambda snap=None: cuts.append(snap))  # reached drained: at_cut(), then the save
        assert cuts == [None] and rig.on_disk(native=False) == ({"*": "1"}, 3) and rig.written() == 1
        assert rig.writes.calls == [] and rig.ck.last is None

    run(body(), timeout=20)


def test_a_format_2_write_sets_the_six_gauges_and_last(tmp_path, monkeypatch):
    async def body():
        rig = Rig(tmp_path, monkeypatch)
        assert rig.ck.consistent() and rig.ck.last is None
        assert await rig.ck.now() is True
        last = rig.ck.last
        assert sorted(last) == GAUGES
        assert {k: rig.metrics.gauges[k]() for k in GAUGES} == last
        assert last["checkpoint_pods"] == 3.0 and last["checkpoint_owed"] == 0.0
        assert last["checkpoint_bytes"] == float(os.path.getsize(rig.path))
        assert rig.on_disk() == ({"*": "1"}, 3) and rig.written() == 1

    run(body(), timeout=20)
