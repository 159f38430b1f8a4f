"""The namespace hand-over protocol on its own (engine/handover.py): both
parties against a Python pod cache, a fake notifier and a temporary directory,
with no API server and no native extension. The end-to-end cases, whole
services against a fake API server, are in test_sharding.py."""

import asyncio
import json
import logging
import os
import time

from conftest import run
from k8s_watcher_amd.engine.handover import NamespaceHandover
from k8s_watcher_amd.metrics import Metrics
from k8s_watcher_amd.ops.cache import make_pod_cache
from k8s_watcher_amd.parallel.shard import layout_of, owner_of, record_layout, shard_of, take_handover, write_handover
from k8s_watcher_amd.utils.config import ShardSettings


class FakeNotifier:
    """``pending_in`` answers from ``answers``, repeating the last; ``probe``
    is sampled at every call."""

    def __init__(self, answers, probe=lambda: None):
        self.answers = list(answers)
        self.probe = probe
        self.probed = []

    def pending_in(self, ns):
        self.probed.append(self.probe())
        return self.answers.pop(0) if len(self.answers) > 1 else self.answers[0]


class Rig:
    def __init__(self, hdir, index=0, count=2, wait=0.3, notifier=None, assignment="hash"):
        self.shard = ShardSettings(count=count, index=index, assignment=assignment, handover_dir=str(hdir),
                                   handover_wait_seconds=wait)
        self.metrics = Metrics()
        self.cache = make_pod_cache(False)
        self.notifier = notifier
        self.stop = asyncio.Event()
        self.calls = []  # ("owed", list) | ("start", ns, primed) | ("forget", set), in call order
        self.messages = []
        self.log = logging.Logger("test.handover")  # not in the logging tree: nothing else hears it
        handler = logging.Handler()
        handler.emit = lambda rec: self.messages.append((rec.levelname, rec.getMessage()))
        self.log.addHandler(handler)
        self.handover = NamespaceHandover(
            self.shard, self.metrics, self.log, self.stop,
            cache=lambda: self.cache, notifier=lambda: self.notifier,
            resubmit_owed=lambda owed: self.calls.append(("owed", owed)),
            start_scope=lambda ns, primed: self.calls.append(("start", ns, primed)),
            forget_namespaces=self._forget)

    def _forget(self, namespaces):
        self.calls.append(("forget", set(namespaces)))
        self.cache.drop_namespaces(namespaces)

    def fill(self, ns, n):
        for i in range(n):
            self.cache.put(f"{ns}-u{i}", str(100 + i), "Running", ns, f"pod-{i}", b'{"phase":"Running"}')

    def pods_of(self, ns):
        return sorted((uid, e[0], e[1], e[3], e[4]) for uid, e in self.cache.items() if e[2] == ns)

    def record_path(self, ns):
        return os.path.join(self.shard.handover_dir, f"{ns}.handover.json")

    def called(self, kind):
        return [c for c in self.calls if c[0] == kind]

    def logged(self, level, text):
        return any(lv == level and text in msg for lv, msg in self.messages)

    async def until(self, cond, timeout=2.0):
        end = time.monotonic() + timeout
        while not cond():
            assert time.monotonic() < end, (self.calls, self.messages)
            await asyncio.sleep(0.01)


# ---------------------------------------------------------------- the old owner
def test_old_owner_writes_the_record_once_nothing_is_owed(tmp_path):
    async def body():
        rig = Rig(tmp_path, wait=0.4)
        rig.notifier = FakeNotifier([2, 0], probe=lambda: os.path.exists(rig.record_path("ns-a")))
        rig.fill("ns-a", 3)
        rig.fill("ns-b", 2)
        pods, kept = rig.pods_of("ns-a"), rig.pods_of("ns-b")
        rig.handover.begin_out("ns-a", 1)
        await rig.until(lambda: rig.called("forget"))
        assert rig.notifier.probed == [False, False]  # asked twice (2, then 0): no record before the 0
        rec = take_handover(str(tmp_path), "ns-a", 1, layout=layout_of(rig.shard))
        assert sorted(rec.pods) == pods and rec.owed == [] and rec.src == 0
        assert rig.called("forget") == [("forget", {"ns-a"})]
        assert rig.pods_of("ns-a") == [] and rig.pods_of("ns-b") == kept
        c = rig.metrics.c
        assert c["shard_handovers_out"] == 1 and c["shard_handover_pods_out"] == 3
        assert c["shard_handover_owed_late"] == 0 and c["shard_handover_errors"] == 0
        await asyncio.sleep(0)
        assert rig.handover._handing == {}

    run(body(), timeout=10)


def test_old_owner_gives_up_waiting_at_half_the_new_owners_patience(tmp_path):
    async def body():
        rig = Rig(tmp_path, wait=0.4, notifier=FakeNotifier([1]))
        rig.fill("ns-a", 2)
        t0 = time.monotonic()
        rig.handover.begin_out("ns-a", 1)
        await rig.until(lambda: os.path.exists(rig.record_path("ns-a")))
        waited = time.monotonic() - t0
        assert 0.2 <= waited < 0.4, waited
        await rig.until(lambda: rig.called("forget"))
        assert rig.metrics.c["shard_handover_owed_late"] == 1 and rig.metrics.c["shard_handovers_out"] == 1
        assert rig.logged("WARNING", "Handing namespace ns-a over with 1 notification(s) for it still owed")

    run(body(), timeout=10)


def test_old_owner_counts_a_failed_write_and_still_forgets(tmp_path):
    async def body():
        (tmp_path / "file").write_text("not a directory")
        rig = Rig(tmp_path / "file" / "handover", notifier=FakeNotifier([0]))
        rig.fill("ns-a", 2)
        rig.fill("ns-b", 1)
        rig.handover.begin_out("ns-a", 1)
        await rig.until(lambda: rig.called("forget"))
        c = rig.metrics.c
        assert c["shard_handover_errors"] == 1
        assert c["shard_handovers_out"] == 0 and c["shard_handover_pods_out"] == 0
        assert rig.logged("ERROR", "Could not write the hand-over of namespace ns-a to shard 1")
        assert rig.called("forget") == [("forget", {"ns-a"})]
        assert rig.pods_of("ns-a") == [] and len(rig.pods_of("ns-b")) == 1

    run(body(), timeout=10)


def test_old_owner_cancelled_when_the_namespace_comes_back(tmp_path):
    async def body():
        rig = Rig(tmp_path, wait=0.4, notifier=FakeNotifier([1]))
        rig.fill("ns-a", 2)
        pods = rig.pods_of("ns-a")
        rig.handover.begin_out("ns-a", 1)
        await asyncio.sleep(0.06)  # inside its wait for the owed notification
        assert rig.handover.cancel_out("ns-a") is True
        assert rig.handover.cancel_out("ns-a") is False
        await asyncio.sleep(0.25)  # past the moment the record would have gone out
        assert not os.path.exists(rig.record_path("ns-a")) and os.listdir(tmp_path) == []
        assert rig.pods_of("ns-a") == pods and rig.called("forget") == []
        assert rig.handover._handing == {}
        assert rig.metrics.c["shard_handovers_out"] == 0 and rig.metrics.c["shard_handover_owed_late"] == 0

    run(body(), timeout=10)


# ---------------------------------------------------------------- the new owner
OWED = [("ns-a-u1", "MODIFIED", "ns-a", "pod-1", b'{"n":1}'), ("ns-a-u0", "DELETED", "ns-a", "pod-0", b'{"n":2}\xff')]
PODS = [("ns-a-u0", "7", "Running", "pod-0", b'{"phase":"Running"}'), ("ns-a-u1", None, None, "pod-1", None)]


def test_new_owner_resends_owed_loads_the_pods_then_starts_the_watch(tmp_path):
    async def body():
        rig = Rig(tmp_path, index=0)
        write_handover(str(tmp_path), "ns-a", 1, 0, PODS, OWED, layout_of(rig.shard))
        rig.handover.begin_gain("ns-a")
        assert rig.handover.gaining() == {"ns-a"} and len(rig.handover.tasks()) == 1
        await rig.until(lambda: rig.called("start"))
        assert rig.calls == [("owed", OWED), ("start", "ns-a", True)]  # owed first, in record order; one start
        assert rig.pods_of("ns-a") == sorted(PODS)
        assert os.listdir(tmp_path) == []  # consumed
        c = rig.metrics.c
        assert c["shard_handovers_in"] == 1 and c["shard_handover_pods_in"] == 2 and c["shard_handover_timeouts"] == 0
        assert rig.handover.gaining() == set() and rig.handover.tasks() == []

    run(body(), timeout=10)


def test_new_owner_times_out_without_a_record(tmp_path):
    async def body():
        rig = Rig(tmp_path, wait=0.2)
        t0 = time.monotonic()
        rig.handover.begin_gain("ns-a")
        await rig.until(lambda: rig.called("start"))
        assert time.monotonic() - t0 >= 0.2
        assert rig.calls == [("start", "ns-a", True)]
        assert rig.metrics.c["shard_handover_timeouts"] == 1 and rig.metrics.c["shard_handovers_in"] == 0
        assert rig.logged("WARNING", "its pods are announced as ADDED again")
        assert rig.handover.gaining() == set()

    run(body(), timeout=10)


def test_new_owner_removes_a_record_of_another_layout_and_times_out(tmp_path):
    async def body():
        rig = Rig(tmp_path, wait=0.2)
        write_handover(str(tmp_path), "ns-a", 1, 0, PODS, OWED, layout_of(ShardSettings(count=5)))
        rig.handover.begin_gain("ns-a")
        await rig.until(lambda: not os.path.exists(rig.record_path("ns-a")))
        assert rig.calls == []  # removed at the first look, long before the wait ends; nothing taken from it
        await rig.until(lambda: rig.called("start"))
        assert rig.calls == [("start", "ns-a", True)] and rig.pods_of("ns-a") == []
        assert rig.metrics.c["shard_handover_timeouts"] == 1 and rig.metrics.c["shard_handovers_in"] == 0

    run(body(), timeout=10)


def test_new_owner_starts_nothing_once_the_service_stops(tmp_path):
    async def body():
        rig = Rig(tmp_path, wait=0.3)
        rig.handover.begin_gain("ns-a")
        await asyncio.sleep(0.06)
        rig.stop.set()
        done, _ = await asyncio.wait(rig.handover.tasks(), timeout=2)
        assert len(done) == 1
        assert rig.calls == [] and rig.metrics.c["shard_handover_timeouts"] == 0

    run(body(), timeout=10)


def test_gain_cancelled_before_its_record_came(tmp_path):
    async def body():
        rig = Rig(tmp_path, wait=0.2)
        rig.handover.begin_gain("ns-a")
        await asyncio.sleep(0.02)
        assert rig.handover.cancel_gain("ns-a") is True and rig.handover.cancel_gain("ns-a") is False
        assert rig.handover.gaining() == set()
        await asyncio.sleep(0.25)
        assert rig.calls == [] and rig.metrics.c["shard_handover_timeouts"] == 0

    run(body(), timeout=10)


# ---------------------------------------------------------------- across a restart
def _names(per_old_shard=6):
    """Namespaces of which shards 0 and 1 of a two-shard layout own ``per_old_shard`` each."""
    names = []
    for old in (0, 1):
        names += [n for n in (f"ns-{i}" for i in range(200)) if shard_of(n, 2) == old][:per_old_shard]
    return sorted(names)


def test_restart_under_a_new_layout_hands_out_and_waits_for_gains(tmp_path):
    names = _names()
    old = ShardSettings(count=2, index=0, handover_dir=str(tmp_path))
    held = [n for n in names if owner_of(n, names, 2, "hash") == 0]
    assert len(held) == 6
    record_layout(str(tmp_path), layout_of(old))
    rig = Rig(tmp_path, index=0, count=3)
    scopes = [n for n in names if owner_of(n, names, 3, "hash") == 0]
    want_out = sorted(n for n in held if n not in scopes)
    kept = sorted(n for n in held if n in scopes)
    want_gains = {n for n in scopes if n not in held}  # not in saved_rvs, and shard 1's under count 2
    assert want_out and kept and want_gains, (want_out, kept, want_gains)
    for k, ns in enumerate(held):
        rig.fill(ns, 1 + k % 3)
    saved_rvs = {ns: "55" for ns in held}
    owed = [("u-out-0", "MODIFIED", want_out[0], "a", b"one"), ("u-kept", "ADDED", kept[0], "b", b"two"),
            ("u-out-1", "DELETED", want_out[0], "c", b"three")]
    cached = {ns: rig.pods_of(ns) for ns in held}

    gains, left = rig.handover.reshard_on_start(scopes, names, saved_rvs, list(owed))

    assert gains == want_gains
    assert left == [owed[1]]
    assert sorted(os.listdir(tmp_path)) == sorted(["layout.json"] + [f"{ns}.handover.json" for ns in want_out])
    layout = layout_of(rig.shard)
    for ns in want_out:
        dst = owner_of(ns, names, 3, "hash")
        assert dst != 0
        rec = take_handover(str(tmp_path), ns, dst, layout=layout)
        assert sorted(rec.pods) == cached[ns] and rec.src == 0
        assert rec.owed == [o for o in owed if o[2] == ns]
    c = rig.metrics.c
    assert c["shard_handovers_out"] == len(want_out)
    assert c["shard_handover_pods_out"] == sum(len(cached[ns]) for ns in want_out)
    assert rig.calls == []  # the cache is the service's to prune: nothing forgotten, nothing started here
    assert rig.logged("INFO", f"waiting for the hand-over of {len(want_gains)} namespace(s)")


def test_first_deployment_and_unchanged_layout_hand_nothing_over(tmp_path):
    names = _names()
    rig = Rig(tmp_path, index=0, count=3)
    scopes = [n for n in names if owner_of(n, names, 3, "hash") == 0]
    assert scopes
    owed = [("u", "ADDED", scopes[0], "a", b"x")]
    assert rig.handover.reshard_on_start(scopes, names, {}, owed) == (set(), owed)  # no history
    assert os.listdir(tmp_path) == ["layout.json"]
    for ns in scopes:
        rig.fill(ns, 1)
    again = Rig(tmp_path, index=0, count=3)  # a restart, same layout
    again.cache = rig.cache
    assert again.handover.reshard_on_start(scopes, names, {ns: "9" for ns in scopes}, owed) == (set(), owed)
    assert os.listdir(tmp_path) == ["layout.json"]
    with open(tmp_path / "layout.json") as f:
        hist = json.load(f)
    assert hist["current"] == layout_of(rig.shard) and hist["previous"] is None
    assert rig.metrics.c["shard_handovers_out"] == again.metrics.c["shard_handovers_out"] == 0


def test_restart_without_a_writable_directory_hands_nothing_over(tmp_path):
    (tmp_path / "file").write_text("not a directory")
    rig = Rig(tmp_path / "file" / "handover", index=0, count=3)
    rig.fill("ns-a", 2)
    owed = [("u", "ADDED", "ns-a", "a", b"x")]
    gains, left = rig.handover.reshard_on_start(["ns-b"], ["ns-a", "ns-b"], {"ns-a": "5"}, owed)
    assert gains == set() and left is owed
    assert rig.logged("ERROR", "Could not record the shard layout in")
    assert len(rig.pods_of("ns-a")) == 2
