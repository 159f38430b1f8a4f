"""Scale-down hand-over on its own (engine/handover.py ``part``,
``reclaim_on_start`` and the parting path of ``_await_handover``): a shard
that shuts down writes parting records and a manifest, the new owner of a
removed ordinal's namespace takes them without a blind wait, and an ordinal
that comes back discards what was taken from it. Same rig as
test_handover.py: Python cache, fake notifier, a temporary directory. The
end-to-end cases are in test_scale_down.py."""

import asyncio
import json
import os
import time

from conftest import run
from k8s_watcher_amd.engine import handover as handover_mod
from k8s_watcher_amd.parallel.shard import (layout_of, read_manifest, record_layout, shard_of, take_parting,
                                            write_handover, write_manifest, write_parting)
from k8s_watcher_amd.utils.config import ShardSettings
from test_handover import OWED, PODS, Rig

OLD = ShardSettings(count=3)  # the layout the removed ordinal (2) ran under
NEW = 2


def _ns_of(old_owner, new_owner, skip=0):
    """A namespace shard ``old_owner`` of three owned and shard ``new_owner`` of two owns."""
    found = [n for n in (f"ns-{i}" for i in range(400)) if shard_of(n, 3) == old_owner and shard_of(n, 2) == new_owner]
    return found[skip]


def _parting_path(d, ns):
    return os.path.join(str(d), f"{ns}.parting.json")


def _resharded_rig(tmp_path, index, names, wait=0.4, saved_rvs=None):
    """Shard ``index`` of two starting where three shards ran before: the
    layout history says so, and its gains are decided."""
    record_layout(str(tmp_path), layout_of(OLD))
    rig = Rig(tmp_path, index=index, count=NEW, wait=wait)
    scopes = [n for n in names if shard_of(n, NEW) == index]
    gains, _ = rig.handover.reshard_on_start(scopes, names, saved_rvs or {}, [])
    return rig, gains


# ---------------------------------------------------------------- the shard that stops
def test_parting_writes_a_record_per_namespace_then_the_manifest(tmp_path, monkeypatch):
    async def body():
        rig = Rig(tmp_path, index=2, count=3)
        rig.fill("ns-a", 3)
        rig.fill("ns-b", 2)
        owed = [("ns-a-u1", "MODIFIED", "ns-a", "pod-1", b'{"n":1}\xff'), ("ns-b-u0", "DELETED", "ns-b", "pod-0", b"x"),
                ("ns-a-u0", "DELETED", "ns-a", "pod-0", b"y")]
        pods = {ns: [(u, e[0], e[1], e[3], e[4]) for u, e in rig.cache.items() if e[2] == ns]
                for ns in ("ns-a", "ns-b", "ns-empty")}
        manifest_seen = []
        real = handover_mod.write_parting

        def probing(directory, ns, *a):
            manifest_seen.append(os.path.exists(os.path.join(directory, "shard-2.parted.json")))
            return real(directory, ns, *a)

        monkeypatch.setattr(handover_mod, "write_parting", probing)
        done = await rig.handover.part(pods, owed, budget=5.0)
        assert sorted(done) == ["ns-a", "ns-b", "ns-empty"]
        assert manifest_seen == [False] * 3  # the manifest comes after every record
        assert sorted(os.listdir(tmp_path)) == ["ns-a.parting.json", "ns-b.parting.json", "ns-empty.parting.json",
                                                "shard-2.parted.json"]
        manifest = read_manifest(str(tmp_path), 2)
        assert manifest["namespaces"] == ["ns-a", "ns-b", "ns-empty"] and manifest["layout"] == layout_of(rig.shard)
        for ns in pods:
            with open(_parting_path(tmp_path, ns)) as f:
                doc = json.load(f)
            assert doc["from"] == 2 and "to" not in doc and doc["layout"] == layout_of(rig.shard)
            assert doc["written_at"] == manifest["written_at"]
            rec = take_parting(str(tmp_path), ns, 2, layout=layout_of(rig.shard))
            assert sorted(rec.pods) == rig.pods_of(ns) and rec.src == 2
            assert rec.owed == [o for o in owed if o[2] == ns]  # its own, in their order
        c = rig.metrics.c
        assert c["shard_partings_out"] == 3 and c["shard_parting_pods_out"] == 5 and c["shard_handover_errors"] == 0
        assert c["shard_handovers_out"] == 0  # the restart path's counters stay its own
        assert rig.calls == [] and len(rig.cache) == 5  # the cache is left as it is: a plain restart needs it

    run(body(), timeout=10)


def test_parting_leaves_a_failed_record_off_the_manifest(tmp_path, monkeypatch):
    async def body():
        rig = Rig(tmp_path, index=2, count=3)
        rig.fill("ns-a", 1)
        rig.fill("ns-b", 2)
        real = handover_mod.write_parting

        def failing(directory, ns, *a):
            if ns == "ns-a":
                raise OSError(28, "No space left on device")
            return real(directory, ns, *a)

        monkeypatch.setattr(handover_mod, "write_parting", failing)
        done = await rig.handover.part({"ns-a": rig.pods_of("ns-a"), "ns-b": rig.pods_of("ns-b")}, [], budget=5.0)
        assert done == ["ns-b"] and read_manifest(str(tmp_path), 2)["namespaces"] == ["ns-b"]
        assert sorted(os.listdir(tmp_path)) == ["ns-b.parting.json", "shard-2.parted.json"]
        c = rig.metrics.c
        assert c["shard_handover_errors"] == 1 and c["shard_partings_out"] == 1 and c["shard_parting_pods_out"] == 2
        assert rig.logged("ERROR", "Could not write the parting record of namespace ns-a")

    run(body(), timeout=10)


def test_parting_past_its_budget_lists_only_what_was_written(tmp_path, monkeypatch):
    async def body():
        rig = Rig(tmp_path, index=2, count=3)
        real = handover_mod.write_parting
        release = []

        def slow(directory, ns, *a):
            if ns == "ns-slow":
                while not release:
                    time.sleep(0.01)
            return real(directory, ns, *a)

        monkeypatch.setattr(handover_mod, "write_parting", slow)
        t0 = time.monotonic()
        try:
            done = await rig.handover.part({"ns-quick": [], "ns-slow": []}, [], budget=0.15)
        finally:
            release.append(True)
        assert 0.15 <= time.monotonic() - t0 < 0.4
        assert done == ["ns-quick"] and read_manifest(str(tmp_path), 2)["namespaces"] == ["ns-quick"]
        assert rig.logged("WARNING", "1 of 2 namespace records not written within 0.15s")

    run(body(), timeout=10)


# ---------------------------------------------------------------- the new owner
def test_gain_from_a_removed_ordinal_takes_its_parting_record_at_once(tmp_path):
    ns = _ns_of(2, 0)
    pods = [(u.replace("ns-a", ns), rv, ph, nm, core) for u, rv, ph, nm, core in PODS]
    owed = [(u.replace("ns-a", ns), et, ns, nm, body) for u, et, _, nm, body in OWED]

    async def body():
        write_parting(str(tmp_path), ns, 2, pods, owed, layout_of(OLD))
        write_manifest(str(tmp_path), 2, layout_of(OLD), [ns])
        rig, gains = _resharded_rig(tmp_path, 0, [ns])
        assert gains == {ns}
        t0 = time.monotonic()
        rig.handover.begin_gain(ns)
        await rig.until(lambda: rig.called("start"))
        assert time.monotonic() - t0 < 0.1
        assert rig.calls == [("owed", owed), ("start", ns, True)]  # owed first, then the primed scope
        assert rig.pods_of(ns) == sorted(pods)
        assert not os.path.exists(_parting_path(tmp_path, ns))  # consumed
        assert os.path.exists(tmp_path / "shard-2.parted.json")  # the manifest is its writer's to remove
        c = rig.metrics.c
        assert c["shard_partings_in"] == 1 and c["shard_parting_pods_in"] == 2
        assert c["shard_handovers_in"] == 0 and c["shard_handover_timeouts"] == 0 and c["shard_parting_missing"] == 0
        assert rig.handover.gaining() == set()

    run(body(), timeout=10)


def test_manifest_without_a_record_starts_the_watch_at_once(tmp_path):
    ns = _ns_of(2, 0)

    async def body():
        write_manifest(str(tmp_path), 2, layout_of(OLD), [])
        rig, gains = _resharded_rig(tmp_path, 0, [ns], wait=0.4)
        assert gains == {ns}
        t0 = time.monotonic()
        rig.handover.begin_gain(ns)
        await rig.until(lambda: rig.called("start"))
        assert time.monotonic() - t0 < 0.1
        assert rig.calls == [("start", ns, True)]
        c = rig.metrics.c
        assert c["shard_parting_missing"] == 1 and c["shard_handover_timeouts"] == 0 and c["shard_partings_in"] == 0
        assert rig.logged("WARNING", f"Shard 2 stopped without a parting record of namespace {ns}")

    run(body(), timeout=10)


def test_without_a_manifest_the_gain_waits_and_times_out(tmp_path):
    ns = _ns_of(2, 0)

    async def body():
        rig, _ = _resharded_rig(tmp_path, 0, [ns], wait=0.3)
        t0 = time.monotonic()
        rig.handover.begin_gain(ns)
        await rig.until(lambda: rig.called("start"))
        assert time.monotonic() - t0 >= 0.3
        assert rig.calls == [("start", ns, True)]
        c = rig.metrics.c
        assert c["shard_handover_timeouts"] == 1 and c["shard_parting_missing"] == 0 and c["shard_partings_in"] == 0
        assert rig.logged("WARNING", "its pods are announced as ADDED again")

    run(body(), timeout=10)


def test_a_record_that_appears_during_the_wait_is_taken(tmp_path):
    ns = _ns_of(2, 0)

    async def body():
        rig, _ = _resharded_rig(tmp_path, 0, [ns], wait=0.4)
        rig.handover.begin_gain(ns)
        await asyncio.sleep(0.12)  # the removed shard is still shutting down
        assert rig.calls == []
        write_parting(str(tmp_path), ns, 2, PODS, None, layout_of(OLD))
        write_manifest(str(tmp_path), 2, layout_of(OLD), [ns])
        await rig.until(lambda: rig.called("start"))
        assert rig.calls == [("start", ns, True)] and len(rig.pods_of(ns)) == 2
        c = rig.metrics.c
        assert c["shard_partings_in"] == 1 and c["shard_handover_timeouts"] == 0 and c["shard_parting_missing"] == 0

    run(body(), timeout=10)


def test_stale_parting_records_are_removed_and_not_taken(tmp_path):
    other, old = _ns_of(2, 0), _ns_of(2, 0, skip=1)

    async def body():
        rig, gains = _resharded_rig(tmp_path, 0, [other, old], wait=0.3)
        assert gains == {other, old}
        # of another layout than the previous one; and of the previous one, but
        # from before anything this reshard could have written
        write_parting(str(tmp_path), other, 2, PODS, OWED, layout_of(ShardSettings(count=5)))
        bound = rig.handover._layout_since - rig.shard.handover_wait_seconds - 60
        write_parting(str(tmp_path), old, 2, PODS, OWED, layout_of(OLD), written_at=bound - 1)
        for ns in (other, old):
            rig.handover.begin_gain(ns)
        await rig.until(lambda: not os.path.exists(_parting_path(tmp_path, other))
                        and not os.path.exists(_parting_path(tmp_path, old)))
        assert rig.calls == []  # removed at the first look, nothing taken
        await rig.until(lambda: len(rig.called("start")) == 2)
        assert rig.called("owed") == [] and len(rig.cache) == 0
        c = rig.metrics.c
        assert c["shard_handover_timeouts"] == 2 and c["shard_partings_in"] == 0

    run(body(), timeout=10)


def test_a_record_at_the_staleness_bound_is_taken(tmp_path):
    ns = _ns_of(2, 0)

    async def body():
        rig, _ = _resharded_rig(tmp_path, 0, [ns], wait=0.3)
        bound = rig.handover._layout_since - rig.shard.handover_wait_seconds - 60
        write_parting(str(tmp_path), ns, 2, PODS, None, layout_of(OLD), written_at=bound)
        rig.handover.begin_gain(ns)
        await rig.until(lambda: rig.called("start"))
        assert rig.metrics.c["shard_partings_in"] == 1

    run(body(), timeout=10)


def test_a_parting_record_of_another_shard_is_left_alone(tmp_path):
    ns = _ns_of(2, 0)

    async def body():
        rig, _ = _resharded_rig(tmp_path, 0, [ns], wait=0.2)
        write_parting(str(tmp_path), ns, 1, PODS, OWED, layout_of(OLD))  # shard 1 never owned it
        rig.handover.begin_gain(ns)
        await rig.until(lambda: rig.called("start"))
        assert rig.calls == [("start", ns, True)] and rig.metrics.c["shard_handover_timeouts"] == 1
        assert os.path.exists(_parting_path(tmp_path, ns))

    run(body(), timeout=10)


def test_gain_from_a_surviving_ordinal_waits_for_its_restart_record(tmp_path):
    ns = _ns_of(1, 0)  # shard 1 is still there under two shards: it restarts and hands over

    async def body():
        rig, gains = _resharded_rig(tmp_path, 0, [ns], wait=0.4)
        assert gains == {ns}
        write_parting(str(tmp_path), ns, 1, PODS, OWED, layout_of(OLD))  # its shutdown's: not for taking
        write_manifest(str(tmp_path), 1, layout_of(OLD), [ns])
        rig.handover.begin_gain(ns)
        await asyncio.sleep(0.12)
        assert rig.calls == [] and os.path.exists(_parting_path(tmp_path, ns))
        write_handover(str(tmp_path), ns, 1, 0, PODS, OWED, layout_of(rig.shard))  # shard 1, restarted
        await rig.until(lambda: rig.called("start"))
        assert rig.calls == [("owed", OWED), ("start", ns, True)]
        c = rig.metrics.c
        assert c["shard_handovers_in"] == 1 and c["shard_partings_in"] == 0 and c["shard_parting_missing"] == 0
        assert os.path.exists(_parting_path(tmp_path, ns))

    run(body(), timeout=10)


def test_live_gains_do_not_use_the_parting_path(tmp_path):
    ns = _ns_of(2, 0)

    async def body():
        rig = Rig(tmp_path, index=0, count=NEW, wait=0.2)
        write_parting(str(tmp_path), ns, 2, PODS, OWED, layout_of(OLD))
        write_manifest(str(tmp_path), 2, layout_of(OLD), [ns])
        rig.handover.begin_gain(ns)  # a namespace-set change, not a start under a new layout
        await rig.until(lambda: rig.called("start"))
        assert rig.calls == [("start", ns, True)] and rig.metrics.c["shard_handover_timeouts"] == 1
        assert os.path.exists(_parting_path(tmp_path, ns))

    run(body(), timeout=10)


# ---------------------------------------------------------------- the ordinal that comes back
def test_returning_ordinal_drops_what_was_taken_and_keeps_the_rest(tmp_path):
    async def body():
        old = Rig(tmp_path, index=2, count=3)
        old.fill("ns-a", 3)
        old.fill("ns-b", 2)
        await old.handover.part({"ns-a": old.pods_of("ns-a"), "ns-b": old.pods_of("ns-b")}, [], budget=5.0)
        assert take_parting(str(tmp_path), "ns-a", 2, layout=layout_of(old.shard)) is not None  # its next owner

        back = Rig(tmp_path, index=2, count=3)
        back.cache = old.cache  # the checkpoint on its retained volume
        kept = back.pods_of("ns-b")
        saved_rvs = {"ns-a": "5", "ns-b": "6"}
        owed = [("ns-a-u0", "MODIFIED", "ns-a", "pod-0", b"a"), ("ns-b-u0", "MODIFIED", "ns-b", "pod-0", b"b")]
        left = back.handover.reclaim_on_start(saved_rvs, owed)
        assert left == [owed[1]] and saved_rvs == {"ns-b": "6"}
        assert back.pods_of("ns-a") == [] and back.pods_of("ns-b") == kept
        assert back.called("forget") == [("forget", {"ns-a"})]
        assert os.listdir(tmp_path) == []  # ns-b's record and the manifest are gone
        assert back.logged("INFO", "1 namespace(s) were taken over from this shard while it was away")

    run(body(), timeout=10)


def test_plain_restart_after_a_parting_keeps_the_whole_checkpoint(tmp_path):
    names = ["ns-a", "ns-b", "ns-c"]

    async def body():
        first = Rig(tmp_path, index=0, count=1)
        assert first.handover.reshard_on_start(names, names, {}, []) == (set(), [])
        for ns in names[:2]:
            first.fill(ns, 2)
        await first.handover.part({ns: first.pods_of(ns) for ns in names}, [], budget=5.0)
        assert len(os.listdir(tmp_path)) == 5  # layout.json, three records, the manifest

        again = Rig(tmp_path, index=0, count=1)
        again.cache = first.cache
        saved_rvs = {ns: "9" for ns in names}
        owed = [("ns-a-u0", "MODIFIED", "ns-a", "pod-0", b"a")]
        left = again.handover.reclaim_on_start(saved_rvs, owed)
        assert left == owed and saved_rvs == {ns: "9" for ns in names} and len(again.cache) == 4
        assert again.handover.reshard_on_start(names, names, saved_rvs, left) == (set(), owed)
        assert os.listdir(tmp_path) == ["layout.json"]
        assert again.calls == []

    run(body(), timeout=10)


def test_start_without_a_manifest_changes_nothing(tmp_path):
    rig = Rig(tmp_path, index=2, count=3)
    rig.fill("ns-a", 2)
    write_parting(str(tmp_path), "ns-a", 2, PODS, None, layout_of(rig.shard))  # killed before the manifest
    owed = [("ns-a-u0", "MODIFIED", "ns-a", "pod-0", b"a")]
    saved_rvs = {"ns-a": "5"}
    assert rig.handover.reclaim_on_start(saved_rvs, owed) is owed
    assert saved_rvs == {"ns-a": "5"} and len(rig.cache) == 2 and rig.calls == []
