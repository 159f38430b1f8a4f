"""Where the hand-over across a restart (engine/handover.py
``reshard_on_start``) and the new owner's wait (``_await_handover``) could lose
or mis-take state: a record that could not be written, a second restart under
the layout a re-shard led to, and a live move that finds an old record of its
own layout. Then a model of whole re-shards: every surviving shard of a random
old and new count, with what each wrote checked against what each was owed.
Same rig as test_handover.py: Python cache, a temporary directory, no API
server and no native extension. The end-to-end case is in test_sharding.py."""

import asyncio
import collections
import json
import os
import random
import time

import pytest
from conftest import run
from k8s_watcher_amd.engine import handover as handover_mod
from k8s_watcher_amd.parallel.shard import (_decode, layout_of, owner_of, owners_of, record_layout, shard_of,
                                            take_handover, write_handover, write_manifest)
from k8s_watcher_amd.utils.config import ShardSettings
from test_handover import PODS, Rig, _names

DAY = 86400.0
NAMES = _names()  # six namespaces each of the two old shards


def _split(names, index=0, old=2, new=3):
    """Shard ``index``'s namespaces under ``old`` shards, under ``new``, and
    of those: handed out, kept, gained."""
    held = [n for n in names if shard_of(n, old) == index]
    scopes = [n for n in names if shard_of(n, new) == index]
    return (held, scopes, sorted(n for n in held if n not in scopes), sorted(n for n in held if n in scopes),
            {n for n in scopes if n not in held})


def _fail_writes(monkeypatch, fails):
    """``write_handover`` raises for the namespaces ``fails(ns)`` says."""
    real = handover_mod.write_handover

    def write(directory, ns, *a, **kw):
        if fails(ns):
            raise OSError(28, "No space left on device")
        return real(directory, ns, *a, **kw)

    monkeypatch.setattr(handover_mod, "write_handover", write)


def _records(hdir):
    return sorted(x for x in os.listdir(hdir) if x.endswith(".handover.json"))


def _set_since(hdir, current, previous, since):
    """The layout history as the first shard under ``current`` left it at ``since``."""
    with open(os.path.join(str(hdir), "layout.json"), "w") as f:
        json.dump({"current": current, "previous": previous, "since": since}, f)


def _restart(tmp_path, names=NAMES, index=0, old=2, new=3, wait=0.3, cache=None, saved=None, owed=()):
    """Shard ``index`` starts under ``new`` shards: ``(rig, gains, owed left)``.
    Without ``saved`` its checkpoint is the one it shut down with under ``old``."""
    held, scopes, _, _, _ = _split(names, index, old, new)
    rig = Rig(tmp_path, index=index, count=new, wait=wait)
    if cache is not None:
        rig.cache = cache
    elif saved is None:
        for k, ns in enumerate(held):
            rig.fill(ns, 1 + k % 3)
    saved = {ns: "55" for ns in held} if saved is None else saved
    gains, left = rig.handover.reshard_on_start(scopes, names, saved, list(owed))
    return rig, gains, left


async def _others_do_their_part(rig, gains, out, old=2):
    """What the other shards of the re-shard do: take the records addressed to
    them, and write the one each of ``rig``'s gains waits for, which it takes."""
    sh = rig.shard
    for ns in out:
        assert take_handover(sh.handover_dir, ns, shard_of(ns, sh.count), layout=layout_of(sh)) is not None
    for ns in sorted(gains):
        write_handover(sh.handover_dir, ns, shard_of(ns, old), sh.index,
                       [(f"{ns}-g", "5", "Running", "pod-g", b'{"phase":"Running"}')], None, layout_of(sh))
        rig.handover.begin_gain(ns)
    await rig.until(lambda: len(rig.called("start")) == len(gains))
    assert rig.handover.gaining() == set() and rig.metrics.c["shard_handovers_in"] == len(gains)
    assert _records(sh.handover_dir) == []


def _checkpoint(rig, scopes):
    """What the shard's next checkpoint holds: its namespaces' pods and resume points."""
    rig.cache.drop_namespaces_except(set(scopes))
    return rig.cache, {ns: "60" for ns in scopes}


# ---------------------------------------------------------------- a record that could not be written
def test_failed_write_keeps_its_owed_notifications(tmp_path, monkeypatch):
    held, scopes, out, kept, _ = _split(NAMES)
    assert len(out) >= 2 and kept
    failing, written = out[0], out[1]
    record_layout(str(tmp_path), layout_of(ShardSettings(count=2)))
    _fail_writes(monkeypatch, lambda ns: ns == failing)
    owed = [("u-f0", "MODIFIED", failing, "a", b"one"), ("u-w", "MODIFIED", written, "b", b"two"),
            ("u-f1", "DELETED", failing, "c", b"three\xff"), ("u-k", "ADDED", kept[0], "d", b"four")]

    rig, _, left = _restart(tmp_path, owed=owed)

    assert left == [owed[0], owed[2], owed[3]]  # the failing namespace's and the kept one's, in their order
    assert _records(tmp_path) == sorted(f"{ns}.handover.json" for ns in out if ns != failing)
    layout = layout_of(rig.shard)
    for ns in out[1:]:
        rec = take_handover(str(tmp_path), ns, shard_of(ns, 3), layout=layout)
        assert rec.owed == ([owed[1]] if ns == written else []) and sorted(rec.pods) == rig.pods_of(ns)
    c = rig.metrics.c
    assert c["shard_handover_errors"] == 1 and c["shard_handovers_out"] == len(out) - 1
    assert c["shard_handover_pods_out"] == sum(len(rig.pods_of(ns)) for ns in out[1:])
    assert rig.logged("ERROR", f"Could not write the hand-over of namespace {failing}")
    assert rig.logged("ERROR", "2 owed notification(s) are re-sent here")


def test_every_write_failing_keeps_the_whole_owed_list(tmp_path, monkeypatch):
    held, scopes, out, kept, want_gains = _split(NAMES)
    record_layout(str(tmp_path), layout_of(ShardSettings(count=2)))
    _fail_writes(monkeypatch, lambda ns: True)
    owed = [("u-0", "MODIFIED", out[0], "a", b"one"), ("u-1", "ADDED", kept[0], "b", b"two"),
            ("u-2", "DELETED", out[1], "c", b"three"), ("u-3", "DELETED", out[0], "d", b"four")]

    rig, gains, left = _restart(tmp_path, owed=owed)

    assert left == owed
    assert gains == want_gains  # what this shard waits for does not depend on what it could write
    assert _records(tmp_path) == []
    c = rig.metrics.c
    assert c["shard_handover_errors"] == len(out) and c["shard_handovers_out"] == 0 == c["shard_handover_pods_out"]


# ---------------------------------------------------------------- the second restart under a layout
def _late_namespace(old_owner, new_owner, old=2, new=3):
    return next(n for n in (f"late-{i}" for i in range(400))
                if shard_of(n, old) == old_owner and shard_of(n, new) == new_owner)


@pytest.mark.parametrize("variant", ["checkpoint_intact", "checkpoint_lost", "new_namespace", "layout_a_day_old"])
def test_second_restart_under_the_same_layout_is_a_plain_restart(tmp_path, variant):
    """The re-shard 2 -> 3 is done for shard 0 once its records are out and its
    gains have ended. Whatever it starts with after that — its checkpoint, no
    checkpoint, a namespace created since that shard 1 would have owned under
    count 2, a layout that began a day ago (another shard started under it
    then; this one a day later, in a slow rolling update) — it waits for
    nobody and writes nothing: nobody would answer, and nobody is waiting."""
    held, scopes, out, kept, want_gains = _split(NAMES)
    l2, l3 = layout_of(ShardSettings(count=2)), layout_of(ShardSettings(count=3))

    async def body():
        record_layout(str(tmp_path), l2)
        if variant == "layout_a_day_old":
            _set_since(tmp_path, l3, l2, time.time() - DAY)
        first, gains, _ = _restart(tmp_path)
        assert gains == want_gains and _records(tmp_path) == sorted(f"{ns}.handover.json" for ns in out)
        await _others_do_their_part(first, gains, out)
        cache, saved = _checkpoint(first, scopes)
        listing = sorted(os.listdir(tmp_path))

        names, owns = list(NAMES), list(scopes)
        if variant == "checkpoint_lost":
            cache, saved = None, {}
        if variant == "new_namespace":
            late = _late_namespace(1, 0)
            names.append(late)
            owns.append(late)
        owed = [("u-k", "MODIFIED", kept[0], "a", b"one"), ("u-g", "DELETED", sorted(gains)[0], "b", b"two")]
        again = Rig(tmp_path, index=0, count=3)
        if cache is not None:
            again.cache = cache
        gains2, left = again.handover.reshard_on_start(owns, names, saved, list(owed))
        assert gains2 == set()
        assert sorted(os.listdir(tmp_path)) == listing and _records(tmp_path) == []
        assert left == owed
        assert again.metrics.c["shard_handovers_out"] == 0 and again.calls == []

    run(body(), timeout=10)


def test_a_reshard_whose_gains_timed_out_or_were_cancelled_is_settled_too(tmp_path):
    held, scopes, out, kept, want_gains = _split(NAMES)
    assert len(want_gains) >= 2

    async def body():
        record_layout(str(tmp_path), layout_of(ShardSettings(count=2)))
        first, gains, _ = _restart(tmp_path, wait=0.1)
        cancelled = sorted(gains)[0]
        for ns in sorted(gains):
            first.handover.begin_gain(ns)
        assert first.handover.cancel_gain(cancelled)  # deleted before its record came
        await first.until(lambda: len(first.called("start")) == len(gains) - 1)
        assert first.metrics.c["shard_handover_timeouts"] == len(gains) - 1
        for ns in out:
            take_handover(str(tmp_path), ns, shard_of(ns, 3))
        listing = sorted(os.listdir(tmp_path))
        again, gains2, _ = _restart(tmp_path, saved={})
        assert gains2 == set() and sorted(os.listdir(tmp_path)) == listing and _records(tmp_path) == []

    run(body(), timeout=10)


def test_a_shard_stopped_while_a_gain_waited_waits_for_it_again(tmp_path):
    held, scopes, out, kept, want_gains = _split(NAMES)
    assert len(want_gains) >= 2
    l3 = layout_of(ShardSettings(count=3))

    async def body():
        record_layout(str(tmp_path), layout_of(ShardSettings(count=2)))
        first, gains, _ = _restart(tmp_path, wait=5.0)
        handed = {ns: first.pods_of(ns) for ns in out}
        assert any(handed.values())
        pending, taken = sorted(gains)[0], sorted(gains)[1:]
        for ns in taken:
            write_handover(str(tmp_path), ns, 1, 0, PODS, None, l3)
        for ns in sorted(gains):
            first.handover.begin_gain(ns)
        await first.until(lambda: len(first.called("start")) == len(taken))
        first.stop.set()  # shard 1 has not restarted yet: pending's record never came
        await asyncio.wait(first.handover.tasks(), timeout=2)
        assert ("start", pending, True) not in first.calls

        # its checkpoint: what it kept and what it took, not the namespace it still waited for
        cache, saved = _checkpoint(first, [n for n in scopes if n != pending])
        second, gains2, _ = _restart(tmp_path, cache=cache, saved=saved, wait=5.0)
        assert gains2 == {pending}  # not settled: shard 1's record is still to come
        # the records of its first start, which nobody has taken yet, are not replaced by empty ones
        assert second.metrics.c["shard_handovers_out"] == 0
        write_handover(str(tmp_path), pending, 1, 0, PODS, None, l3)
        second.handover.begin_gain(pending)
        await second.until(lambda: second.called("start"))
        assert second.metrics.c["shard_handovers_in"] == 1 and second.metrics.c["shard_handover_timeouts"] == 0
        for ns in out:  # the other shards, starting only now, find what the first start left them
            assert sorted(take_handover(str(tmp_path), ns, shard_of(ns, 3), layout=l3).pods) == handed[ns]

        cache, saved = _checkpoint(second, scopes)
        listing = sorted(os.listdir(tmp_path))
        third, gains3, _ = _restart(tmp_path, cache=cache, saved=saved)
        assert gains3 == set() and sorted(os.listdir(tmp_path)) == listing and _records(tmp_path) == []
        assert third.metrics.c["shard_handovers_out"] == 0

    run(body(), timeout=10)


def test_an_unsettled_restart_writes_again_what_was_taken_or_is_too_old(tmp_path):
    """Before its part is done a shard runs the re-shard again. For a namespace
    it no longer holds it writes an empty record ("do not wait for me") unless
    its own earlier record is still there for the taking: one that was taken,
    or that the new owner would refuse as older than the layout, is written."""
    held, scopes, out, kept, want_gains = _split(NAMES)
    assert len(out) >= 3
    record_layout(str(tmp_path), layout_of(ShardSettings(count=2)))
    first, gains, _ = _restart(tmp_path)
    taken, old, there = out[0], out[1], out[2:]
    assert take_handover(str(tmp_path), taken, shard_of(taken, 3)) is not None
    _age_record(first.record_path(old), 3600)
    cache, saved = _checkpoint(first, [ns for ns in scopes if ns not in gains])
    second, gains2, _ = _restart(tmp_path, cache=cache, saved=saved)
    assert gains2 == gains and second.metrics.c["shard_handovers_out"] == 2
    layout = layout_of(second.shard)
    for ns in (taken, old):
        rec = take_handover(str(tmp_path), ns, shard_of(ns, 3), not_before=second.handover._layout_since - 60,
                            layout=layout)
        assert rec is not None and rec.pods == []
    assert _records(tmp_path) == sorted(f"{ns}.handover.json" for ns in there)


def test_going_back_to_an_earlier_layout_is_a_new_reshard(tmp_path):
    """2 -> 3 -> 2 -> 3: every start under a count that differs from the one
    before hands out and gains as the first did, although shard 0 has settled
    under count 3 before — that was another time."""
    _, under3, out3, _, gains3 = _split(NAMES, old=2, new=3)
    _, under2, out2, _, gains2 = _split(NAMES, old=3, new=2)
    assert out2 and gains2
    l2, l3 = layout_of(ShardSettings(count=2)), layout_of(ShardSettings(count=3))

    async def body():
        record_layout(str(tmp_path), l2)
        first, gains, _ = _restart(tmp_path)
        await _others_do_their_part(first, gains, out3)
        cache, saved = _checkpoint(first, under3)

        back, gains, _ = _restart(tmp_path, old=3, new=2, cache=cache, saved=saved)
        assert gains == gains2
        assert _records(tmp_path) == sorted(f"{ns}.handover.json" for ns in out2)
        assert back.metrics.c["shard_handovers_out"] == len(out2)
        for ns in out2:
            rec = take_handover(str(tmp_path), ns, 1, layout=l2)
            assert rec is not None and rec.src == 0
        # stopped before its gains came: not settled under count 2, its checkpoint what it kept
        cache, saved = _checkpoint(back, [ns for ns in under2 if ns in under3])
        again, gains, _ = _restart(tmp_path, old=2, new=3, cache=cache, saved=saved)
        assert gains == {ns for ns in under3 if ns not in under2}
        assert again.metrics.c["shard_handovers_out"] == len([ns for ns in under2 if ns not in under3])

    run(body(), timeout=10)


# ---------------------------------------------------------------- an old record of the same layout
def _age_record(path, seconds):
    with open(path) as f:
        doc = json.load(f)
    doc["written_at"] = time.time() - seconds
    with open(path, "w") as f:
        json.dump(doc, f)


def _live_rig(tmp_path, wait):
    """Shard 0 of two, running under a layout that began a day ago."""
    rig = Rig(tmp_path, index=0, count=2, wait=wait)
    _set_since(tmp_path, layout_of(rig.shard), None, time.time() - DAY)
    assert rig.handover.reshard_on_start(["ns-b"], ["ns-a", "ns-b"], {"ns-b": "5"}, []) == (set(), [])
    assert rig.handover._layout_since < time.time() - DAY + 60
    return rig


def test_live_gain_removes_an_old_record_of_its_own_layout_and_times_out(tmp_path):
    async def body():
        rig = _live_rig(tmp_path, wait=0.2)
        write_handover(str(tmp_path), "ns-a", 1, 0, PODS, [("u", "DELETED", "ns-a", "p", b"x")], layout_of(rig.shard))
        _age_record(rig.record_path("ns-a"), 3600)  # an earlier move's, whose new owner had timed out
        rig.handover.begin_gain("ns-a")  # the namespace set changed: a live move
        await rig.until(lambda: not os.path.exists(rig.record_path("ns-a")))
        assert rig.calls == []  # removed at the first look, not taken
        await rig.until(lambda: rig.called("start"))
        assert rig.calls == [("start", "ns-a", True)] and rig.pods_of("ns-a") == []
        c = rig.metrics.c
        assert c["shard_handover_timeouts"] == 1 and c["shard_handovers_in"] == 0 and c["shard_handover_pods_in"] == 0

    run(body(), timeout=10)


def test_live_gain_takes_the_record_written_while_it_waits(tmp_path):
    async def body():
        rig = _live_rig(tmp_path, wait=2.0)
        write_handover(str(tmp_path), "ns-a", 1, 0, PODS[:1], None, layout_of(rig.shard))
        _age_record(rig.record_path("ns-a"), 3600)
        rig.handover.begin_gain("ns-a")
        await rig.until(lambda: not os.path.exists(rig.record_path("ns-a")))
        write_handover(str(tmp_path), "ns-a", 1, 0, PODS, None, layout_of(rig.shard))  # this move's
        await rig.until(lambda: rig.called("start"))
        assert rig.calls == [("start", "ns-a", True)] and rig.pods_of("ns-a") == sorted(PODS)
        c = rig.metrics.c
        assert c["shard_handovers_in"] == 1 and c["shard_handover_pods_in"] == 2 and c["shard_handover_timeouts"] == 0

    run(body(), timeout=10)


def test_start_time_gain_takes_a_record_written_since_the_layout_began(tmp_path):
    """The other direction: the old owner restarted 90 s ago under a layout
    that began 100 s ago, and this shard only now. Older than any live move's
    record may be (60 s), and still this re-shard's."""
    held, scopes, out, kept, want_gains = _split(NAMES)
    l2, l3 = layout_of(ShardSettings(count=2)), layout_of(ShardSettings(count=3))

    async def body():
        record_layout(str(tmp_path), l2)
        _set_since(tmp_path, l3, l2, time.time() - 100)
        rig, gains, _ = _restart(tmp_path, wait=0.3)
        assert gains == want_gains
        ns = sorted(gains)[0]
        write_handover(str(tmp_path), ns, 1, 0, PODS, None, l3)
        _age_record(rig.record_path(ns), 90)
        rig.handover.begin_gain(ns)
        await rig.until(lambda: rig.called("start"))
        assert rig.metrics.c["shard_handovers_in"] == 1 and rig.metrics.c["shard_handover_timeouts"] == 0
        assert len(rig.pods_of(ns)) == 2

    run(body(), timeout=10)


# ---------------------------------------------------------------- a model of whole re-shards
SEEDS = 200


@pytest.mark.parametrize("assignment", ["hash", "balanced"])
def test_owners_of_answers_as_owner_of_does(assignment):
    names = [f"ns-{i}" for i in range(23)]
    for count in (1, 2, 3, 5):
        owner = owners_of(names, count, assignment)
        for ns in names + ["not-in-the-set"]:
            assert owner(ns) == owner_of(ns, names, count, assignment), (count, ns)


def _model_seed(hdir, seed, fail_p, monkeypatch):
    """One re-shard ``a`` -> ``b`` shards, every surviving shard simulated on
    the shared directory ``hdir``; asserts the invariants (module doc of the
    test below)."""
    rng = random.Random(seed)
    a, b = rng.sample(range(2, 6), 2)
    assignment = rng.choice(["hash", "balanced"])
    names = sorted({f"ns-{rng.randrange(10 ** 6)}" for _ in range(40)})[:rng.randint(8, 30)]
    rng.shuffle(names)
    tag = f"seed {seed}: {a} -> {b} shards, {assignment}, {len(names)} namespaces, failing writes {fail_p}"
    was = {n: owner_of(n, names, a, assignment) for n in names}
    now = {n: owner_of(n, names, b, assignment) for n in names}
    old_layout = layout_of(ShardSettings(count=a, assignment=assignment))
    record_layout(hdir, old_layout)
    failed = set()  # namespaces whose record could not be written

    def failing(ns):
        if rng.random() < fail_p:
            failed.add(ns)
            return True
        return False

    _fail_writes(monkeypatch, failing)
    order = list(range(b))
    rng.shuffle(order)
    shards, records = {}, {}
    for i in order:
        rig = Rig(hdir, index=i, count=b, wait=0.0, assignment=assignment)
        held = [n for n in names if was[n] == i]  # nothing for an ordinal the old count did not have
        for ns in held:
            rig.fill(ns, rng.randint(0, 2))
        owed = [(f"u{i}-{k}", rng.choice(["ADDED", "MODIFIED", "DELETED"]), rng.choice(held), f"pod-{k}",
                 b"body-%d" % k) for k in range(rng.randint(0, 6))] if held else []
        scopes = [n for n in names if now[n] == i]
        before = set(os.listdir(hdir))
        tried = set(failed)
        gains, left = rig.handover.reshard_on_start(scopes, names, {ns: "7" for ns in held}, list(owed))
        wrote = {}
        for x in sorted(set(os.listdir(hdir)) - before):
            if x.endswith(".handover.json"):
                with open(os.path.join(hdir, x)) as f:
                    wrote[x[:-len(".handover.json")]] = json.load(f)
        not_written = failed - tried
        # conservation
        assert left == [o for o in owed if o[2] in scopes or o[2] in not_written], tag
        carried = collections.Counter(left)
        for ns, doc in wrote.items():
            assert doc["from"] == i and doc["namespace"] == ns and ns not in records, (tag, ns)
            rec = _decode(doc)
            assert rec.owed == [o for o in owed if o[2] == ns], (tag, ns)
            assert sorted(rec.pods) == rig.pods_of(ns), (tag, ns)
            carried.update(rec.owed)
        assert carried == collections.Counter(owed), tag
        assert set(wrote) == {ns for ns in held if now[ns] != i} - not_written, tag
        assert gains == {ns for ns in scopes if was[ns] != i}, tag
        c = rig.metrics.c
        assert c["shard_handovers_out"] == len(wrote) and c["shard_handover_errors"] == len(not_written), tag
        records.update(wrote)
        shards[i] = (rig, scopes, gains, owed)
    for ns, doc in records.items():  # no stray record
        assert doc["to"] == now[ns] and ns in shards[doc["to"]][2], (tag, ns)
    for i, (_, _, gains, _) in shards.items():  # no orphan gain
        for ns in gains:
            if was[ns] < b:
                assert (ns in records) != (ns in failed), (tag, i, ns)
                assert ns in failed or (records[ns]["from"], records[ns]["to"]) == (was[ns], i), (tag, i, ns)
    monkeypatch.undo()

    # settling: every gain ends (a removed ordinal's manifest says it left nothing), then
    # each shard starts again, with the checkpoint it would have by then and with none
    for gone in range(b, a):
        write_manifest(hdir, gone, old_layout, [])

    async def gain_all():
        for rig, _, gains, _ in shards.values():
            for ns in sorted(gains):
                rig.handover.begin_gain(ns)
        await asyncio.gather(*(t for rig, _, _, _ in shards.values() for t in rig.handover.tasks()))
        for rig, _, gains, _ in shards.values():
            assert len(rig.called("start")) == len(gains), tag

    run(gain_all(), timeout=10)
    taken = sum(rig.metrics.c["shard_handovers_in"] for rig, _, _, _ in shards.values())
    assert taken == len(records) and _records(hdir) == [], tag
    listing = sorted(os.listdir(hdir))
    for i, (rig, scopes, _, owed) in shards.items():
        rig.cache.drop_namespaces_except(set(scopes))
        for cache, saved in ((rig.cache, {ns: "8" for ns in scopes}), (None, {})):
            again = Rig(hdir, index=i, count=b, wait=0.0, assignment=assignment)
            if cache is not None:
                again.cache = cache
            kept = [o for o in owed if o[2] in scopes]
            assert again.handover.reshard_on_start(scopes, names, saved, list(kept)) == (set(), kept), (tag, i)
            assert sorted(os.listdir(hdir)) == listing and again.metrics.c["shard_handovers_out"] == 0, (tag, i)


@pytest.mark.parametrize("fail_p", [0.0, 0.2], ids=["writes_succeed", "a_fifth_of_writes_fail"])
def test_model_of_whole_reshards(tmp_path, monkeypatch, fail_p):
    """Every surviving shard of a re-shard between two counts of 2..5, ``hash``
    or ``balanced``, over 8-30 namespaces, each with the checkpoint it shut
    down with (0-2 pods a namespace, 0-6 owed notifications), started in a
    shuffled order on one directory. For each shard, of what it is owed: what
    it keeps to re-send plus what its records carry is the whole list, each
    part in the original order, and it keeps exactly the notifications of
    namespaces it still owns and of records it could not write (conservation).
    Every record is addressed to the namespace's new owner, who waits for it
    (no stray record). Every gain from an ordinal that still exists has its one
    record, unless that write failed (no orphan gain). And once all gains have
    ended, a further start of any shard, with or without a checkpoint, gains
    nothing and writes nothing (settling)."""
    t0 = time.monotonic()
    for seed in range(SEEDS):
        hdir = tmp_path / str(seed)
        hdir.mkdir()
        with monkeypatch.context() as m:
            _model_seed(str(hdir), seed, fail_p, m)
    print(f"{SEEDS} seeds, failing writes {fail_p}: {time.monotonic() - t0:.1f}s")
