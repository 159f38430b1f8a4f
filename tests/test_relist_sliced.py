"""The sliced native relist (``ops/csrc/relist.inc``) where its slices matter:
a namespace past the 4096-pod shortcut, hash tables large enough that the
collect walk stops inside a shard, and other scopes at work on the same
``PodCache`` between two slices — a second relist, watch events, a rehash of
every shard table, ``Relist.restart()`` in mid-page and in mid-sweep, and a
hand-over's ``drop_namespaces``. Plus the LIST's ``remainingItemCount`` hint,
which must never cost more than its cap (``test_size_hint_is_bounded``).

Slicing is deterministic: every native slice runs with ``budget_us = 0``,
which (``parse_budget`` and the loops) is one 128-item batch per ``step``,
one stop per 1024 buckets of the collect walk and one stop per 64 deletions
of ``sweep``. Nothing here depends on wall time.

The oracle is the Python engine over a Python ``PodCache`` shared by one
``EventPipeline`` per scope, populated identically, with everything applied
unsliced: the other scope's watch lines through ``handle_batch``, each relist
as one ``reconcile(..., scope_ns=...)``. A scope's relist touches only its own
namespace's entries, so the other scope's events commute with it and the
unsliced run is a valid oracle for the interleaved one. Expected
``Relist.stats()`` counts come from how each scenario is built (``shape``).

The ``check_*`` functions are called by the host tier too
(``tests/test_gpu_host_relist.py``)."""

import functools
import json
import random
import subprocess
import sys

import pytest

from conftest import ROOT
from k8s_watcher_amd.ops.cache import make_pod_cache
from k8s_watcher_amd.ops.decode import PyDecoder
from k8s_watcher_amd.ops.native import load
from k8s_watcher_amd.testing.podgen import PodFactory, event_line
from test_native_relist import COUNTERS, make, norm_cache, python_relist, strip_ts, with_rv

ENV = "staging"  # no critical filter, no namespace filter: every change is a notification
SHARDS = 16  # PodStore::SHARDS (ops/csrc/podcache.inc): the tables the collect walk goes through
HINT = 300_000  # remainingItemCount of a relist's first page: ~19k buckets per shard table
HINT_GROW = 900_000  # ... of the relist that makes every shard table rehash (case 5)
BIG_PODS = 4200  # just past sweep_collect's 4096-pod for_each_in shortcut
STAT_KEYS = ("listed", "added", "modified", "unchanged", "deleted")
POOLS = [False, True]
POOL_IDS = ["no-pool", "shared-pool3"]


@functools.lru_cache(maxsize=None)
def shared_pool():
    """One ``DecodePool(3)`` for every pipeline of every case, as
    ``WatcherService._scope_pipeline`` shares the runtime's pool."""
    return load().DecodePool(3)


# ----------------------------------------------------------------------------- scenarios

def bare_pod(ns, i, rv, phase):
    return {"metadata": {"name": f"p{i}", "namespace": ns, "uid": f"{ns}-u{i:05d}", "resourceVersion": str(rv)},
            "status": {"phase": phase}}


class Shape:
    """One namespace: what is cached before the relist (``lines`` through the
    watch path, so with a payload core; ``puts`` with ``core=None``), the LIST
    of its later state, and the counts that construction implies."""

    def __init__(self, ns, lines, puts, items, expect):
        self.ns, self.lines, self.puts, self.items, self.expect = ns, lines, puts, items, expect


@functools.lru_cache(maxsize=None)
def shape(ns, seed, n, rich, new):
    """``n`` cached pods, the first ``rich`` of them from podgen watch lines.
    The LIST keeps every second one, a third of those with a new
    resourceVersion, and has ``new`` pods the cache lacks. Never mutated."""
    f = PodFactory(seed, [ns])
    lines, puts, items = [], [], []
    expect = dict.fromkeys(STAT_KEYS, 0)
    for i in range(n):
        keep = i % 2 == 0
        changed = keep and (i // 2) % 3 == 0
        if i < rich:
            pod = f.running(f.new_pod(ns))
            lines.append(event_line("ADDED", with_rv(pod, 1000 + i)))
            later = with_rv(f.terminated(pod), 5000 + i) if changed else with_rv(pod, 1000 + i)
        else:
            puts.append((f"{ns}-u{i:05d}", str(1000 + i), "Running", ns, f"p{i}"))
            later = bare_pod(ns, i, 5000 + i, "Succeeded") if changed else bare_pod(ns, i, 1000 + i, "Running")
        if not keep:
            expect["deleted"] += 1  # cached, not listed: swept
            continue
        items.append(later)
        expect["listed"] += 1
        expect["modified" if changed else "unchanged"] += 1
    for k in range(new):
        items.append(with_rv(f.running(f.new_pod(ns)), 9000 + k) if k % 10 == 0
                     else bare_pod(ns, n + k, 9000 + k, "Running"))
        expect["listed"] += 1
        expect["added"] += 1
    random.Random(seed).shuffle(items)
    return Shape(ns, b"".join(lines), tuple(puts), items, expect)


def big():
    return shape("big", 31, BIG_PODS, 300, 100)


def big2():
    return shape("big2", 32, BIG_PODS, 40, 100)


def small():
    return shape("small", 33, 40, 10, 4)


def list_body(items, remaining=None, cont=None, rv="99999"):
    md = {"resourceVersion": rv}
    if cont:
        md["continue"] = cont
    if remaining is not None:
        md["remainingItemCount"] = remaining
    return json.dumps({"kind": "PodList", "apiVersion": "v1", "metadata": md, "items": items},
                      separators=(",", ":"), ensure_ascii=False).encode()


def bodies(items, hint=HINT, page=1000):
    """The LIST in pages of ``page`` items; the first carries the size hint."""
    out = []
    for i in range(0, max(1, len(items)), page):
        last = i + page >= len(items)
        out.append(list_body(items[i:i + page], remaining=hint if i == 0 else None,
                             cont=None if last else f"tok{i + page}"))
    return out


def add_expect(*shapes):
    return {k: sum(s.expect[k] for s in shapes) for k in STAT_KEYS}


# ----------------------------------------------------------------------------- the two engines

class World:
    """One engine's side of a case: a pipeline per scope name over one cache."""

    def __init__(self, native, names, pool):
        self.native = native
        self.cache = make_pod_cache(native)
        self.pipes, self.recs, self.metrics, self.c0 = {}, {}, {}, {}
        for name in names:
            self.pipes[name], self.recs[name], self.metrics[name] = make(
                ENV, {}, native, pool=(shared_pool() if pool else 0) if native else None, cache=self.cache)
            assert self.pipes[name].cache is self.cache

    def populate(self, name, sh):
        p = self.pipes[name]
        if sh.lines:
            ctrl = (p.handle_raw(sh.lines, 0, framed=False) if self.native
                    else p.handle_batch(PyDecoder(ENV).feed(sh.lines), 0))
            assert ctrl == []
        for rec in sh.puts:
            self.cache.put(*rec)

    def settle(self):
        """The cache is built: what follows is what the case compares."""
        for name, rec in self.recs.items():
            rec.calls.clear()
            self.c0[name] = {k: self.metrics[name].c[k] for k in COUNTERS}

    def delta(self, name):
        return {k: self.metrics[name].c[k] - self.c0[name][k] for k in COUNTERS}

    def watch(self, name, lines):
        p = self.pipes[name]
        ctrl = (p.handle_raw(lines, 0, framed=False) if self.native
                else p.handle_batch(PyDecoder(ENV).feed(lines), 0))
        assert ctrl == []


def worlds(names, pool, content):
    """(python, native), each with ``content``: (pipeline name, shape) pairs."""
    py, nat = World(False, names, pool), World(True, names, pool)
    for w in (py, nat):
        for name, sh in content:
            w.populate(name, sh)
    assert norm_cache(py.cache) == norm_cache(nat.cache)
    py.settle()
    nat.settle()
    return py, nat


def slices(p, rl, pages):
    """The native relist one slice per ``next()``: ("step" | "sweep", done)."""
    for body in pages:
        rl.page(body)
        done = False
        while not done:
            done, ctrl = p.native_slice(rl.step, 0, 0)
            assert ctrl == []
            yield "step", done
    done = False
    while not done:
        done, ctrl = p.native_slice(rl.sweep, 0, 0)
        assert ctrl == []
        yield "sweep", done


def deleted(rec):
    return [c for c in rec.calls if c[1] == "DELETED"]


def assert_no_duplicates(calls):
    seen = set()
    for c in calls:
        assert (c[0], c[1]) not in seen, f"sent twice: {c[0]} {c[1]}"
        seen.add((c[0], c[1]))


def assert_parity(py, nat):
    for name in py.pipes:
        assert_no_duplicates(nat.recs[name].calls)
        assert strip_ts(py.recs[name].calls) == strip_ts(nat.recs[name].calls), name
        assert py.delta(name) == nat.delta(name), name
    assert norm_cache(py.cache) == norm_cache(nat.cache)


def stats(rl):
    st = rl.stats()
    return {k: st[k] for k in STAT_KEYS}


def run_counting_walk(p, rec, rl, pages):
    """Run the relist to its end; the sweep's not-done slices before the
    first DELETED, which is how many times the collect walk stopped."""
    walk = 0
    for phase, done in slices(p, rl, pages):
        if phase == "sweep" and not done and not deleted(rec):
            walk += 1
    return walk


@functools.lru_cache(maxsize=None)
def undisturbed_walk():
    """The collect walk's stops for ``big`` with nothing else going on: what
    case 5's walks are compared with to show that their tables grew."""
    w = World(True, ["big"], False)
    w.populate("big", big())
    w.populate("big", small())
    w.settle()
    return run_counting_walk(w.pipes["big"], w.recs["big"], w.pipes["big"].native.relist("big", True),
                             bodies(big().items))


# ----------------------------------------------------------------------------- cases 1-7

def check_resumed_walk_namespace(pool):
    """Case 1: ``big`` alone, the walk resumed from ``sweep_bucket`` within each shard."""
    py, nat = worlds(["big"], pool, [("big", big()), ("big", small())])
    assert python_relist(py.pipes["big"], big().items, "big") == []
    p = nat.pipes["big"]
    rl = p.native.relist("big", True)
    walk = run_counting_walk(p, nat.recs["big"], rl, bodies(big().items))
    # more stops than shard tables: at least one table was left and re-entered
    # in mid-walk (otherwise this case tests nothing the shortcut does not)
    assert walk > SHARDS, walk
    assert_parity(py, nat)
    assert stats(rl) == big().expect
    assert len(deleted(nat.recs["big"])) == big().expect["deleted"]


def check_resumed_walk_cluster(pool):
    """Case 2: an unscoped relist of the same cache content, alone on its pipeline."""
    py, nat = worlds(["all"], pool, [("all", big()), ("all", small())])
    items = big().items + small().items
    random.Random(2).shuffle(items)
    assert python_relist(py.pipes["all"], items, None) == []
    p = nat.pipes["all"]
    rl = p.native.relist(None, True)
    walk = run_counting_walk(p, nat.recs["all"], rl, bodies(items))
    assert walk > SHARDS, walk  # as in case 1
    assert_parity(py, nat)
    assert stats(rl) == add_expect(big(), small())


def check_two_relists_at_once(pool):
    """Case 3: two scopes' relists over one cache, one slice each in turn."""
    py, nat = worlds(["big", "big2"], pool, [("big", big()), ("big2", big2())])
    for sh in (big(), big2()):
        assert python_relist(py.pipes[sh.ns], sh.items, sh.ns) == []
    rls = {sh.ns: nat.pipes[sh.ns].native.relist(sh.ns, True) for sh in (big(), big2())}
    live = [slices(nat.pipes[sh.ns], rls[sh.ns], bodies(sh.items)) for sh in (big(), big2())]
    turns = 0
    while live:
        for g in list(live):
            if next(g, None) is None:
                live.remove(g)
        turns += 1
    assert turns > SHARDS
    assert_parity(py, nat)
    for sh in (big(), big2()):
        assert stats(rls[sh.ns]) == sh.expect, sh.ns


def watch_batches(seed, ns):
    """Endless watch batches for ``ns``: four ADDED and, from the second on,
    DELETED of half of the batch before."""
    f = PodFactory(seed, [ns])
    prev, rv = [], 20000
    while True:
        pods = []
        for _ in range(4):
            rv += 1
            pods.append(with_rv(f.running(f.new_pod(ns)), rv))
        yield b"".join([event_line("ADDED", p) for p in pods]
                       + [event_line("DELETED", p) for p in prev[:len(prev) // 2]])
        prev = pods


def check_watch_between_slices(pool):
    """Case 4: another scope's watch inserts and erases between ``big``'s slices."""
    py, nat = worlds(["big", "other"], pool, [("big", big()), ("other", small())])
    p = nat.pipes["big"]
    rl = p.native.relist("big", True)
    traffic = watch_batches(44, "other")
    fed = []
    phases = {"step": 0, "sweep": 0}
    for phase, done in slices(p, rl, bodies(big().items)):
        fed.append(next(traffic))
        nat.watch("other", fed[-1])
        phases[phase] += 1
    assert phases["step"] > 2 and phases["sweep"] > SHARDS
    py.watch("other", b"".join(fed))
    assert python_relist(py.pipes["big"], big().items, "big") == []
    assert len(nat.recs["other"].calls) == 4 * len(fed) + 2 * (len(fed) - 1)  # by construction of the batches
    assert_parity(py, nat)
    assert stats(rl) == big().expect


def check_rehash_in_mid_walk(pool, where):
    """Case 5: every shard table grows while ``big``'s collect walk is under
    way (``where``: early, middle or late in it): the walk starts its current
    shard again and still reports every pod once."""
    quiet = undisturbed_walk()
    at = {"early": 2, "middle": quiet // 2, "late": quiet - 4}[where]
    assert 0 < at < quiet
    py, nat = worlds(["big", "small"], pool, [("big", big()), ("small", small())])
    p, rec = nat.pipes["big"], nat.recs["big"]
    rl = p.native.relist("big", True)
    rl_small = nat.pipes["small"].native.relist("small", True)
    walk = 0
    for phase, done in slices(p, rl, bodies(big().items)):
        if phase != "sweep" or done or deleted(rec):
            continue
        walk += 1
        if walk == at:  # the other scope's relist, whole, with the larger hint
            for _ in slices(nat.pipes["small"], rl_small, bodies(small().items, hint=HINT_GROW)):
                pass
    # the tables grew: the rest of the walk had more buckets to go through
    # than the undisturbed one (a walk that was over at `at` would count `at`)
    assert walk > quiet, (walk, quiet)
    for sh in (big(), small()):
        assert python_relist(py.pipes[sh.ns], sh.items, sh.ns) == []
    assert_parity(py, nat)
    assert stats(rl) == big().expect
    assert stats(rl_small) == small().expect


def check_restart_under_slicing(pool, again):
    """Case 6: ``restart()`` after exactly one batch of a page that has a
    ``continue`` token, then the whole LIST unpaginated. ``again``: a second
    ``restart()`` and the LIST once more, five slices into the sweep ("walk":
    still collecting) or once deletions are out ("deletes"); None for neither.
    What the abandoned pages applied is a prefix of the same LIST, so in the
    end every pod is reported once, as in the one-shot oracle."""
    py, nat = worlds(["big"], pool, [("big", big()), ("big", small())])
    assert python_relist(py.pipes["big"], big().items, "big") == []
    p, rec = nat.pipes["big"], nat.recs["big"]
    items = big().items
    rl = p.native.relist("big", True)
    first = bodies(items)[0]
    rl.page(first)
    done, ctrl = p.native_slice(rl.step, 0, 0)
    assert not done and ctrl == []
    batch = 128  # RELIST_BATCH: what one step with no budget applies
    assert stats(rl)["listed"] == batch
    assert rl.page_meta() == ("99999", "tok1000")
    rl.restart()
    whole = [list_body(items, remaining=HINT)]
    relisted = 1
    n = 0
    for phase, done in slices(p, rl, whole):
        n += phase == "sweep"
        if (again == "walk" and n == 5) or (again == "deletes" and len(deleted(rec)) >= 128):
            assert not done
            assert (len(deleted(rec)) == 0) == (again == "walk")
            break
    if again:
        rl.restart()
        relisted = 2
        for _ in slices(p, rl, whole):
            pass
    assert_parity(py, nat)
    e = big().expect
    # every item seen counts as listed; one applied by an abandoned pass is unchanged in the next
    assert stats(rl) == {"listed": batch + relisted * e["listed"], "added": e["added"], "modified": e["modified"],
                         "unchanged": e["unchanged"] + batch + (relisted - 1) * e["listed"],
                         "deleted": e["deleted"]}


def check_handover_between_sweep_slices(pool):
    """Case 7: the namespace is handed over (``drop_namespaces``) once the
    collect walk is done and some deletions are out."""
    py, nat = worlds(["big"], pool, [("big", big()), ("big", small())])
    assert python_relist(py.pipes["big"], big().items, "big") == []
    p, rec = nat.pipes["big"], nat.recs["big"]
    rl = p.native.relist("big", True)
    dropped = None
    for phase, done in slices(p, rl, bodies(big().items)):
        if dropped is None and len(deleted(rec)) >= 3 * 64:
            assert phase == "sweep" and not done
            dropped = nat.cache.drop_namespaces(["big"])
    e = big().expect
    sent = deleted(rec)
    assert dropped == e["listed"] + e["deleted"] - len(sent)  # what the LIST had, and what was still to sweep
    assert 0 < len(sent) < e["deleted"]
    assert_no_duplicates(rec.calls)
    oracle = strip_ts(py.recs["big"].calls)
    assert set(strip_ts(sent)) <= set(oracle)
    assert strip_ts(c for c in rec.calls if c[1] != "DELETED") == [c for c in oracle if c[1] != "DELETED"]
    assert nat.cache.count_namespace("big") == 0
    assert norm_cache(nat.cache) == {u: ent for u, ent in norm_cache(py.cache).items() if ent[2] != "big"}
    assert nat.cache.count_namespace("small") == len(small().puts) + small().lines.count(b"\n")


@pytest.mark.parametrize("pool", POOLS, ids=POOL_IDS)
def test_resumed_walk_namespace(pool):
    check_resumed_walk_namespace(pool)


@pytest.mark.parametrize("pool", POOLS, ids=POOL_IDS)
def test_resumed_walk_cluster(pool):
    check_resumed_walk_cluster(pool)


@pytest.mark.parametrize("pool", POOLS, ids=POOL_IDS)
def test_two_relists_at_once(pool):
    check_two_relists_at_once(pool)


@pytest.mark.parametrize("pool", POOLS, ids=POOL_IDS)
def test_watch_between_slices(pool):
    check_watch_between_slices(pool)


@pytest.mark.parametrize("where", ["early", "middle", "late"])
@pytest.mark.parametrize("pool", POOLS, ids=POOL_IDS)
def test_rehash_in_mid_walk(pool, where):
    check_rehash_in_mid_walk(pool, where)


@pytest.mark.parametrize("again", [None, "walk", "deletes"], ids=["once", "again-in-walk", "again-after-deletes"])
@pytest.mark.parametrize("pool", POOLS, ids=POOL_IDS)
def test_restart_under_slicing(pool, again):
    check_restart_under_slicing(pool, again)


@pytest.mark.parametrize("pool", POOLS, ids=POOL_IDS)
def test_handover_between_sweep_slices(pool):
    check_handover_between_sweep_slices(pool)


# ----------------------------------------------------------------------------- case 8: contract pins

def test_page_on_unconsumed_page_raises():
    p, _, _ = make(ENV, {}, True, pool=0)
    rl = p.native.relist(None, True)
    rl.page(list_body(big().items[:300]))
    with pytest.raises(RuntimeError, match="not consumed"):
        rl.page(list_body([]))
    assert p.native_slice(rl.step, 0, 0) == (False, [])  # one batch in: still unconsumed
    with pytest.raises(RuntimeError, match="not consumed"):
        rl.page(list_body([]))


def test_step_without_page_raises():
    p, _, _ = make(ENV, {}, True, pool=0)
    rl = p.native.relist(None, True)
    with pytest.raises(RuntimeError, match="no page"):
        rl.step(0, 0)
    rl.page(list_body([]))
    assert p.native_slice(rl.step, 0, 0) == (True, [])
    with pytest.raises(RuntimeError, match="no page"):  # a consumed page is released
        rl.step(0, 0)


@pytest.mark.parametrize("pool", POOLS, ids=POOL_IDS)
def test_silent_relist_at_this_shape(pool):
    py, nat = worlds(["big"], pool, [("big", big()), ("big", small())])
    assert python_relist(py.pipes["big"], big().items, "big", notify=False) == []
    p = nat.pipes["big"]
    rl = p.native.relist("big", False)
    walk = run_counting_walk(p, nat.recs["big"], rl, bodies(big().items))
    assert walk > SHARDS
    assert py.recs["big"].calls == nat.recs["big"].calls == []
    ca, cb = norm_cache(py.cache), norm_cache(nat.cache)
    assert set(ca) == set(cb)
    assert {u: e[:4] for u, e in ca.items()} == {u: e[:4] for u, e in cb.items()}
    e = big().expect
    assert nat.cache.count_namespace("big") == e["listed"]


# ----------------------------------------------------------------------------- the size hint

# relist.inc clamps remainingItemCount to RELIST_HINT_MAX = 2^22 pods before
# PodStore::reserve. A bucket of the shard tables is one pointer (8 bytes), so
# the hint costs at most 2^22 x 8 B = 32 MiB of bucket arrays over the whole
# store. The bound on what one step may add to the process is 8 times that.
HINT_CAP = 1 << 22
HINT_RSS_BOUND = 8 * HINT_CAP * 8  # 256 MiB
HINT_VALUES = ["99999999999", "4294967296", "3000000000", "100000000000", "-5", "1.5e9", '"7"', "null", "true"]

_HINT_CHILD = r"""
import json, resource, sys
resource.setrlimit(resource.RLIMIT_AS, (8 << 30, 8 << 30))
root, values = sys.argv[1], json.loads(sys.argv[2])
sys.path[:0] = [root, root + "/tests"]
from test_native_relist import make

def rss():  # (high-water mark, now), bytes
    with open("/proc/self/statm") as fh:
        now = int(fh.read().split()[1]) * resource.getpagesize()
    return resource.getrusage(resource.RUSAGE_SELF).ru_maxrss * 1024, now

def item(rv):
    return json.dumps({"metadata": {"name": "a", "namespace": "default", "uid": "ua", "resourceVersion": rv},
                       "status": {"phase": "Running"}})

def page(hint, rv):
    return ('{"kind":"PodList","metadata":{"resourceVersion":"7","remainingItemCount":%s},"items":[%s]}'
            % (hint, item(rv))).encode()

out = []
for text in values:
    p, rec, _ = make("staging", {}, True, pool=0)
    for i in range(3):
        p.cache.put("old%d" % i, "1", "Running", "default", "old%d" % i)
    rl = p.native.relist(None, True)
    rl.page(page(text, "1"))
    before = rss()
    done, ctrl = p.native_slice(rl.step, 0, 0)
    after = rss()
    assert done and ctrl == [], (text, done, ctrl)
    assert [(c[0], c[1]) for c in rec.calls] == [("ua", "ADDED")], (text, rec.calls)
    assert p.cache.get("ua")[:4] == ["1", "Running", "default", "a"], text
    while not p.native_slice(rl.sweep, 0, 0)[0]:
        pass
    assert sorted((c[0], c[1]) for c in rec.calls[1:]) == [("old%d" % i, "DELETED") for i in range(3)], text
    assert len(p.cache) == 1 and rl.stats()["deleted"] == 3, text
    rl = p.native.relist(None, True)  # and the cache still takes a second relist
    rl.page(page(text, "2"))
    assert p.native_slice(rl.step, 0, 0) == (True, []), text
    while not p.native_slice(rl.sweep, 0, 0)[0]:
        pass
    assert [(c[0], c[1]) for c in rec.calls[4:]] == [("ua", "MODIFIED")], text
    assert len(p.cache) == 1 and p.cache.get("ua")[0] == "2", text
    out.append({"hint": text, "maxrss": after[0] - before[0], "rss": after[1] - before[1]})
print(json.dumps(out))
"""


def test_size_hint_is_bounded():
    """``metadata.remainingItemCount`` exists to avoid a rehash: whatever the
    server sends there, the page is applied, the relist and the next one work,
    and the step adds less than ``HINT_RSS_BOUND`` to the process — in a child
    with an 8 GiB address-space limit, where an unclamped hint of 3e9 pods and
    more ends the process (std::bad_alloc, status 134)."""
    res = subprocess.run([sys.executable, "-c", _HINT_CHILD, ROOT, json.dumps(HINT_VALUES)], capture_output=True,
                         text=True, cwd=ROOT, timeout=120)
    assert res.returncode == 0, (res.returncode, res.stdout[-1000:], res.stderr[-2000:])
    rows = json.loads(res.stdout.strip().splitlines()[-1])
    print(rows)
    assert [r["hint"] for r in rows] == HINT_VALUES
    for r in rows:
        assert r["maxrss"] < HINT_RSS_BOUND and r["rss"] < HINT_RSS_BOUND, r
