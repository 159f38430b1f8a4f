"""The native pod cache (``_kwcore.PodCache``, ops/csrc/podcache.inc) behaves
exactly like the Python ``PodCache`` (ops/cache.py) under any sequence of
operations, including None fields, non-ASCII text and checkpoint round trips."""

import json

from hypothesis import given, settings, strategies as st

from k8s_watcher_amd.engine.checkpoint import load_checkpoint, save_checkpoint
from k8s_watcher_amd.ops.cache import MISSING, PodCache, make_pod_cache

UIDS = ("u1", "u2", "ü3", None)
NAMESPACES = ["Running", "Pending", "", "ns-é", "default"]
uids = st.sampled_from(UIDS)
texts = st.one_of(st.none(), st.sampled_from(NAMESPACES))
sigs = st.sampled_from([0, 1, 2**64 - 1])
times = st.sampled_from([0, -2**63, 2**63 - 1, 100])
scopes = st.one_of(st.none(), st.sampled_from(NAMESPACES), st.just("never-seen"))
cores = st.one_of(st.none(), st.sampled_from([b'{"a":1}', '{"n":"é"}'.encode()]))
ops = st.lists(st.one_of(
    st.tuples(st.just("observe"), st.sampled_from(["ADDED", "MODIFIED", "DELETED"]), uids, texts, texts, texts,
              texts),
    st.tuples(st.just("set_core"), uids, st.sampled_from([b"{}", b'{"x":"y"}'])),
    st.tuples(st.just("put"), uids, texts, texts, texts, texts, cores),
    st.tuples(st.just("pop"), uids),
    st.tuples(st.sampled_from(["swap_failure", "swap_condition", "swap_terminating"]), uids, sigs),
    st.tuples(st.sampled_from(["set_deadline", "set_pending_since"]), uids, st.one_of(st.none(), times)),
    st.tuples(st.just("keep_core"), uids, st.sampled_from([b"{}", b'{"k":"pending"}'])),
    st.tuples(st.sampled_from(["take_overdue", "take_pending_overdue"]), times, times, scopes),
), max_size=40)


def snapshot(c):
    # The Python entry list grows a slot per signature once a swap_* stored one
    # and the native get/items never show them: the first five elements are the
    # entry both engines expose (all of it when no signature was swapped in).
    return sorted(((u or "", u is None), e[:5]) for u, e in c.items())


def entry(c, u):
    e = c.get(u)
    return e if e is None else e[:5]  # as snapshot()


def alert_state(c):
    return ([(c.deadline(u), c.pending_since(u), c.core_kept(u)) for u in UIDS], c.tracked(), c.pending_tracked())


@settings(max_examples=200, deadline=None)
@given(seq=ops)
def test_native_cache_matches_python(seq):
    py, nat = PodCache(), make_pod_cache(True)
    for op in seq:
        name, args = op[0], op[1:]
        r1 = getattr(py, name)(*args)
        r2 = getattr(nat, name)(*args)
        if name == "observe":
            assert (r1 is MISSING) == (r2 is MISSING) and (r1 is MISSING or r1 == r2)
        elif name.startswith("take_"):
            assert sorted(r1, key=repr) == sorted(r2, key=repr)
        elif name == "pop":
            assert (r1 if r1 is None else r1[:5]) == r2  # as snapshot()
        else:
            assert r1 == r2
        assert len(py) == len(nat)
        assert alert_state(py) == alert_state(nat)
    assert snapshot(py) == snapshot(nat)
    for u in UIDS:
        assert (u in py) == (u in nat)
        assert entry(py, u) == entry(nat, u)
        for swap in ("swap_failure", "swap_condition", "swap_terminating"):
            assert getattr(py, swap)(u, 0) == getattr(nat, swap)(u, 0)
    recs = sorted(nat.to_records(), key=json.dumps)
    assert recs == sorted(py.to_records(), key=json.dumps)
    again = make_pod_cache(True, recs)
    assert snapshot(again) == snapshot(py)


def test_native_cache_checkpoint_round_trip(tmp_path):
    nat = make_pod_cache(True)
    nat.observe("ADDED", "a", "1", "Running", "default", "p-é")
    nat.set_core("a", '{"name":"p-é"}'.encode())
    nat.observe("ADDED", "b", "2", None, None, None)
    path = str(tmp_path / "ck.json")
    save_checkpoint(path, {"*": "2"}, nat)
    scopes, loaded, _, _ = load_checkpoint(path, native_cache=True)
    assert scopes == {"*": "2"}
    assert type(loaded) is type(nat)
    assert snapshot(loaded) == snapshot(nat)
    _, py, _, _ = load_checkpoint(path)
    assert snapshot(py) == snapshot(nat)


def test_count_namespace_native_matches_python():
    from k8s_watcher_amd.ops.cache import PodCache
    from k8s_watcher_amd.ops.native import load
    caches = [load().PodCache(), PodCache()]
    for c in caches:
        for i in range(30):
            c.put(f"u{i}", str(i), "Running", None if i % 7 == 0 else f"ns{i % 3}", f"p{i}", None)
        c.pop("u4")
    for ns in ("ns0", "ns1", "ns2", "nope", None):
        assert caches[0].count_namespace(ns) == caches[1].count_namespace(ns)
    assert caches[0].count_namespace("nope") == 0
