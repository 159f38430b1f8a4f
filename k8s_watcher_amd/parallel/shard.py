"""Sharding the pod space across watcher processes.

The reference is one process watching the whole cluster (SURVEY §5.7,
``/root/reference/watcher/pod_watcher.py:264``, client-side namespace filter
``:226-229``). For clusters whose event rate exceeds one core,
``watcher.shard.count`` watcher processes split the work.

Two ways to decide which shard owns what:

* **per event** (``namespace_scope: client``, or ``shard.key: uid``): every
  process watches the whole cluster and keeps the pods with
  ``crc32(key) % count == index`` — ``key`` is the namespace or the uid.
  Simple, but every process still receives every event.
* **per watch** (``namespace_scope: server`` with a namespace list, or
  ``namespace_scope: discover``): each process opens watches only for the
  namespaces it owns, so the API server sends each event to exactly one
  shard and the work really divides by ``count``. Which namespaces a shard
  owns is computed by every shard from the same namespace set:

  - ``shard.assignment: hash`` (default) — ``crc32(namespace) % count``:
    each namespace's owner depends on nothing else, so namespaces created or
    deleted later never move the others. Balance is statistical;
  - ``shard.assignment: balanced`` — consistent hashing with bounded loads
    (Mirrokni, Thorup & Zadimoghaddam, SODA 2018): namespaces, in hash
    order, take the first shard clockwise on a ring of virtual nodes that
    still has room under ``ceil(n / count)``, so every shard owns ``floor``
    or ``ceil`` of ``n / count`` namespaces. Meant for a fixed namespace
    set: when ``ceil(n / count)`` changes, a few namespaces move to another
    shard.

A namespace that moves is handed over when ``shard.handover_dir`` names a
directory all shards share (a ReadWriteMany volume,
``deploy/k8s/statefulset-sharded.yaml``). It moves in three ways:

* **live** — ``balanced`` on a namespace-set change: the old owner stops its
  watch, waits until clusterapi has acknowledged (or given up) every
  notification it still owes for the namespace (``pending_in``: a retried
  MODIFIED cannot land after the new owner's notifications for the same
  pod), then writes its cached pods there (:func:`write_handover`, one JSON
  file, atomically renamed);
* **across a restart** — a new shard count (``replicas`` and
  ``K8S_WATCHER_SHARD_COUNT`` changed together restart every shard): each
  shard notes the layout in the directory's history (:func:`record_layout`),
  so every shard, new ones included, knows the previous layout and which
  namespaces it gains from whom. An old owner, starting with a checkpoint
  that holds namespaces it no longer owns, writes their record — pods and the
  checkpoint's owed notifications for them — before it starts any watch.
  Each shard does that once: with its records out and its gains ended it
  leaves ``shard-<index>.settled.json`` (:func:`write_settled`), and a later
  start under the same layout, begun at the same time, is a plain restart;
* **at a scale-down** — a removed ordinal never starts under the new count,
  so it cannot write that record. Instead every shard that shuts down
  gracefully writes, from the cut of its final checkpoint, a *parting
  record* for each namespace it watches (:func:`write_parting`: pods and owed
  notifications, addressed to nobody, ``<namespace>.parting.json``) and then
  one manifest (:func:`write_manifest`, ``shard-<index>.parted.json``): "this
  shard has stopped watching, and these records are complete". A new owner
  whose namespace belonged to an ordinal the new count no longer has takes
  the parting record as soon as it is there; with the manifest there and no
  record it starts at once (the pods are re-announced, but nothing waits);
  with neither, the old shard is still watching, or was killed, and the wait
  below applies. A shard that does come back finds its own manifest: records
  still there are deleted (its checkpoint is the truth), namespaces whose
  record was taken are dropped from its checkpoint's state.

The new owner waits for that record (``shard.handover_wait_seconds``; while
the old owner has not restarted yet it still watches the namespace, so the
wait loses nothing), sends the record's owed notifications first, loads the
pods into its cache and only then LISTs — so pods that stayed are not
re-announced and a pod deleted while neither shard watched is reported
``DELETED`` by the new owner's reconcile, exactly once. Without the directory
(or if the old owner is gone and the wait runs out) the new owner's LIST
re-announces the pods as ``ADDED`` (at-least-once) and a deletion inside that
window is not reported; a record that comes after such a timeout is stale and
is discarded, not taken by a later move.

Both kinds of record are one format: :func:`_encode`, :func:`_decode`, and
:func:`_take` for what is stale.

crc32 is stable across processes and Python versions, unlike ``hash()``.
"""

from __future__ import annotations

import base64
import bisect
import json
import os
import time
import zlib
from typing import Callable, Dict, Iterable, List, NamedTuple, Optional, Sequence, Tuple

from ..utils.atomic import write_atomically
from ..utils.config import ShardSettings

VNODES = 64  # ring points per shard


def shard_of(key: Optional[str], count: int) -> int:
    if count <= 1:
        return 0
    return zlib.crc32((key or "").encode("utf-8")) % count


def _h(s: str) -> int:
    return zlib.crc32(s.encode("utf-8"))


def balanced_assignment(names: Iterable[str], count: int) -> Dict[str, int]:
    """Namespace → shard for ``count`` shards, with at most ``ceil(n / count)``
    namespaces per shard (bounded-load consistent hashing, see module doc).
    Deterministic: every shard computes the same map from the same set."""
    uniq = sorted(set(names))
    if count <= 1:
        return {n: 0 for n in uniq}
    ring = sorted((_h(f"shard-{s}#{v}"), s) for s in range(count) for v in range(VNODES))
    points = [p for p, _ in ring]
    cap = -(-len(uniq) // count)
    load = [0] * count
    out: Dict[str, int] = {}
    for name in sorted(uniq, key=lambda n: (_h(n), n)):
        i = bisect.bisect_left(points, _h(name))
        for step in range(len(ring)):
            s = ring[(i + step) % len(ring)][1]
            if load[s] < cap:
                break
        load[s] += 1
        out[name] = s
    return out


def owner_of(namespace: str, names: Iterable[str], count: int, assignment: str) -> int:
    """The shard owning ``namespace`` when the namespace set is ``names``."""
    if count <= 1:
        return 0
    if assignment == "hash":
        return shard_of(namespace, count)
    return balanced_assignment(list(names) + [namespace], count).get(namespace, 0)


def owners_of(names: Iterable[str], count: int, assignment: str) -> Callable[[str], int]:
    """:func:`owner_of` for many namespaces of one set: ``balanced`` is worked
    out once for ``names``, not once per question."""
    if count <= 1 or assignment == "hash":
        return lambda ns: shard_of(ns, count)
    names = set(names)
    table = balanced_assignment(names, count)
    return lambda ns: table[ns] if ns in table else owner_of(ns, names, count, assignment)


# ---------------------------------------------------------------- hand-over
HANDOVER_VERSION = 2

Pod = Tuple[str, Optional[str], Optional[str], Optional[str], Optional[bytes]]
Owed = Tuple[str, str, Optional[str], Optional[str], bytes]


class HandOver(NamedTuple):
    """A namespace's state from its old owner: its cached pods and the
    notifications for them that clusterapi had not acknowledged (the new
    owner sends those first, before anything of its own)."""
    pods: List[Pod]
    owed: List[Owed]
    src: int
    written_at: float


def _path(directory: str, stem: str, kind: str) -> str:
    """``<namespace>.handover.json``, ``<namespace>.parting.json``, ``shard-<index>.parted.json``,
    ``shard-<index>.settled.json``."""
    return os.path.join(directory, f"{stem}.{kind}.json")


def _encode(namespace: str, src: int, dst: Optional[int], pods: List[Pod], owed: Optional[List[Owed]],
            layout: Optional[dict], written_at: Optional[float]) -> dict:
    """The one record format, for both kinds of file: ``"to"`` only where the
    record is addressed to a shard. The keys stay in this order: shards of two
    versions share the directory during a rolling update."""
    doc = {"version": HANDOVER_VERSION, "namespace": namespace, "from": src}
    if dst is not None:
        doc["to"] = dst
    doc.update({"written_at": time.time() if written_at is None else written_at, "layout": layout,
                "pods": [[u, rv, ph, nm, core.decode("utf-8", "replace") if core is not None else None]
                         for u, rv, ph, nm, core in pods],
                "owed": [[u, et, ns, nm, base64.b64encode(body).decode("ascii")]
                         for u, et, ns, nm, body in owed or ()]})
    return doc


def _write_record(path: str, namespace: str, *fields) -> str:
    # (dumps: the C encoder, one pass. Encoded once the temporary file is open: a writer thread
    # whose first act is a system call lets go of the interpreter lock, and parting starts eight)
    write_atomically(path, lambda f: f.write(json.dumps(_encode(namespace, *fields), separators=(",", ":"))),
                     f".{namespace}.")
    return path


def _load(path: str, expect: dict) -> Optional[dict]:
    """The JSON document at ``path`` if it is of this version and says what
    ``expect`` says, else None (no file, half a file, somebody else's)."""
    try:
        with open(path) as f:
            doc = json.load(f)
    except (OSError, ValueError):
        return None
    if doc.get("version") != HANDOVER_VERSION or any(doc.get(k) != v for k, v in expect.items()):
        return None
    return doc


def _unlink(path: str) -> None:
    try:
        os.unlink(path)
    except OSError:
        pass


def _decode(doc: dict) -> HandOver:
    return HandOver([(u, rv, ph, nm, core.encode("utf-8") if core is not None else None)
                     for u, rv, ph, nm, core in doc.get("pods", [])],
                    [(u, et, ns, nm, base64.b64decode(body)) for u, et, ns, nm, body in doc.get("owed", [])],
                    int(doc.get("from", -1)), float(doc.get("written_at", 0.0)))


def _take(path: str, expect: dict, not_before: float, layout: Optional[dict]) -> Optional[HandOver]:
    """The record at ``path`` that says what ``expect`` says, consumed: the
    file goes, and a stale record — written before ``not_before``, or under
    another shard layout than ``layout`` — is not taken."""
    doc = _load(path, expect)
    if doc is None:
        return None
    stale = doc.get("written_at", 0.0) < not_before or (layout is not None and doc.get("layout") != layout)
    _unlink(path)
    return None if stale else _decode(doc)


def write_handover(directory: str, namespace: str, src: int, dst: int, pods: List[Pod],
                   owed: Optional[List[Owed]] = None, layout: Optional[dict] = None) -> str:
    """The old owner's cached pods of ``namespace`` — ``(uid, rv, phase, name,
    core)`` — and its owed notifications ``(uid, etype, ns, name, body)`` for
    shard ``dst``, stamped with the time and the shard layout it was written
    under; renamed into place, so a reader sees the whole record or none."""
    return _write_record(_path(directory, namespace, "handover"), namespace, src, dst, pods, owed, layout, None)


def take_handover(directory: str, namespace: str, dst: int, not_before: float = 0.0,
                  layout: Optional[dict] = None) -> Optional[HandOver]:
    """The record for shard ``dst`` if one is there (consumed: the file is
    removed), else None. Records addressed to another shard are left alone; a
    stale record for ``dst`` (an old move's whose new owner timed out, say) is
    removed and not taken: a late record must not prime a later move."""
    return _take(_path(directory, namespace, "handover"), {"namespace": namespace, "to": dst}, not_before, layout)


def has_handover(directory: str, namespace: str, src: int, not_before: float, layout: dict) -> bool:
    """Shard ``src``'s record of ``namespace`` is there, not taken yet, and its
    new owner would take it: written under ``layout``, not before ``not_before``."""
    doc = _load(_path(directory, namespace, "handover"), {"namespace": namespace, "from": src, "layout": layout})
    return doc is not None and doc.get("written_at", 0.0) >= not_before


# ---------------------------------------------------------------- parting (scale-down)
def write_parting(directory: str, namespace: str, src: int, pods: List[Pod], owed: Optional[List[Owed]] = None,
                  layout: Optional[dict] = None, written_at: Optional[float] = None) -> str:
    """Shard ``src``'s state of ``namespace`` as it stops watching: the same
    record as :func:`write_handover`'s, but addressed to nobody (a shard that
    shuts down does not know whether it will be back, nor who would own the
    namespace instead) and in a file of its own, ``<namespace>.parting.json``."""
    return _write_record(_path(directory, namespace, "parting"), namespace, src, None, pods, owed, layout, written_at)


def take_parting(directory: str, namespace: str, src: int, not_before: float = 0.0,
                 layout: Optional[dict] = None) -> Optional[HandOver]:
    """Shard ``src``'s parting record of ``namespace`` if one is there
    (consumed), else None. Another shard's record is left alone; a stale one
    of ``src`` (``layout``: the one ``src`` owned the namespace under) is
    removed and not taken, as :func:`take_handover` does."""
    return _take(_path(directory, namespace, "parting"), {"namespace": namespace, "from": src}, not_before, layout)


def discard_parting(directory: str, namespace: str, src: int) -> bool:
    """Remove shard ``src``'s own parting record of ``namespace``: True if it
    was still there (nobody took it), False if it is gone or another shard's."""
    path = _path(directory, namespace, "parting")
    if _load(path, {"namespace": namespace, "from": src}) is None:
        return False
    _unlink(path)
    return True


def write_manifest(directory: str, index: int, layout: dict, namespaces: Iterable[str],
                   written_at: Optional[float] = None) -> str:
    """Shard ``index`` has stopped watching, and the parting records of
    ``namespaces`` are complete: written after them, renamed atomically."""
    path = _path(directory, f"shard-{index}", "parted")
    doc = {"version": HANDOVER_VERSION, "shard": index, "layout": layout,
           "written_at": time.time() if written_at is None else written_at, "namespaces": sorted(namespaces)}
    write_atomically(path, lambda f: f.write(json.dumps(doc)), f".shard-{index}.")
    return path


def read_manifest(directory: str, index: int) -> Optional[dict]:
    """Shard ``index``'s manifest, or None: still running, or killed."""
    return _load(_path(directory, f"shard-{index}", "parted"), {"shard": index})


def remove_manifest(directory: str, index: int) -> None:
    _unlink(_path(directory, f"shard-{index}", "parted"))


# ---------------------------------------------------------------- layout history
def layout_of(s: ShardSettings) -> dict:
    """What decides namespace ownership: the shard count and the assignment."""
    return {"count": s.count, "assignment": s.assignment, "key": s.key}


def record_layout(directory: str, layout: dict) -> Tuple[Optional[dict], float]:
    """Note ``layout`` in the shared directory's history and return the layout
    before it and when this one began: ``(previous, since)``. Every shard of a
    resharded deployment (count 2 -> 3, say) sees the same previous layout,
    whichever starts first — the first to start under the new layout moves
    ``current`` to ``previous``; the others find ``current`` already theirs.
    ``(None, now)`` for a first deployment."""
    path = os.path.join(directory, "layout.json")
    try:
        with open(path) as f:
            hist = json.load(f)
    except (OSError, ValueError):
        hist = {}
    if hist.get("current") == layout:
        return hist.get("previous"), float(hist.get("since", 0.0))
    new = {"current": layout, "previous": hist.get("current"), "since": time.time()}
    write_atomically(path, lambda f: f.write(json.dumps(new)), ".layout.")
    return new["previous"], new["since"]


def write_settled(directory: str, index: int, layout: dict, since: float) -> str:
    """Shard ``index`` has done its part of the re-shard that led to ``layout``
    at ``since`` (:func:`record_layout`'s): its records are out and its
    start-time gains have ended. ``shard-<index>.settled.json``, one file per
    shard, so that no two shards rewrite the same one."""
    path = _path(directory, f"shard-{index}", "settled")
    doc = {"version": HANDOVER_VERSION, "shard": index, "layout": layout, "since": since}
    write_atomically(path, lambda f: f.write(json.dumps(doc)), f".shard-{index}.")
    return path


def is_settled(directory: str, index: int, layout: dict, since: float) -> bool:
    """Shard ``index``'s marker is there and names this ``layout`` and this
    ``since``: the same layout begun at another time (2 -> 3 -> 2) is another
    re-shard."""
    return _load(_path(directory, f"shard-{index}", "settled"),
                 {"shard": index, "layout": layout, "since": since}) is not None


class ShardFilter:
    __slots__ = ("count", "index", "by_uid", "active", "assignment")

    def __init__(self, s: ShardSettings) -> None:
        self.count = s.count
        self.index = s.index
        self.by_uid = s.key == "uid"
        self.active = s.count > 1
        self.assignment = getattr(s, "assignment", "hash")

    def owns(self, uid: Optional[str], namespace: Optional[str]) -> bool:
        """Per-event ownership (cluster-wide watches)."""
        if not self.active:
            return True
        return shard_of(uid if self.by_uid else namespace, self.count) == self.index

    def namespaces(self, namespaces: Sequence[str]) -> List[str]:
        """The subset of ``namespaces`` this shard watches server-side, in the given order."""
        ns = list(dict.fromkeys(namespaces))
        if not self.active or self.by_uid:
            return ns
        if self.assignment == "hash":
            return [n for n in ns if shard_of(n, self.count) == self.index]
        owner = balanced_assignment(ns, self.count)
        return [n for n in ns if owner[n] == self.index]
