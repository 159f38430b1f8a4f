"""Durable resume point: resourceVersion(s) + pod cache (BASELINE config #5).

The reference keeps its resume point only inside the library's ``Watch``
object (``pod_watcher.py:16``), so every restart replays every pod as
``ADDED``. Here the reflector's resourceVersion per watch scope and the pod
cache are written atomically (temp file + fsync + rename). On restart the
watcher resumes the watch from the saved resourceVersion without a LIST; if
that version has been compacted (410) the relist is diffed against the saved
cache, so unchanged pods are not re-notified.

Two formats:

* **2 (native engine and notifier core)** — ``_kwcore.PodCache.snapshot``
  (``ops/csrc/checkpoint.inc``) takes a *consistent cut* between two
  event-loop callbacks: the cache entries (payload cores by reference, not
  copied) plus every notification clusterapi has not acknowledged yet. No
  watch is paused and the notifier is not drained; the snapshot is serialised
  and fsynced on an executor thread while the watch goes on. A restart first
  re-submits the owed notifications, then resumes the watches — so nothing
  acknowledged is sent again except those, and nothing unacknowledged is lost.
* **1 (Python engine / asyncio pool)** — one JSON document written at a
  *quiescent* point (watches paused, notifier drained), as before.

:class:`Checkpointer` decides when either is written: on request, every
``checkpoint.interval_seconds`` and as shutdown's final cut.
"""

from __future__ import annotations

import asyncio
import json
import logging
import os
import time
from typing import Callable, Dict, List, Optional, Tuple

from ..metrics import Metrics
from ..ops.cache import PodCache, make_pod_cache
from ..utils.atomic import write_atomically
from ..utils.config import CheckpointSettings

FORMAT_VERSION = 1
NATIVE_FORMAT_VERSION = 2
NATIVE_MAGIC = b"KWCKPT02"


def save_checkpoint(path: str, scopes: Dict[str, Optional[str]], cache: PodCache,
                    meta: Optional[dict] = None) -> None:
    doc = {"version": FORMAT_VERSION, "scopes": scopes, "meta": meta or {},
           "cache": cache.to_records()}
    write_atomically(path, lambda fh: json.dump(doc, fh, separators=(",", ":")), ".ckpt-")


def native_header(scopes: Dict[str, Optional[str]], meta: Optional[dict] = None) -> bytes:
    return json.dumps({"version": NATIVE_FORMAT_VERSION, "scopes": scopes, "meta": meta or {}},
                      separators=(",", ":")).encode("utf-8")


def native_snapshot(cache, notifier_core=None):
    """The consistent cut (call on the event-loop thread); write it with
    ``snap.write(path, native_header(...))`` on an executor."""
    return cache.snapshot(notifier_core)


def write_native(snap, path: str, scopes: Dict[str, Optional[str]], meta: Optional[dict] = None) -> Tuple[int, float]:
    os.makedirs(os.path.dirname(os.path.abspath(path)) or ".", exist_ok=True)
    return snap.write(path, native_header(scopes, meta))


def load_checkpoint(path: str, native_cache: bool = False
                    ) -> Optional[Tuple[Dict[str, Optional[str]], PodCache, dict, List[tuple]]]:
    """``(scopes, cache, meta, owed)`` or None when absent/unreadable/incompatible.

    ``native_cache`` loads into a ``_kwcore.PodCache`` (native pipeline);
    ``owed`` lists the notifications a format-2 checkpoint still owed, as
    ``(uid, type, ns, name, body)`` to re-submit before watching."""
    try:
        with open(path, "rb") as fh:
            head = fh.read(8)
    except OSError:
        return None
    if head == NATIVE_MAGIC:
        if not native_cache:
            return None  # written by the native engine; the Python engine relists
        cache = make_pod_cache(True)
        try:
            header, owed = cache.load_checkpoint(path)
            doc = json.loads(header)
        except (OSError, ValueError):
            return None
        if doc.get("version") != NATIVE_FORMAT_VERSION:
            return None
        return doc.get("scopes") or {}, cache, doc.get("meta") or {}, owed
    try:
        with open(path, "r", encoding="utf-8") as fh:
            doc = json.load(fh)
    except (OSError, ValueError):
        return None
    if not isinstance(doc, dict) or doc.get("version") != FORMAT_VERSION:
        return None
    return (doc.get("scopes") or {}, make_pod_cache(native_cache, doc.get("cache") or []),
            doc.get("meta") or {}, [])


class Checkpointer:
    """When the checkpoint is written, and in what order: one cut and its
    write at a time, so a later cut is never overwritten by an earlier one,
    and a periodic write whose task was cancelled mid-way (it goes on, on its
    thread) lands before the final cut. The cut, ``at_cut`` and format 1's
    save run on the loop thread, format 2's write on an executor thread.

    Like ``NamespaceHandover`` it does not know the service: it is given late-
    bound accessors for the pod cache, the notifier and the reflectors (their
    ``scope`` and ``rv`` are the resume points; format 1 pauses them)."""

    def __init__(self, settings: CheckpointSettings, native: bool, clusterapi_enabled: bool, metrics: Metrics,
                 log: logging.Logger, cache: Callable[[], object], notifier: Callable[[], object],
                 reflectors: Callable[[], list]) -> None:
        self.path = settings.path
        self.interval = settings.interval_seconds
        self.native = native
        self.clusterapi_enabled = clusterapi_enabled
        self.metrics = metrics
        self.log = log
        self._cache = cache  # -> the pod cache, None before the pipeline exists
        self._notifier = notifier
        self._reflectors = reflectors
        self._lock = asyncio.Lock()  # one checkpoint snapshot+write at a time, in cut order
        self._inflight: Optional[asyncio.Future] = None  # a format-2 write on its executor thread
        self.last: Optional[dict] = None  # the six checkpoint_* gauges of the last format-2 write

    def consistent(self) -> bool:
        """Format 2 (consistent cut, no pause/drain): native cache + native notifier core."""
        notifier = self._notifier()
        return (self.native and hasattr(self._cache(), "snapshot")
                and (notifier is None or hasattr(notifier, "core") or not self.clusterapi_enabled))

    def _snapshot(self):
        return native_snapshot(self._cache(), getattr(self._notifier(), "core", None))

    def _scopes(self) -> Dict[str, Optional[str]]:
        return {r.scope: r.rv for r in self._reflectors()}

    async def wait_inflight(self) -> None:
        fut = self._inflight
        if fut is not None and not fut.done():
            try:
                await fut
            except Exception as exc:  # noqa: BLE001 - the final write below reports its own errors
                self.log.warning(f"Checkpoint write in progress at shutdown failed: {exc}")

    async def _write_snapshot(self, at_cut=None) -> None:
        """Format 2. ``at_cut(snap)`` is called where the cut is taken: what
        else has to be of that moment (shutdown's parting records)."""
        async with self._lock:
            await self.wait_inflight()
            scopes = self._scopes()
            meta = {"written_at": time.time()}
            snap = self._snapshot()
            if at_cut is not None:
                at_cut(snap)
            st = snap.stats()
            loop = asyncio.get_running_loop()
            self._inflight = loop.run_in_executor(None, write_native, snap, self.path, scopes, meta)
            nbytes, secs = await asyncio.shield(self._inflight)
        self.last = {"checkpoint_stall_ms": st["snapshot_seconds"] * 1e3, "checkpoint_write_ms": secs * 1e3,
                     "checkpoint_bytes": float(nbytes), "checkpoint_pods": float(st["entries"]),
                     "checkpoint_owed": float(st["owed"]), "checkpoint_written_at": meta["written_at"]}
        for k, v in self.last.items():
            self.metrics.gauges[k] = (lambda v=v: v)
        self.metrics.c["checkpoints_written"] += 1

    async def _save(self) -> None:
        """Format 1, at a quiescent point the caller has made."""
        async with self._lock:
            save_checkpoint(self.path, self._scopes(), self._cache(), {"written_at": time.time()})
        self.metrics.c["checkpoints_written"] += 1

    async def now(self, drain_timeout: float = 30.0) -> bool:
        """Write a checkpoint now: format 2's cut (a few ms per 100k pods)
        while the watches keep running, or, for format 1, pause the readers,
        drain the notifier, save, resume. False if nothing could be written."""
        writable = bool(self.path) and self._cache() is not None
        if self.consistent():
            if writable:
                await self._write_snapshot()
            return writable
        notifier = self._notifier()
        for r in self._reflectors():
            r.set_paused(True)
        try:
            ok = await notifier.drain(drain_timeout) if notifier is not None else True
            if ok and writable:
                await self._save()
            return ok
        finally:
            saturated = getattr(notifier, "saturated", False)
            for r in self._reflectors():
                r.set_paused(saturated)

    async def loop(self) -> None:
        """A checkpoint every ``interval`` seconds in which something changed."""
        last = None
        while True:
            await asyncio.sleep(self.interval)
            state = (tuple(r.rv for r in self._reflectors()), len(self._cache()))  # (started once there is a cache)
            if state == last:
                continue
            if await self.now():
                last = state

    async def final_cut(self, at_cut=None) -> None:
        """Shutdown's checkpoint, after any write still in flight, so that it
        is the one that stays on disk. ``at_cut(snap=None)`` is called at the
        cut, with format 2's snapshot (``snap.owed()``: what the notifier
        still owes) even where there is no path to write it to."""
        await self.wait_inflight()
        if self._cache() is None:
            return
        if not self.path:  # no checkpoint to write: a cut all the same
            if at_cut is not None:
                at_cut(self._snapshot() if self.consistent() else None)
        elif self.consistent():
            await self._write_snapshot(at_cut)
        else:
            if at_cut is not None:
                at_cut()
            await self._save()
