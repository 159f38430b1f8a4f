"""Namespace hand-over between shards (``watcher.shard.handover_dir``).

When a namespace moves from one shard to another — live, because the namespace
set changed under ``balanced`` assignment, or across a restart with a new
``shard.count`` — its old owner writes its cached pods (and, at a restart, the
notifications it still owes for them) to a shared directory, and the new owner
loads them before its watch starts: its first LIST then reconciles against
that state instead of announcing every pod as ADDED again. The record format
and the layout history are ``parallel/shard.py``'s; this is the protocol's two
parties.

:class:`NamespaceHandover` does not know the service: it is given the shard
settings, where to count and log, late-bound accessors for the cache and the
notifier (both built when the service starts) and three callables for what
only the service can do.
"""

from __future__ import annotations

import asyncio
import logging
import time
from typing import Callable, Dict, Iterable, List, Set

from ..metrics import Metrics
from ..ops.cache import CORE, NAME, NS, PHASE, RV
from ..parallel.shard import layout_of, owner_of, record_layout, take_handover, write_handover
from ..utils.config import ShardSettings


class NamespaceHandover:
    def __init__(self, shard: ShardSettings, metrics: Metrics, log: logging.Logger, stop: asyncio.Event,
                 cache: Callable[[], object], notifier: Callable[[], object],
                 resubmit_owed: Callable[[list], None], start_scope: Callable[..., object],
                 forget_namespaces: Callable[[Set[str]], None]) -> None:
        self.shard = shard
        self.metrics = metrics
        self.log = log
        self._stop = stop
        self._cache = cache  # -> the pod cache, None before the pipeline exists
        self._notifier = notifier
        self._resubmit_owed = resubmit_owed
        self._start_scope = start_scope  # (ns, primed=True)
        self._forget_namespaces = forget_namespaces
        # namespaces gained from another shard, waiting for its hand-over record
        # before their watch starts
        self._gaining: Dict[str, asyncio.Task] = {}
        # namespaces handed to another shard whose record waits for this shard's
        # owed notifications of them to be acknowledged (_handover_out)
        self._handing: Dict[str, asyncio.Task] = {}
        self._layout_since = 0.0  # when the shard layout in handover_dir's history began (record_layout)

    # ------------------------------------------------------------------ what the service asks for
    def begin_out(self, ns: str, dst: int) -> None:
        """This shard's watch of ``ns`` has stopped and shard ``dst`` owns it
        now: its pods stay cached until the record is written."""
        self._handing[ns] = asyncio.ensure_future(self._handover_out(ns, dst))

    def cancel_out(self, ns: str) -> bool:
        """``ns`` came back before its record went out: still ours, cache and all."""
        handing = self._handing.pop(ns, None)
        if handing is None:
            return False
        handing.cancel()
        return True

    def begin_gain(self, ns: str) -> None:
        """``ns`` was another shard's: its record first, then its watch."""
        self._gaining[ns] = asyncio.ensure_future(self._await_handover(ns))

    def cancel_gain(self, ns: str) -> bool:
        """``ns`` was deleted, or handed on, before its watch started: nothing
        of it is cached here."""
        gaining = self._gaining.pop(ns, None)
        if gaining is None:
            return False
        gaining.cancel()
        return True

    def gaining(self) -> Set[str]:
        return set(self._gaining)

    def abandon_unwritten(self) -> None:
        """Shutdown: records not written yet stay unwritten. Their pods stay in
        the checkpoint, and the restart hands them over (:meth:`reshard_on_start`)."""
        for t in self._handing.values():
            t.cancel()
        self._handing.clear()

    def tasks(self) -> List[asyncio.Task]:
        """What shutdown cancels and awaits: the gains still waiting."""
        return list(self._gaining.values())

    # ------------------------------------------------------------------ the protocol
    def _cached_pods_of(self, cache, ns: str) -> list:
        return [(uid, e[RV], e[PHASE], e[NAME], e[CORE]) for uid, e in cache.items() if e[NS] == ns]

    async def _handover_out(self, ns: str, dst: int) -> None:
        """The old owner's half of a live namespace hand-over: with its watch
        stopped, wait until clusterapi has acknowledged (or this shard has
        given up) every notification still owed for the namespace — a retried
        MODIFIED (clusterapi answering 503, say) must not land after the new
        owner's notifications for the same pod — then write this shard's
        cached pods of ``ns`` to the shared directory for shard ``dst``
        (parallel/shard.py) and forget them. The wait is bounded by half of
        ``shard.handover_wait_seconds`` (the new owner's patience): past it the
        record goes out anyway and the late notifications are counted
        (``shard_handover_owed_late``)."""
        sh = self.shard
        loop = asyncio.get_running_loop()
        try:
            deadline = loop.time() + sh.handover_wait_seconds / 2
            pending_in = getattr(self._notifier(), "pending_in", None)
            late = 0
            while pending_in is not None and not self._stop.is_set():
                late = pending_in(ns)
                if late == 0 or loop.time() >= deadline:
                    break
                await asyncio.sleep(0.05)
            if late:
                self.metrics.c["shard_handover_owed_late"] += late
                self.log.warning(f"Handing namespace {ns} over with {late} notification(s) for it still owed "
                                 f"to clusterapi: they may arrive after shard {dst}'s")
            cache = self._cache()
            if cache is None:
                return
            pods = self._cached_pods_of(cache, ns)
            try:
                # (json + fsync on a shared volume: off the loop)
                await loop.run_in_executor(None, write_handover, sh.handover_dir, ns, sh.index, dst, pods, None,
                                           layout_of(sh))
            except OSError as exc:
                self.metrics.c["shard_handover_errors"] += 1
                self.log.error(f"Could not write the hand-over of namespace {ns} to shard {dst} "
                               f"({exc}): its new owner will re-announce its pods")
            else:
                self.metrics.c["shard_handovers_out"] += 1
                self.metrics.c["shard_handover_pods_out"] += len(pods)
                self.log.info(f"Handed namespace {ns} ({len(pods)} cached pods) over to shard {dst}")
            if self._handing.get(ns) is asyncio.current_task():
                self._forget_namespaces({ns})
        finally:
            if self._handing.get(ns) is asyncio.current_task():
                del self._handing[ns]

    def reshard_on_start(self, scopes, names: Iterable[str], saved_rvs: dict, owed: list):
        """A new shard layout (``shard.count`` changed, every shard restarted):
        the hand-over across a restart (parallel/shard.py). Notes the layout in
        ``handover_dir``'s history, writes a record for every namespace this
        shard held (its checkpoint) or owned under the previous layout that
        another shard owns now — with the checkpoint's owed notifications for
        it, which then are not re-sent here — and returns the namespaces this
        shard now owns that were another's, which wait for their record.
        ``scopes`` are this shard's watch scopes, ``names`` every namespace
        there is. Returns ``(gains, owed left to re-send here)``."""
        sh = self.shard
        layout = layout_of(sh)
        try:
            prev, self._layout_since = record_layout(sh.handover_dir, layout)
        except OSError as exc:
            self.log.error(f"Could not record the shard layout in {sh.handover_dir} ({exc}): no hand-over")
            return set(), owed
        names = set(names)
        owned = {x for x in scopes if x}
        cache = self._cache()
        held = {ns for ns in cache.namespaces() if ns is not None} | {k for k in saved_rvs if k != "*"}
        resharded = bool(prev and prev != layout and prev.get("key", "namespace") == "namespace")
        was_mine = set()
        if resharded:
            was_mine = {ns for ns in names if owner_of(ns, names, prev["count"], prev["assignment"]) == sh.index}
        out = sorted(ns for ns in (held | was_mine) if ns in names and ns not in owned)
        for ns in out:
            dst = owner_of(ns, names, sh.count, sh.assignment)
            pods = self._cached_pods_of(cache, ns)
            mine = [o for o in owed if o[2] == ns]
            try:
                write_handover(sh.handover_dir, ns, sh.index, dst, pods, mine, layout)
            except OSError as exc:
                self.metrics.c["shard_handover_errors"] += 1
                self.log.error(f"Could not write the hand-over of namespace {ns} to shard {dst} ({exc})")
                continue
            self.metrics.c["shard_handovers_out"] += 1
            self.metrics.c["shard_handover_pods_out"] += len(pods)
            self.log.info(f"New shard layout {layout}: handed namespace {ns} ({len(pods)} cached pods, "
                          f"{len(mine)} owed notifications) over to shard {dst}")
        gone = set(out)
        owed = [o for o in owed if o[2] not in gone]
        gains: Set[str] = set()
        if resharded:
            gains = {ns for ns in owned if ns not in saved_rvs
                     and owner_of(ns, names, prev["count"], prev["assignment"]) != sh.index}
            if gains:
                self.log.info(f"New shard layout {layout} (was {prev}): waiting for the hand-over of "
                              f"{len(gains)} namespace(s) from their old owners")
        return gains, owed

    async def _await_handover(self, ns: str) -> None:
        """The new owner's half: wait for the old owner's record, send the
        notifications it still owed for the namespace (before anything of this
        shard's), load its pods into the cache, then start the watch — its
        first LIST reconciles against that state (unchanged pods stay quiet,
        pods gone meanwhile are DELETED), as a relist after a 410 would.
        Records written before this wait could have been meant for it (an
        older move's, whose new owner timed out) or under another layout are
        stale and discarded."""
        sh = self.shard
        loop = asyncio.get_running_loop()
        deadline = loop.time() + sh.handover_wait_seconds
        # a live move's record is written after the old owner saw the change
        # (seconds around ours); a restart's since the layout began
        not_before = min(time.time() - max(60.0, sh.handover_wait_seconds),
                         self._layout_since - 60.0 if self._layout_since else time.time())
        layout = layout_of(sh)
        while True:
            rec = take_handover(sh.handover_dir, ns, sh.index, not_before=not_before, layout=layout)
            if rec is not None or loop.time() >= deadline or self._stop.is_set():
                break
            await asyncio.sleep(0.05)
        if self._gaining.get(ns) is not asyncio.current_task() or self._stop.is_set():
            return
        del self._gaining[ns]
        if rec is None:
            self.metrics.c["shard_handover_timeouts"] += 1
            self.log.warning(f"No hand-over of namespace {ns} from its old owner after "
                             f"{sh.handover_wait_seconds}s: its pods are announced as ADDED again")
        else:
            if rec.owed:  # the old owner's unacknowledged notifications: first, in their order
                self._resubmit_owed(list(rec.owed))
            cache = self._cache()
            for uid, rv, phase, name, core in rec.pods:
                cache.put(uid, rv, phase, ns, name, core)
            self.metrics.c["shard_handovers_in"] += 1
            self.metrics.c["shard_handover_pods_in"] += len(rec.pods)
            self.log.info(f"Took over namespace {ns} ({len(rec.pods)} pods, {len(rec.owed)} owed "
                          f"notifications from shard {rec.src})")
        self._start_scope(ns, primed=True)
