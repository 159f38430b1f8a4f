"""Namespace hand-over between shards (``watcher.shard.handover_dir``).

The protocol's parties; the three ways a namespace moves (live, across a
restart, at a scale-down), the record codec and the layout history are
``parallel/shard.py``'s. The old owner writes the namespace's cached pods and
the notifications it still owes for them, the new owner loads them before its
watch starts, a shard that shuts down writes *parting records* of what it
watches (:meth:`NamespaceHandover.part_cut`, which also groups shutdown's cut
of the cache by namespace: :func:`pods_by_namespace`, the one place a cache
entry becomes a record's pod), and one that comes back clears them away
(:meth:`NamespaceHandover.reclaim_on_start`).

:class:`NamespaceHandover` does not know the service: it is given the shard
settings, where to count and log, late-bound accessors for the cache and the
notifier (both built when the service starts) and three callables for what
only the service (resending what is owed) and its scope set (``scopes.py``:
starting a watch, forgetting a namespace's pods) can do.
"""

from __future__ import annotations

import asyncio
import concurrent.futures
import gc
import logging
import time
from typing import Callable, Dict, Iterable, List, Optional, Set

from ..metrics import Metrics
from ..ops.cache import CORE, NAME, NS, PHASE, RV
from ..parallel.shard import (discard_parting, has_handover, is_settled, layout_of, owners_of, read_manifest,
                              record_layout, remove_manifest, take_handover, take_parting, write_handover,
                              write_manifest, write_parting, write_settled)
from ..utils.config import ShardSettings

PARTING_WRITERS = 8  # parting records written at a time (part)


def pods_by_namespace(items, watched: Iterable[str]) -> Dict[str, list]:
    """The pod cache's ``items`` as records' pods ``(uid, rv, phase, name,
    core)``, for each namespace of ``watched``."""
    out: Dict[str, list] = {ns: [] for ns in watched}
    for uid, e in items:
        pods = out.get(e[NS])
        if pods is not None:
            pods.append((uid, e[RV], e[PHASE], e[NAME], e[CORE]))
    return out


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
        # gains whose previous owner is an ordinal the current count no longer
        # has (reshard_on_start): they wait for its parting record, under the
        # layout it ran under
        self._parted_from: Dict[str, int] = {}
        self._prev_layout: Optional[dict] = None
        # the gains reshard_on_start returned that have not ended yet: their
        # record may be as old as the layout, and when the last of them has
        # ended this shard's part of the re-shard is done (_gain_ended)
        self._start_gains: Set[str] = set()

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
        # a start-time gain from a removed ordinal (reshard_on_start) waits for
        # that shard's parting record; every other gain for the hand-over record
        self._gaining[ns] = asyncio.ensure_future(
            self._await_handover(ns, self._parted_from.pop(ns, None), ns in self._start_gains))

    def cancel_gain(self, ns: str) -> bool:
        """``ns`` was deleted, or handed on, before its watch started: nothing
        of it is cached here."""
        gaining = self._gaining.pop(ns, None)
        if gaining is None:
            return False
        gaining.cancel()
        self._gain_ended(ns)
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
    def _went_out(self, pods: list, exc: Optional[OSError], done: str, failed: str) -> None:
        """Count and log a hand-over record that went out, or why it did not."""
        if exc is not None:
            self.metrics.c["shard_handover_errors"] += 1
            self.log.error(failed)
            return
        self.metrics.c["shard_handovers_out"] += 1
        self.metrics.c["shard_handover_pods_out"] += len(pods)
        self.log.info(done)

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
        (``shard_handover_owed_late``).

        What is owed is what the notifier still holds (``pending_in``: queued,
        in flight, retrying). Notifications it has moved to the durable spool
        (``clusterapi.spool``, off by default) are not counted: the spool's
        replay sends them from this shard later, possibly after the new
        owner's for the same pod. With the spool on, the order across a live
        hand-over is not guaranteed."""
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
            pods = pods_by_namespace(cache.items(), {ns})[ns]
            exc = None
            try:
                # (json + fsync on a shared volume: off the loop)
                await loop.run_in_executor(None, write_handover, sh.handover_dir, ns, sh.index, dst, pods, None,
                                           layout_of(sh))
            except OSError as e:
                exc = e
            self._went_out(pods, exc, f"Handed namespace {ns} ({len(pods)} cached pods) over to shard {dst}",
                           f"Could not write the hand-over of namespace {ns} to shard {dst} "
                           f"({exc}): its new owner will re-announce its pods")
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
        it, which then are not re-sent here (those of a record that could not
        be written are) — and returns the namespaces this shard now owns that
        were another's, which wait for their record.

        That is this shard's part of the re-shard, done once: when its records
        are out and those gains have ended it leaves a marker in the directory
        (:meth:`_gain_ended`), and a later start under the same layout, begun
        at the same time, is a plain restart — nobody would answer a gain, and
        nobody waits for a record. What it *holds* of namespaces it does not
        own is handed out as on any start.

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
        resharded = bool(prev and prev != layout and prev.get("key", "namespace") == "namespace"
                         and not is_settled(sh.handover_dir, sh.index, layout, self._layout_since))
        was_mine = set()
        if resharded:
            was = owners_of(names, prev["count"], prev["assignment"])  # under the previous layout
            was_mine = {ns for ns in names if was(ns) == sh.index}
        out = sorted(ns for ns in (held | was_mine) if ns in names and ns not in owned)
        cached = pods_by_namespace(cache.items(), out) if out else {}
        gone = set()  # namespaces whose record is out: what is owed for them is the new owner's to send
        owner = owners_of(names, sh.count, sh.assignment) if out else None
        for ns in out:
            dst = owner(ns)
            pods = cached[ns]
            mine = [o for o in owed if o[2] == ns]
            if ns not in held and not mine and has_handover(sh.handover_dir, ns, sh.index,
                                                            self._layout_since - 60.0, layout):
                # this shard's record from an earlier start of this re-shard, which was cut
                # short, and not taken yet: it says what this start no longer knows
                continue
            exc = None
            try:
                write_handover(sh.handover_dir, ns, sh.index, dst, pods, mine, layout)
                gone.add(ns)
            except OSError as e:
                exc = e
            self._went_out(pods, exc, f"New shard layout {layout}: handed namespace {ns} ({len(pods)} cached pods, "
                                      f"{len(mine)} owed notifications) over to shard {dst}",
                           f"Could not write the hand-over of namespace {ns} to shard {dst} ({exc}): its new owner "
                           f"will re-announce its pods, and its {len(mine)} owed notification(s) are re-sent here")
        owed = [o for o in owed if o[2] not in gone]
        gains: Set[str] = set()
        if resharded:
            gains = {ns for ns in owned if ns not in saved_rvs and was(ns) != sh.index}
            if gains:
                self.log.info(f"New shard layout {layout} (was {prev}): waiting for the hand-over of "
                              f"{len(gains)} namespace(s) from their old owners")
            # an old owner below the new count restarts and writes the record
            # above; one at or past it is gone for good: its parting record
            self._prev_layout = prev
            for ns in gains:
                if was(ns) >= sh.count:
                    self._parted_from[ns] = was(ns)
            self._start_gains = set(gains)
            if not gains:
                self._settle()
        return gains, owed

    def _gain_ended(self, ns: str) -> None:
        """A gain of ``ns`` has ended — its record taken, the wait run out or
        pointless, or the gain cancelled. With the last of those
        :meth:`reshard_on_start` returned, this shard's part of the re-shard is
        done. (A gain cut short by shutdown has not ended: the next start
        waits for it again.)"""
        if ns in self._start_gains:
            self._start_gains.discard(ns)
            if not self._start_gains:
                self._settle()

    def _settle(self) -> None:
        sh = self.shard
        try:
            write_settled(sh.handover_dir, sh.index, layout_of(sh), self._layout_since)
        except OSError as exc:
            # (the next start takes the previous layout for a re-shard again)
            self.metrics.c["shard_handover_errors"] += 1
            self.log.error(f"Could not note in {sh.handover_dir} that this shard's part of the re-shard is done "
                           f"({exc})")

    async def _await_handover(self, ns: str, parted_from: Optional[int] = None, at_start: bool = False) -> None:
        """The new owner's half: wait for the old owner's record, send the
        notifications it still owed for the namespace (before anything of this
        shard's), load its pods into the cache, then start the watch — its
        first LIST reconciles against that state (unchanged pods stay quiet,
        pods gone meanwhile are DELETED), as a relist after a 410 would.
        Records written before this wait could have been meant for it (an
        older move's, whose new owner timed out) or under another layout are
        stale and discarded. Which record, :meth:`_source` says."""
        sh = self.shard
        loop = asyncio.get_running_loop()
        deadline = loop.time() + sh.handover_wait_seconds
        poll, taken, pods_taken, gave_up = self._source(ns, parted_from, at_start)
        while True:
            rec, pointless = poll()
            if rec is not None or pointless or loop.time() >= deadline or self._stop.is_set():
                break
            await asyncio.sleep(0.05)
        if self._gaining.get(ns) is not asyncio.current_task() or self._stop.is_set():
            return
        del self._gaining[ns]
        if rec is None:
            counter, warning = gave_up if pointless else (
                "shard_handover_timeouts", f"No hand-over of namespace {ns} from its old owner after "
                                           f"{sh.handover_wait_seconds}s: its pods are announced as ADDED again")
            self.metrics.c[counter] += 1
            self.log.warning(warning)
        else:
            if rec.owed:  # the old owner's unacknowledged notifications: first, in their order
                self._resubmit_owed(list(rec.owed))
            cache = self._cache()
            for uid, rv, phase, name, core in rec.pods:
                cache.put(uid, rv, phase, ns, name, core)
            self.metrics.c[taken] += 1
            self.metrics.c[pods_taken] += len(rec.pods)
            self.log.info(f"Took over namespace {ns} ({len(rec.pods)} pods, {len(rec.owed)} owed "
                          f"notifications from shard {rec.src})")
        self._start_scope(ns, primed=True)
        self._gain_ended(ns)

    def _source(self, ns: str, parted_from: Optional[int], at_start: bool = False) -> tuple:
        """What a gain of ``ns`` waits for: ``(poll, counter of records taken,
        of their pods, (counter, warning) for giving up)``, where ``poll() ->
        (the record if it is there, waiting has become pointless)``.

        ``parted_from`` is the old owner when that is an ordinal the current
        count no longer has: it never restarts, so what there is to wait for
        is the parting record of its shutdown (:meth:`part`), and its manifest
        says when waiting is pointless — the shard has stopped and wrote no
        record for this namespace. Without a manifest it is still running (and
        watching: the wait loses nothing) or was killed (the wait runs out)."""
        sh = self.shard
        if parted_from is None:
            # a start-time gain's record (at_start: reshard_on_start returned it) was
            # written since the layout began, however long ago the old owner
            # restarted under it; a live move's after the old owner saw the change
            # (seconds around ours): anything older, of this layout too, is an
            # earlier move's
            if at_start and self._layout_since:
                not_before = self._layout_since - 60.0
            else:
                not_before = time.time() - max(60.0, sh.handover_wait_seconds)
            layout = layout_of(sh)
            return (lambda: (take_handover(sh.handover_dir, ns, sh.index, not_before=not_before, layout=layout), False),
                    "shard_handovers_in", "shard_handover_pods_in", None)
        # written when the old shard went down, at most the wait before the
        # first shard started under this layout
        not_before = self._layout_since - sh.handover_wait_seconds - 60.0
        layout = self._prev_layout

        def poll():
            # the manifest first: it is written after the records, so a
            # record it vouches for is there by the time it is
            manifest = read_manifest(sh.handover_dir, parted_from)
            rec = take_parting(sh.handover_dir, ns, parted_from, not_before=not_before, layout=layout)
            return rec, rec is None and manifest is not None and manifest.get("layout") == layout

        return (poll, "shard_partings_in", "shard_parting_pods_in",
                ("shard_parting_missing", f"Shard {parted_from} stopped without a parting record of namespace {ns}: "
                                          f"its pods are announced as ADDED again"))

    # ------------------------------------------------------------------ scale-down
    async def part_cut(self, cut: dict, budget: float) -> List[str]:
        """:meth:`part` from shutdown's cut: ``watched`` namespaces, the pod
        cache's ``items`` and the notifications ``owed``, all of one moment."""
        # the cut's copy of a large cache is a million objects, none of them
        # cyclic: a full collection started by a writer thread meanwhile would
        # walk them all with the GIL held (110 ms of the loop at 100k pods)
        collecting = gc.isenabled()
        gc.disable()
        try:
            # (grouping a large cache takes as long as cutting it did: off the loop,
            # and the items are let go there, on that thread)
            pods = await asyncio.get_running_loop().run_in_executor(
                None, lambda: pods_by_namespace(cut.pop("items"), cut["watched"]))
            return await self.part(pods, cut["owed"], budget)
        finally:
            if collecting:
                gc.enable()

    async def part(self, pods_by_namespace: Dict[str, list], owed: Iterable[tuple] = (),
                   budget: float = 10.0) -> List[str]:
        """Shutdown: this shard has stopped watching. One parting record per
        namespace of ``pods_by_namespace`` (what it watched: cached pods as
        ``(uid, rv, phase, name, core)``) with that namespace's share of
        ``owed``, then the manifest naming the records that were written —
        whoever owns a namespace next (nobody, if this is a plain restart)
        finds its state complete or not at all. The files are written on
        threads, :data:`PARTING_WRITERS` at a time; after ``budget`` seconds
        the records not begun are given up and the manifest lists the rest.
        Returns the namespaces in the manifest."""
        sh = self.shard
        loop = asyncio.get_running_loop()
        layout = layout_of(sh)
        written_at = time.time()
        owed_in: Dict[str, list] = {}
        for o in owed:
            owed_in.setdefault(o[2], []).append(o)
        done: List[str] = []
        pods_out = 0
        pool = concurrent.futures.ThreadPoolExecutor(PARTING_WRITERS, thread_name_prefix="kw-parting")
        try:
            writes = {loop.run_in_executor(pool, write_parting, sh.handover_dir, ns, sh.index, pods,
                                           owed_in.get(ns), layout, written_at): ns
                      for ns, pods in sorted(pods_by_namespace.items())}
            pending = set(writes)
            if pending:
                _, pending = await asyncio.wait(pending, timeout=budget)
            for fut in pending:
                fut.cancel()  # not begun: never written; begun: finishes on its thread, unlisted
            if pending:
                self.log.warning(f"Parting: {len(pending)} of {len(writes)} namespace records not written "
                                 f"within {budget:g}s; their new owners re-announce their pods")
            for fut, ns in writes.items():
                if fut in pending:
                    continue
                exc = fut.exception()
                if exc is None:
                    done.append(ns)
                    pods_out += len(pods_by_namespace[ns])
                else:
                    self.metrics.c["shard_handover_errors"] += 1
                    self.log.error(f"Could not write the parting record of namespace {ns} ({exc})")
            try:
                # (not on the pool: its threads may all be in writes that outlast the budget)
                await loop.run_in_executor(None, write_manifest, sh.handover_dir, sh.index, layout, done, written_at)
            except OSError as exc:
                self.metrics.c["shard_handover_errors"] += 1
                self.log.error(f"Could not write this shard's parting manifest in {sh.handover_dir} ({exc}): "
                               f"its namespaces' new owners wait for their hand-over in vain")
                return []
        finally:
            pool.shutdown(wait=False, cancel_futures=True)
        self.metrics.c["shard_partings_out"] += len(done)
        self.metrics.c["shard_parting_pods_out"] += pods_out
        self.log.info(f"Parting: wrote the state of {len(done)} namespace(s) ({pods_out} cached pods) "
                      f"to {sh.handover_dir}")
        return done

    def reclaim_on_start(self, saved_rvs: dict, owed: list) -> list:
        """This shard is back after a graceful shutdown (its own manifest is
        there). A parting record still there was taken by nobody: the loaded
        checkpoint is the truth for that namespace, and the record goes. One
        that is gone was taken by the namespace's next owner (the count had
        shrunk below this ordinal): what the checkpoint says of it is
        superseded — its pods leave the cache, its resume point ``saved_rvs``
        and its notifications ``owed``, and the namespace is, if this shard
        owns it again, an ordinary gain. Then the manifest goes. Returns the
        owed notifications left."""
        sh = self.shard
        manifest = read_manifest(sh.handover_dir, sh.index)
        if manifest is None:
            return owed
        taken = {ns for ns in manifest.get("namespaces", []) if not discard_parting(sh.handover_dir, ns, sh.index)}
        remove_manifest(sh.handover_dir, sh.index)
        if taken:
            self._forget_namespaces(taken)
            for ns in taken:
                saved_rvs.pop(ns, None)
            kept = [o for o in owed if o[2] not in taken]
            self.log.info(f"{len(taken)} namespace(s) were taken over from this shard while it was away: "
                          f"dropped their checkpointed pods and {len(owed) - len(kept)} owed notification(s)")
            owed = kept
        return owed

