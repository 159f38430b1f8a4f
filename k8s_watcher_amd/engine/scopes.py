"""The watch scopes of one shard: which exist, and what state each is in.

A scope is one pod watch: the cluster (``None``, key ``"*"``) or one
namespace. :class:`ScopeSet` resolves this shard's scopes for the three scope
modes (``watcher.namespace_scope``), starts and stops their reflectors, and —
with ``discover`` — turns every change of the namespace set
(``engine/namespaces.py``) into started watches, drained ones (a deleted
namespace), gains and hand-overs (``engine/handover.py``).

Like :class:`~.handover.NamespaceHandover` it does not know the service: it is
given the watcher settings, where to count and log, the service's stop event,
late-bound accessors for the cache and the hand-over, and two factories — a
reflector for ``(namespace, resource_version, primed)`` and the namespace
watcher for a change callback. It never sees a decoder, a pipeline or the API.
"""

from __future__ import annotations

import asyncio
import logging
from typing import Callable, Dict, Iterable, List, Optional, Set, Tuple

from ..metrics import Metrics
from ..parallel.shard import ShardFilter, owner_of
from ..utils.config import WatcherSettings

DRAIN_STEP_SECONDS = 0.05  # how often a deleted namespace's drain looks at the cache
OVERDUE_CHECK_SECONDS = 1.0  # how often the live scopes look for pods past their deletion deadline


class SetupError(Exception):
    """The Kubernetes client could not be set up (reference ``:246``)."""


def first_exception(tasks: Iterable["asyncio.Future"]) -> Optional[BaseException]:
    """The first exception among the finished ones of ``tasks``."""
    for t in tasks:
        if t.done() and not t.cancelled() and t.exception() is not None:
            return t.exception()
    return None


class ScopeSet:
    def __init__(self, watcher: WatcherSettings, metrics: Metrics, log: logging.Logger, stop: asyncio.Event,
                 cache: Callable[[], object], handover: Callable[[], object],
                 make_reflector: Callable[[Optional[str], Optional[str], bool], object],
                 make_namespace_watcher: Callable[[Callable[[Set[str]], None]], object]) -> None:
        self.w = watcher
        self.metrics = metrics
        self.log = log
        self._stop = stop
        self._cache = cache  # -> the pod cache, None before the pipeline exists
        self._handover = handover  # -> begin_gain, cancel_gain, begin_out, cancel_out, gaining
        self._make_reflector = make_reflector
        self._make_namespace_watcher = make_namespace_watcher
        self._owner = ShardFilter(watcher.shard)
        self._scopes: Dict[str, Tuple[object, asyncio.Task]] = {}  # key -> (reflector, its run()), in start order
        self._retiring: Dict[str, asyncio.TimerHandle] = {}  # deleted namespaces draining their pod watch
        self._ns_seen: Set[str] = set()  # the namespace set the last ownership decision used
        self.multi = False  # several (or dynamic) watch scopes, each with its own pipeline
        self.live = False  # scopes follow namespace changes once go_live() has replayed the first
        self._list_gate: Optional[asyncio.Semaphore] = None
        self._saturated = False  # the notifier is: scopes do not read, new ones start paused
        self.saved_rvs: Dict[str, Optional[str]] = {}  # the checkpoint's resume points, by scope key
        self.failure: Optional[asyncio.Future] = None  # a scope's permanent failure
        self.ns_watcher = None  # namespace_scope: discover
        self._ns_task: Optional[asyncio.Task] = None

    # ------------------------------------------------------------------ what there is
    def __len__(self) -> int:
        return len(self._scopes)

    def reflectors(self) -> list:
        """The running scopes' reflectors, in start order."""
        return [r for r, _ in self._scopes.values()]

    def watched(self) -> Set[str]:
        """The namespaces watched now (shutdown's cut)."""
        return {r.namespace for r, _ in self._scopes.values() if r.namespace}

    def names(self) -> Iterable[str]:
        """Every namespace there is, as far as this configuration says."""
        return self._ns_seen if self.ns_watcher is not None else self.w.namespaces

    def tasks(self) -> List[asyncio.Task]:
        """What shutdown cancels and awaits: the namespace watch and every scope's."""
        ns = [self._ns_task] if self._ns_task is not None else []
        return ns + [t for _, t in self._scopes.values()]

    def ending(self) -> list:
        """What ends the service by ending: the namespace watch, a scope's
        permanent failure, and a lone watch (one of several is restarted by
        the next namespace change or not missed)."""
        out = [t for t in (self._ns_task, self.failure) if t is not None]
        return out if self.multi else out + [t for _, t in self._scopes.values()]

    def synced(self) -> "asyncio.Future":
        """Done once every scope present now has synced."""
        return asyncio.ensure_future(asyncio.gather(*[r.synced.wait() for r, _ in self._scopes.values()]))

    @property
    def list_gate(self) -> Optional[asyncio.Semaphore]:
        """``watcher.relist_concurrency``, shared by every scope."""
        if self._list_gate is None and self.w.relist_concurrency > 0:
            self._list_gate = asyncio.Semaphore(self.w.relist_concurrency)
        return self._list_gate

    def _owned(self, names: Iterable[str]) -> List[str]:
        return self._owner.namespaces(sorted(names))

    def _cached_in(self, ns: str) -> int:
        cache = self._cache()
        return 0 if cache is None else cache.count_namespace(ns)

    async def overdue_loop(self, clock: Callable[[], float]) -> None:
        """``watcher.alerts.terminating_overdue_seconds``,
        ``pending_overdue_seconds`` and ``unready_overdue_seconds``: once a
        period, every live scope reports its pods still there past their
        deletion deadline, still Pending or Running but not Ready
        (``Reflector.check_overdue``; a scope not yet synced or in a relist
        sits the tick out). A non-leader has no scopes: nothing happens."""
        while not self._stop.is_set():
            await asyncio.sleep(OVERDUE_CHECK_SECONDS)
            now_s = int(clock())
            for r in self.reflectors():
                try:
                    r.check_overdue(now_s)
                except Exception as exc:  # the next tick tries again: the sweep marks only what it sent
                    self.log.warning(f"Overdue check of scope {r.scope} failed: {exc!r}")

    # ------------------------------------------------------------------ start-up
    async def resolve(self) -> List[Optional[str]]:
        """The watch scopes of this shard: the cluster (``None``), its share of
        the configured namespaces, or of the discovered ones once the
        namespace watch has listed them."""
        w = self.w
        self.failure = asyncio.get_running_loop().create_future()
        if w.namespace_scope == "discover":
            self.ns_watcher = self._make_namespace_watcher(self.on_namespaces)
            self._ns_task = asyncio.ensure_future(self.ns_watcher.run())
            synced = asyncio.ensure_future(self.ns_watcher.synced.wait())
            await asyncio.wait([synced, self._ns_task], return_when=asyncio.FIRST_COMPLETED)
            if not synced.done():
                synced.cancel()
                raise first_exception([self._ns_task]) or SetupError("namespace watch ended before the initial list")
            self._ns_seen = set(self.ns_watcher.names)
            scopes: List[Optional[str]] = list(self._owned(self._ns_seen))
        elif w.namespace_scope == "server" and w.namespaces:
            scopes = list(self._owner.namespaces(w.namespaces))
        else:
            scopes = [None]
        self.multi = w.namespace_scope == "discover" or len(scopes) > 1
        if w.shard.count > 1:
            self.log.info(f"Shard {w.shard.index}/{w.shard.count} "
                          f"(key={w.shard.key}); watch scopes: {[x or '*' for x in scopes]}")
        return scopes

    async def start_all(self, scopes: List[Optional[str]], gains: Set[str]) -> None:
        """Start every scope's watch, a gained namespace's once its record is in."""
        for i, ns in enumerate(scopes):
            if ns in gains:  # another shard's under the previous layout: its record first
                self._handover().begin_gain(ns)
            else:
                self.start(ns, primed=bool(self.saved_rvs))
            if i % 64 == 63:  # a thousand namespaces: let the started scopes (and the loop) run meanwhile
                await asyncio.sleep(0)
                if self._stop.is_set():
                    break

    def go_live(self) -> None:
        """From here the scopes follow the namespace watch."""
        self.live = True
        if self.ns_watcher is not None:
            self.on_namespaces(self.ns_watcher.names)  # changes seen while the first scopes started

    # ------------------------------------------------------------------ one scope
    def start(self, ns: Optional[str], primed: bool):
        key = ns or "*"
        r = self._make_reflector(ns, self.saved_rvs.get(key), primed)
        if self._saturated:
            r.set_paused(True)
        task = asyncio.ensure_future(r.run())
        self._scopes[key] = (r, task)
        task.add_done_callback(lambda t, k=key: self._scope_done(k, t))
        return r

    def _scope_done(self, key: str, task: "asyncio.Task") -> None:
        if self._scopes.get(key, (None, None))[1] is not task:
            return  # stopped on purpose (namespace gone or handed over)
        if task.cancelled() or self._stop.is_set():
            return
        exc = task.exception()
        if exc is not None and self.failure is not None and not self.failure.done():
            self.failure.set_exception(exc)

    def stop_scope(self, ns: str, handover_to: Optional[int] = None) -> None:
        timer = self._retiring.pop(ns, None)
        if timer is not None:
            timer.cancel()
        self._handover().cancel_gain(ns)  # handed on before its watch started: nothing of it is cached here
        r, task = self._scopes.pop(ns, (None, None))
        if r is not None:
            r.stop()
            if not task.done():
                task.cancel()
            if handover_to is not None:
                # the namespace's pods stay cached until the record is written
                self._handover().begin_out(ns, handover_to)
                return
        self.forget({ns})

    def set_saturated(self, saturated: bool) -> None:
        """The notifier is saturated (or no longer): no scope reads meanwhile."""
        self._saturated = saturated
        for r, _ in self._scopes.values():
            r.set_paused(saturated)

    def stop(self) -> None:
        if self.ns_watcher is not None:
            self.ns_watcher.stop()
        for r, _ in self._scopes.values():
            r.stop()

    # ------------------------------------------------------------------ the cache of what is not watched
    def forget(self, namespaces: Set[str]) -> None:
        """Drop cached pods of namespaces this shard stopped watching, silently:
        they are now the business of another shard (or gone with the namespace).
        Both caches index entries by namespace: only those namespaces' pods are touched."""
        cache = self._cache()
        if cache is not None:
            cache.drop_namespaces(namespaces)

    def _synthesizing(self, ns: str, warning: Callable[[int], str]) -> None:
        """Count and log that ``ns``'s cached pods are about to be notified DELETED."""
        n = self._cached_in(ns)
        self.metrics.c["namespace_deleted_synthesized"] += n
        self.log.warning(warning(n))

    def reconcile_cache(self, scopes: List[Optional[str]], delete_scope: Callable[[str], Iterable[tuple]]) -> None:
        """A restart with a checkpoint, before any watch starts: namespaces
        deleted while the watcher was down get their pods DELETED from the
        cache through ``delete_scope(ns) -> control events``, as
        :meth:`_retire` and a relist would (only this shard had them cached:
        each shard's checkpoint is its own); then pods of namespaces this shard
        no longer watches go, which would never be reconciled."""
        cache = self._cache()
        if self.ns_watcher is not None:
            existing = set(self.ns_watcher.names)
            for ns in sorted(ns for ns in cache.namespaces() if ns is not None and ns not in existing):
                self._synthesizing(ns, lambda n: f"Namespace {ns} was deleted while the watcher was down: "
                                                 f"notifying its {n} cached pod(s) as DELETED")
                for ev in delete_scope(ns):
                    self.log.warning(f"Skipping undecodable cached entry ({ev[0]}): {ev[8]}")
        cache.drop_namespaces_except(set(scopes))

    # ------------------------------------------------------------------ following the namespace set
    def on_namespaces(self, names: Set[str]) -> None:
        """NamespaceWatcher callback: start/stop reflectors to match the owned set.

        A namespace handed to another shard stops at once (its pods are that
        shard's business now). A *deleted* namespace drains first: the namespace
        watch and the namespace's pod watch are separate streams, read in
        whatever order their bytes arrive, so its pods' DELETED events may still
        be on the way when the namespace's own DELETED is seen (kube-apiserver
        deletes the pods before the namespace, but nothing orders two streams)."""
        if not self.live or self._stop.is_set():
            return
        sh = self.w.shard
        handover = self._handover()
        prev, self._ns_seen = self._ns_seen, set(names)
        owned = set(self._owned(names))
        current = set(self._scopes) | handover.gaining()
        for ns in sorted(owned & set(self._retiring)):  # deleted and created again: keep watching
            self._retiring.pop(ns).cancel()
        for ns in sorted(owned - current):
            handover.cancel_out(ns)  # back before its record went out: still ours, cache and all
            self.metrics.c["scopes_started"] += 1
            self.log.info(f"Watching namespace {ns} (new or now owned by shard {sh.index})")
            if sh.handover_dir and ns in prev and owner_of(ns, prev, sh.count, sh.assignment) != sh.index:
                handover.begin_gain(ns)  # moved here from another shard: its state first
            else:
                self.start(ns, primed=True)
        for ns in sorted(current - owned):
            if ns not in names and handover.cancel_gain(ns):  # deleted before its hand-over came
                continue
            if ns not in names:
                if ns not in self._retiring:  # already draining: its timer is running
                    self._retire(ns)
                continue
            self.metrics.c["scopes_stopped"] += 1
            self.log.info(f"Stopped watching namespace {ns} (owned by another shard)")
            self.stop_scope(ns, owner_of(ns, names, sh.count, sh.assignment) if sh.handover_dir else None)

    def _retire(self, ns: str, waited: float = 0.0) -> None:
        """Keep a deleted namespace's pod watch until every pod cached there has
        been seen DELETED, or ``watcher.namespace_drain_seconds`` passed; then
        notify any pod still cached there as DELETED from its cached state (as a
        relist that no longer finds it would) and stop the watch."""
        if self._stop.is_set() or ns not in self._scopes:
            self._retiring.pop(ns, None)
            return
        limit = self.w.namespace_drain_seconds
        if self._cached_in(ns) and waited < limit:
            old = self._retiring.get(ns)
            if old is not None:
                old.cancel()  # one drain timer per namespace, whoever scheduled it
            self._retiring[ns] = asyncio.get_running_loop().call_later(
                DRAIN_STEP_SECONDS, self._retire, ns, waited + DRAIN_STEP_SECONDS)
            return
        self._retiring.pop(ns, None)
        if self._cached_in(ns):
            self._synthesizing(ns, lambda n: f"Namespace {ns} deleted: {n} pod(s) without a DELETED event after "
                                             f"{limit:g}s; notifying them as DELETED from the cache")
            self._scopes[ns][0].notify_cached_deleted()
        self.metrics.c["scopes_stopped"] += 1
        self.log.info(f"Stopped watching namespace {ns} (deleted)")
        self.stop_scope(ns)
