"""In-memory pod cache: phase-change diffing and relist reconciliation.

The reference README promises "Trigger an API call on phase changes"
(``/root/reference/README.md:7``) but ``handle_pod_event`` notifies on every
event (``pod_watcher.py:214-241``). This cache provides both modes
(``watcher.notify_on: all | phase_change``) and is also what lets the
reflector turn a post-410 relist into exact ADDED/MODIFIED/DELETED diffs
 and survive restarts through the checkpoint.

One entry per live pod: ``uid -> [resourceVersion, phase, namespace, name, core]``
where ``core`` is the last serialized payload core (or ``None`` if the pod
was never notified). On top of that an entry has alert state, addressed by
kind and in memory only: none of it is in ``to_records``, so none reaches a
checkpoint, a hand-over or a parting record.

* A "last signature" slot per alert that compares one (``swap_failure`` for
  ``watcher.alerts.container_failures``, ``swap_condition`` for
  ``pod_conditions``, ``swap_terminating`` for ``terminating``): each stores a
  signature and returns the previous one, and the slots are independent.
* A timer per overdue sweep, with the mark that says the sweep reported it:
  the deletion deadline of a terminating pod
  (``watcher.alerts.terminating_overdue_seconds``: ``set_deadline``,
  ``deadline``, ``tracked``, ``take_overdue``) and the creation time of a pod
  still ``Pending`` (``watcher.alerts.pending_overdue_seconds``:
  ``set_pending_since``, ``pending_since``, ``pending_tracked``,
  ``take_pending_overdue``) and the time the ``Ready`` condition of a
  ``Running`` pod turned ``False`` (``watcher.alerts.unready_overdue_seconds``:
  ``set_unready_since``, ``unready_since``, ``unready_tracked``,
  ``take_unready_overdue``).
* With the latter two options the core of a ``Pending`` (or ``Running`` and
  unready) line nobody sent is kept for the sweep to report from
  (``keep_core``): marked as kept, it is dropped when a timer of a kind that
  keeps cores is cleared (and the other such kind holds none), the one rule
  that depends on the kind, and a send (``set_core``) replaces it. A checkpoint writes a kept core like any
  core, and after a restart it counts as an ordinary one.

Two implementations share this interface: :class:`PodCache` (a dict of
lists, used by the Python engine) and ``_kwcore.PodCache`` (C++,
``ops/csrc/podcache.inc`` over the store of ``podstore.inc``), which the fused native pipeline updates without
creating Python objects. Callers other than the two pipelines use only the
methods below; ``get``/``items``/``pop`` of the native cache return copies.
"""

from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Tuple

RV, PHASE, NS, NAME, CORE = range(5)
# PodCache only: a signature's slot in the entry list, there only once a swap
# stored one (with zeros for the slots before it)
FAILURE, CONDITION, TERMINATING = range(5, 8)
DEADLINE, PENDING, UNREADY = range(3)  # PodCache.timers
KEEPS_CORE = (PENDING, UNREADY)  # the kinds whose timer a kept core lives as long as
MISSING = object()


class _Timer:
    """One kind of timer: uid -> a time (s since the epoch) of the entries
    that have one, and the uids among them the sweep already reported."""
    __slots__ = ("at", "reported")

    def __init__(self) -> None:
        self.at: Dict[str, int] = {}
        self.reported: set = set()

    def set(self, uid: str, at: int) -> None:
        self.at[uid] = at  # (the mark stays: a timer that moves does not re-alert)

    def get(self, uid: str) -> Optional[int]:
        return self.at.get(uid)

    def count(self) -> int:
        return len(self.at)

    def drop(self, uid: str) -> None:
        self.at.pop(uid, None)
        self.reported.discard(uid)

    def clear(self) -> None:
        self.at.clear()
        self.reported.clear()

    def take(self, entries: Dict[str, list], now_s: int, after_s: int, scope_ns: Optional[str]) -> List[tuple]:
        """``(uid, namespace, name, core, at)`` of every entry ``after_s``
        seconds or more past its time at ``now_s``, not yet reported, that has
        a payload core (of namespace ``scope_ns`` only, if given); each one is
        marked reported. An entry without a core is left unmarked."""
        out = []
        for uid, at in self.at.items():
            if now_s - at < after_s or uid in self.reported:
                continue
            ent = entries[uid]
            if ent[CORE] is None or (scope_ns is not None and ent[NS] != scope_ns):
                continue
            out.append((uid, ent[NS], ent[NAME], ent[CORE], at))
        self.reported.update(t[0] for t in out)
        return out


class PodCache:
    __slots__ = ("entries", "timers", "kept")

    def __init__(self) -> None:
        self.entries: Dict[str, list] = {}
        self.timers = (_Timer(), _Timer(), _Timer())  # by DEADLINE, PENDING, UNREADY
        self.kept: set = set()  # the uids whose core is a kept one

    def __len__(self) -> int:
        return len(self.entries)

    def __contains__(self, uid: str) -> bool:
        return uid in self.entries

    def get(self, uid: str) -> Optional[list]:
        return self.entries.get(uid)

    def observe(self, etype: str, uid: str, rv: Optional[str], phase: Optional[str],
                ns: Optional[str], name: Optional[str]):
        """Apply one event; return the previous phase or :data:`MISSING`."""
        ent = self.entries.get(uid)
        prev = MISSING if ent is None else ent[PHASE]
        if etype == "DELETED":
            if ent is not None:
                del self.entries[uid]
                self._untrack(uid)
        elif ent is None:
            self.entries[uid] = [rv, phase, ns, name, None]
        else:
            ent[RV] = rv
            ent[PHASE] = phase
        return prev

    def set_core(self, uid: str, core: bytes) -> None:
        ent = self.entries.get(uid)
        if ent is not None:
            ent[CORE] = core
            if self.kept:
                self.kept.discard(uid)

    def keep_core(self, uid: str, core: bytes) -> None:
        """Store the core of an unsent ``Pending`` (or ``Running`` and unready)
        line, marked as kept: clearing that timer drops it, :meth:`set_core`
        replaces it."""
        ent = self.entries.get(uid)
        if ent is not None:
            ent[CORE] = core
            self.kept.add(uid)

    def core_kept(self, uid: str) -> bool:
        return uid in self.kept

    def _swap(self, uid: str, slot: int, sig: int) -> int:
        ent = self.entries.get(uid)
        if ent is None:
            return 0
        if len(ent) > slot:
            prev = ent[slot]
            ent[slot] = sig
            return prev
        if sig:
            ent.extend([0] * (slot - len(ent)))
            ent.append(sig)
        return 0

    def swap_failure(self, uid: str, sig: int) -> int:
        """Store the pod's failure signature (models/findings.py); returns the
        previous one, 0 for none. A pod not cached stores nothing."""
        return self._swap(uid, FAILURE, sig)

    def swap_condition(self, uid: str, sig: int) -> int:
        """As :meth:`swap_failure`, for the signature of the pod's condition
        findings; the two are independent."""
        return self._swap(uid, CONDITION, sig)

    def swap_terminating(self, uid: str, sig: int) -> int:
        """As :meth:`swap_failure`, for the terminating signature (1 or 0);
        independent of the other two."""
        return self._swap(uid, TERMINATING, sig)

    def put(self, uid: str, rv: Optional[str], phase: Optional[str], ns: Optional[str],
            name: Optional[str], core: Optional[bytes] = None) -> None:
        self.entries[uid] = [rv, phase, ns, name, core]
        self._untrack(uid)  # a whole new entry: nothing known of its deletion

    def pop(self, uid: str, default=None):
        self._untrack(uid)
        return self.entries.pop(uid, default)

    def clear(self) -> None:
        self.entries.clear()
        for t in self.timers:
            t.clear()
        self.kept.clear()

    def _untrack(self, uid: str) -> None:
        """The entry is gone or a whole new one: nothing is known of it."""
        for t in self.timers:
            if t.at:  # (the usual case, no alert option on: no call per event)
                t.drop(uid)
        if self.kept:
            self.kept.discard(uid)

    def _set_timer(self, kind: int, uid: str, at: Optional[int]) -> None:
        if at is None:
            self.timers[kind].drop(uid)
            # a kept core lives as long as the timer of a kind that keeps cores
            # (the other such kind's, if a line just set it, holds the core on)
            if kind in KEEPS_CORE and uid in self.kept and not any(uid in self.timers[k].at for k in KEEPS_CORE):
                self.kept.discard(uid)
                self.entries[uid][CORE] = None
        elif uid in self.entries:
            self.timers[kind].set(uid, at)

    # -- deletion deadlines (watcher.alerts.terminating_overdue_seconds) --------
    def set_deadline(self, uid: str, due: Optional[int]) -> None:
        """Store the pod's deletion deadline. ``None`` clears it and the
        reported mark; a value keeps the mark (a deadline that moves does not
        re-alert). A pod not cached stores nothing."""
        self._set_timer(DEADLINE, uid, due)

    def deadline(self, uid: str) -> Optional[int]:
        return self.timers[DEADLINE].get(uid)

    def tracked(self) -> int:
        """How many entries have a deadline."""
        return self.timers[DEADLINE].count()

    def take_overdue(self, now_s: int, after_s: int, scope_ns: Optional[str] = None) -> List[tuple]:
        """``(uid, namespace, name, core, deadline)`` of the entries overdue
        by ``after_s`` at ``now_s``, each marked reported (:meth:`_Timer.take`)."""
        return self.timers[DEADLINE].take(self.entries, now_s, after_s, scope_ns)

    # -- pods still Pending (watcher.alerts.pending_overdue_seconds) -------------
    def set_pending_since(self, uid: str, since: Optional[int]) -> None:
        """Store the creation time of a pod still ``Pending``. ``None`` clears
        it, its reported mark and a kept core; a value keeps the mark. A pod
        not cached stores nothing."""
        self._set_timer(PENDING, uid, since)

    def pending_since(self, uid: str) -> Optional[int]:
        return self.timers[PENDING].get(uid)

    def pending_tracked(self) -> int:
        """How many entries have a pending-since."""
        return self.timers[PENDING].count()

    def take_pending_overdue(self, now_s: int, after_s: int, scope_ns: Optional[str] = None) -> List[tuple]:
        """As :meth:`take_overdue`: ``(uid, namespace, name, core, since)`` of
        the entries still ``Pending`` ``after_s`` or more after their creation."""
        return self.timers[PENDING].take(self.entries, now_s, after_s, scope_ns)

    # -- pods Running but not Ready (watcher.alerts.unready_overdue_seconds) ------
    def set_unready_since(self, uid: str, since: Optional[int]) -> None:
        """Store the time the ``Ready`` condition of a ``Running`` pod turned
        ``False``. ``None`` clears it, its reported mark and a kept core; a
        value keeps the mark. A pod not cached stores nothing."""
        self._set_timer(UNREADY, uid, since)

    def unready_since(self, uid: str) -> Optional[int]:
        return self.timers[UNREADY].get(uid)

    def unready_tracked(self) -> int:
        """How many entries have an unready-since."""
        return self.timers[UNREADY].count()

    def take_unready_overdue(self, now_s: int, after_s: int, scope_ns: Optional[str] = None) -> List[tuple]:
        """As :meth:`take_overdue`: ``(uid, namespace, name, core, since)`` of
        the entries ``Running`` and not ``Ready`` for ``after_s`` seconds or more."""
        return self.timers[UNREADY].take(self.entries, now_s, after_s, scope_ns)

    def items(self) -> List[Tuple[str, list]]:
        return list(self.entries.items())

    def count_namespace(self, ns: Optional[str]) -> int:
        return sum(1 for ent in self.entries.values() if ent[NS] == ns)

    def namespaces(self) -> Dict[Optional[str], int]:
        out: Dict[Optional[str], int] = {}
        for ent in self.entries.values():
            out[ent[NS]] = out.get(ent[NS], 0) + 1
        return out

    def drop_namespaces(self, names) -> int:
        """Forget every pod of these namespaces; returns how many."""
        names = set(names)
        gone = [uid for uid, ent in self.entries.items() if ent[NS] in names]
        for uid in gone:
            del self.entries[uid]
            self._untrack(uid)
        return len(gone)

    def drop_namespaces_except(self, names) -> int:
        keep = set(names)
        gone = [uid for uid, ent in self.entries.items() if ent[NS] not in keep]
        for uid in gone:
            del self.entries[uid]
            self._untrack(uid)
        return len(gone)

    def to_records(self) -> List[list]:
        return [[uid] + ent[:4] + [ent[CORE].decode("utf-8") if ent[CORE] else None]
                for uid, ent in self.entries.items()]

    def load_records(self, records: List[list]) -> None:
        for r in records:
            uid, rv, phase, ns, name, core = r
            self.entries[uid] = [rv, phase, ns, name, core.encode("utf-8") if core else None]
            self._untrack(uid)  # a whole new entry, as put()

    @classmethod
    def from_records(cls, records: List[list]) -> "PodCache":
        c = cls()
        c.load_records(records)
        return c


def make_pod_cache(native: bool, records: Optional[List[list]] = None):
    """A :class:`PodCache` or, for the native pipeline, a ``_kwcore.PodCache``."""
    if native:
        from .native import load
        cache = load().PodCache(MISSING)
    else:
        cache = PodCache()
    if records:
        cache.load_records(records)
    return cache


def phase_changed(etype: str, prev, phase: Optional[str]) -> bool:
    """``notify_on: phase_change`` decision given the cache's previous phase."""
    if etype == "DELETED" or prev is MISSING:
        return True
    return prev != phase
