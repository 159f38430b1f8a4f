"""In-memory pod cache: phase-change diffing and relist reconciliation.

The reference README promises "Trigger an API call on phase changes"
(``/root/reference/README.md:7``) but ``handle_pod_event`` notifies on every
event (``pod_watcher.py:214-241``). This cache provides both modes
(``watcher.notify_on: all | phase_change``) and is also what lets the
reflector turn a post-410 relist into exact ADDED/MODIFIED/DELETED diffs
 and survive restarts through the checkpoint.

One entry per live pod: ``uid -> [resourceVersion, phase, namespace, name, core]``
where ``core`` is the last serialized payload core (or ``None`` if the pod
was never notified). With ``watcher.alerts.container_failures`` an entry also
remembers the pod's failure signature (``swap_failure``), and with
``watcher.alerts.pod_conditions`` the signature of its condition findings
(``swap_condition``), and with ``watcher.alerts.terminating`` whether its
graceful deletion had begun (``swap_terminating``), all in memory only: none
is in ``to_records``, so none reaches a checkpoint, a hand-over or a parting
record. The same holds for the deletion deadline of a terminating pod and the
mark that says it was reported overdue
(``watcher.alerts.terminating_overdue_seconds``: ``set_deadline``,
``deadline``, ``tracked``, ``take_overdue``), and for the creation time of a
pod still ``Pending`` with a mark of its own
(``watcher.alerts.pending_overdue_seconds``: ``set_pending_since``,
``pending_since``, ``pending_tracked``, ``take_pending_overdue``). With that
option the core of a ``Pending`` line nobody sent is kept for the sweep to
report from (``keep_core``): marked as kept, it is dropped when the
pending-since is cleared, and a send (``set_core``) replaces it. The mark is in
memory only: a checkpoint writes a kept core like any core, and after a restart
it counts as an ordinary one.

Two implementations share this interface: :class:`PodCache` (a dict of
lists, used by the Python engine) and ``_kwcore.PodCache`` (C++,
``ops/csrc/podcache.inc``), which the fused native pipeline updates without
creating Python objects. Callers other than the two pipelines use only the
methods below; ``get``/``items``/``pop`` of the native cache return copies.
"""

from __future__ import annotations

from typing import Dict, Iterator, List, Optional, Tuple

RV, PHASE, NS, NAME, CORE = range(5)
FAILURE = 5  # PodCache only, and only once swap_failure stored one
CONDITION = 6  # PodCache only, and only once swap_condition stored one
TERMINATING = 7  # PodCache only, and only once swap_terminating stored one
MISSING = object()


class PodCache:
    __slots__ = ("entries", "deadlines", "reported", "pendings", "pending_reported", "kept")

    def __init__(self) -> None:
        # a sixth element, the failure signature, is appended by swap_failure
        # only; a seventh, the condition signature, by swap_condition only;
        # an eighth, the terminating signature, by swap_terminating only
        self.entries: Dict[str, list] = {}
        # uid -> deletion deadline (s since the epoch) of the entries that have
        # one, and the uids among them already reported overdue
        self.deadlines: Dict[str, int] = {}
        self.reported: set = set()
        # uid -> creation time of the entries still Pending, the uids among them
        # already reported pending-overdue, and the uids whose core is a kept one
        self.pendings: Dict[str, int] = {}
        self.pending_reported: set = set()
        self.kept: set = set()

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
        """Store the core of an unsent ``Pending`` line, marked as kept:
        clearing the pending-since drops it, :meth:`set_core` replaces it."""
        ent = self.entries.get(uid)
        if ent is not None:
            ent[CORE] = core
            self.kept.add(uid)

    def core_kept(self, uid: str) -> bool:
        return uid in self.kept

    def swap_failure(self, uid: str, sig: int) -> int:
        """Store the pod's failure signature (models/findings.py); returns the
        previous one, 0 for none. A pod not cached stores nothing."""
        ent = self.entries.get(uid)
        if ent is None:
            return 0
        if len(ent) > FAILURE:
            prev = ent[FAILURE]
            ent[FAILURE] = sig
            return prev
        if sig:
            ent.append(sig)
        return 0

    def swap_condition(self, uid: str, sig: int) -> int:
        """As :meth:`swap_failure`, for the signature of the pod's condition
        findings; the two are independent."""
        ent = self.entries.get(uid)
        if ent is None:
            return 0
        if len(ent) > CONDITION:
            prev = ent[CONDITION]
            ent[CONDITION] = sig
            return prev
        if sig:
            if len(ent) == FAILURE:
                ent.append(0)
            ent.append(sig)
        return 0

    def swap_terminating(self, uid: str, sig: int) -> int:
        """As :meth:`swap_failure`, for the terminating signature (1 or 0);
        independent of the other two."""
        ent = self.entries.get(uid)
        if ent is None:
            return 0
        if len(ent) > TERMINATING:
            prev = ent[TERMINATING]
            ent[TERMINATING] = sig
            return prev
        if sig:
            ent.extend([0] * (TERMINATING - len(ent)))
            ent.append(sig)
        return 0

    def put(self, uid: str, rv: Optional[str], phase: Optional[str], ns: Optional[str],
            name: Optional[str], core: Optional[bytes] = None) -> None:
        self.entries[uid] = [rv, phase, ns, name, core]
        self._untrack(uid)  # a whole new entry: nothing known of its deletion

    def pop(self, uid: str, default=None):
        self._untrack(uid)
        return self.entries.pop(uid, default)

    def clear(self) -> None:
        self.entries.clear()
        self.deadlines.clear()
        self.reported.clear()
        self.pendings.clear()
        self.pending_reported.clear()
        self.kept.clear()

    def _untrack(self, uid: str) -> None:
        """The entry is gone or a whole new one: nothing is known of it."""
        self._untrack_deadline(uid)
        if self.pendings or self.kept:
            self.pendings.pop(uid, None)
            self.pending_reported.discard(uid)
            self.kept.discard(uid)

    # -- deletion deadlines (watcher.alerts.terminating_overdue_seconds) --------
    def _untrack_deadline(self, uid: str) -> None:
        if self.deadlines:
            self.deadlines.pop(uid, None)
            self.reported.discard(uid)

    def set_deadline(self, uid: str, due: Optional[int]) -> None:
        """Store the pod's deletion deadline. ``None`` clears it and the
        reported mark; a value keeps the mark (a deadline that moves does not
        re-alert). A pod not cached stores nothing."""
        if due is None:
            self._untrack_deadline(uid)
        elif uid in self.entries:
            self.deadlines[uid] = due

    def deadline(self, uid: str) -> Optional[int]:
        return self.deadlines.get(uid)

    def tracked(self) -> int:
        """How many entries have a deadline."""
        return len(self.deadlines)

    def take_overdue(self, now_s: int, after_s: int, scope_ns: Optional[str] = None) -> List[tuple]:
        """``(uid, namespace, name, core, deadline)`` of every entry ``after_s``
        seconds or more past its deadline at ``now_s``, not yet reported, that
        has a payload core (of namespace ``scope_ns`` only, if given); each one
        is marked reported. An entry without a core is left unmarked."""
        out = []
        for uid, due in self.deadlines.items():
            if now_s - due < after_s or uid in self.reported:
                continue
            ent = self.entries[uid]
            if ent[CORE] is None or (scope_ns is not None and ent[NS] != scope_ns):
                continue
            out.append((uid, ent[NS], ent[NAME], ent[CORE], due))
        self.reported.update(t[0] for t in out)
        return out

    # -- pods still Pending (watcher.alerts.pending_overdue_seconds) -------------
    def set_pending_since(self, uid: str, since: Optional[int]) -> None:
        """Store the creation time of a pod still ``Pending``. ``None`` clears
        it, its reported mark and a kept core; a value keeps the mark. A pod
        not cached stores nothing."""
        if since is None:
            if self.pendings or self.kept:
                self.pendings.pop(uid, None)
                self.pending_reported.discard(uid)
                if uid in self.kept:
                    self.kept.discard(uid)
                    self.entries[uid][CORE] = None
        elif uid in self.entries:
            self.pendings[uid] = since

    def pending_since(self, uid: str) -> Optional[int]:
        return self.pendings.get(uid)

    def pending_tracked(self) -> int:
        """How many entries have a pending-since."""
        return len(self.pendings)

    def take_pending_overdue(self, now_s: int, after_s: int, scope_ns: Optional[str] = None) -> List[tuple]:
        """As :meth:`take_overdue`: ``(uid, namespace, name, core, since)`` of
        every entry still ``Pending`` ``after_s`` seconds or more after its
        creation at ``now_s``, not yet reported as that, that has a core."""
        out = []
        for uid, since in self.pendings.items():
            if now_s - since < after_s or uid in self.pending_reported:
                continue
            ent = self.entries[uid]
            if ent[CORE] is None or (scope_ns is not None and ent[NS] != scope_ns):
                continue
            out.append((uid, ent[NS], ent[NAME], ent[CORE], since))
        self.pending_reported.update(t[0] for t in out)
        return out

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
