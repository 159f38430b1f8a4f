"""Watch-stream decoding: NDJSON bytes → compact event tuples.

This is the per-event hot path the reference pays inside the ``kubernetes``
library (line iteration, ``json.loads``, reflective ``V1Pod`` deserialisation;
SURVEY §3.2 "Hot loop"). Two engines share one interface:

* :class:`PyDecoder` — stdlib ``json`` + :mod:`..models.payload`; the
  semantic reference for the native engine.
* ``NativeDecoder`` (:mod:`.native`) — C++ single-pass extractor
  (``ops/csrc/kwcore.cpp``) that never builds Python objects for the pod body
  and emits the payload core bytes directly.

Event tuple layout (index constants below)::

    (type, uid, namespace, name, resourceVersion, phase, has_status, obj, extra)

``obj`` is the pod dict (Python engine) or the payload core bytes (native);
call ``decoder.core(ev)`` to get core bytes either way. ``extra`` carries the
``Status`` dict of an ``ERROR`` event, the error text of an ``INVALID`` line,
or — on a ``BOOKMARK`` — whether it ends a WatchList's initial events.

With ``watcher.alerts.container_failures`` on, a pod event carries a tenth
field, ``E_FAILURE``: the failure signature of the pod's container findings
(:mod:`..models.findings`; 0 for none). With the option off tuples keep their
nine fields. With ``watcher.alerts.pod_conditions`` on, a pod event carries an
eleventh, ``E_CONDITION``: the signature of the pod's condition findings
(``E_FAILURE`` is then present too, 0 while container failures are off). With
``watcher.alerts.terminating`` on, a twelfth, ``E_TERMINATING``: 1 when the
pod's graceful deletion has begun, else 0 (the two before it are then present
too, 0 while their options are off). With
``watcher.alerts.terminating_overdue_seconds`` above 0, a thirteenth,
``E_DEADLINE``: the pod's deletion deadline in seconds since the epoch
(:func:`..models.findings.deletion_deadline`) or ``None``, and ``None`` on
``DELETED``. With ``watcher.alerts.pending_overdue_seconds`` above 0, a
fourteenth, ``E_PENDING_SINCE``: the creation time of a pod still ``Pending``
(:func:`..models.findings.pending_since`) or ``None``, and ``None`` on
``DELETED`` (the four before it are then present too, 0 or ``None`` while
their options are off). With ``watcher.alerts.unready_overdue_seconds`` above
0, a fifteenth, ``E_UNREADY_SINCE``: the time the ``Ready`` condition of a
``Running`` pod turned ``False`` (:func:`..models.findings.unready_since`) or
``None``, and ``None`` on ``DELETED`` (the five before it likewise present).
"""

from __future__ import annotations

import json
from typing import Any, Dict, List, Optional, Tuple

from ..models.findings import (condition_findings, condition_rules, condition_signature, container_findings,
                               deletion_deadline, failure_signature, pending_since, reason_set, terminating_signature,
                               unready_since)
from ..models.payload import build_core, repr_states_ok
from ..net.http import json_input

E_TYPE, E_UID, E_NS, E_NAME, E_RV, E_PHASE, E_HAS_STATUS, E_OBJ, E_EXTRA = range(9)
E_FAILURE = 9  # only with watcher.alerts.container_failures (or pod_conditions)
E_CONDITION = 10  # only with watcher.alerts.pod_conditions (or terminating)
E_TERMINATING = 11  # only with watcher.alerts.terminating
E_DEADLINE = 12  # only with watcher.alerts.terminating_overdue_seconds > 0 (which needs terminating)
E_PENDING_SINCE = 13  # only with watcher.alerts.pending_overdue_seconds > 0
E_UNREADY_SINCE = 14  # only with watcher.alerts.unready_overdue_seconds > 0

ADDED, MODIFIED, DELETED, BOOKMARK, ERROR, INVALID = (
    "ADDED", "MODIFIED", "DELETED", "BOOKMARK", "ERROR", "INVALID")

_POD_TYPES = (ADDED, MODIFIED, DELETED)

# WatchList (``sendInitialEvents=true``): annotation on the BOOKMARK that ends the initial state
INITIAL_EVENTS_END = "k8s.io/initial-events-end"


def _s(v: Any) -> Optional[str]:
    """Identity fields are strings; anything else (null, numbers) reads as None."""
    return v if isinstance(v, str) else None


def event_from_object(etype: str, obj: Dict[str, Any]) -> tuple:
    if etype == ERROR:
        return (ERROR, None, None, None, None, None, False, None, obj)
    md = obj.get("metadata")
    if not isinstance(md, dict):  # not an object: absent (as the native engine reads it)
        md = {}
    st = obj.get("status")
    if st is not None and not isinstance(st, dict):
        st = None
    extra = None
    if etype == BOOKMARK:  # True on the WatchList end-of-initial-events marker
        ann = md.get("annotations")
        extra = isinstance(ann, dict) and ann.get(INITIAL_EVENTS_END) == "true"
    return (etype, _s(md.get("uid")), _s(md.get("namespace")), _s(md.get("name")),
            _s(md.get("resourceVersion")), _s(st.get("phase")) if st is not None else None,
            st is not None, obj, extra)


class PyDecoder:
    name = "python"

    def __init__(self, environment: str, state_format: str = "structured", extra: int = 0,
                 failures: bool = False, failure_reasons=None, conditions: bool = False,
                 rules=None, terminating: bool = False, overdue: bool = False, pending: bool = False,
                 unready: bool = False) -> None:
        self.environment = environment
        self.state_format = state_format
        self.extra = extra
        self.failures = failures
        self.reasons = reason_set(failure_reasons)
        self.conditions = conditions
        self.rules = condition_rules(rules)
        self.terminating = terminating
        self.overdue = overdue and terminating
        self.pending = pending
        self.unready = unready
        self._partial = b""
        self._cbuf = b""
        self._cremain = 0
        self._cstate = 0  # 0 size line, 1 data, 2 data CRLF, 3 trailers, 4 done

    def reset(self) -> None:
        self._partial = b""
        self._cbuf = b""
        self._cremain = 0
        self._cstate = 0

    def body_done(self) -> bool:
        return self._cstate == 4

    def feed_chunked(self, data: bytes) -> List[tuple]:
        """Like :meth:`feed` for input that still carries HTTP chunked framing."""
        buf = self._cbuf + data if self._cbuf else data
        self._cbuf = b""
        out: List[tuple] = []
        i, n = 0, len(buf)
        while i < n and self._cstate != 4:
            st = self._cstate
            if st == 1:
                take = min(self._cremain, n - i)
                out.extend(self.feed(buf[i:i + take]))
                i += take
                self._cremain -= take
                if self._cremain == 0:
                    self._cstate = 2
                continue
            nl = buf.find(b"\n", i)
            if nl < 0:
                if st != 2:
                    self._cbuf = buf[i:]
                break
            line = buf[i:nl].rstrip(b"\r")
            i = nl + 1
            if st == 0:
                size = int(line.split(b";", 1)[0].strip(), 16)
                if size == 0:
                    self._cstate = 3
                else:
                    self._cremain = size
                    self._cstate = 1
            elif st == 2:
                self._cstate = 0
            elif st == 3 and not line:
                self._cstate = 4
        return out

    def feed(self, data: bytes) -> List[tuple]:
        buf = self._partial + data if self._partial else data
        lines = buf.split(b"\n")
        self._partial = lines.pop()
        out = []
        for line in lines:
            if not line.strip():
                continue
            out.append(self.decode_line(line))
        return out

    def decode_line(self, line: bytes) -> tuple:
        try:
            doc = json.loads(line)
            etype = doc["type"]
            obj = doc["object"]
            if not isinstance(etype, str):
                raise ValueError("type is not a JSON string")
            if not isinstance(obj, dict):
                raise ValueError("object is not a JSON object")
            if self.state_format == "python_repr" and etype in _POD_TYPES and not repr_states_ok(obj):
                raise ValueError("container state is not an object")
        except (ValueError, KeyError, TypeError) as exc:
            return (INVALID, None, None, None, None, None, False, None, f"{exc}: {line[:200]!r}")
        except RecursionError:  # nested deeper than json.loads can follow
            return (INVALID, None, None, None, None, None, False, None, f"nested too deeply: {line[:200]!r}")
        return self._event(etype, obj)

    def _event(self, etype: str, obj: Dict[str, Any]) -> tuple:
        ev = event_from_object(etype, obj)
        unready = self.unready
        pending = self.pending or unready  # (the slot is there; the value only with its own option)
        if (self.failures or self.conditions or self.terminating or pending) and etype in _POD_TYPES:
            live = etype != DELETED
            ev += (failure_signature(container_findings(obj, self.reasons)) if live and self.failures else 0,)
            if self.conditions or self.terminating or pending:
                ev += (condition_signature(condition_findings(obj, self.rules)) if live and self.conditions else 0,)
            if self.terminating or pending:
                ev += (terminating_signature(obj) if live and self.terminating else 0,)
                if self.overdue or pending:
                    ev += (deletion_deadline(obj) if live and self.overdue else None,)
                if pending:
                    ev += (pending_since(obj) if live and self.pending else None,)
                if unready:
                    ev += (unready_since(obj) if live else None,)
        return ev

    def decode_list(self, body: bytes) -> Tuple[Optional[str], Optional[str], List[tuple]]:
        """``ValueError``, and nothing else, for a body that is not JSON (or is
        nested deeper than json.loads can follow), has trailing data, is not an
        object, or whose ``metadata`` / ``items`` is neither object / array nor null."""
        try:
            doc = json.loads(json_input(body))  # a LIST page over 4 MiB arrives as an mmap
        except RecursionError:
            raise ValueError("invalid list body: nested too deeply") from None
        if not isinstance(doc, dict):
            raise ValueError("invalid list body: not a JSON object")
        md = doc.get("metadata")
        if md is None:
            md = {}
        elif not isinstance(md, dict):
            raise ValueError("invalid list body: metadata is not an object")
        items = doc.get("items")
        if items is None:
            items = []
        elif not isinstance(items, list):
            raise ValueError("invalid list body: items is not an array")
        return (_s(md.get("resourceVersion")), _s(md.get("continue")) or None,
                [self._event(ADDED, it) for it in items if isinstance(it, dict)])

    def core(self, ev: tuple) -> bytes:
        return build_core(ev[E_OBJ], self.environment, self.state_format, self.extra, self.reasons, self.rules)

    def core_from_summary(self, uid: str, ns: Optional[str], name: Optional[str],
                          phase: Optional[str]) -> bytes:
        pod = {"metadata": {"uid": uid, "namespace": ns, "name": name}}
        if phase is not None:
            pod["status"] = {"phase": phase}
        return build_core(pod, self.environment, self.state_format, self.extra, self.reasons, self.rules)


VALIDATE_MODES = {"off": 0, "payload": 1, "full": 2}


def make_decoder(engine: str, environment: str, state_format: str = "structured", extra: int = 0,
                 validate: str = "payload", failures: bool = False, failure_reasons=None,
                 conditions: bool = False, condition_rules=None, terminating: bool = False,
                 overdue: bool = False, pending: bool = False, unready: bool = False):
    """``engine="native"`` requires the C++ extension and raises if it is missing.
    ``extra`` is a :func:`..models.payload.extra_mask`; ``validate`` is
    ``watcher.validate`` (the Python engine always has json.loads' verdict);
    ``failures`` / ``failure_reasons`` are ``watcher.alerts.container_failures``
    and ``container_failure_reasons`` (None: the default set), ``conditions`` /
    ``condition_rules`` are ``watcher.alerts.pod_conditions`` and
    ``pod_condition_rules`` (None: the default rules), ``terminating`` is
    ``watcher.alerts.terminating``, ``overdue`` whether
    ``watcher.alerts.terminating_overdue_seconds`` is above 0, ``pending``
    whether ``watcher.alerts.pending_overdue_seconds`` is, ``unready`` whether
    ``watcher.alerts.unready_overdue_seconds`` is."""
    if engine == "python":
        return PyDecoder(environment, state_format, extra, failures, failure_reasons, conditions, condition_rules,
                         terminating, overdue, pending, unready)
    from .native import NativeDecoder
    return NativeDecoder(environment, state_format, extra, validate, failures, failure_reasons, conditions,
                         condition_rules, terminating, overdue, pending, unready)
