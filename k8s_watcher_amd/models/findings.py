"""Container failure findings (``watcher.alerts.container_failures``).

The reference's critical filter looks at the pod phase only
(``/root/reference/watcher/pod_watcher.py:204-212``), and the failures an
operator most wants an alert for do not move it: a container in
``CrashLoopBackOff`` or one that was ``OOMKilled`` and restarted leaves the pod
``Running``; ``ImagePullBackOff`` leaves it ``Pending``.

:func:`container_findings` is a pure function of the pod object and the
semantic reference for the native walker (``ops/csrc/findings.inc``). It walks
``status.initContainerStatuses``, then ``status.containerStatuses`` (ephemeral
containers are not looked at), each element that is a JSON object, in order:

* ``waiting`` — ``state.waiting.reason`` is a string of the configured set;
* ``terminated`` — only without a ``waiting`` finding:
  ``state.terminated.exitCode`` is an integer other than 0;
* ``restarted`` — ``restartCount`` is an integer above 0 and
  ``lastState.terminated.exitCode`` is an integer other than 0.

"Integer" is a JSON integer token: ``true`` is none, nor are ``1.0`` and
``1e2`` (json.loads makes those floats). A value of the wrong JSON type reads
as absent, as everywhere else (docs/DEVIATIONS.md, hostile but valid JSON).

Pod condition findings (``watcher.alerts.pod_conditions``) close the same gap
for the scheduler's side: an unschedulable pod stays ``Pending`` with
``PodScheduled=False:Unschedulable``, a pod about to be preempted or evicted
gets ``DisruptionTarget=True`` while it is still ``Running``.
:func:`condition_findings` walks ``status.conditions``, each element that is a
JSON object, in order, and keeps those a rule of
``watcher.alerts.pod_condition_rules`` matches: ``Type=Status`` (any reason, or
none) or ``Type=Status:Reason``, compared exactly as decoded text. A finding is
type, status and reason only — never ``message`` or the times, which the
scheduler rewrites at every attempt.

Terminating (``watcher.alerts.terminating``) is the third member: a pod whose
graceful deletion has begun keeps its phase until the kubelet has stopped it
and every finalizer is gone. :func:`terminating` is true when the pod's
``metadata`` is a JSON object whose ``deletionTimestamp`` is a JSON string, of
any text; the finding is that boolean alone, so a later change of the
timestamp (a forced delete with a shorter grace period) is no new finding.

The deletion deadline (``watcher.alerts.terminating_overdue_seconds``) is the
time the timestamp names: Kubernetes sets it to the moment the pod is expected
to be gone. :func:`deletion_deadline` reads a terminating pod's decoded
timestamp by one exact grammar, ASCII only,
``YYYY-MM-DDTHH:MM:SS[.f{1,9}](Z|+HH:MM|-HH:MM)`` with every field in its
calendar range (year 0001-9999, no second 60, offset 00:00-23:59), and gives
seconds since 1970-01-01T00:00:00Z, the offset applied and the fraction
dropped. Text of any other shape has no deadline: the pod is terminating and
never overdue.

The pending-since (``watcher.alerts.pending_overdue_seconds``) is the creation
time of a pod that is still ``Pending``: :func:`pending_since` reads
``metadata.creationTimestamp`` by that same grammar when ``status`` is an object
whose ``phase`` is the string ``Pending`` and the pod is not terminating.

The unready-since (``watcher.alerts.unready_overdue_seconds``) is the time the
``Ready`` condition of a pod that is ``Running`` turned ``False``:
:func:`unready_since` has a value only when ``status`` is an object whose
``phase`` is the string ``Running``, the pod is not terminating,
``status.conditions`` is a list, the first element of that list that is an
object with ``type`` equal to the string ``Ready`` has ``status`` equal to the
string ``"False"`` (``"Unknown"``, ``"false"`` and ``false`` are not), and that
element's ``lastTransitionTime`` is a string in that same grammar. Later
``Ready`` elements are ignored; a timestamp that is absent or of another shape
gives no value, and such a pod is never overdue.
"""

from __future__ import annotations

import re
from typing import Any, Dict, FrozenSet, Iterable, List, Optional, Tuple

DEFAULT_FAILURE_REASONS: Tuple[str, ...] = (
    "CrashLoopBackOff", "ImagePullBackOff", "ErrImagePull", "ErrImageNeverPull", "InvalidImageName",
    "CreateContainerConfigError", "CreateContainerError", "RunContainerError")

FINDING_FIELDS = ("container", "init", "kind", "reason", "exit_code", "restart_count")

DEFAULT_CONDITION_RULES: Tuple[str, ...] = (
    "PodScheduled=False:Unschedulable", "PodScheduled=False:SchedulerError", "DisruptionTarget=True")

MAX_CONDITION_RULES = 32

CONDITION_FIELDS = ("type", "status", "reason")

ConditionRule = Tuple[str, str, Optional[str]]

_DEFAULT_SET = frozenset(DEFAULT_FAILURE_REASONS)


def reason_set(reasons: Optional[Iterable[str]]) -> FrozenSet[str]:
    return _DEFAULT_SET if reasons is None else frozenset(reasons)


def _int(v: Any) -> Optional[int]:
    return v if isinstance(v, int) and not isinstance(v, bool) else None


def _str(v: Any) -> Optional[str]:
    return v if isinstance(v, str) else None


def _sub(d: Any, key: str) -> Dict[str, Any]:
    """``d[key]`` when both are JSON objects, else nothing."""
    v = d.get(key) if isinstance(d, dict) else None
    return v if isinstance(v, dict) else {}


def container_findings(pod: Dict[str, Any], reasons: Optional[Iterable[str]] = None) -> List[Dict[str, Any]]:
    """The pod's findings, each a dict of :data:`FINDING_FIELDS`; ``[]`` for a healthy pod."""
    rs = reasons if isinstance(reasons, frozenset) else reason_set(reasons)
    st = pod.get("status") if isinstance(pod, dict) else None
    out: List[Dict[str, Any]] = []
    if not isinstance(st, dict):
        return out
    for key, init in (("initContainerStatuses", True), ("containerStatuses", False)):
        arr = st.get(key)
        if not isinstance(arr, list):
            continue
        for cs in arr:
            if not isinstance(cs, dict):
                continue
            name = _str(cs.get("name"))
            rc = _int(cs.get("restartCount"))
            state = cs.get("state")
            wr = _str(_sub(state, "waiting").get("reason"))
            if wr is not None and wr in rs:
                out.append({"container": name, "init": init, "kind": "waiting", "reason": wr,
                            "exit_code": None, "restart_count": rc})
            else:
                term = _sub(state, "terminated")
                ec = _int(term.get("exitCode"))
                if ec is not None and ec != 0:
                    out.append({"container": name, "init": init, "kind": "terminated",
                                "reason": _str(term.get("reason")), "exit_code": ec, "restart_count": rc})
            if rc is not None and rc > 0:
                term = _sub(cs.get("lastState"), "terminated")
                ec = _int(term.get("exitCode"))
                if ec is not None and ec != 0:
                    out.append({"container": name, "init": init, "kind": "restarted",
                                "reason": _str(term.get("reason")), "exit_code": ec, "restart_count": rc})
    return out


def failure_signature(findings: List[Dict[str, Any]]) -> int:
    """Stands for the list: equal exactly when the lists are equal, 0 for the
    empty one. A 64-bit hash, good for this process only (it is never stored)."""
    if not findings:
        return 0
    h = hash(tuple(tuple(f[k] for k in FINDING_FIELDS) for f in findings)) & 0xFFFFFFFFFFFFFFFF
    return h or 1


def parse_condition_rule(text: Any) -> ConditionRule:
    """``Type=Status`` or ``Type=Status:Reason`` -> (type, status, reason or None).
    Split at the first ``=``, the rest at the first ``:``; ``ValueError`` when
    the type, the status or a given reason is empty."""
    if not isinstance(text, str):
        raise ValueError(f"not a string: {text!r}")
    ctype, eq, rest = text.partition("=")
    status, colon, reason = rest.partition(":")
    if not eq or not ctype or not status or (colon and not reason):
        raise ValueError(f"expected Type=Status or Type=Status:Reason, got {text!r}")
    return (ctype, status, reason if colon else None)


def condition_rules(rules: Optional[Iterable[Any]]) -> Tuple[ConditionRule, ...]:
    """The compiled rule set (None: the default rules). Takes the configured
    strings or an already compiled set."""
    src = DEFAULT_CONDITION_RULES if rules is None else rules
    out = tuple(r if isinstance(r, tuple) else parse_condition_rule(r) for r in src)
    if len(out) > MAX_CONDITION_RULES:
        raise ValueError(f"{len(out)} rules, at most {MAX_CONDITION_RULES}")
    return out


_DEFAULT_RULES = condition_rules(None)


def condition_findings(pod: Dict[str, Any], rules: Optional[Iterable[Any]] = None) -> List[Dict[str, Any]]:
    """The pod's condition findings, each a dict of :data:`CONDITION_FIELDS`
    (``reason`` None when absent); ``[]`` when no rule matches."""
    rs = _DEFAULT_RULES if rules is None else condition_rules(rules)
    st = pod.get("status") if isinstance(pod, dict) else None
    out: List[Dict[str, Any]] = []
    conds = st.get("conditions") if isinstance(st, dict) else None
    if not isinstance(conds, list):
        return out
    for cond in conds:
        if not isinstance(cond, dict):
            continue
        ctype, status, reason = _str(cond.get("type")), _str(cond.get("status")), _str(cond.get("reason"))
        for rt, rstat, rreason in rs:
            if rt == ctype and rstat == status and (rreason is None or rreason == reason):
                out.append({"type": ctype, "status": status, "reason": reason})
                break
    return out


def condition_signature(findings: List[Dict[str, Any]]) -> int:
    """As :func:`failure_signature`, of the condition findings."""
    if not findings:
        return 0
    h = hash(tuple(tuple(f[k] for k in CONDITION_FIELDS) for f in findings)) & 0xFFFFFFFFFFFFFFFF
    return h or 1


def terminating(pod: Dict[str, Any]) -> bool:
    """Whether the pod's graceful deletion has begun: ``metadata`` is an object
    and its ``deletionTimestamp`` a string (any other JSON type reads as absent)."""
    md = pod.get("metadata") if isinstance(pod, dict) else None
    return isinstance(md, dict) and isinstance(md.get("deletionTimestamp"), str)


def terminating_signature(pod: Dict[str, Any]) -> int:
    """1 for a terminating pod, 0 otherwise: the text of the timestamp is no part of it."""
    return 1 if terminating(pod) else 0


_DEADLINE = re.compile(r"([0-9]{4})-([0-9]{2})-([0-9]{2})T([0-9]{2}):([0-9]{2}):([0-9]{2})(?:\.[0-9]{1,9})?"
                       r"(?:Z|([+-])([0-9]{2}):([0-9]{2}))")
_MONTH_DAYS = (31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31)


def days_from_civil(y: int, m: int, d: int) -> int:
    """Days from 1970-01-01 to y-m-d in the proleptic Gregorian calendar."""
    y -= m <= 2
    era = y // 400
    yoe = y - era * 400
    doy = (153 * (m + (-3 if m > 2 else 9)) + 2) // 5 + d - 1
    doe = yoe * 365 + yoe // 4 - yoe // 100 + doy
    return era * 146097 + doe - 719468


def timestamp_seconds(text: str) -> Optional[int]:
    """Seconds since the epoch of a timestamp in the deadline grammar, else None."""
    m = _DEADLINE.fullmatch(text)
    if m is None:
        return None
    year, month, day, hour, minute, second = (int(g) for g in m.groups()[:6])
    if year < 1 or not 1 <= month <= 12 or hour > 23 or minute > 59 or second > 59:
        return None
    leap = year % 4 == 0 and (year % 100 != 0 or year % 400 == 0)
    if not 1 <= day <= _MONTH_DAYS[month - 1] + (month == 2 and leap):
        return None
    out = days_from_civil(year, month, day) * 86400 + hour * 3600 + minute * 60 + second
    if m.group(7):
        oh, om = int(m.group(8)), int(m.group(9))
        if oh > 23 or om > 59:
            return None
        off = oh * 3600 + om * 60
        out -= off if m.group(7) == "+" else -off
    return out


def deletion_deadline(pod: Dict[str, Any]) -> Optional[int]:
    """The time a terminating pod is expected to be gone, in seconds since the
    epoch: its ``deletionTimestamp`` read by the module's grammar. None for a
    pod that is not terminating or whose timestamp is of another shape."""
    if not terminating(pod):
        return None
    return timestamp_seconds(pod["metadata"]["deletionTimestamp"])


def pending_since(pod: Dict[str, Any]) -> Optional[int]:
    """The creation time of a pod that is still ``Pending``, in seconds since
    the epoch (``watcher.alerts.pending_overdue_seconds``): its
    ``metadata.creationTimestamp`` read by the module's grammar, when ``status``
    is an object whose ``phase`` is the string ``Pending`` and the pod is not
    terminating (the terminating alerts own that state). None otherwise, and
    for a timestamp that is no string or of another shape."""
    status = pod.get("status")
    if not isinstance(status, dict) or terminating(pod):
        return None
    phase = status.get("phase")
    if not isinstance(phase, str) or phase != "Pending":
        return None
    meta = pod.get("metadata")
    stamp = meta.get("creationTimestamp") if isinstance(meta, dict) else None
    return timestamp_seconds(stamp) if isinstance(stamp, str) else None


def unready_since(pod: Dict[str, Any]) -> Optional[int]:
    """The time the ``Ready`` condition of a ``Running`` pod turned ``False``,
    in seconds since the epoch (``watcher.alerts.unready_overdue_seconds``):
    the ``lastTransitionTime``, read by the module's grammar, of the first
    element of ``status.conditions`` that is an object whose ``type`` is the
    string ``Ready``, when that element's ``status`` is the string ``"False"``,
    ``status.phase`` is the string ``Running`` and the pod is not terminating
    (the terminating alerts own that state). None otherwise, and for a
    timestamp that is no string or of another shape."""
    status = pod.get("status")
    if not isinstance(status, dict) or terminating(pod):
        return None
    phase = status.get("phase")
    if not isinstance(phase, str) or phase != "Running":
        return None
    conditions = status.get("conditions")
    if not isinstance(conditions, list):
        return None
    for cond in conditions:
        if not isinstance(cond, dict):
            continue
        ctype = cond.get("type")
        if not isinstance(ctype, str) or ctype != "Ready":
            continue
        state = cond.get("status")
        if not isinstance(state, str) or state != "False":
            return None
        stamp = cond.get("lastTransitionTime")
        return timestamp_seconds(stamp) if isinstance(stamp, str) else None
    return None
