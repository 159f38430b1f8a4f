"""bench.py's contract with the driver.

Round 4's last stdout line grew to 22-27 KB of per-second rows; the driver
keeps only the tail of the output (~8.5 KB), so BENCH_r04.json had
``parsed: null`` and the round's headline went unmeasured. The last line is now
a compact headline (< 4,096 bytes) with BASELINE.json's metric and config and
the latency / spread / exactly-once figures; every diagnostic goes to the full
record (``--json-out``, default a file under /tmp named in the headline).
Also: stderr carries one line, and no process of the bench outlives it (the
driver counted ``procs_at_end: 2`` in r03/r04: the stub sink's forked workers,
still writing their final dump, were never waited for).
"""

import json
import os
import subprocess
import sys
import uuid

import numpy as np
import pytest

from conftest import HEADLINE_MAX_BYTES, ROOT, bench_result

sys.path.insert(0, ROOT)
import bench  # noqa: E402

BASELINE = json.load(open(os.path.join(ROOT, "BASELINE.json")))

HEADLINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "timed_seconds",
                 "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "p50_latency_ms",
                 "p99_latency_ms", "latency_1k", "loop_lag_1k", "rate_series", "exactly_once",
                 "reference_equiv_events_per_s", "staging", "placement_apart", "validate_full", "detail_json")


def tagged_processes(tag: str) -> list:
    """Processes whose environment carries ``tag`` (the bench and everything it started)."""
    out = []
    for pid in os.listdir("/proc"):
        if not pid.isdigit():
            continue
        try:
            with open(f"/proc/{pid}/environ", "rb") as fh:
                if f"K8S_BENCH_TAG={tag}".encode() in fh.read().split(b"\0"):
                    with open(f"/proc/{pid}/cmdline", "rb") as fc:
                        out.append((int(pid), fc.read().replace(b"\0", b" ").decode(errors="replace")))
        except OSError:
            pass
    return out


def run_driver_shape(tmp_path, extra=(), timeout=600):
    """The driver's command (``--steps 20 --warmup 5``, every phase on) shortened via --pods-per-step."""
    tag = uuid.uuid4().hex
    out = str(tmp_path / "full.json")
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "20", "--warmup", "5",
                           "--pods-per-step", "200", "--rounds-per-step", "2", "--latency-seconds", "2",
                           "--latency-seconds-high", "2", "--ref-events", "300", "--staging-steps", "1",
                           *extra, "--json-out", out],
                          capture_output=True, text=True, timeout=timeout, cwd=ROOT,
                          env=dict(os.environ, K8S_BENCH_TAG=tag))
    left = tagged_processes(tag)  # at once: the driver looks right after the exit
    return proc, out, left


def check_headline(proc, out, left):
    d = bench_result(proc, out)
    head = d["_headline"]
    last = proc.stdout.strip().splitlines()[-1]
    assert len(last.encode()) < HEADLINE_MAX_BYTES
    for key in HEADLINE_KEYS:
        assert key in head, key
    assert head["metric"] == BASELINE["metric"]
    assert head["steps"] == 20 and head["warmup"] == 5 and head["n_gpus"] == 1
    assert head["value"] > 0 and head["higher_is_better"] is True and head["scaling"] == "weak"
    assert head["exactly_once"] is True and head["notify_failed"] == 0
    assert head["staging"]["exactly_once"] and head["placement_apart"]["exactly_once"]
    # the headline's work level is named, with the rate at the reference's (every byte JSON-checked)
    assert {head["config"][k] for k in ("engine", "validate", "state_format")} == {"native", "payload", "structured"}
    assert head["validate_full"]["exactly_once"] and head["validate_full"]["value"] > 0
    assert d["validate_full"]["validate"] == "full"
    assert head["reference_equiv_events_per_s"] > 0 and head["vs_baseline"] > 0
    assert head["p50_latency_ms"] > 0 and head["latency_1k"]["p99_ms"] >= head["latency_1k"]["p50_ms"] > 0
    lag = head["loop_lag_1k"]
    assert lag["seconds"] >= 1 and lag["max_ms"] >= lag["median_max_ms"] >= 0
    # every second of the 1k ev/s phase with a > 1 ms notification names its cause
    rows = d["latency_high_seconds_rank0"]["rows"]
    assert rows and all("loop_lag_max_ms" in r and "sampler_ms" in r and "lat_n" in r for r in rows)
    assert all(r.get("cause") in bench.PhaseSampler.CAUSES for r in rows if r.get("lat_over_1ms"))
    assert sum(r["lat_n"] for r in rows) == head["latency_1k"]["samples"]
    # stderr: the one line naming the full record
    assert len(proc.stderr.strip().splitlines()) <= 2, proc.stderr[-2000:]
    assert not left, left
    return d


def test_driver_shape_headline_is_compact_and_nothing_outlives_the_bench(tmp_path):
    check_headline(*run_driver_shape(tmp_path, extra=("--no-placement", "--sink-workers", "1")))


def test_plain_run_times_the_steps_and_dumps_the_last_steps_outputs(tmp_path):
    """Without ``--full`` the bench sets up, warms up, times ``--steps`` steps
    and prints the result line: no latency phase, exactly-once count,
    reference-equivalent or further run, whatever their options say. With
    ``--dump-outputs`` the notifications of the last timed step are written as
    float64 arrays; they are the ones the seeded replay model makes notifiable."""
    from k8s_watcher_amd.testing.cluster_replay import ClusterModel, namespace_names
    pods, rounds, steps, warmup, n_ns = 300, 2, 3, 1, 8
    out, dump = str(tmp_path / "plain.json"), tmp_path / "dump"
    proc = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                           "--warmup", str(warmup), "--pods-per-step", str(pods), "--rounds-per-step", str(rounds),
                           "--namespaces", str(n_ns), "--latency-seconds", "2", "--ref-events", "300",
                           "--sink-workers", "1", "--no-placement", "--dump-outputs", str(dump), "--json-out", out],
                          capture_output=True, text=True, timeout=120, cwd=ROOT)
    d = bench_result(proc, out)
    head = d["_headline"]
    assert head["metric"] == BASELINE["metric"] and head["unit"] == "pod-events/s" and head["dtype"] == "n/a"
    assert head["steps"] == steps and head["warmup"] == warmup and head["higher_is_better"] is True
    assert d["per_rank"][0]["events"] == steps * rounds * pods * 5
    # ms_per_step is the timed region over --steps: value x that time gives the timed steps' events back
    assert head["ms_per_step"] > 0
    assert head["value"] * head["ms_per_step"] * steps / 1000 == pytest.approx(steps * rounds * pods * 5, rel=1e-3)
    for key in ("p50_latency_ms", "latency_1k", "exactly_once", "reference_equiv_events_per_s", "vs_baseline",
                "staging", "placement_apart", "validate_full"):
        assert head[key] is None, key
    assert d["latency_samples"] == 0 and d["verify"] is None and d["notify_failed"] == 0

    assert sorted(os.listdir(dump)) == ["counts.npy", "notifications.npy"]
    rows, counts = np.load(dump / "notifications.npy"), np.load(dump / "counts.npy")
    assert rows.dtype == np.float64 and counts.dtype == np.float64
    names = namespace_names(n_ns)
    m = ClusterModel(names, pods, targets=bench.target_namespaces("even", names), critical_only=True)
    et = {0: "ADDED", 4: "DELETED"}
    want = sorted((float(s), float(m.ev_pod[g]), float(bench.DUMP_EVENT_TYPES.index(et.get(int(m.ev_stage[g]), "MODIFIED"))),
                   float(bench.DUMP_PHASES.index(m.proto_phase[int(m.ev_pod[g]) % len(m.protos)][int(m.ev_stage[g])])),
                   -1.0, 1.0)
                  for s in range((warmup + steps - 1) * rounds, (warmup + steps) * rounds)
                  for g in np.flatnonzero(m.notifiable))
    assert len(want) > 0 and rows.shape == (len(want), 6)
    assert np.array_equal(rows, np.array(want))
    per_step = rounds * int(m.notifiable.sum())
    assert counts.tolist() == [steps * rounds * pods * 5, per_step, per_step]


def test_notification_rows_are_sorted_and_sampled_with_a_fixed_seed(monkeypatch):
    keys = {"%08x-0000-4000-8000-%012x|%s|%s" % (s, p, e, ph): n
            for s, p, e, ph, n in ((7, 2, "DELETED", "Running", 1), (7, 1, "MODIFIED", "Failed", 2),
                                   (6, 9, "ADDED", "Pending", 1), (8, 0, "DELETED", "Succeeded", 1),
                                   (7, 1, "DELETED", "Failed", 1))}
    keys["%08x-0000-4000-8000-%012x|MODIFIED|Running|12" % (7, 3)] = 1
    rows, received, distinct = bench.notification_rows(keys, 7, 8)
    assert rows.tolist() == [[7, 1, 1, 3, -1, 2], [7, 1, 2, 3, -1, 1], [7, 2, 2, 1, -1, 1], [7, 3, 1, 1, 12, 1]]
    assert (received, distinct) == (5.0, 4.0)
    monkeypatch.setattr(bench, "DUMP_MAX_ROWS", 2)
    a, received, distinct = bench.notification_rows(keys, 7, 8)
    b, _, _ = bench.notification_rows(dict(reversed(list(keys.items()))), 7, 8)
    assert a.shape == (2, 6) and np.array_equal(a, b) and (received, distinct) == (5.0, 4.0)
    assert all(r in rows.tolist() for r in a.tolist()) and a.tolist() == sorted(a.tolist())


def test_attribution_names_the_segment_that_took_the_time():
    """PhaseSampler._attribute on synthetic (read, submit, sent, ack) samples:
    per-second counts by ack time, and each slow second's dominant segment."""
    s = object.__new__(bench.PhaseSampler)
    s.t0_mono_ns = 10_000_000_000
    s.rows = [{"t": 1.0}, {"t": 2.0}, {"t": 3.0}]
    ms = 1_000_000
    t = s.t0_mono_ns
    samples = [
        # second 0: fast ones only
        (t + 100 * ms, t + 100 * ms + 50_000, t + 100 * ms + 60_000, t + 100 * ms + 300_000),
        (t + 200 * ms, t + 200 * ms + 50_000, t + 200 * ms + 60_000, t + 200 * ms + 200_000),
        # second 1: one slow in the sink round trip
        (t + 1100 * ms, t + 1100 * ms + 50_000, t + 1100 * ms + 60_000, t + 1100 * ms + 3 * ms),
        # second 2: a slow one waiting for the loop (read -> submit)
        (t + 2100 * ms, t + 2100 * ms + 2 * ms, t + 2100 * ms + 2 * ms + 10_000, t + 2100 * ms + 2 * ms + 90_000),
        # submitted before detail was on (no submit stamp): ignored
        (t + 2200 * ms, 0, t + 2200 * ms, t + 2200 * ms + 9 * ms),
    ]
    s._attribute(np.array(samples, dtype=np.int64).tobytes())
    r0, r1, r2 = s.rows
    assert r0["lat_n"] == 2 and r0["lat_over_1ms"] == 0 and "cause" not in r0
    assert r1["lat_n"] == 1 and r1["lat_over_1ms"] == 1 and r1["cause"] == "sink_rtt"
    assert r1["outlier_ms"]["sink_rtt"] == pytest.approx(2.94, abs=0.01)
    assert r2["lat_n"] == 1 and r2["cause"] == "reader_to_loop"
    summary = bench.lag_summary([dict(r, loop_lag_max_ms=0.1) for r in s.rows])
    assert summary["seconds_lat_over_1ms"] == 2 and summary["causes"] == {"sink_rtt": 1, "reader_to_loop": 1}
    # the same seconds when the scheduler kept the loop thread (or the sink)
    # runnable but off a CPU for >= 1 ms: the cause is the preemption
    s.rows = [{"t": 1.0}, {"t": 2.0, "sink_runq_ms": 1.7}, {"t": 3.0, "loop_runq_ms": 2.4}]
    s._attribute(np.array(samples, dtype=np.int64).tobytes())
    assert [r.get("cause") for r in s.rows] == [None, "sink_preempted", "loop_preempted"]


def test_loop_lag_probe_sees_a_blocked_loop():
    """_kwcore.LoopLag: a 20 ms block of the loop shows as a lag of that
    order (the ticker thread itself may be preempted on a loaded test box, so
    the bound is loose); an idle loop's ticks are answered in well under a
    millisecond."""
    import asyncio
    import time

    from k8s_watcher_amd.ops import native

    async def body():
        p = native.load().LoopLag(500)
        loop = asyncio.get_running_loop()
        loop.add_reader(p.fd(), p.ack)
        await asyncio.sleep(0.3)
        p.take()
        await asyncio.sleep(0.3)
        idle = p.take()
        time.sleep(0.02)  # block the loop
        await asyncio.sleep(0.05)
        blocked = p.take()
        loop.remove_reader(p.fd())
        p.close()
        return idle, blocked

    idle, blocked = asyncio.run(body())
    assert idle["n"] >= 300  # ~600 ticks at 500 us; a loaded test box may skip some
    assert blocked["max_us"] >= 10000 and blocked["over_1ms"] >= 1
    # the shared CPU may preempt the loop (or the ticker) now and then, more
    # so under a parallel test run: most idle ticks are answered fast
    assert idle["over_1ms"] <= max(3, idle["n"] // 10) and idle["mean_us"] < 1000, idle


def test_set_overrides_fold_into_one_nested_dict():
    """bench --set KEY=VALUE (repeatable, main.py --set's syntax): every
    per-setting bench flag of earlier rounds is one of these now (round-6
    pruning: 63 -> 45 flags)."""
    args = bench.parse_args(["--set", "clusterapi.pool.io_thread=on", "--set", "watcher.watch_tls_threads=5",
                             "--set", "watcher.thread_pinning=none", "--set", "watcher.validate=full"])
    ov = bench.set_overrides(args)
    # values are YAML (as main.py --set): "on" is true, which io_thread reads as "on"
    assert ov == {"clusterapi": {"pool": {"io_thread": True}},
                  "watcher": {"watch_tls_threads": 5, "thread_pinning": "none", "validate": "full"}}
    assert bench.set_value(args, "watcher.thread_pinning", "auto") == "none"
    assert bench.set_value(args, "watcher.decode_threads", "auto") == "auto"
    assert bench.set_value(bench.parse_args([]), "watcher.thread_pinning", "auto") == "auto"
    import re
    flags = re.findall(r'add_argument\("(--[a-z0-9-]+)"', open(bench.__file__).read())
    assert 40 <= len(flags) <= 50, len(flags)
