"""The reader hub's stall guard (``ReaderHub.set_stall_guard``, readerhub.inc).

The hub takes polling off a stream in several places (no buffer, no byte
budget, the stream's read-ahead used up, a pause) and relies on a later call to
put it back. Round 6's stall was a wake-up lost between the two: streams with
unread bytes stayed unpolled, and nothing reported it. The guard measures how
long bytes have waited on a stream the hub is not polling, re-arms a stream
after ``watcher.watch_reader_stall_seconds`` and, where that cannot help, fails
``/readyz``. The known bug is fixed, so these tests leave a stream the way a
lost wake-up would with ``strand()``, the hub's diagnostics hook.
"""

import asyncio
import logging
import os
import random
import socket
import threading
import time

import pytest

from conftest import run

from k8s_watcher_amd.ops.native import load

GUARD = 0.2  # seconds; the tick is then min(250 ms, GUARD / 4)
TICK = GUARD / 4
IN_STARVED = -1  # stream_state: how often the stream's sid is in the starved queue


def _take(core, got, arrived=None):
    """One take(): append every view to got[sid], hand the buffer back."""
    n = 0
    for sid, buf, view, _ns, _err in core.take():
        if view is None:
            continue
        got[sid] += bytes(view)
        view.release()
        core.release(buf)
        n += 1
        if arrived is not None:
            arrived[sid] = time.monotonic()
    return n


def _close(core, pairs):
    core.close()
    for a, b in pairs:
        a.close()
        b.close()


@pytest.mark.parametrize("readers", [1, 2])
def test_stranded_stream_is_recovered(readers):
    """Four streams, one left as a lost wake-up leaves it (EPOLLIN off, in no
    queue), a thousand bytes sent to each. The three deliver at once; the
    stranded one's age shows while it waits, and it delivers once the guard has
    passed — no earlier, and within 2 s (a cap for a loaded machine: by
    construction the guard plus two ticks)."""
    core = load().ReaderHub(64 << 10, 8)
    core.set_readers(readers)
    core.set_stall_guard(GUARD)
    pairs = [socket.socketpair() for _ in range(4)]
    try:
        sids = [core.add(os.dup(b.fileno())) for _a, b in pairs]
        lost = sids[2]
        t_strand = time.monotonic()
        assert core.strand(lost)
        payload = {sid: os.urandom(1000) for sid in sids}
        for (a, _b), sid in zip(pairs, sids):
            a.sendall(payload[sid])
        got = {sid: bytearray() for sid in sids}
        arrived = {}
        seen_age = 0.0
        while len(got[lost]) < 1000 and time.monotonic() - t_strand < 2.0:
            _take(core, got, arrived)
            if lost not in arrived:
                seen_age = max(seen_age, core.oldest_unread())
            time.sleep(0.002)
        others = [sid for sid in sids if sid != lost]
        assert all(bytes(got[sid]) == payload[sid] for sid in others)
        assert lost in arrived, core.stream_state(lost)
        assert all(arrived[sid] < arrived[lost] and arrived[sid] - t_strand < GUARD for sid in others)
        assert GUARD <= arrived[lost] - t_strand <= 2.0
        assert seen_age > 0
        assert bytes(got[lost]) == payload[lost]  # intact and in order
        st = core.stats()
        assert st["stall_recoveries"] == 1 and core.stall_recoveries() == 1
        assert core.oldest_unread() == 0 and st["oldest_unread_ns"] == 0
        sid, age, state = core.last_stall()
        assert sid == lost and age >= GUARD
        assert state[0] == 0 and state[IN_STARVED] == 0  # as strand() left it: not polled, in no queue
        assert core.stream_state(lost)[IN_STARVED] <= 1
    finally:
        _close(core, pairs)


def test_guard_off_changes_nothing():
    """With the guard off a stranded stream stays stranded (nothing arrives,
    no age, no recovery): the hub behaves as before. Turning the guard on then
    delivers the bytes, so it was the hook that stranded it and nothing else."""
    core = load().ReaderHub(64 << 10, 8)
    pairs = [socket.socketpair()]
    try:
        assert core.stats()["stall_guard_ns"] == 0
        sid = core.add(os.dup(pairs[0][1].fileno()))
        assert core.strand(sid) and not core.strand(sid + 1)
        data = os.urandom(1000)
        pairs[0][0].sendall(data)
        got = {sid: bytearray()}
        t0 = time.monotonic()
        while time.monotonic() - t0 < 0.6:
            assert _take(core, got) == 0
            assert core.oldest_unread() == 0 and core.stall_recoveries() == 0
            time.sleep(0.01)
        assert core.last_stall() is None
        core.set_stall_guard(GUARD)
        t0 = time.monotonic()
        while len(got[sid]) < len(data) and time.monotonic() - t0 < 2.0:
            _take(core, got)
            time.sleep(0.002)
        assert bytes(got[sid]) == data
        assert core.stall_recoveries() == 1 and core.last_stall()[0] == sid
        with pytest.raises(ValueError):
            core.set_stall_guard(-1.0)
    finally:
        _close(core, pairs)


def _hold_two_buffers(core, a, sid, data):
    """Send ``data`` (three 4 KiB buffers' worth or more) and take the stream's
    two buffers of read-ahead without handing them back; returns (sender
    thread, [(buf, bytes)])."""
    t = threading.Thread(target=a.sendall, args=(data,))
    t.start()
    held = []
    t0 = time.monotonic()
    while len(held) < 2 and time.monotonic() - t0 < 2.0:
        for _s, buf, view, _ns, _e in core.take():
            if view is not None:
                held.append((buf, bytes(view)))
                view.release()
        time.sleep(0.002)
    assert len(held) == 2, core.stream_state(sid)
    return t, held


@pytest.mark.parametrize("readers", [1, 2])
def test_honest_wait_is_reported_not_recovered(readers):
    """One stream at its read-ahead limit (two buffers taken, neither handed
    back) with a third buffer's worth in the socket: the hub may not poll it,
    so its age is reported and grows past the guard, and no recovery is
    counted — re-arming changes nothing. Handing the buffers back brings the
    rest, and the age is 0 again within two ticks."""
    core = load().ReaderHub(4096, 16)  # every buffer 4 KiB, depth 2
    core.set_readers(readers)
    core.set_stall_guard(GUARD)
    pairs = [socket.socketpair()]
    try:
        sid = core.add(os.dup(pairs[0][1].fileno()))
        data = os.urandom(3 * 4096)
        t, held = _hold_two_buffers(core, pairs[0][0], sid, data)
        time.sleep(0.5)
        assert core.take() == []
        assert core.oldest_unread() >= GUARD and core.stall_recoveries() == 0
        assert core.stats()["oldest_unread_ns"] >= GUARD * 1e9
        got = {sid: bytearray(b"".join(x for _b, x in held))}
        for buf, _x in held:
            core.release(buf)
        t0 = time.monotonic()
        zero_at = None
        while (len(got[sid]) < len(data) or zero_at is None) and time.monotonic() - t0 < 2.0:
            _take(core, got)
            if zero_at is None and core.oldest_unread() == 0:
                zero_at = time.monotonic()
            time.sleep(0.002)
        t.join()
        assert bytes(got[sid]) == data
        assert zero_at is not None and zero_at - t0 <= 2 * TICK, zero_at
        assert core.stall_recoveries() == 0 and core.last_stall() is None
    finally:
        _close(core, pairs)


@pytest.mark.parametrize("readers,seed", [(1, 0), (1, 1), (2, 0), (2, 1)])
def test_no_false_recoveries_under_real_starvation(readers, seed):
    """The starved-streams rounds (48 streams over a one-buffer byte budget;
    tests/test_reader_hub.py) with a 2 s guard: streams go off and on all the
    time, for want of budget — every byte arrives, none is "recovered", and
    the largest age seen stays below the guard."""
    guard = 2.0
    rng = random.Random(seed)
    n = 48
    core = load().ReaderHub(64 << 10, 64, 64 << 10)
    core.set_readers(readers)
    core.set_stall_guard(guard)
    pairs = [socket.socketpair() for _ in range(n)]
    for a, _b in pairs:
        a.setblocking(True)
    sids = [core.add(os.dup(b.fileno())) for _a, b in pairs]
    idx = {sid: i for i, sid in enumerate(sids)}
    got = [0] * n
    oldest = 0.0
    try:
        for r in range(10):
            sizes = [rng.choice((0, 300, 300, 300, 300, 300, 150_000)) for _ in range(n)]
            want = [g + s for g, s in zip(got, sizes)]
            ths = [threading.Thread(target=a.sendall, args=(b"y" * s,)) for (a, _b), s in zip(pairs, sizes) if s]
            for t in ths:
                t.start()
            last = time.monotonic()
            while got != want:
                items = core.take()
                for sid, buf, view, _ns, _err in items:
                    if view is not None:
                        got[idx[sid]] += len(view)
                        view.release()
                        core.release(buf)
                oldest = max(oldest, core.oldest_unread())
                if items:
                    last = time.monotonic()
                else:
                    stalled = [(i, want[i] - got[i], core.stream_state(sids[i])) for i in range(n) if got[i] != want[i]]
                    assert time.monotonic() - last < 3.0, f"round {r}: stalled {stalled[:4]}"
                time.sleep(0.0003)
            for t in ths:
                t.join()
        print(f"readers={readers} seed={seed}: largest oldest_unread {oldest:.4f}s")
        assert core.stall_recoveries() == 0 and core.last_stall() is None
        assert oldest < guard
    finally:
        _close(core, pairs)


def test_drained_or_paused_stream_does_not_count():
    """A paused stream with bytes waiting (the pause is the caller's wish, its
    clock is stopped) and an unpolled stream whose socket is empty (nothing
    waits) leave the age at 0, tick after tick, and are never "recovered"."""
    core = load().ReaderHub(64 << 10, 8)
    core.set_stall_guard(GUARD)
    pairs = [socket.socketpair() for _ in range(2)]
    try:
        paused, empty = [core.add(os.dup(b.fileno())) for _a, b in pairs]
        core.pause(paused, True)
        pairs[0][0].sendall(b"p" * 1000)
        assert core.strand(empty)
        got = {paused: bytearray(), empty: bytearray()}
        t0 = time.monotonic()
        while time.monotonic() - t0 < max(3 * TICK, 1.5 * GUARD):
            assert _take(core, got) == 0
            assert core.oldest_unread() == 0
            time.sleep(0.005)
        assert core.stall_recoveries() == 0
        core.pause(paused, False)
        t0 = time.monotonic()
        while len(got[paused]) < 1000 and time.monotonic() - t0 < 2.0:
            _take(core, got)
            time.sleep(0.002)
        assert bytes(got[paused]) == b"p" * 1000 and core.stall_recoveries() == 0
    finally:
        _close(core, pairs)


class _Http:
    """What NativeRuntime.start_reader_hub needs of the HTTP client."""
    ssl_context = None
    reader_hub = None


async def _get(port: int, path: str):
    reader, writer = await asyncio.open_connection("127.0.0.1", port)
    writer.write(f"GET {path} HTTP/1.1\r\nHost: x\r\n\r\n".encode())
    await writer.drain()
    raw = await reader.read()
    writer.close()
    head, _, body = raw.partition(b"\r\n\r\n")
    return int(head.split()[1]), body.decode()


def test_readyz_fails_while_bytes_wait_past_twice_the_guard():
    """/readyz: 200 ``ready`` with no check registered, as ever. With the
    runtime's hub (guard 0.1 s) at its read-ahead limit and bytes in the
    socket for more than 0.2 s it answers 503 and names the watch reader; with
    the buffers handed back, 200 again. /metrics carries both gauges; closing
    the runtime takes the check away."""
    from k8s_watcher_amd.engine.runtime import NativeRuntime
    from k8s_watcher_amd.metrics import Metrics, start_metrics_server
    from k8s_watcher_amd.utils.config import WatcherSettings

    async def body():
        metrics = Metrics()
        metrics.ready = True
        server = await start_metrics_server(metrics, "127.0.0.1", 0)
        port = server.sockets[0].getsockname()[1]
        pairs = [socket.socketpair()]
        rt = NativeRuntime(WatcherSettings(watch_reader_stall_seconds=0.1, watch_read_bytes=64 << 10),
                           metrics, logging.getLogger("test"))
        try:
            assert await _get(port, "/readyz") == (200, "ready\n")
            metrics.ready = False
            assert await _get(port, "/readyz") == (503, "not ready\n")
            metrics.ready = True
            rt.start_reader_hub(_Http(), multi=False, framing="off", readers=1, multi_read_ahead=0)
            hub = rt.reader_hub
            assert len(metrics.ready_checks) == 1
            asyncio.get_running_loop().remove_reader(hub._fd)  # this test is the consumer, not the loop
            core = hub.core
            sid = core.add(os.dup(pairs[0][1].fileno()))
            data = os.urandom(100_000)  # buffers of 16 KiB here: two are read, the rest waits
            t, held = _hold_two_buffers(core, pairs[0][0], sid, data)
            await asyncio.sleep(0.35)
            status, text = await _get(port, "/readyz")
            assert status == 503 and text.startswith("not ready: watch reader") and text.endswith("\n"), text
            _status, prom = await _get(port, "/metrics")
            assert "k8s_watcher_watch_reader_oldest_unread_seconds 0." in prom
            assert "k8s_watcher_watch_reader_stall_recoveries 0.0" in prom
            got = {sid: bytearray(b"".join(x for _b, x in held))}
            for buf, _x in held:
                core.release(buf)
            t0 = time.monotonic()
            while len(got[sid]) < len(data) and time.monotonic() - t0 < 2.0:
                _take(core, got)
                await asyncio.sleep(0.002)
            t.join()
            assert bytes(got[sid]) == data
            await asyncio.sleep(0.1)  # the guard's tick is 25 ms
            assert await _get(port, "/readyz") == (200, "ready\n")
            assert hub.oldest_unread() == 0
        finally:
            rt.close()
            server.close()
            await server.wait_closed()
            for a, b in pairs:
                a.close()
                b.close()
        assert metrics.ready_checks == [] and hub.oldest_unread() == 0.0  # closed
        return True

    assert run(body(), timeout=30)


def test_recovery_is_logged_once_by_the_hub(caplog):
    """WatchReaderHub(stall_seconds=...): a recovery is one WARNING naming the
    stream, from the hub's own timer; close() cancels the timer."""
    from k8s_watcher_amd.net.reader import WatchReaderHub

    async def body():
        hub = WatchReaderHub(64 << 10, 8, stall_seconds=GUARD)
        hub.STALL_CHECK_S = 0.05
        hub._stall_timer.cancel()
        hub._stall_timer = hub.loop.call_later(hub.STALL_CHECK_S, hub._check_stalls)
        a, b = socket.socketpair()
        try:
            sid = hub.core.add(os.dup(b.fileno()))
            hub.core.strand(sid)
            a.sendall(b"x" * 100)
            t0 = time.monotonic()
            while hub._stalls_seen == 0 and time.monotonic() - t0 < 3.0:
                await asyncio.sleep(0.02)
            await asyncio.sleep(0.15)  # further checks log nothing more
        finally:
            hub.close()
            a.close()
            b.close()
        assert hub._stall_timer is None and hub.oldest_unread() == 0.0
        return sid

    with caplog.at_level(logging.WARNING, logger="k8s_watcher_amd.reader"):
        sid = run(body(), timeout=30)
    lines = [r.getMessage() for r in caplog.records if r.name == "k8s_watcher_amd.reader"]
    assert len(lines) == 1 and f"stream {sid}" in lines[0] and "re-armed 1 stalled" in lines[0], lines


def test_config_key_reaches_the_hub(monkeypatch, capsys):
    """watcher.watch_reader_stall_seconds: 30 by default, 0 (off) and floats
    accepted, negative rejected; ``--set`` carries it to the hub."""
    from k8s_watcher_amd import cli
    from k8s_watcher_amd.engine.runtime import NativeRuntime
    from k8s_watcher_amd.metrics import Metrics
    from k8s_watcher_amd.utils.config import ConfigError, load_settings

    def stall(value=None):
        ov = {} if value is None else {"watcher": {"watch_reader_stall_seconds": value}}
        return load_settings("staging", overrides=ov, environ={}).watcher.watch_reader_stall_seconds

    assert stall() == 30.0 and stall(0) == 0.0 and stall(2.5) == 2.5
    for env in ("development", "production"):
        assert load_settings(env, environ={}).watcher.watch_reader_stall_seconds == 30.0
    with pytest.raises(ConfigError):
        stall(-1)
    with pytest.raises(ConfigError):
        stall("soon")

    seen = []

    async def spy(settings, check_only):
        metrics = Metrics()
        rt = NativeRuntime(settings.watcher, metrics, logging.getLogger("test"))
        rt.start_reader_hub(_Http(), multi=False, framing="off", readers=1, multi_read_ahead=0)
        seen.append((settings.watcher.watch_reader_stall_seconds, rt.reader_hub.stall_seconds,
                     rt.reader_hub.core.stats()["stall_guard_ns"], len(metrics.ready_checks),
                     sorted(k for k in metrics.gauges if "unread" in k or "stall" in k)))
        rt.close()
        return 0

    monkeypatch.setattr(cli, "_run_service", spy)
    monkeypatch.setattr(cli, "setup_logging", lambda *a, **k: logging.getLogger("test"))
    assert cli.main(["staging", "--set", "watcher.watch_reader_stall_seconds=0"]) == 0
    assert cli.main(["staging", "--set", "watcher.watch_reader_stall_seconds=1.5"]) == 0
    assert cli.main(["staging"]) == 0
    capsys.readouterr()
    names = ["watch_reader_oldest_unread_seconds", "watch_reader_stall_recoveries"]
    assert seen == [(0.0, 0.0, 0, 0, names), (1.5, 1.5, 1_500_000_000, 1, names),
                    (30.0, 30.0, 30_000_000_000, 1, names)]
