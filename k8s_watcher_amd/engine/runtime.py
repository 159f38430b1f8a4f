"""The native engine's threads and the C heap: what ``WatcherService`` builds,
places on CPUs and tears down around the event path, in the order it asks.

One :class:`NativeRuntime` per service (a leader's every term builds a new
one). It owns the shared decode pool, the watch reader hub and the thread
placement, and the glibc tuning with its periodic trim. The fixed choices
(reader count, framing, read-ahead, trim threshold) are module constants of
the service: it passes them in, nothing here is tunable.
"""

from __future__ import annotations

import asyncio
import logging
import os
import time

from ..metrics import Metrics
from ..utils.config import WatcherSettings


class NativeRuntime:
    def __init__(self, watcher: WatcherSettings, metrics: Metrics, log: logging.Logger) -> None:
        self.watcher = watcher
        self.metrics = metrics
        self.log = log
        self.decode_pool = None  # 0 once started with no workers, else the pool
        self.reader_hub = None
        self.thread_placement = None
        self._http = None  # the HTTP client the hub is attached to
        self._ready_check = None  # the hub's entry in metrics.ready_checks
        self._loop_affinity = None

    # ------------------------------------------------------------------ C heap
    def tune_heap(self) -> None:
        """With the periodic trim on, before any thread or buffer exists."""
        if self.watcher.malloc_trim_seconds > 0:
            # fixed glibc thresholds before the cache and the buffers exist:
            # blocks >= 512 KiB on their own mappings (unmapped when freed),
            # so multi-MiB transients leave no holes in the arenas (round-5
            # soak: RSS grew with retained free bytes; kwcore.cpp malloc_tune)
            from ..ops.native import load
            load().malloc_tune(512 << 10, 4 << 20)

    def add_heap_gauges(self) -> None:
        """Memory accounting: the C heap (glibc), in use vs retained free."""
        from ..ops.native import load
        _mi = load().malloc_info
        self.metrics.gauges["malloc_in_use_bytes"] = lambda: float(_mi()["in_use_bytes"])
        self.metrics.gauges["malloc_free_bytes"] = lambda: float(_mi()["free_bytes"])
        self.metrics.gauges["malloc_arenas"] = lambda: float(len(load().malloc_arenas()))

    def heap_trimmer(self, min_free: int):
        """The trim loop to run as a task, or None with ``watcher.malloc_trim_seconds: 0``."""
        period = self.watcher.malloc_trim_seconds
        return malloc_trim_loop(self.metrics, self.log, period, min_free) if period > 0 else None

    # ------------------------------------------------------------------ threads
    def start_decode(self):
        """The partitioned apply path with its gauges, then one decode pool for
        every watch scope (they share the loop thread). Returns the pool, 0
        with no workers."""
        from ..ops.native import load
        from ..utils.cpus import auto_decode_spin_us, auto_decode_threads, pin_to_l3_domain
        _kw = load()
        _kw.set_partitioned_apply(True)
        # which apply path ran, and how much of it (cumulative, process-wide)
        for _key in ("partitioned_batches", "partitioned_lines", "tail_serial_lines", "tail_submits",
                     "tail_lock_runs", "serial_batches", "serial_lines", "payload_built", "payload_prefiltered"):
            self.metrics.gauges["apply_" + _key] = (lambda k=_key: float(_kw.apply_stats()[k]))
        w = self.watcher
        n = w.decode_threads if w.decode_threads >= 0 else auto_decode_threads()
        if n > 0:
            # Workers started below inherit the mask. Measured on a chiplet
            # host (BENCHMARKS.md): 3 workers spread over CCDs were slower than
            # none; the same 3 inside the loop thread's L3 ran ~1.6x faster.
            # A process already inside one L3 domain (a launcher placed it)
            # stays where it is.
            dom = pin_to_l3_domain(min_cpus=n + 1, only_if_split=True)
            if dom:
                self.log.info(f"Decode pool pinned to L3 domain CPUs {sorted(dom)}")
        spin = auto_decode_spin_us()
        self.decode_pool = _kw.DecodePool(n, spin) if n > 0 else 0
        return self.decode_pool

    def start_reader_hub(self, http, multi: bool, framing: str, readers: int, multi_read_ahead: int) -> None:
        """``watcher.watch_reader: native``: watch bodies read (and, for https,
        decrypted) on a native thread (net/reader.py), attached to ``http``.
        ``multi``: several watch scopes. No hub for https without the native
        TLS context."""
        w = self.watcher
        if w.watch_reader != "native" or not (http.ssl_context is None
                                              or getattr(http.ssl_context, "kw_tls", None) is not None):
            return
        from ..net.reader import WatchReaderHub
        from ..utils.cpus import auto_reader_threads, auto_tls_threads
        hub = WatchReaderHub(w.watch_read_bytes or (4 << 20), w.watch_reader_buffers,
                             max_bytes=w.watch_reader_max_bytes or (multi_read_ahead if multi else 0),
                             frame=framing == "on" or (framing == "auto" and multi),
                             readers=readers or auto_reader_threads(multi),
                             tls_records=w.watch_tls_records == "native",
                             tls_threads=w.watch_tls_threads if w.watch_tls_threads >= 0 else auto_tls_threads(),
                             stall_seconds=w.watch_reader_stall_seconds)
        self.reader_hub = hub
        self._http = http
        http.reader_hub = hub
        g = self.metrics.gauges
        g["watch_reader_streams"] = lambda: float(len(hub.protos))
        g["watch_reader_reads"] = lambda: float(hub.stats().get("reads", 0))
        g["watch_reader_wakeups"] = lambda: float(hub.stats().get("signals", 0))
        # reads whose chunk framing and line split ran on the reader thread (watcher.hub_framing)
        g["watch_reader_framed_reads"] = lambda: float(hub.stats().get("framed_reads", 0))
        # memory accounting: read buffers allocated (up to watch_reader_buffers x watch_read_bytes)
        g["watch_reader_allocated_bytes"] = lambda: float(hub.stats().get("allocated_bytes", 0))
        g["watch_reader_held_bytes"] = lambda: float(hub.stats().get("held_bytes", 0))
        # https watches on the hub's own TLS 1.3 record layer (ops/csrc/tls13.inc):
        # ciphertext rings (inside watch_reader_allocated_bytes), streams taken
        # over / left on SSL_read, records opened and key updates followed
        for key, name in (("tls_ring_bytes", "watch_reader_tls_ring_bytes"),
                          ("tls_taken", "watch_tls_streams_native"), ("tls_kept", "watch_tls_streams_openssl"),
                          ("tls_records", "watch_tls_records"), ("tls_key_updates", "watch_tls_key_updates")):
            g[name] = lambda key=key: float(hub.stats().get(key, 0))
        # the stall guard (watcher.watch_reader_stall_seconds): how long bytes
        # have waited on a stream the hub is not polling (an upper bound: since
        # polling stopped), and streams it re-armed after that long
        g["watch_reader_oldest_unread_seconds"] = hub.oldest_unread
        g["watch_reader_stall_recoveries"] = lambda: float(hub.stats().get("stall_recoveries", 0))
        if w.watch_reader_stall_seconds > 0:
            self._ready_check = reader_stall_check(hub, w.watch_reader_stall_seconds)
            self.metrics.ready_checks.append(self._ready_check)

    def pin_threads(self) -> None:
        """``watcher.thread_pinning: auto``: keep one physical core of the L3
        domain free for the event-loop thread (which applies every event in
        stream order, the rate's bound): the decode workers and the reader
        thread are pinned to the rest. The loop thread itself stays free to
        move — pinned hard, it could not escape another process scheduled on
        its core, and the latency tail grew to ~10 ms (profiles/latency_curve_*)."""
        mode = self.watcher.thread_pinning
        if mode == "none":
            return
        from ..utils.cpus import loop_core_split, reader_core_split
        try:
            split = loop_core_split(os.sched_getaffinity(0))
        except (AttributeError, OSError):
            return
        if split is None:
            return
        loop_cpus, rest = split
        tids = list(self.decode_pool.thread_ids()) if self.decode_pool else []
        # the hub's TLS pool threads (https watches) were made with the loop
        # thread's whole domain: left there, three of them ran on the loop's
        # core and it waited 5.8 ms/s for a CPU (profiles/r6/tls_timeline)
        if self.reader_hub is not None:
            tids += list(self.reader_hub.core.tls_thread_ids())
            # reader threads past the first run beside the workers (the first
            # gets a core of its own below)
            tids += list(self.reader_hub.core.thread_ids())[1:]
        reader_cpus = None
        reader_tid = self.reader_hub.core.thread_id() if self.reader_hub is not None else 0
        if reader_tid and mode == "auto":
            # the reader thread gets a core of its own too: it copies the watch
            # bodies out of the kernel and bounds the single-stream rate
            rsplit = reader_core_split(rest)
            if rsplit is not None:
                reader_cpus, rest = rsplit
        if reader_tid and reader_cpus is None:
            tids.append(reader_tid)
        try:
            if reader_cpus is not None:
                os.sched_setaffinity(reader_tid, reader_cpus)
            for tid in tids:
                if tid:
                    os.sched_setaffinity(tid, rest)
            # the loop thread moves to the free core now (its caches follow
            # it) but keeps the whole domain to run on
            self._loop_affinity = os.sched_getaffinity(0)
            os.sched_setaffinity(0, loop_cpus)
            os.sched_setaffinity(0, self._loop_affinity)
        except OSError as exc:
            self.log.warning(f"Thread pinning skipped: {exc}")
            return
        self.thread_placement = {"loop": sorted(loop_cpus), "workers": sorted(rest),
                                 **({"reader": sorted(reader_cpus)} if reader_cpus is not None else {})}
        self.log.info(f"CPUs {sorted(loop_cpus)} kept for the event-loop thread; {len(tids)} worker threads on the rest")

    def close(self) -> None:
        """Detach and close the hub, end the pool's threads, give the loop
        thread its affinity back."""
        if self._ready_check is not None:
            if self._ready_check in self.metrics.ready_checks:
                self.metrics.ready_checks.remove(self._ready_check)
            self._ready_check = None
        if self.reader_hub is not None:
            self._http.reader_hub = None
            self._http = None
            self.reader_hub.close()
            self.reader_hub = None
        if self.decode_pool:
            # its threads end now, not when the garbage collector frees this
            # service (a leader's every term builds a new one; the shared
            # Metrics gauges keep the old one reachable until the next term)
            self.decode_pool.close()
        if self._loop_affinity is not None:
            try:
                os.sched_setaffinity(0, self._loop_affinity)
            except OSError:
                pass
            self._loop_affinity = None


def reader_stall_check(hub, stall_seconds: float):
    """The ``/readyz`` check of the reader hub's stall guard: bytes have been
    waiting on a stream the hub does not poll for more than twice
    ``watcher.watch_reader_stall_seconds`` — the guard's re-arm has had its
    turn and did not help (the pool, the byte budget or the stream's
    read-ahead is used up and the loop is not handing buffers back)."""
    limit = 2.0 * stall_seconds

    def check():
        age = hub.oldest_unread()
        if age > limit:
            return (f"watch reader: bytes unread for up to {age:.1f}s on a stream it is not polling "
                    f"(watcher.watch_reader_stall_seconds: {stall_seconds:g})")
        return None

    return check


async def malloc_trim_loop(metrics: Metrics, log: logging.Logger, period: float, min_free: int) -> None:
    """The decode workers, the reader hub and the notifier allocate on
    several threads; glibc keeps what each thread's arena freed. Handing
    the free pages back now and then keeps the RSS at what is in use
    (soak: RSS grew ~1-2 MiB/hour with no growth in use).

    A trim locks each arena while it walks it, and a thread allocating
    from that arena waits: it runs only when the heap retains at least
    ``min_free`` free (the service's ``MALLOC_TRIM_MIN_FREE``), and
    every trim is timed (``malloc_trim_last_ms`` / ``malloc_trim_max_ms`` gauges,
    ``malloc_trim_us`` counter) so a latency outlier can be checked
    against it. It waits for half a second
    without events (up to nine periods; then it trims anyway), so a trim
    does not stall notifications in flight."""
    from ..ops.native import load
    kw = load()
    trim, info = kw.malloc_trim, kw.malloc_info
    loop = asyncio.get_running_loop()
    c, g = metrics.c, metrics.gauges
    last = {"last_ms": 0.0, "max_ms": 0.0}
    g["malloc_trim_last_ms"] = lambda: last["last_ms"]
    g["malloc_trim_max_ms"] = lambda: last["max_ms"]

    def timed_trim() -> float:
        t = time.perf_counter()
        trim()
        return time.perf_counter() - t

    async def quiet_moment() -> bool:
        # a trim makes every allocating thread wait on its arena while it
        # walks it (7.5-15 ms on the MI355X host with the heap the
        # saturated bench leaves): a notification in flight then waits
        # too. Wait, up to one period, for half a second with no event.
        deadline = time.monotonic() + period
        while time.monotonic() < deadline:
            n0 = c["events_received"]
            await asyncio.sleep(0.5)
            if c["events_received"] == n0:
                return True
        return False

    deferred = 0
    while True:
        await asyncio.sleep(period)
        if min_free > 0 and info()["free_bytes"] < min_free:
            c["malloc_trims_skipped"] += 1
            continue
        # a watcher that is never quiet still trims, every tenth period
        if deferred < 9 and not await quiet_moment():
            deferred += 1
            c["malloc_trims_deferred"] += 1
            continue
        deferred = 0
        try:
            secs = await loop.run_in_executor(None, timed_trim)
        except RuntimeError as exc:  # the executor is going away (shutdown)
            log.debug(f"malloc_trim skipped: {exc}")
            continue
        last["last_ms"] = secs * 1e3
        last["max_ms"] = max(last["max_ms"], secs * 1e3)
        c["malloc_trims"] += 1
        c["malloc_trim_us"] += int(secs * 1e6)
