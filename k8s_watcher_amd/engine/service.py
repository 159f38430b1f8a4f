"""Watcher service orchestrator (SURVEY C6 + C7, layer L4).

Reference: ``PodWatcher.setup_k8s_client`` + ``start_watching``
(``/root/reference/watcher/pod_watcher.py:110-157,243-277``). The same log
messages (§2.4) are emitted in the same order; the behavioural fixes are:

* the connectivity probe is ``GET /version`` (``CoreV1Api.get_api_version``
  at ``:140`` does not exist and makes the reference fail setup);
* the namespace sample is bounded (``limit=5``) instead of listing them all;
* setup failure is an error the CLI turns into exit status 1 (the reference
  returns and exits 0, ``:245-247``);
* the clusterapi notifier is enabled and health-checked (``:14,236,250-253``
  are commented out in the reference);
* SIGTERM and SIGINT both stop the watch, drain the notifier and write a
  final checkpoint.

With ``watcher.namespace_scope: server`` one reflector per target namespace
watches ``/api/v1/namespaces/<ns>/pods``, so the API server only sends the
pods the watcher cares about (the reference always watches the whole cluster
and filters client-side). With ``namespace_scope: discover`` the
namespace set itself is watched (``engine/namespaces.py``) and one reflector
runs per namespace this shard owns — the sharded form of the reference's
all-namespaces watch: reflectors start and stop as namespaces come and go.

The service owns the order of start-up and shutdown, and builds what a watch
scope runs on: the API client, the notifier, the decoders and pipelines
(``_make_reflector``). The native threads (``runtime.py``), the watch scopes
(``scopes.py`` ``ScopeSet``: which exist, how they start, stop and drain, and
what a change of the namespace set does), the namespace hand-over
(``handover.py``) and the checkpoint's cut and write (``checkpoint.py``
``Checkpointer``) are classes of their own, which it hands what they need.
"""

from __future__ import annotations

import asyncio
import gc
import logging
import os
import time
from typing import List, Optional, Set

from ..kube.api import ApiError, KubeApi
from ..kube.kubeconfig import ConfigException, KubeEndpoint, load_incluster_config, load_kube_config
from ..metrics import Metrics, start_metrics_server
from ..net.http import HttpError
from ..ops.cache import make_pod_cache
from ..ops.decode import make_decoder
from ..parallel.native_notifier import NativeNotifierPool
from ..parallel.notifier import NotifierPool, NullNotifier
from ..parallel.spool import Spool, SpoolReplayer
from ..utils.config import Settings
from ..utils.fastlog import EventLog
from ..utils.logsetup import SERVICE_LOGGER
from .checkpoint import Checkpointer, load_checkpoint
from .handover import NamespaceHandover
from .namespaces import NamespaceWatcher
from .pipeline import EventPipeline
from .reflector import Reflector, WatchFailed
from .runtime import NativeRuntime
from .scopes import ScopeSet, SetupError, first_exception


# Fixed choices that were settings until round 6 (each one's A/B is in
# BENCHMARKS.md; tests monkeypatch these module attributes, read when start()
# runs: what engine/runtime.py needs of them it is handed as arguments):
# the descriptor table grown once at start to hold this many fds (a watch per
# namespace opens two each; growing it later, with threads running, waits an
# RCU grace period per doubling: utils/fds.py)
FD_TABLE_RESERVE = 16384
# once every scope has synced, collect and freeze what start-up left
# (gc.freeze): later full collections walk only objects made since, not the
# service's long-lived ones (a 1,000-scope relist storm's gen-2 pauses);
# unfrozen at shutdown. Start-up objects that later become cyclic garbage stay
# until shutdown. Skipped when something is already frozen (an embedding
# application's own freeze)
GC_FREEZE = True
# the reader hub's thread de-chunks and splits watch bodies (readerhub.inc
# HubFramer): auto = with several watch scopes (namespace watches: the reader
# has time, the loop has per-stream work), not for the one cluster-wide
# watch, whose reader thread is the bound (profiles/r5/framing_ab,
# r5/framing_many); on | off for tests
HUB_FRAMING = "auto"
# reader-hub threads (net/reader.py; readerhub.inc set_readers): 0 = auto
# (utils/cpus.py auto_reader_threads: two for several watch scopes on a CPU
# share of 12+, else one)
HUB_READERS = 0
# read-ahead over all streams when there are several watch scopes and
# watcher.watch_reader_max_bytes is 0: with the whole pool (256 MiB) the
# namespace watches' buffers waited 13-28 ms for the loop and were out of the
# L3 by then, and the pool ran short (starved streams); 8 MiB keeps them young.
# 64 namespaces, interleaved on the box: 2.45-2.54M (one reader, the pool),
# 2.59-2.94M (one reader, 8 MiB), 3.05-3.13M (two readers, 8 MiB)
# (profiles/r6/readers/final). One cluster-wide watch keeps the pool: its two
# buffers of 4 MiB are its read-ahead anyway.
HUB_MULTI_READ_AHEAD = 8 << 20
MALLOC_TRIM_MIN_FREE = 16 << 20  # the periodic heap trim runs only when the C heap keeps this much free
SPOOL_REPLAY_BATCH = 1000  # owed notifications re-submitted from the spool per replay pass
# shutdown's parting step (engine/handover.py part) gives up the records it has
# not begun after this long: with shutdown's default drain (10 s) and the final
# checkpoint (tenths of a second per 100k pods) it stays inside the sharded
# StatefulSet's terminationGracePeriodSeconds of 30
PARTING_BUDGET_SECONDS = 10.0


def required_permissions(s: Settings) -> List[tuple]:
    """``(verb, resource, api group, namespace or None, name or None)`` this
    configuration needs — what ``--check`` asks the API server about and what
    ``deploy/k8s/rbac.yaml`` must grant (``tests/test_deploy.py`` holds them equal).

    The reference needs list/watch on pods cluster-wide and list on namespaces
    (``pod_watcher.py:146,264``); server-side scopes need them per namespace,
    namespace discovery also watches namespaces, leader election its Lease."""
    w = s.watcher
    wanted = []
    scopes = w.namespaces if w.namespace_scope == "server" and w.namespaces else [None]
    for ns in scopes:
        wanted += [("list", "pods", "", ns, None), ("watch", "pods", "", ns, None)]
    wanted.append(("list", "namespaces", "", None, None))
    if w.namespace_scope == "discover":
        wanted.append(("watch", "namespaces", "", None, None))
    le = w.leader_election
    if le.enabled:
        from .leader import default_lease_namespace, shard_lease
        lease = shard_lease(s)
        ns = lease.lease_namespace or default_lease_namespace()
        wanted += [("get", "leases", "coordination.k8s.io", ns, lease.lease_name),
                   ("update", "leases", "coordination.k8s.io", ns, lease.lease_name),
                   ("create", "leases", "coordination.k8s.io", ns, None)]
    return wanted


class WatcherService:
    def __init__(self, settings: Settings, endpoint: Optional[KubeEndpoint] = None,
                 metrics: Optional[Metrics] = None, notifier_factory=None, serve_metrics: bool = True) -> None:
        self.settings = settings
        self.serve_metrics = serve_metrics  # False when an outer runner owns the metrics server
        self.endpoint = endpoint
        self.metrics = metrics or Metrics()
        self.notifier_factory = notifier_factory
        self.log = logging.getLogger(SERVICE_LOGGER)
        self.api: Optional[KubeApi] = None
        self.notifier = None
        self.pipeline: Optional[EventPipeline] = None
        self._gc_frozen = False
        # the native engine's threads and the C heap
        self.runtime = NativeRuntime(settings.watcher, self.metrics, self.log)
        self.decoder = None
        self._stop = asyncio.Event()
        self._tasks: List[asyncio.Task] = []
        self._metrics_server = None
        self.started = asyncio.Event()
        self.server_version: Optional[str] = None
        self.spool = None
        self.spool_replayer = None
        # which watch scopes exist and what state each is in
        self.scopes = ScopeSet(
            settings.watcher, self.metrics, self.log, self._stop, cache=self._cache, handover=lambda: self.handover,
            make_reflector=self._make_reflector,
            make_namespace_watcher=lambda on_change: NamespaceWatcher(self.api, settings, self.metrics, on_change))
        # namespaces moving between this shard and another (watcher.shard.handover_dir)
        self.handover = NamespaceHandover(
            settings.watcher.shard, self.metrics, self.log, self._stop,
            cache=self._cache, notifier=lambda: self.notifier, resubmit_owed=self._resubmit_owed,
            start_scope=self.scopes.start, forget_namespaces=self.scopes.forget)
        # when the checkpoint is cut and written, periodically and at shutdown
        self.checkpointer = Checkpointer(
            settings.watcher.checkpoint, self._native_pipeline(), settings.clusterapi.enabled, self.metrics, self.log,
            cache=self._cache, notifier=lambda: self.notifier, reflectors=lambda: self.reflectors)

    # what the benchmark and the tests read of the scopes and the runtime
    @property
    def reflectors(self) -> List[Reflector]:
        return self.scopes.reflectors()

    @property
    def _decode_pool(self):
        return self.runtime.decode_pool

    @property
    def _reader_hub(self):
        return self.runtime.reader_hub

    @property
    def thread_placement(self):
        return self.runtime.thread_placement

    # ------------------------------------------------------------------ setup
    def load_endpoint(self) -> KubeEndpoint:
        k = self.settings.kubernetes
        if self.endpoint is not None:
            return self.endpoint
        if k.use_incluster_config:
            self.log.info("Using in-cluster configuration")
            return load_incluster_config()
        if k.config_file:
            self.log.info(f"Loading kubeconfig from: {k.config_file}")
            if not os.path.exists(k.config_file):
                self.log.error(f"Kubeconfig file not found: {k.config_file}")
                raise SetupError(f"kubeconfig not found: {k.config_file}")
            return load_kube_config(config_file=k.config_file, context=k.context)
        self.log.info("Using default kubeconfig")
        return load_kube_config(context=k.context)

    async def setup_k8s_client(self) -> bool:
        """Reference-compatible setup: returns False (after logging) on failure."""
        try:
            ep = self.load_endpoint()
            self.endpoint = ep
            self.api = KubeApi(ep, timeout=self.settings.kubernetes.request_timeout,
                               compression=self.settings.kubernetes.compression,
                               keepalive=self.settings.kubernetes.tcp_keepalive_seconds)
            ver = await self.api.get_version()
            self.server_version = ver.get("gitVersion") or f"{ver.get('major')}.{ver.get('minor')}"
            self.log.info(f"Successfully connected to Kubernetes API version: {self.server_version}")
            try:
                nss = await self.api.list_namespaces(limit=5)
                names = [(i.get("metadata") or {}).get("name") for i in (nss.get("items") or [])[:5]]
                self.log.info(f"Sample namespaces: {names}")
            except ApiError as exc:
                # RBAC may not grant namespace list; the watch itself only needs pods.
                self.log.warning(f"Could not list namespaces: {exc}")
            return True
        except ConfigException as exc:
            self.log.error(f"Kubernetes config error: {exc}")
        except SetupError:
            pass
        except (ApiError, HttpError, OSError, ValueError) as exc:
            self.log.error(f"Error setting up k8s client: {exc}")
        if self.api is not None:
            await self.api.close()
            self.api = None
        return False

    async def preflight(self) -> bool:
        """``--check``: the RBAC permissions this configuration needs (SelfSubjectAccessReview)
        and the clusterapi health endpoint. Logs one line per item; True if all pass."""
        assert self.api is not None
        s = self.settings
        wanted = required_permissions(s)
        ok = True
        for verb, res, group, ns, name in wanted:
            what = f"{verb} {group + '/' if group else ''}{res}" + (f" in {ns}" if ns else " (cluster-wide)")
            try:
                allowed, reason = await self.api.can_i(verb, res, group, ns, name)
            except (ApiError, HttpError) as exc:
                self.log.warning(f"Permission check for {what} unavailable: {exc}")
                continue
            if allowed:
                self.log.info(f"Permission OK: {what}")
            else:
                ok = False
                self.log.error(f"Permission missing: {what}" + (f" ({reason})" if reason else ""))
        if s.clusterapi.enabled:
            self.event_log = EventLog(self.log)
            notifier = self._make_notifier()
            try:
                if await notifier.health_check():
                    self.log.info(f"ClusterAPI health check passed: {s.clusterapi.base_url}{s.clusterapi.health}")
                else:
                    ok = False
                    self.log.error(f"ClusterAPI health check failed: {s.clusterapi.base_url}{s.clusterapi.health}")
            finally:
                await notifier.close()
        return ok

    def _make_notifier(self):
        c = self.settings.clusterapi
        w = self.settings.watcher
        if self.notifier_factory is not None:
            return self.notifier_factory(self)
        if not c.enabled:
            return NullNotifier(self.metrics)
        log_events = w.log_events if w.log_events is not None else self.log.isEnabledFor(logging.INFO)
        if w.engine == "native" and c.pool.native:
            # per-request work in C++ (ops/csrc/engine.inc), TLS included
            return NativeNotifierPool(c, self.metrics, ts_mode=w.event_timestamp, log_events=log_events,
                                      on_saturation=self.scopes.set_saturated, event_log=self.event_log)
        return NotifierPool(c, self.metrics, ts_mode=w.event_timestamp, log_events=log_events,
                            on_saturation=self.scopes.set_saturated, native=w.engine == "native",
                            event_log=self.event_log)

    # ------------------------------------------------------------------ run
    async def start(self) -> None:
        """Setup + start background tasks; returns once every scope has synced."""
        self._prepare_process()
        await self._connect()
        scopes = await self._resolve_scopes()
        cache, gains = self._restore_state(scopes)
        self._add_gauges(cache)
        await self._launch(scopes, gains)
        await self._wait_synced()
        if self._gc_frozen and not self._stop.is_set():
            # the scopes' long-lived objects join the frozen set; only the young
            # generations are collected first (a full pass over a 1,000-scope
            # start's objects would hold the loop ~30 ms; cyclic garbage already
            # in the old generation stays frozen until shutdown unfreezes it)
            gc.collect(1)
            gc.freeze()
        self.metrics.ready = True
        self.started.set()

    def _prepare_process(self) -> None:
        """What has to happen before any thread or buffer exists."""
        # before the decode pool, reader and I/O threads exist: growing a
        # shared descriptor table later stalls the opening thread ~150 ms
        # per doubling on a 256-CPU host (utils/fds.py)
        from ..utils.fds import reserve_fd_table
        reserve_fd_table(FD_TABLE_RESERVE)
        if self._native_pipeline():
            self.runtime.tune_heap()
        if GC_FREEZE and gc.get_freeze_count() == 0:
            # what import and configuration made is permanent: the full
            # collections that starting a thousand scopes triggers then walk
            # only the scopes' own objects (70-140 ms gen-2 pauses otherwise).
            # Only when nothing is frozen yet: an embedding application that
            # froze its own objects keeps control of the permanent generation
            # (shutdown's unfreeze would thaw its objects too)
            gc.freeze()
            self._gc_frozen = True

    async def _connect(self) -> None:
        """The API server, then the notifier with its health check and warm-up,
        then the spool and its replayer."""
        s = self.settings
        if not await self.setup_k8s_client():
            self.log.error("Failed to setup Kubernetes client")
            raise SetupError("Failed to setup Kubernetes client")
        assert self.api is not None
        self.event_log = EventLog(self.log)  # after logging is configured: picks the fast path
        self.notifier = self._make_notifier()
        if s.clusterapi.enabled and s.clusterapi.health_check_on_start:
            if await self.notifier.health_check():
                self.log.info("ClusterAPI health check passed")
            else:
                self.log.warning("ClusterAPI health check failed, but continuing...")
        if s.clusterapi.enabled and hasattr(self.notifier, "warm_up"):
            await self.notifier.warm_up()
        sp = s.clusterapi.spool
        if s.clusterapi.enabled and sp.path and hasattr(self.notifier, "attach_spool"):
            self.spool = Spool(sp.path, sp.max_bytes, sp.segment_bytes, sp.fsync, self.metrics)
            self.notifier.attach_spool(self.spool)
            self.metrics.gauges["spool_records"] = lambda: float(len(self.spool))
            self.metrics.gauges["spool_bytes"] = lambda: float(self.spool.bytes)
            if len(self.spool):
                self.log.warning(f"Spool {sp.path} holds {len(self.spool)} notifications from an earlier run")
            self.spool_replayer = SpoolReplayer(self.spool, self.notifier, self.metrics,
                                                sp.replay_interval_seconds, SPOOL_REPLAY_BATCH)
            self._tasks.append(asyncio.ensure_future(self.spool_replayer.run()))

    async def _resolve_scopes(self) -> List[Optional[str]]:
        """The shared decoder, then this shard's watch scopes (``ScopeSet.resolve``)."""
        self.decoder = self._make_decoder()
        return await self.scopes.resolve()

    def _restore_state(self, scopes: List[Optional[str]]):
        """The checkpoint's cache and resume points, the pipeline over them
        (with the native threads), then what is owed from before: hand-over
        across a new shard layout, the checkpoint's unacknowledged
        notifications, and the cached pods this shard no longer watches.
        Returns ``(cache, namespaces to gain from their old owners)``."""
        s = self.settings
        cache = make_pod_cache(self._native_pipeline())
        saved_rvs = {}
        owed: list = []
        ck = s.watcher.checkpoint.path
        if ck:
            loaded = load_checkpoint(ck, native_cache=self._native_pipeline())
            if loaded is not None:
                saved_rvs, cache, _, owed = loaded
                self.log.info(f"Resuming from checkpoint {ck}: {len(cache)} cached pods"
                              + (f", {len(owed)} owed notifications" if owed else ""))
        self.scopes.saved_rvs = saved_rvs
        self.pipeline = EventPipeline(s, self.decoder, self.notifier, self.metrics, cache, self.event_log,
                                      event_sharding=self._event_sharding())
        if self._native_pipeline():
            # the pool before the hub, both before their threads are placed
            self.pipeline.attach_native(self.runtime.start_decode())
            self.runtime.start_reader_hub(self.api.http, self.scopes.multi, framing=HUB_FRAMING, readers=HUB_READERS,
                                          multi_read_ahead=HUB_MULTI_READ_AHEAD)
            self.runtime.pin_threads()
        gains: Set[str] = set()
        if self._hands_over():
            # back after a graceful shutdown: what other shards took meanwhile
            # (the count had shrunk below this ordinal) is no longer this checkpoint's to say
            owed = self.handover.reclaim_on_start(saved_rvs, owed)
            gains, owed = self.handover.reshard_on_start(scopes, self.scopes.names(), saved_rvs, owed)
        if owed:
            # the checkpoint's cut: clusterapi never acknowledged these; send them
            # (in their original order) before anything newer — the watches that
            # resume after them, and the DELETEDs synthesized just below, which
            # must be the last word for their pods
            self._resubmit_owed(owed)
        if saved_rvs and None not in scopes:
            # namespaces deleted while the watcher was down, and those this shard no longer watches
            self.scopes.reconcile_cache(scopes, lambda ns: self.pipeline.delete_scope(ns, time.monotonic_ns()))
        return cache, gains

    def _add_gauges(self, cache) -> None:
        """The gauges over what now exists: the cache, the C heap, the notifier, the scopes."""
        self.metrics.gauges["cached_pods"] = lambda: float(len(cache))
        if hasattr(cache, "memory"):  # native cache: bytes held (cores + keys), for memory accounting
            self.metrics.gauges["cache_bytes"] = lambda: float(sum(v for k, v in cache.memory().items()
                                                                   if k.endswith("_bytes")))
        if self._native_pipeline():
            self.runtime.add_heap_gauges()
        self.metrics.gauges["notify_outstanding"] = lambda: float(self.notifier.outstanding())
        if hasattr(self.notifier, "outstanding_bytes"):
            self.metrics.gauges["notify_outstanding_bytes"] = lambda: float(self.notifier.outstanding_bytes())
        self.metrics.gauges["watch_scopes"] = lambda: float(len(self.scopes))
        if self.settings.watcher.terminating_overdue_seconds > 0:
            # terminating pods with a deletion deadline, reported overdue or not yet
            self.metrics.gauges["pods_terminating_tracked"] = lambda: float(cache.tracked())
        if self.settings.watcher.pending_overdue_seconds > 0:
            # pods still Pending with a creation time, reported overdue or not yet
            self.metrics.gauges["pods_pending_tracked"] = lambda: float(cache.pending_tracked())
        if self.settings.watcher.unready_overdue_seconds > 0:
            # pods Running with Ready=False and a transition time, reported overdue or not yet
            self.metrics.gauges["pods_unready_tracked"] = lambda: float(cache.unready_tracked())

    async def _launch(self, scopes: List[Optional[str]], gains: Set[str]) -> None:
        """Start every scope's watch (a gained namespace's once its record is
        in), then the service's own loops; from here the scopes follow the
        namespace watch."""
        s = self.settings
        self.log.info(f"Starting Pod watcher in {s.environment} environment...")
        if s.watcher.namespaces:
            self.log.info(f"Monitoring namespaces: {s.watcher.namespaces}")
        else:
            self.log.info("Monitoring all namespaces")
        await self.scopes.start_all(scopes, gains)
        if s.metrics.enabled and self.serve_metrics:
            self._metrics_server = await start_metrics_server(self.metrics, s.metrics.host, s.metrics.port,
                                                              debug=s.metrics.debug)
        if s.watcher.checkpoint.path:
            self._tasks.append(asyncio.ensure_future(self.checkpointer.loop()))
        trimmer = self.runtime.heap_trimmer(MALLOC_TRIM_MIN_FREE) if self._native_pipeline() else None
        if trimmer is not None:
            self._tasks.append(asyncio.ensure_future(trimmer))
        if (s.watcher.terminating_overdue_seconds > 0 or s.watcher.pending_overdue_seconds > 0
                or s.watcher.unready_overdue_seconds > 0):
            self._tasks.append(asyncio.ensure_future(self.scopes.overdue_loop(time.time)))
        self.scopes.go_live()

    # ------------------------------------------------------------------ what a watch scope runs on
    def _event_sharding(self) -> bool:
        """Per-event shard filtering: off when the watches themselves are the
        shard's namespaces (server-side scopes keyed by namespace)."""
        w = self.settings.watcher
        scoped = w.namespace_scope == "discover" or (w.namespace_scope == "server" and bool(w.namespaces))
        return not (scoped and w.shard.key == "namespace")

    def _hands_over(self) -> bool:
        """Namespaces move between shards through ``shard.handover_dir``."""
        sh = self.settings.watcher.shard
        return bool(sh.handover_dir) and self.scopes.multi and sh.key == "namespace"

    def _make_decoder(self):
        s = self.settings
        return make_decoder(s.watcher.engine, s.environment, s.watcher.state_format, s.watcher.payload_extra,
                            s.watcher.validate, s.watcher.container_failures, s.watcher.container_failure_reasons,
                            s.watcher.pod_conditions, s.watcher.pod_condition_rules, s.watcher.terminating,
                            s.watcher.terminating_overdue_seconds > 0, s.watcher.pending_overdue_seconds > 0,
                            s.watcher.unready_overdue_seconds > 0)

    def _make_reflector(self, ns: Optional[str], resource_version: Optional[str], primed: bool) -> Reflector:
        """A scope's reflector (``ScopeSet.start``): on the service's decoder
        and pipeline, or with several scopes on its own."""
        if self.scopes.multi:
            # Each scope decodes its own stream: give it a private decoder.
            dec = self._make_decoder()
            pipe = self._scope_pipeline(dec)
        else:
            dec, pipe = self.decoder, self.pipeline
        return Reflector(self.api, self.settings, dec, pipe, self.metrics, namespace=ns,
                         resource_version=resource_version, primed=primed, list_gate=self.scopes.list_gate)

    def _cache(self):
        """The pod cache, None before the pipeline exists."""
        return self.pipeline.cache if self.pipeline is not None else None

    def _scope_pipeline(self, decoder) -> EventPipeline:
        assert self.pipeline is not None
        p = EventPipeline(self.settings, decoder, self.notifier, self.metrics, self.pipeline.cache,
                          self.event_log, event_sharding=self._event_sharding())
        if self._native_pipeline():
            p.attach_native(self._decode_pool)
        return p

    def _native_pipeline(self) -> bool:
        return self.settings.watcher.engine == "native"

    async def _wait_synced(self) -> None:
        synced = self.scopes.synced()
        runs = list(self._tasks) + self.scopes.tasks()
        done, _ = await asyncio.wait([synced] + runs, return_when=asyncio.FIRST_COMPLETED)
        if synced not in done:
            synced.cancel()
            raise first_exception(runs) or SetupError("watch ended before the initial sync")

    async def wait(self) -> None:
        """Run until :meth:`stop` or a watch fails permanently."""
        stopper = asyncio.ensure_future(self._stop.wait())
        done, _ = await asyncio.wait(list(self._tasks) + [stopper] + self.scopes.ending(),
                                     return_when=asyncio.FIRST_COMPLETED)
        err = first_exception(done)
        if not stopper.done():
            stopper.cancel()
        if err is not None:
            raise err

    def stop(self) -> None:
        self._stop.set()
        self.scopes.stop()

    async def shutdown(self, drain_timeout: float = 10.0, checkpoint: bool = True) -> None:
        """Stop watching, drain the notifier, write the final checkpoint.

        The checkpoint is written only if every notification was delivered:
        a resourceVersion saved with notifications still queued would skip
        them on restart; the previous (quiescent) checkpoint replays them
        instead. ``checkpoint=False`` (a leader that lost its lease) never
        writes — the new leader owns the file now.

        With a spool, notifications still owed after the drain are written to
        it first (closing the notifier), so the checkpoint can be written
        anyway: a restart resumes exactly and replays the spool. A leader that
        lost its lease drops what it still owes instead of spooling it — the
        new leader relists, and an old record replayed in a later term could
        overwrite newer state.
        """
        self.log.info("Stopping Pod watcher...")
        if self._gc_frozen:  # this service's objects are collectable again (a leader's next term)
            self._gc_frozen = False
            gc.unfreeze()
        self.scopes.stop()
        self.handover.abandon_unwritten()  # their pods stay in the checkpoint: the restart hands them over
        drained = True
        closed = False
        if self.notifier is not None:
            if not checkpoint and self.spool is not None:
                self.notifier.detach_spool()
            drained = await self.notifier.drain(drain_timeout)
            if not drained and checkpoint and self.spool is not None:
                await self.notifier.close()  # spools the rest
                closed = drained = True
        if checkpoint and (drained or self.checkpointer.consistent()):
            await self._final_cut()
        tasks = list(self._tasks) + self.scopes.tasks() + self.handover.tasks()
        for t in tasks:
            if not t.done():
                t.cancel()
        for t in tasks:
            try:
                await t
            except (asyncio.CancelledError, WatchFailed, Exception):  # noqa: BLE001
                pass
        if self._metrics_server is not None:
            self._metrics_server.close()
        if self.notifier is not None and not closed:
            await self.notifier.close()  # with a spool, whatever is still owed is written to it
        if self.spool is not None:
            self.spool.close()
        self.runtime.close()  # the hub, the pool's threads, the loop thread's affinity
        if self.api is not None:
            await self.api.close()

    async def run(self) -> None:
        try:
            await self.start()
            await self.wait()
        finally:
            await self.shutdown()

    # ------------------------------------------------------------------ checkpoint
    def _resubmit_owed(self, owed: list) -> None:
        core = getattr(self.notifier, "core", None)
        if core is None:
            self.log.warning(f"{len(owed)} owed notifications in the checkpoint: no native notifier to resend them")
            return
        now = time.monotonic_ns()
        for uid, etype, ns, name, body in owed:
            core.submit_body(uid, etype, ns, name, body, now)
        self.metrics.c["checkpoint_owed_resent"] += len(owed)
        self.notifier.flush()

    async def _final_cut(self) -> None:
        """Shutdown's last word, all of it from one cut of the cache and of
        what the notifier still owes: the final checkpoint (format 2 carries
        the owed notifications; engine/checkpoint.py picks the format) and,
        where namespaces are handed over, a parting record for every namespace
        this shard watches — if the shard count shrinks and this ordinal does
        not come back, their next owners start from those (engine/handover.py).
        Without a notifier core this is only reached drained, and nothing is owed."""
        if self.pipeline is None or not self._hands_over():
            await self.checkpointer.final_cut()
            return
        cache = self.pipeline.cache
        cut: dict = {}

        def at_cut(snap=None) -> None:
            cut.update(watched=self.scopes.watched(), items=cache.items(),
                       owed=snap.owed() if snap is not None else ())

        await self.checkpointer.final_cut(at_cut)
        await self.handover.part_cut(cut, PARTING_BUDGET_SECONDS)

    @property
    def last_checkpoint(self) -> Optional[dict]:
        """The six ``checkpoint_*`` gauges of the last format-2 write."""
        return self.checkpointer.last

    async def checkpoint_now(self, drain_timeout: float = 30.0) -> bool:
        """Write a checkpoint now (engine/checkpoint.py ``Checkpointer.now``)."""
        return await self.checkpointer.now(drain_timeout)
