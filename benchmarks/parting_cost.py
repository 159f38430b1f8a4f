#!/usr/bin/env python3
"""What shutdown's parting step costs (engine/handover.py ``part``).

    python -m benchmarks.parting_cost [--namespaces 1000] [--pods 100] [--dir DIR] [--out f.json]

One native-engine shard watches ``--namespaces`` namespaces (discovered from a
fake API server) with ``watcher.shard.handover_dir`` and a checkpoint under
``--dir`` (a local directory). One real pod goes through the pipeline for its
payload core; the cache is then filled to ``--pods`` pods per namespace with
cores of that size, and the service is shut down. Reported, all from that one
shutdown:

* ``parting_ms`` — grouping the cut's pods by namespace plus ``part()``: every
  record and the manifest written and renamed;
* ``checkpoint_write_ms`` / ``checkpoint_stall_ms`` — the final checkpoint's
  write (executor thread) and its cut (loop thread), as ``/metrics`` has them;
* ``loop_held_ms`` — the longest the event loop went without running a 1 ms
  ticker while the parting step ran;
* ``cut_items_ms`` — what the parting step adds to the cut itself: one
  ``cache.items()`` on the loop thread;
* ``manifest_namespaces`` / ``records`` — what the manifest lists and the
  record files there are, ``budget_s`` the step's budget.
"""

from __future__ import annotations

import argparse
import asyncio
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


async def measure(args) -> dict:
    from k8s_watcher_amd.engine import handover as handover_mod
    from k8s_watcher_amd.engine import service as service_mod
    from k8s_watcher_amd.engine.service import WatcherService
    from k8s_watcher_amd.kube.kubeconfig import KubeEndpoint
    from k8s_watcher_amd.metrics import Metrics
    from k8s_watcher_amd.testing.fake_apiserver import FakeApiServer
    from k8s_watcher_amd.testing.podgen import PodFactory
    from k8s_watcher_amd.testing.stub_sink import StubSink
    from k8s_watcher_amd.utils.config import load_settings

    nss = [f"ns-{i:04d}" for i in range(args.namespaces)]
    srv = FakeApiServer(namespaces=nss)
    await srv.start()
    sink = StubSink(record=False)
    await sink.start()
    hdir = os.path.join(args.dir, "handover")
    s = load_settings("staging", overrides={
        "clusterapi": {"base_url": sink.url, "health_check_on_start": False},
        "watcher": {"engine": "native", "namespace_scope": "discover",
                    "shard": {"count": 1, "index": 0, "handover_dir": hdir},
                    "checkpoint": {"path": os.path.join(args.dir, "ck.bin"), "interval_seconds": 3600}}})
    svc = WatcherService(s, endpoint=KubeEndpoint(server=srv.url), metrics=Metrics())
    await svc.start()
    f = PodFactory(seed=5, namespaces=nss)
    seed = srv.create(f.running(f.new_pod(namespace=nss[0])))
    await sink.state.wait_for(1, timeout=20)
    await svc.notifier.drain(5)
    cache = svc.pipeline.cache
    rv, phase, _, name, core = cache.get(seed["metadata"]["uid"])
    for i, ns in enumerate(nss):
        for k in range(args.pods - (1 if i == 0 else 0)):
            cache.put(f"{i:08x}-{k:04x}-4000-8000-000000000000", rv, phase, ns, f"{name}-{k}", core)

    loop = asyncio.get_running_loop()
    out = {"namespaces": len(nss), "pods": len(cache), "core_bytes": len(core),
           "budget_s": service_mod.PARTING_BUDGET_SECONDS}
    held = [0.0]

    async def ticker():
        while True:
            t = loop.time()
            await asyncio.sleep(0.001)
            held[0] = max(held[0], loop.time() - t - 0.001)

    group, part = handover_mod.pods_by_namespace, svc.handover.part
    t_part = [0.0, 0.0]
    tick = []

    def timed_group(items, watched):  # on its executor thread: the step begins here
        t_part[0] = time.monotonic()
        loop.call_soon_threadsafe(lambda: tick.append(asyncio.ensure_future(ticker())))
        return group(items, watched)

    async def timed_part(*a, **kw):
        try:
            return await part(*a, **kw)
        finally:
            t_part[1] = time.monotonic()
            for t in tick:
                t.cancel()

    handover_mod.pods_by_namespace, svc.handover.part = timed_group, timed_part
    t0 = time.monotonic()
    svc.stop()
    await svc.shutdown()
    out["shutdown_ms"] = (time.monotonic() - t0) * 1e3
    out["parting_ms"] = (t_part[1] - t_part[0]) * 1e3
    out["loop_held_ms"] = held[0] * 1e3
    out["checkpoint_write_ms"] = svc.last_checkpoint["checkpoint_write_ms"]
    out["checkpoint_stall_ms"] = svc.last_checkpoint["checkpoint_stall_ms"]
    out["checkpoint_bytes"] = svc.last_checkpoint["checkpoint_bytes"]
    t0 = time.monotonic()
    cache.items()
    out["cut_items_ms"] = (time.monotonic() - t0) * 1e3
    with open(os.path.join(hdir, "shard-0.parted.json")) as fh:
        out["manifest_namespaces"] = len(json.load(fh)["namespaces"])
    records = [x for x in os.listdir(hdir) if x.endswith(".parting.json")]
    out["records"] = len(records)
    out["record_bytes"] = sum(os.path.getsize(os.path.join(hdir, x)) for x in records)
    out["partings_out"] = svc.metrics.c["shard_partings_out"]
    out["errors"] = svc.metrics.c["shard_handover_errors"]
    await sink.stop()
    await srv.stop()
    return out


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--namespaces", type=int, default=1000)
    ap.add_argument("--pods", type=int, default=100, help="pods per namespace")
    ap.add_argument("--dir", default=None, help="a local directory (default: a temporary one)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        args.dir = d
        out = asyncio.run(measure(args))
    line = json.dumps(out)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
