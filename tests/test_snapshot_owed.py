"""``CacheSnapshot.owed()`` (ops/csrc/checkpoint.inc): the owed notifications
of a consistent cut, read from the snapshot itself — what shutdown's parting
records carry — are what ``load_checkpoint`` returns from the file that same
snapshot writes."""

import asyncio

from conftest import run
from k8s_watcher_amd.engine.checkpoint import load_checkpoint, native_snapshot, write_native
from k8s_watcher_amd.testing.fake_apiserver import FakeApiServer
from k8s_watcher_amd.testing.podgen import PodFactory
from k8s_watcher_amd.testing.stub_sink import StubSink
from k8s_watcher_amd.utils.config import load_settings


def test_snapshot_owed_is_what_its_checkpoint_file_says(tmp_path):
    from k8s_watcher_amd.engine.service import WatcherService
    from k8s_watcher_amd.kube.kubeconfig import KubeEndpoint
    from k8s_watcher_amd.metrics import Metrics

    async def body():
        srv = FakeApiServer()
        await srv.start()
        sink = StubSink()
        await sink.start()
        s = load_settings("staging", overrides={
            "clusterapi": {"base_url": sink.url, "health_check_on_start": False,
                           "retry": {"delay_seconds": 30, "max_attempts": 1000, "max_delay_seconds": 30}},
            "watcher": {"engine": "native"}})
        svc = WatcherService(s, endpoint=KubeEndpoint(server=srv.url), metrics=Metrics())
        await svc.start()
        f = PodFactory(seed=21, namespaces=["ns-a", "ns-b"])
        first = srv.create(f.new_pod())
        await sink.state.wait_for(1, timeout=10)
        await svc.notifier.drain(5)
        quiet = native_snapshot(svc.pipeline.cache, svc.notifier.core)
        assert quiet.owed() == [] and quiet.stats()["owed"] == 0
        sink.state.down = True  # 503: everything from here stays owed (retried in 30 s)
        pods = [srv.create(f.new_pod()) for _ in range(3)]  # one notification per pod: nothing to coalesce
        srv.delete(first["metadata"]["namespace"], first["metadata"]["name"])
        for _ in range(500):
            if svc.notifier.outstanding() == 4 and svc.metrics.c["notify_retried"] >= 1:
                break
            await asyncio.sleep(0.01)
        snap = native_snapshot(svc.pipeline.cache, svc.notifier.core)
        owed = snap.owed()
        write_native(snap, str(tmp_path / "ck.bin"), {"*": "1"}, {})
        _, _, _, from_file = load_checkpoint(str(tmp_path / "ck.bin"), native_cache=True)
        svc.stop()
        await svc.shutdown(drain_timeout=0, checkpoint=False)
        await sink.stop()
        await srv.stop()
        return owed, from_file, [p["metadata"]["uid"] for p in pods], first["metadata"]["uid"]

    owed, from_file, uids, first = run(body(), timeout=60)
    assert owed == from_file  # the same tuples, in the same order
    assert [type(x) for x in owed[0]] == [str, str, str, str, bytes]
    assert [(o[0], o[1]) for o in owed] == [(uids[0], "ADDED"), (uids[1], "ADDED"), (uids[2], "ADDED"),
                                            (first, "DELETED")]
    assert owed is not from_file and len({o[4] for o in owed}) == 4
