"""The reader hub's stall guard on the MI355X box's CPUs (``-m gpu``, host tier).

The guard's tick runs on the reader threads, beside the reads of up to a
thousand watch streams: what must hold on the deployment host is that a
stranded stream is recovered there too, that an honest wait and real
starvation are told apart from a stall with the host's many cores racing the
threads, and that a run of the namespace-watch shape neither needs nor
counts a recovery.
"""

import os
import sys

import pytest

from conftest import ROOT, run_bench

pytestmark = pytest.mark.gpu


def test_stall_guard_on_host():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_stall_guard as tsg
    for readers in (1, 3):
        tsg.test_stranded_stream_is_recovered(readers)
        tsg.test_honest_wait_is_reported_not_recovered(readers)
        for seed in (0, 1):
            tsg.test_no_false_recoveries_under_real_starvation(readers, seed)


def test_discover_bench_needs_no_recovery_on_host():
    """64 namespace watches over the 8 MiB read-ahead (the shape round 6's
    stall was seen in), the guard on as by default: exactly-once, no stream
    re-armed by the guard, and the bench line carries the guard's figures."""
    line = run_bench(["--steps", "2", "--warmup", "1",
                      "--rounds-per-step", "1", "--apart", "off", "--staging", "off", "--ref-events", "0",
                      "--latency-seconds", "0", "--latency-seconds-high", "0", "--watch-scope", "discover",
                      "--namespaces", "64"])
    assert line["verify"]["exactly_once"] and line["per_rank"][0]["scopes"] == 64
    hub = line["watch_reader_rank0"]
    assert hub["mode"] == "native" and hub["stall_guard_ns"] == 30_000_000_000
    assert hub["stall_recoveries"] == 0 and "oldest_unread_ns" in hub
