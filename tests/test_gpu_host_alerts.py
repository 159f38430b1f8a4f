"""``watcher.alerts.container_failures`` on the deployment host, where the
host CPU picks the scanner's SIMD level: the pod's life through both engines,
the extra field from both decoders, the partitioned apply against the serial
one, and one bench line with the option on."""

import os
import sys

import pytest

from conftest import ROOT, run_bench

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tests"))


def test_pod_life_on_host():
    import test_container_failures as t
    t.check_pod_life()


def test_extra_field_on_host():
    import test_container_failures as t
    t.check_extra_field()


def test_partitioned_apply_on_host():
    import test_container_failures as t
    t.check_partitioned_matches_serial()


def test_bench_line_with_container_failures():
    """The fixture's pods have no failing containers: the same notifications, exactly once."""
    line = run_bench(["--steps", "2", "--warmup", "1", "--rounds-per-step", "1", "--apart", "off", "--staging", "off",
                      "--pods-per-step", "1000", "--ref-events", "500", "--latency-seconds", "1",
                      "--latency-seconds-high", "1", "--set", "watcher.alerts.container_failures=true"])
    assert line["value"] > 0 and line["steps"] == 2
    assert line["notify_failed"] == 0
    assert line["verify"]["exactly_once"]
