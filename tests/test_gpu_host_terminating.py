"""``watcher.alerts.terminating`` on the deployment host, where the host CPU
picks the scanner's SIMD level: the corpus through both engines, the pod's
life, the partitioned apply against the serial one, the relist, and one bench
line with the option on."""

import os
import sys

import pytest

from conftest import ROOT, run_bench

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tests"))

BENCH = ["--steps", "2", "--warmup", "1", "--rounds-per-step", "1", "--apart", "off", "--staging", "off",
         "--pods-per-step", "1000", "--ref-events", "500", "--latency-seconds", "1", "--latency-seconds-high", "1",
         "--set", "watcher.alerts.terminating=true"]


def test_corpus_on_host():
    import test_terminating_alerts as t
    t.check_corpus()


def test_pod_life_on_host():
    import test_terminating_alerts as t
    t.check_pod_life()


def test_partitioned_apply_on_host():
    import test_terminating_alerts as t
    t.check_partitioned_matches_serial()


@pytest.mark.parametrize("native", [True, False], ids=["native-relist", "python-reconcile"])
def test_relist_on_host(native):
    import test_terminating_alerts as t
    t.check_relist(native)


def test_bench_line_with_terminating():
    """The fixture sets ``deletionTimestamp`` on DELETED events only
    (``testing/podgen.py``, ``deleting``), and those pass every filter anyway:
    the same notifications as without the option, exactly once."""
    line = run_bench(BENCH)
    assert line["value"] > 0 and line["steps"] == 2
    assert line["notify_failed"] == 0
    assert line["verify"]["exactly_once"]
