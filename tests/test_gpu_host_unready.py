"""``watcher.alerts.unready_overdue_seconds`` on the deployment host, where the
host CPU picks the scanner's SIMD level: the corpus and the seeded mutations
through both engines, a pod's life with sweeps, the partitioned apply against
the serial one followed by a sweep, the relist and the restart, and one bench
line with the option on."""

import os
import sys

import pytest

from conftest import ROOT, run_bench

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tests"))

BENCH = ["--steps", "2", "--warmup", "1", "--rounds-per-step", "1", "--apart", "off", "--staging", "off",
         "--pods-per-step", "1000", "--ref-events", "500", "--latency-seconds", "1", "--latency-seconds-high", "1"]
ON = ["--set", "watcher.alerts.unready_overdue_seconds=4000000000"]


def test_corpus_on_host():
    import test_unready_overdue as t
    t.check_corpus()
    t.check_option_off()
    t.check_fuzz()


def test_pod_life_on_host():
    import test_unready_overdue as t
    t.check_pod_life()


def test_partitioned_apply_on_host():
    import test_unready_overdue as t
    t.check_partitioned_matches_serial()


@pytest.mark.parametrize("native", [True, False], ids=["native-relist", "python-reconcile"])
def test_relist_on_host(native):
    import test_unready_overdue as t
    t.check_relist(native)
    t.check_shared_cache(native)


def test_bench_line_with_the_option_on():
    """The replay's ``Running`` lines are all ``Ready=True``
    (``testing/podgen.py``), so no line has an unready-since and this line
    prices the conditions walk alone: the fixture counts what a watcher
    without the option notifies (``verify.expected``), and exactly those
    arrive, once each."""
    line = run_bench(BENCH + ON)
    assert line["value"] > 0 and line["steps"] == 2
    assert line["notify_failed"] == 0
    v = line["verify"]
    assert v["exactly_once"] and v["received"] == v["expected"] == v["unique"] and v["duplicates"] == 0
