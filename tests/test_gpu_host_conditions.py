"""``watcher.alerts.pod_conditions`` on the deployment host, where the host CPU
picks the scanner's SIMD level: the corpus through both engines, the pod's
life, the partitioned apply against the serial one, the relist, and two bench
lines with the option on."""

import os
import sys

import pytest

from conftest import ROOT, run_bench

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tests"))

BENCH = ["--steps", "2", "--warmup", "1", "--rounds-per-step", "1", "--apart", "off", "--staging", "off",
         "--pods-per-step", "1000", "--ref-events", "500", "--latency-seconds", "1", "--latency-seconds-high", "1",
         "--set", "watcher.alerts.pod_conditions=true"]

_lines = {}


def bench_line(*more):
    """One run per argument list, shared by the tests that read it."""
    if more not in _lines:
        _lines[more] = run_bench(BENCH + list(more))
    return _lines[more]


def test_corpus_on_host():
    import test_pod_condition_alerts as t
    t.check_corpus()


def test_pod_life_on_host():
    import test_pod_condition_alerts as t
    t.check_pod_life()


def test_partitioned_apply_on_host():
    import test_pod_condition_alerts as t
    t.check_partitioned_matches_serial()


@pytest.mark.parametrize("native", [True, False], ids=["native-relist", "python-reconcile"])
def test_relist_on_host(native):
    import test_pod_condition_alerts as t
    t.check_relist(native)


def test_bench_line_with_pod_conditions():
    """The fixture's pods carry PodScheduled=True and Ready=False:ContainersNotReady,
    which the default rules do not match: the same notifications, exactly once."""
    line = bench_line()
    assert line["value"] > 0 and line["steps"] == 2
    assert line["notify_failed"] == 0
    assert line["verify"]["exactly_once"]


def test_bench_line_with_a_rule_that_matches():
    """``Ready=False:ContainersNotReady`` does match fixture pods (Pending ones,
    which the critical filter drops otherwise), so more is sent than with the
    default rules. The bench's ``verify`` block compares what the sink
    received with the fixture's own count of notifiable events (the phase
    rule), which the extra notifications exceed: only ``notify_failed`` is
    asserted here, not ``exactly_once``."""
    first = bench_line()
    line = bench_line("--set", 'watcher.alerts.pod_condition_rules=["Ready=False:ContainersNotReady"]')
    assert line["value"] > 0 and line["steps"] == 2
    assert line["notify_failed"] == 0
    assert line["verify"]["received"] >= first["verify"]["received"] > 0
