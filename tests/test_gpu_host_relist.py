"""The sliced native relist on the deployment host, where the scanner's SIMD
level and the core count (so the decode pool's scheduling) differ: cases 1-7
of ``tests/test_relist_sliced.py``, each with no decode pool and with the
shared one. Nothing here depends on time, so no rate is recorded. The size
hint's test stays in the CPU tier: its child process may end in an abort,
which has no place on a shared machine."""

import os
import sys

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(ROOT, "tests"))

POOLS = pytest.mark.parametrize("pool", [False, True], ids=["no-pool", "shared-pool3"])


@POOLS
def test_resumed_walk_namespace_on_host(pool):
    import test_relist_sliced as t
    t.check_resumed_walk_namespace(pool)


@POOLS
def test_resumed_walk_cluster_on_host(pool):
    import test_relist_sliced as t
    t.check_resumed_walk_cluster(pool)


@POOLS
def test_two_relists_at_once_on_host(pool):
    import test_relist_sliced as t
    t.check_two_relists_at_once(pool)


@POOLS
def test_watch_between_slices_on_host(pool):
    import test_relist_sliced as t
    t.check_watch_between_slices(pool)


@pytest.mark.parametrize("where", ["early", "middle", "late"])
@POOLS
def test_rehash_in_mid_walk_on_host(pool, where):
    import test_relist_sliced as t
    t.check_rehash_in_mid_walk(pool, where)


@pytest.mark.parametrize("again", [None, "walk", "deletes"], ids=["once", "again-in-walk", "again-after-deletes"])
@POOLS
def test_restart_under_slicing_on_host(pool, again):
    import test_relist_sliced as t
    t.check_restart_under_slicing(pool, again)


@POOLS
def test_handover_between_sweep_slices_on_host(pool):
    import test_relist_sliced as t
    t.check_handover_between_sweep_slices(pool)
