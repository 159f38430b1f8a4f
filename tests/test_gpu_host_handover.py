"""Host tier (``-m gpu``): a restart after a settled re-shard on the MI355X
box, native engine — the restarted shard's lost checkpoint is rebuilt by the
native pipeline's first LISTs there, with nothing waiting for a hand-over."""

import pytest

import test_sharding

pytestmark = pytest.mark.gpu


def test_restart_after_a_settled_reshard_on_the_host(tmp_path):
    test_sharding.test_restart_after_a_settled_reshard_is_a_plain_restart(tmp_path, engine="native")
