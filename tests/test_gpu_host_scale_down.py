"""Host tier (``-m gpu``): the scale-down hand-over on the MI355X box, native
engine — the parting records are written from the native snapshot's cut on the
host's executor threads and taken by the new owners there."""

import pytest

import test_scale_down

pytestmark = pytest.mark.gpu


def test_three_to_two_on_the_host(tmp_path):
    test_scale_down.test_three_to_two_hands_the_removed_shards_namespaces_over(tmp_path, engine="native")
