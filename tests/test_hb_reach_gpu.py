"""The engine against the oracle after every hop of the hb_steps scenarios
(scenarios.HB_STEPS): every step of the heartbeat's mesh maintenance, in the
whole-wave and in the half-wave instantiation of the heartbeat kernel's topic
loop (tests/test_hb_reach.py pins that the runs hold them)."""
import pytest

import p6_check
import scenarios
from pubsub_amd import PRODUCT_LIB

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(scenarios.HB_STEPS))
def test_hb_steps_equal_oracle_every_hop(oracle_path, name):
    _, ref = p6_check.oracle_snaps(oracle_path, name)
    _, got = p6_check.hop_snaps(PRODUCT_LIB, name)
    assert p6_check.first_difference(ref, got) is None
    _, again = p6_check.hop_snaps(PRODUCT_LIB, name)
    assert p6_check.first_difference(got, again) is None, "two GPU runs differ"
