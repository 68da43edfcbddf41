"""What the hb_steps scenarios (scenarios.HB_STEPS) are there for, pinned on
the oracle: every step of the heartbeat's mesh maintenance (tests/hb_reach.py
names them and the condition each is counted on) happens in some heartbeat of
the run with a node of more than 32 peers, where the heartbeat kernel's topic
loop handles one topic per wave, and of the run with at most 32 peers per node
and two joined topics, where it handles one per half-wave.  A change of seed
that empties one of these counts would leave tests/test_hb_reach_gpu.py and the
goldens comparing runs in which that step never runs."""
import numpy as np
import pytest

import hb_reach
import scenarios
from pubsub_amd import graphs


@pytest.mark.parametrize("name, k", [("hb_steps_40", 40), ("hb_steps_32", 32)])
def test_every_step_is_reached(oracle_path, olib, name, k):
    assert scenarios.SCENARIOS[name] is scenarios.HB_STEPS[name]
    g = graphs.random_regular(64, k, scenarios.HB_STEPS_SEED)
    deg = np.diff(g[0])
    assert (deg.max() > 32) if k > 32 else (deg.max() <= 32)
    got = hb_reach.reach(oracle_path, olib, name, g, scenarios.HB_STEPS_PARAMS, scenarios.HB_STEPS_SEED)
    print(name, "max degree", int(deg.max()), "heartbeats with each step:", got)
    assert set(got) == set(hb_reach.STEPS)
    assert all(n >= 1 for n in got.values()), got
