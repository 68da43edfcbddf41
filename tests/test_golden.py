"""Golden vectors (tests/golden/scenarios.json, made by make_golden.py): the
oracle on CPU and the HIP engine on the GPU must both reproduce every counter
and every readback digest of every parity scenario."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

import scenarios  # noqa: E402
from make_golden import digest  # noqa: E402

GOLDEN = json.load(open(os.path.join(HERE, "golden", "scenarios.json")))


@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_oracle_reproduces_golden(oracle_path, name):
    assert digest(scenarios.run(oracle_path, name)) == GOLDEN[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GOLDEN))
def test_gpu_reproduces_golden(name):
    from pubsub_amd import PRODUCT_LIB
    assert digest(scenarios.run(PRODUCT_LIB, name)) == GOLDEN[name]


# Races show up as run-to-run differences before they show up as a wrong
# digest: the scenarios with the most cross-lane LDS and global atomics in
# phase B (IWANT serving, IHAVE handling, spam, cuts) run three more times.
RACE_PRONE = ["gossipsub_dense_dhi", "c5shape", "adversarial_mix", "spam_ihave_2t", "churn_graft",
              # full waves: 64 peers per node, 64 topics / 64 senders per validation queue
              "ladder_64t", "ladder_adversarial",
              # a young-slot table with every age 1..maxAge in it at every hop
              "win_gossip_edge"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in RACE_PRONE if n in GOLDEN])
def test_gpu_golden_repeatable(name):
    from pubsub_amd import PRODUCT_LIB
    for _ in range(3):
        assert digest(scenarios.run(PRODUCT_LIB, name)) == GOLDEN[name]


# mcache.peertx spills (mcache.go:66-80 keeps an unbounded map): with 4 slots
# per node, every node that serves more than 4 (message, requester) IWANT
# entries within its cache window takes the rest in the rank's overflow table
# (gs_set_peertx_capacity); the heartbeat's rebuild moves survivors back when
# a node's own table has room.  The goldens must not move.
PEERTX_SPILL = ["c3shape", "adversarial_mix", "gossipsub_slot_reuse", "churn_scored", "c4shape", "px_adversarial",
                # a host serving 64 peers from 4 slots spills at once
                "ladder_scored",
                # peertx entries of slots that are used again at retireHops
                "win_gossip_edge", "win_adv_edge"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in PEERTX_SPILL if n in GOLDEN])
def test_gpu_peertx_overflow_reproduces_golden(name):
    from pubsub_amd import PRODUCT_LIB, WithPeertxCapacity
    # (2^20 overflow entries: c3shape alone spills more than the default 2^16)
    assert digest(scenarios.run(PRODUCT_LIB, name, extra=(WithPeertxCapacity(2, 20),))) == GOLDEN[name]


@pytest.mark.gpu
def test_gpu_peertx_overflow_full_is_capacity_error():
    """An overflow table too small for the live entries is GS_ECAPACITY, not a
    silent miscount."""
    from pubsub_amd import PRODUCT_LIB, GossipEngineError, WithPeertxCapacity, _abi
    with pytest.raises(GossipEngineError) as ei:
        scenarios.run(PRODUCT_LIB, "c3shape", extra=(WithPeertxCapacity(2, 8),))
    assert ei.value.code == _abi.GS_ECAPACITY and "overflow table" in str(ei.value)


def _largest_home_bits():
    """The largest gs_set_peertx_capacity home_bits whose row (4 << home_bits
    bytes, staged in LDS by the heartbeat's rebuild) fits the device's LDS per
    workgroup; 16 is the API's own limit."""
    import probe
    lim = probe.lds_limit()
    fits = [b for b in range(2, 17) if (4 << b) <= lim]
    assert fits, lim
    return max(fits), lim


@pytest.mark.gpu
def test_gpu_peertx_largest_home_bits_reproduces_golden():
    """The heartbeat's rebuild with the largest row the device's LDS holds (15
    where a workgroup has 160 KiB: 128 KiB of dynamic LDS per launch)."""
    from pubsub_amd import PRODUCT_LIB, WithPeertxCapacity
    bits, lim = _largest_home_bits()
    print(f"LDS per workgroup {lim} bytes: largest home_bits {bits}")
    assert digest(scenarios.run(PRODUCT_LIB, "c3shape", extra=(WithPeertxCapacity(bits, 16),))) == GOLDEN["c3shape"]


@pytest.mark.gpu
def test_gpu_peertx_home_bits_above_lds_is_capacity_error():
    """One above that is refused by name when the tables are sized, before any
    kernel runs, not by a failed launch at the first heartbeat."""
    from pubsub_amd import PRODUCT_LIB, GossipEngineError, WithPeertxCapacity, _abi
    bits, lim = _largest_home_bits()
    assert bits < 16  # (gs_set_peertx_capacity itself stops at 16)
    with pytest.raises(GossipEngineError) as ei:
        scenarios.run(PRODUCT_LIB, "c3shape", extra=(WithPeertxCapacity(bits + 1, 16),))
    msg = str(ei.value)
    assert ei.value.code == _abi.GS_ECAPACITY
    assert f"home_bits {bits + 1}" in msg and str(4 << (bits + 1)) in msg and str(lim) in msg
