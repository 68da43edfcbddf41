"""The engine against the oracle after every hop of the P6 scenarios
(scenarios.P6): the IP colocation factor over its threshold, recounted by
k_p6 while connections come and go, at refresh hops (expired records) and
between them, and the host-side count at the start with and without a
whitelist.

gs_read_scores recomputes every score from the state, so a score memo (S0 /
S1, gs_kernels.h) that a recount left stale shows only in what the engine
decided with it: the counters, the meshes, the backoffs.  The next refresh
repairs the memo, so the comparison is made hop by hop and the first
difference names its hop; tests/test_p6.py pins that the runs hold such
recounts."""
import pytest

import p6_check
import scenarios
from pubsub_amd import PRODUCT_LIB

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(scenarios.P6))
def test_p6_equals_oracle_every_hop(oracle_path, name):
    _, ref = p6_check.oracle_snaps(oracle_path, name)
    _, got = p6_check.hop_snaps(PRODUCT_LIB, name)
    assert p6_check.first_difference(ref, got) is None
    _, again = p6_check.hop_snaps(PRODUCT_LIB, name)
    assert p6_check.first_difference(got, again) is None, "two GPU runs differ"
