"""The heartbeat's peertx rebuild (k_ptx_rebuild, k_ptxo_collect,
k_ptxo_reinsert, k_ptxo_fin of csrc/gs_kernels_ctl.h) launched alone through
the probe, by the engine's own launch function (ptx_rebuild_launch: the
engine's grids, blocks and dynamic LDS), against the dict of
tests/tables_ref.py.  The tables are filled by the product's insert path
(probe.PeerTx.run), rebuilt, looked up by the product's lookup path and
incremented again, as a run does between heartbeats.  Bit-exact: after every
rebuild every survivor is there once with its count, nothing else is, ptxN and
ptxOCnt are right, no node with a free slot keeps an overflow entry, and
ptx_count_g / ptxo_count find exactly the survivors (tables_ref.run_case).
tests/test_tables_ref.py shows on the CPU which path each case reaches."""
import numpy as np
import pytest

import probe
import tables_ref as T

pytestmark = pytest.mark.gpu

CASES = T.rebuild_cases()
INVALID = 1  # hipErrorInvalidValue


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_rebuild_case(case):
    stats = T.run_case(case, probe.PeerTx(case["bits"], case["obits"], T.GR, case["n_nodes"]))
    assert len(stats) == sum(1 for s in case["steps"] if s[0] == "rebuild")


def test_reference_hash_is_the_device_hash():
    """The cases pick colliding keys with tables_ref.ptx_hash."""
    rng = np.random.default_rng(T.SEED + 110)
    keys = np.concatenate([rng.integers(0, 1 << 28, 4000, dtype=np.uint32) & np.uint32(0xFFFFFF00),
                           np.array([0, T.ptx_key((1 << 14) - 1, 63)], dtype=np.uint32)])
    for bits in (2, 4, 6, 7, 8, 9, 10, 15):
        assert probe.ptx_hash(keys, bits).tolist() == [T.ptx_hash(k, bits) for k in keys.tolist()]


def test_outer_rows_with_foreign_neighbours():
    """Rows of 4 between neighbours whose words would survive any bitmap of
    the node in the middle if its wave read them: five nodes, node 2 drops
    everything, and its neighbours' rows come back word for word (their keys
    keep the home slots the inserts gave them: one key per home slot)."""
    bits, n = 2, 5
    by_home = {}
    for s in range(256):
        by_home.setdefault(T.ptx_hash(T.ptx_key(s, 1), bits), []).append(T.ptx_key(s, 1))
    keys = {v: [by_home[h][v] for h in range(4)] for v in range(n)}  # one key per home slot: no probing
    tx = probe.PeerTx(bits, 6, T.GR, n)
    rounds = [[(v, k) for v in range(n) for k in keys[v]]] * 2
    tx.run(rounds=rounds)
    before = tx.rows.copy().reshape(n, 4)
    assert (before != 0).all()
    lastw = np.zeros((n, 4), dtype=np.uint64)
    for k in keys[2]:
        lastw[2, (k >> 14) >> 6] |= np.uint64(1 << ((k >> 14) & 63))
    tx.rebuild(T.hist_ring(2, 0, lastw), 0)
    after = tx.rows.reshape(n, 4)
    assert (after[2] == 0).all() and tx.ptxn.tolist() == [4, 4, 0, 4, 4]
    for v in (0, 1, 3, 4):
        assert (after[v] == before[v]).all()


def test_entry_point_refuses_what_it_cannot_run_safely():
    """Checked on the host before any launch (hipErrorInvalidValue)."""
    hist = np.zeros((1, 1, 4), dtype=np.uint64)

    def refused(tx, h=hist, last=0):
        with pytest.raises(probe.ProbeError, match=f"HIP error {INVALID}$"):
            tx.rebuild(h, last)

    tx = probe.PeerTx(2, 3, T.GR)
    tx.rows[1] = T.ptx_key(256, 0) | 1  # a slot outside hist's 4 words
    refused(tx)
    tx = probe.PeerTx(2, 3, T.GR)
    tx.ovf[0] = (2 << 32) | T.ptx_key(1, 0) | 1  # the tag of a node that is not there
    refused(tx)
    tx = probe.PeerTx(2, 3, T.GR)
    tx.ovf[0] = (1 << 32) | T.ptx_key(300, 0) | 1
    refused(tx)
    tx = probe.PeerTx(2, 3, T.GR)
    tx.ocnt[2] = 1  # the staging index would not start at 0
    refused(tx)
    refused(probe.PeerTx(2, 3, T.GR), last=1)
    refused(probe.PeerTx(1, 3, T.GR))  # a row shorter than one 16-byte read
    assert (4 << 16) > probe.lds_limit()
    refused(probe.PeerTx(16, 3, T.GR))  # a row the device's LDS cannot stage
