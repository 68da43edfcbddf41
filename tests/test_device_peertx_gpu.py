"""The peertx hash tables of csrc/gs_kernels_ctl.h (ptx_settle, ptx_count_g,
ptxo_settle, ptxo_count) launched alone through the probe (tests/probe.py)
against a dict of counts.  The stored count is held at GR + 1, the returned
count is min(old + 1, GR + 2), `ins` is set exactly on first insertion.  The
call sites never run two increments of one key concurrently, so the probe runs
rounds: keys distinct within a round, rounds separated by a launch.  Which
slot a key lands in depends on the race, so tables are compared as multisets.
A full row spills into the overflow table; with both full the insert returns 0
and sets the engine's own error code E_PEERTX (every loop is bounded by the
table sizes)."""
import collections

import numpy as np
import pytest

import probe
import select_ref as R

pytestmark = pytest.mark.gpu

GR = 3


def _keys(rng, n, node_edges=64):
    """n distinct peertx keys slot << 14 | in-edge << 8 (count bits zero), key 0
    (slot 0 at in-edge 0) among them."""
    perm = rng.permutation(1 << 14)
    slots = np.concatenate([[0], perm[perm != 0][:n - 1]]).astype(np.uint32)
    edges = rng.integers(0, node_edges, n).astype(np.uint32)
    edges[0] = 0
    keys = (slots << np.uint32(14)) | (edges << np.uint32(8))
    assert len(set(keys.tolist())) == n
    return keys


class Model:
    """mcache.peertx as a dict; follows which table took each key."""

    def __init__(self, tx):
        self.tx, self.count, self.dropped = tx, collections.Counter(), set()

    def check_round(self, round_, ret, ins):
        for (v, k), r, i in zip(round_, ret, ins):
            k = int(k)
            if r == 0:  # both tables full: nothing stored
                assert (v, k) not in self.count and not i
                self.dropped.add((v, k))
                continue
            old = self.count[(v, k)]
            assert r == min(old + 1, self.tx.gr + 2), (v, hex(k), r, old)
            assert bool(i) == (old == 0), (v, hex(k))
            self.count[(v, k)] = min(old + 1, self.tx.gr + 1)

    def check_tables(self):
        """Every key present exactly once across its row and the overflow table
        with its count, no other non-zero word, ptxOCnt = overflow entries."""
        tx = self.tx
        found = collections.Counter()
        for v in range(tx.n_nodes):
            for w in tx.rows[v << tx.bits:(v + 1) << tx.bits].tolist():
                if w:
                    found[(v, w & ~0xFF)] += 1
                    assert w & 0xFF == self.count.get((v, w & ~0xFF)), (v, hex(w))
        in_ovf = 0
        for w in tx.ovf.tolist():
            if w:
                v, k = (w >> 32) - 1, w & 0xFFFFFF00
                found[(v, k)] += 1
                in_ovf += 1
                assert w & 0xFF == self.count.get((v, k)), (v, hex(w))
        assert found == collections.Counter(self.count.keys())
        assert int(tx.ocnt[0]) == in_ovf and tx.ocnt[1] == 0 and tx.ocnt[2] == 0
        return in_ovf

    def check_lookups(self, extra=()):
        """ptx_count_g of every key held, of the dropped ones and of `extra`
        absent ones; ptxo_count agrees wherever the key lives in the overflow table."""
        tx = self.tx
        q = list(self.count) + list(self.dropped) + list(extra)
        _, cg, co = tx.run(queries=q)
        ovf = {((w >> 32) - 1, w & 0xFFFFFF00): w & 0xFF for w in tx.ovf.tolist() if w}
        for (v, k), g, o in zip(q, cg, co):
            assert g == self.count.get((v, k), 0), (v, hex(k), g)
            assert o == ovf.get((v, k), 0), (v, hex(k), o)


def _same_home(bits, n, rng):
    """n distinct keys whose home slot (ptx_hash on the device) is the same."""
    cand = _keys(rng, 1 << 14)
    home = probe.ptx_hash(cand, bits)
    slot = np.bincount(home, minlength=1 << bits).argmax()
    keys = cand[home == slot][:n]
    assert len(keys) == n, "not enough keys with one home slot"
    return keys, int(slot)


@pytest.mark.parametrize("bits", [2, 4, 8], ids=["row4", "row16", "row256"])
def test_one_home_slot_race_and_counts_past_gr(bits):
    """64 keys racing for one home slot in one round (rows of 4 and 16 spill
    into the overflow table), then the same keys incremented past GR + 1."""
    rng = np.random.default_rng(R.SEED + 30 + bits)
    keys, _ = _same_home(bits, 64, rng)
    tx = probe.PeerTx(bits, 7, GR)
    m = Model(tx)
    round_ = [(0, int(k)) for k in keys]
    rounds = [round_] + [round_[:40]] * (GR + 3) + [round_[20:]]
    for r, (ret, ins) in zip(rounds, tx.run(rounds=rounds)[0]):
        m.check_round(r, ret, ins)
    assert tx.err[0] == 0
    assert m.check_tables() == max(0, 64 - (1 << bits))
    assert m.count[(0, int(keys[0]))] == GR + 1 and m.count[(0, int(keys[50]))] == 2
    absent = [(0, int(k)) for k in _keys(rng, 200)[1:] if (0, int(k)) not in m.count]
    m.check_lookups(absent)


def test_nodes_share_the_overflow_table():
    """Three nodes with rows of 4: the same keys in every node, told apart in
    the overflow table by the node tag."""
    rng = np.random.default_rng(R.SEED + 40)
    keys = _keys(rng, 12)
    tx = probe.PeerTx(2, 6, GR, n_nodes=3)
    m = Model(tx)
    round_ = [(v, int(k)) for v in range(3) for k in keys]
    rounds = [round_, round_[::2], round_]
    for r, (ret, ins) in zip(rounds, tx.run(rounds=rounds)[0]):
        m.check_round(r, ret, ins)
    assert tx.err[0] == 0 and m.check_tables() == 3 * 8
    m.check_lookups([(v, int(k)) for v in range(3) for k in _keys(rng, 30)[1:] if (v, int(k)) not in m.count])


def test_both_tables_full_sets_e_peertx_and_keeps_entries():
    e_peertx = probe.consts()["E_PEERTX"]
    rng = np.random.default_rng(R.SEED + 50)
    keys = [(0, int(k)) for k in _keys(rng, 40)]
    tx = probe.PeerTx(2, 3, GR)  # 4 + 8 entries in all
    m = Model(tx)
    (ret, ins), (ret2, ins2) = tx.run(rounds=[keys[:12], keys[:12]])[0]
    m.check_round(keys[:12], ret, ins)
    m.check_round(keys[:12], ret2, ins2)
    assert tx.err[0] == 0 and m.check_tables() == 8 and (ret > 0).all()
    rows, ovf = tx.rows.copy(), tx.ovf.copy()
    # absent keys looked up with every slot of both tables taken
    m.check_lookups(keys[12:])
    assert tx.err[0] == 0
    # inserts into the full tables: refused with the engine's error code
    (ret, ins), = tx.run(rounds=[keys[12:]])[0]
    m.check_round(keys[12:], ret, ins)
    assert (ret == 0).all() and not ins.any()
    assert tx.err[0] == e_peertx
    assert (tx.rows == rows).all() and (tx.ovf == ovf).all() and tx.ocnt[0] == 8
    # the entries present still count, up to the cap, with the error standing
    (ret, ins), = tx.run(rounds=[keys[:12]])[0]
    m.check_round(keys[:12], ret, ins)
    assert (ret == 3).all() and tx.err[0] == e_peertx
    m.check_tables()
    m.check_lookups()


def test_partial_overflow_in_one_round():
    """More keys in one round than both tables hold: exactly the surplus is
    refused, whichever keys lose the race."""
    rng = np.random.default_rng(R.SEED + 60)
    keys = [(0, int(k)) for k in _keys(rng, 64)]
    tx = probe.PeerTx(4, 4, GR)  # 16 + 16 entries
    m = Model(tx)
    (ret, ins), = tx.run(rounds=[keys])[0]
    m.check_round(keys, ret, ins)
    assert int((ret == 0).sum()) == 32 and int(ins.sum()) == 32
    assert tx.err[0] == probe.consts()["E_PEERTX"]
    assert m.check_tables() == 16
    m.check_lookups()
