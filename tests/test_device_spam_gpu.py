"""The IWANT spammers' peertx counters, a nibble per (in-edge row, slot) in
spamCnt: spam_incr (csrc/gs_device.h) and the clear of recycled slots in
k_retire (csrc/gs_kernels.h), launched alone through the probe against the
nibble array of tests/tables_ref.py.  spam_incr returns min(old + 1, GR + 2)
and stores min(old + 1, GR + 1); the nibble peaks at GR + 2 <= 15 between its
add and the take-back, so no carry may reach the next nibble or word (the host
refuses GR >= 14).  Bit-exact."""
import numpy as np
import pytest

import probe
import tables_ref as T

pytestmark = pytest.mark.gpu

S = 128  # 16 words of 8 nibbles per row
WORD = 5  # the word under test, words on both sides


@pytest.mark.parametrize("gr", [3, 13])
def test_every_nibble_from_zero_past_the_cap(gr):
    """A row per (nibble, neighbours' value): the nibble goes from 0 past
    GR + 1 one request per round while the other seven nibbles of its word sit
    at 0, at GR + 1 or mid-range, between a word of ones and a word of zeros."""
    held = [0, gr + 1, (gr + 1) // 2]
    rows = [(j, h) for j in range(8) for h in held]
    m = T.SpamModel(len(rows), S, gr)
    for r, (j, h) in enumerate(rows):
        m.nib[r, 8 * WORD:8 * WORD + 8] = h
        m.nib[r, 8 * WORD + j] = 0
        m.nib[r, 8 * (WORD - 1):8 * WORD] = 15
    cnt = m.words()
    assert (cnt[:, WORD - 1] == 0xFFFFFFFF).all() and (cnt[:, WORD + 1] == 0).all()
    round_ = [(r, 8 * WORD + j) for r, (j, _) in enumerate(rows)]
    for i in range(gr + 4):
        ret, = probe.spam(S, gr, cnt, rounds=[round_])
        assert ret.tolist() == [min(i + 1, gr + 2)] * len(rows)
        assert [m.incr(r, s) for r, s in round_] == ret.tolist()
        assert (cnt == m.words()).all(), f"after request {i + 1}"
    assert (m.nib[np.arange(len(rows)), [s for _, s in round_]] == gr + 1).all()


@pytest.mark.parametrize("gr", [3, 13])
def test_concurrent_requests_in_one_word(gr):
    """All eight nibbles of a word, and of its neighbours, counted in one
    launch, round after round until every one is past the cap; rounds in one
    call too."""
    rng = np.random.default_rng(T.SEED + 120 + gr)
    m = T.SpamModel(4, S, gr)
    cnt = m.words()
    rounds = []
    for i in range(gr + 5):
        pick = rng.random((4, S)) < (1.0 if i % 3 == 0 else 0.8)
        pick[3, 64:] = False  # a part of the table nobody asks for
        rounds.append([(int(r), int(s)) for r, s in zip(*np.nonzero(pick))])
    half = len(rounds) // 2
    for part in (rounds[:half], rounds[half:]):
        rets = probe.spam(S, gr, cnt, rounds=part)
        for round_, ret in zip(part, rets):
            assert [m.incr(r, s) for r, s in round_] == ret.tolist()
        assert (cnt == m.words()).all()
    assert m.nib.max() == gr + 1 and (m.nib[3, 64:] == 0).all() and (m.nib[:3] > 0).all()


def _retire_setup(gr, rng, s=256):
    m = T.SpamModel(6, s, gr)
    m.nib[:] = rng.integers(1, gr + 2, m.nib.shape)  # every nibble non-zero: a clear shows
    rowptr = [0, 3, 5, 7, 7]  # node 3 has no edge
    spam_row = [1, -1, 2, -1, -1, 4, 3]  # rows 0 and 5: edges of nodes that are not here
    pubmask = np.array([0x8000000000010081, 0xFFFFFFFFFFFFFFFF, 0x00FF00000F000001 | (1 << 63), 0], dtype=np.uint64)
    words = [0, 2, 3]  # word 1 is not listed, whatever its mask; word 3 is listed with an empty mask
    pmask_row = [1, -1, 0, -1]
    pmask = rng.integers(1, 1 << 63, (3, s)).astype(np.uint64)  # row 2: no node's
    return m, rowptr, spam_row, pubmask, words, pmask_row, pmask


@pytest.mark.parametrize("gr", [3, 13])
@pytest.mark.parametrize("cur", [0, 1])
def test_retire_clears_exactly_the_recycled_slots(gr, cur):
    rng = np.random.default_rng(T.SEED + 130 + gr)
    m, rowptr, spam_row, pubmask, words, pmask_row, pmask = _retire_setup(gr, rng)
    cnt, before, pm_before = m.words(), m.nib.copy(), pmask.copy()
    probe.spam(256, gr, cnt, retire=dict(cur=cur, rowptr=rowptr, spam_row=spam_row, pubmask=pubmask, words=words,
                                         pmask_row=pmask_row, pmask=pmask))
    m.retire(rowptr, spam_row, pubmask, words)
    assert (cnt == m.words()).all()
    # what the model cleared is what the issue says: the nibbles of pubmask's
    # bits, in the listed words, in the rows of the nodes' own spammer edges
    bits = np.zeros(256, dtype=bool)
    for w in words:
        bits[64 * w:64 * w + 64] = [(int(pubmask[w]) >> b) & 1 for b in range(64)]
    assert bits.sum() == 4 + 14 and not bits[64:128].any() and not bits[192:].any()
    for r in range(6):
        if r in (1, 2, 3, 4):
            assert (m.nib[r, bits] == 0).all() and (m.nib[r, ~bits] == before[r, ~bits]).all()
        else:
            assert (m.nib[r] == before[r]).all()
    want = pm_before.copy()
    want[0, bits] = 0
    want[1, bits] = 0
    assert (pmask == want).all() and (pmask[2] == pm_before[2]).all()


def test_retire_halves_alone():
    """No spammer edges (spamRow == nullptr): only pmask; no pmask rows: only spamCnt."""
    gr = 3
    rng = np.random.default_rng(T.SEED + 140)
    m, rowptr, spam_row, pubmask, words, pmask_row, pmask = _retire_setup(gr, rng)
    cnt, pm_before = m.words(), pmask.copy()
    probe.spam(256, gr, cnt, retire=dict(cur=0, rowptr=rowptr, spam_row=None, pubmask=pubmask, words=words,
                                         pmask_row=pmask_row, pmask=pmask))
    assert (cnt == m.words()).all() and (pmask != pm_before).any() and (pmask[2] == pm_before[2]).all()
    pmask[:] = pm_before
    probe.spam(256, gr, cnt, retire=dict(cur=1, rowptr=rowptr, spam_row=spam_row, pubmask=pubmask, words=words,
                                         pmask_row=None, pmask=None))
    m.retire(rowptr, spam_row, pubmask, words)
    assert (cnt == m.words()).all() and (pmask == pm_before).all()


def test_increments_after_a_retire_start_from_zero():
    gr = 3
    rng = np.random.default_rng(T.SEED + 150)
    m, rowptr, spam_row, pubmask, words, _, _ = _retire_setup(gr, rng)
    cnt = m.words()
    probe.spam(256, gr, cnt, retire=dict(cur=0, rowptr=rowptr, spam_row=spam_row, pubmask=pubmask, words=words))
    m.retire(rowptr, spam_row, pubmask, words)
    round_ = [(r, s) for r in range(6) for s in (0, 7, 16, 63, 64, 128, 191, 255)]
    rets = probe.spam(256, gr, cnt, rounds=[round_] * 2)
    for ret in rets:
        assert [m.incr(r, s) for r, s in round_] == ret.tolist()
    assert (cnt == m.words()).all()
    assert rets[0][8] == 1 and rets[0][11] == 1 and rets[1][8] == 2  # row 1's cleared slots count from 1 again


def test_entry_point_refuses_out_of_range_requests():
    cnt = np.zeros((2, S // 8), dtype=np.uint32)
    for bad in ([(2, 0)], [(0, S)], [(0, -1)]):
        with pytest.raises(probe.ProbeError, match="HIP error 1$"):
            probe.spam(S, 3, cnt, rounds=[bad])
    with pytest.raises(probe.ProbeError, match="HIP error 1$"):
        probe.spam(S, 14, cnt, rounds=[[(0, 0)]])
    with pytest.raises(probe.ProbeError, match="HIP error 1$"):
        probe.spam(S, 3, cnt, retire=dict(cur=0, rowptr=[0, 1], spam_row=[2], pubmask=[0, 0], words=[0]))
    with pytest.raises(probe.ProbeError, match="HIP error 1$"):
        probe.spam(S, 3, cnt, retire=dict(cur=0, rowptr=[0, 1], spam_row=[0], pubmask=[0, 0], words=[2]))
    assert not cnt.any()
