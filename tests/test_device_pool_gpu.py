"""pool_take (csrc/gs_device.h) launched alone through the probe: lane 0 of
every block asks for ids of the hop's arena, whose segment is split into
poolSub sub-arenas with a bump counter each.  The first sub-arena tried is
block % poolSub & poolS0Mask; a full one hands the request on to the next, and
only a request no sub-arena can take is refused (~0, E_POOL).  Bit-exact: the
ids handed out are disjoint, never straddle two sub-arenas, and with unit
requests the whole segment is used before anything is refused.  (A request
of several ids that a sub-arena cannot take leaves that sub-arena's counter
past its cap, so with mixed sizes the last few ids of a sub-arena may stay
unused: the tests of mixed sizes claim only what holds whatever the order.)"""
import numpy as np
import pytest

import probe
import tables_ref as T

pytestmark = pytest.mark.gpu

NONE = (1 << 64) - 1
BASE0 = 1000  # a rank's segment does not start at 0
CAP = 5


def _spilled(sub, mask, out, cap=CAP, base0=BASE0):
    """Requests granted by another sub-arena than the first one they tried."""
    return sum(1 for b, g in enumerate(out.tolist()) if g != NONE and (g - base0) // cap != (b % sub) & mask)


@pytest.mark.parametrize("cur", [0, 1])
@pytest.mark.parametrize("mask_all", [True, False], ids=["spread", "all_start_at_0"])
@pytest.mark.parametrize("sub", [1, 2, 8])
def test_unit_requests_use_the_whole_segment(sub, mask_all, cur):
    e_pool = probe.consts()["E_POOL"]
    mask = sub - 1 if mask_all else 0
    total = sub * CAP
    segment = list(range(BASE0, BASE0 + total))
    # fewer than the segment holds, exactly as many, one more
    for n_blocks in (total - 1, total, total + 1):
        n = np.ones(n_blocks, dtype=np.uint64)
        out, cnt, err = probe.pool_take(sub, mask, CAP, BASE0, cur, n)
        granted, refused = T.check_pool(sub, CAP, BASE0, n, out, cnt[cur], err, e_pool)
        ids = sorted(g for g in out.tolist() if g != NONE)
        if n_blocks <= total:
            assert refused == 0 and err == 0 and len(set(ids)) == n_blocks and set(ids) <= set(segment)
        else:
            assert refused == 1 and err == e_pool and ids == segment  # still a permutation of the segment
        if n_blocks == total:
            assert ids == segment
        assert not cnt[1 - cur].any()  # the other hop's counters
        if not mask_all and sub > 1 and n_blocks >= total:
            assert _spilled(sub, mask, out) == total - CAP  # everything past sub-arena 0's share was handed on
        if mask_all and n_blocks <= total:
            assert _spilled(sub, mask, out) == 0  # blocks spread evenly: nobody had to


@pytest.mark.parametrize("sub", [1, 2, 8])
def test_skewed_blocks_spill_to_the_next_sub_arenas(sub):
    """With the spreading mask, blocks that all map to one sub-arena
    (blockIdx % poolSub == 0 only asks) still get the whole segment."""
    e_pool = probe.consts()["E_POOL"]
    total = sub * CAP
    n = np.zeros(total * sub, dtype=np.uint64)
    n[::sub] = 1  # only the blocks whose first sub-arena is 0 ask; the others make no call
    out, cnt, err = probe.pool_take(sub, sub - 1, CAP, BASE0, 0, n)
    T.check_pool(sub, CAP, BASE0, n, out, cnt[0], err, e_pool)
    assert err == 0 and sorted(out[::sub].tolist()) == list(range(BASE0, BASE0 + total))
    assert _spilled(sub, sub - 1, np.where(n != 0, out, np.uint64(NONE))) == total - CAP


@pytest.mark.parametrize("load", [0.7, 1.5], ids=["fits", "overloaded"])
@pytest.mark.parametrize("sub", [1, 2, 8])
def test_mixed_requests_stay_disjoint_inside_one_sub_arena(sub, load):
    e_pool = probe.consts()["E_POOL"]
    rng = np.random.default_rng(T.SEED + 160 + sub)
    cap = 16
    n = []
    while sum(n) < load * sub * cap:
        n.append(int(rng.integers(1, 8)))
    if load < 1:
        n.pop()  # (below the load, so that one sub-arena alone takes it all)
    n = np.array(n, dtype=np.uint64)
    spills = 0
    for mask in sorted({sub - 1, 0}):
        out, cnt, err = probe.pool_take(sub, mask, cap, BASE0, 1, n)
        granted, refused = T.check_pool(sub, cap, BASE0, n, out, cnt[1], err, e_pool)
        assert granted + refused == n.size
        spills += _spilled(sub, mask, out, cap)
        if load > 1:
            assert refused > 0 and err == e_pool
        elif sub == 1:
            assert refused == 0 and err == 0
    if sub > 1 and load > 1:
        assert spills > 0


def test_entry_point_refuses_bad_arguments():
    one = np.ones(4, dtype=np.uint64)
    for args in ((3, 0, CAP, 0, 0), (2, 1, -1, 0, 0), (2, 1, CAP, 0, 2), (128, 0, CAP, 0, 0)):
        with pytest.raises(probe.ProbeError, match="HIP error 1$"):
            probe.pool_take(*args, one)
    with pytest.raises(probe.ProbeError, match="HIP error 1$"):
        probe.pool_take(2, 1, CAP, 0, 0, np.array([1 << 40], dtype=np.uint64))
