"""The headers shared with the host, as the device compiler builds them:
include/gs_rng.h (Philox4x32-10 and the key helpers) against the Random123
vectors and the oracle's host compilation of the same header, include/gs_fp.h
(gs_quantum_div's __umul64hi branch, gs_add_ones / gs_add_ones_capped) against
Python's // and the serial `x += 1` loop.  Everything bit for bit, through the
probe (tests/probe.py).  CPU counterparts: tests/test_rng.py, tests/test_fp_steps.py."""
import numpy as np
import pytest

import probe
import select_ref as R

pytestmark = pytest.mark.gpu

F = 0xFFFFFFFF


def test_philox_known_answers_on_the_device():
    ctr = [[0, 0, 0, 0], [F, F, F, F], [0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344]]
    key = [[0, 0], [F, F], [0xA4093822, 0x299F31D0]]
    want = [[0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8], [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD],
            [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1]]
    assert probe.philox(ctr, key).tolist() == want


def _key_args():
    """[n][6] = seed, site, a, b, c, d: random words, the ids 2j and 2j + 1 of
    one block next to each other, id 0 and the largest id, all-zero / all-one words."""
    rng = np.random.default_rng(R.SEED + 20)
    n = 5000
    args = rng.integers(0, 1 << 32, (n, 6), dtype=np.uint64)
    args[:, 1] = rng.integers(1, 16, n)                   # GS_SITE_*
    args[::3, 2:4] = rng.integers(0, 100000, (len(args[::3]), 2))  # node / hop sized words
    args[::5, 4] = rng.integers(0, 20000, len(args[::5]))  # small message ids
    args[0] = 0
    args[1] = F
    args[2, 4] = 0
    args[3, 4] = F
    args[4, 4] = F - 1
    pair = np.repeat(args, 2, axis=0)                    # rows 2i, 2i + 1: the two ids of one block
    pair[0::2, 4] &= ~np.uint64(1)
    pair[1::2, 4] |= np.uint64(1)
    return pair.astype(np.uint32)


def test_keys_equal_the_host_compilation(olib):
    args = _key_args()
    assert len(args) == 10000
    k64, kmid, kx2, unit = probe.keys(args)
    rows = args.tolist()
    want64 = np.array([olib.orng_key64(*r) for r in rows], dtype=np.uint64)
    wantmid = np.array([olib.orng_key64_mid(*r) for r in rows], dtype=np.uint64)
    assert (k64 == want64).all()
    assert (kmid == wantmid).all()
    # gs_key64x2: half 0 is gs_key64, and its halves are the gs_key64_mid of ids 2c and 2c + 1
    assert (kx2[:, 0] == want64).all()
    small = args[:, 4] < (1 << 31)
    two = np.array([[olib.orng_key64_mid(r[0], r[1], r[2], r[3], 2 * r[4] + h, r[5]) for h in (0, 1)]
                    for r, ok in zip(rows, small) if ok], dtype=np.uint64)
    assert (kx2[small] == two).all()
    # ids 2j and 2j + 1 (adjacent rows) are the two halves of one block
    blk = np.array([[olib.orng_key64(r[0], r[1], r[2], r[3], r[4] >> 1, r[5])] for r in rows[0::2]], dtype=np.uint64)
    assert (kmid[0::2] == blk[:, 0]).all()
    mid_pair = probe.keys(np.concatenate([args[0::2, :4], (args[0::2, 4:5] >> 1), args[0::2, 5:]], axis=1))[2]
    assert (kmid[0::2] == mid_pair[:, 0]).all() and (kmid[1::2] == mid_pair[:, 1]).all()
    # gs_key_to_unit: the 53 high bits scaled by 2^-53 (exact in float64)
    want_unit = ((want64 >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)).view(np.uint64)
    assert (unit == want_unit).all()


QUANTA = [1, 2, 3, 7, 1000, 1000000000, 1000000007, 60000000000, (1 << 40) + 3, (1 << 62) + 1, (1 << 63) - 1]
I63 = (1 << 63) - 1


def test_quantum_div_on_the_device():
    """The case families of tests/test_fp_steps.py's QSRC, 4000 times per quantum."""
    rng = np.random.default_rng(R.SEED + 21)
    mt, q = [], []
    for quantum in QUANTA:
        g = [int(x) for x in rng.integers(0, 1 << 64, 4000, dtype=np.uint64)]
        h = [int(x) for x in rng.integers(0, 3, 4000)]
        for it in range(4000):
            fam = it % 4
            if fam == 0:
                t = g[it] >> 1                                  # any int64 >= 0
            elif fam == 1:
                t = g[it] % 100000000000000                     # hours of ns
            elif fam == 2:
                t = (g[it] % 1000) * quantum + h[it] - 1        # right around the multiples of q
            else:
                t = g[it] % 4096
            mt.append(min(max(t, 0), I63))
            q.append(quantum)
        for t in (0, 1, quantum - 1, quantum, quantum + 1, I63 - 1, I63, I63 // quantum * quantum,
                  I63 // quantum * quantum - 1):
            mt.append(min(max(t, 0), I63))
            q.append(quantum)
    magic = [(1 << 64) // x if x >= 2 else 0 for x in q]
    got = probe.quantum_div(mt, q, np.array(magic, dtype=np.uint64))
    want = np.array([t // x for t, x in zip(mt, q)], dtype=np.int64)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(mt[i], q[i], int(got[i]), int(want[i])) for i in bad[:10]]


def _serial_add_ones(x, n, cap=None):
    """n[i] steps of `x += 1` (each one rounded), with cap: stop at the first
    step above cap, which becomes cap.  Vectorised over the step count."""
    x = x.copy()
    live = np.ones(len(x), dtype=bool)
    for step in range(int(n.max())):
        live &= n > step
        if not live.any():
            break
        x[live] += 1.0
        if cap is not None:
            over = live & (x > cap)
            x[over] = cap[over]
            live &= ~over
    return x


def test_add_ones_on_the_device():
    """The five families of tests/test_fp_steps.py's SRC, n up to 5000."""
    rng = np.random.default_rng(R.SEED + 22)
    n_cases = 20000
    u = rng.random(n_cases)
    x = np.empty(n_cases)
    fam = np.arange(n_cases) % 5
    x[fam == 0] = u[fam == 0]                                             # [0, 1)
    x[fam == 1] = u[fam == 1] * 300.0                                      # decayed counters
    m = fam == 2                                                           # just below a power of two
    x[m] = np.ldexp(1.0, rng.integers(0, 40, m.sum())) - u[m] * 4.0
    x[fam == 3] = u[fam == 3] * 1e15                                       # large magnitudes
    m = fam == 4                                                           # decayed: d * 0.9^k
    d = u[m] * 50.0
    for k, cnt in enumerate(rng.integers(0, 30, m.sum())):
        for _ in range(cnt):
            d[k] *= 0.9
    x[m] = d
    x = np.maximum(x, 0.0)
    steps = np.where(np.arange(n_cases) % 7 == 0, rng.integers(0, 5000, n_cases), rng.integers(0, 300, n_cases))
    steps[:5] = (0, 1, 4999, 5000, 300)
    cap = rng.random(n_cases) * 400.0
    plain, capped = probe.add_ones(x, steps, cap)
    assert (plain.view(np.uint64) == _serial_add_ones(x, steps).view(np.uint64)).all()
    assert (capped.view(np.uint64) == _serial_add_ones(x, steps, cap).view(np.uint64)).all()
