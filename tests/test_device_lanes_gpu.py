"""The lane primitives of csrc/gs_device.h, gs_kernels.h and gs_kernels_ctl.h
launched alone through the probe (tests/probe.py), one case per wave, against
plain numpy references, bit for bit: the DPP prefix sum and its users, the
wave sums, lane_rank, the half-wave swaps, the lane reads, the 64 x 64 bit
transpose, kth_bit, item_sender and the two layouts of dlt_get / dlt_put."""
import itertools

import numpy as np
import pytest

import probe
import select_ref as R

pytestmark = pytest.mark.gpu

EDGE_LANES = (0, 15, 16, 31, 32, 47, 48, 63)  # around the DPP row boundaries


def _i32(a):
    return np.asarray(a, dtype=np.uint64).astype(np.uint32).view(np.int32)


def _u(a):
    """int32 operands as the probe takes them: the low 32 bits of a uint64."""
    return np.asarray(a, dtype=np.int32).view(np.uint32).astype(np.uint64)


@pytest.fixture(scope="module")
def int_rows():
    rng = np.random.default_rng(R.SEED + 10)
    rows = [rng.integers(-1000, 1000, 64), rng.integers(0, 5, 64), np.ones(64), np.zeros(64),
            np.full(64, (2**31 - 1) // 64), rng.integers((2**31 - 1) // 64 - 100, (2**31 - 1) // 64 + 1, 64)]
    for lane in EDGE_LANES:
        for v in (1, -7, 123456):
            r = np.zeros(64)
            r[lane] = v
            rows.append(r)
    return np.stack(rows).astype(np.int32)


def test_wave_incl_sum(int_rows):
    got, _ = probe.lanes(probe.OP_INCL_SUM, _u(int_rows))
    assert (_i32(got) == np.cumsum(int_rows, axis=1, dtype=np.int64).astype(np.int32)).all()
    bad = R.check_incl_sum(int_rows, _i32(got))
    assert not bad, "\n".join(bad[:20])


def test_lane_prefix_wave_last_wave_sum_int(int_rows):
    incl = np.cumsum(int_rows, axis=1, dtype=np.int64).astype(np.int32)
    total = np.repeat(incl[:, 63:], 64, axis=1)
    pre, tot = probe.lanes(probe.OP_LANE_PREFIX, _u(int_rows))
    assert (_i32(pre) == incl - int_rows).all() and (_i32(tot) == total).all()
    last, _ = probe.lanes(probe.OP_WAVE_LAST, _u(int_rows))
    assert (_i32(last) == np.repeat(int_rows[:, 63:], 64, axis=1)).all()
    s, _ = probe.lanes(probe.OP_SUM_INT, _u(int_rows))
    assert (_i32(s) == total).all()


def test_wave_sum_ll(int_rows):
    rng = np.random.default_rng(R.SEED + 11)
    rows = np.concatenate([int_rows.astype(np.int64), rng.integers(-2**56, 2**56, (8, 64)),
                           np.full((1, 64), (2**63 - 1) // 64)])
    got, _ = probe.lanes(probe.OP_SUM_LL, rows.view(np.uint64))
    want = np.repeat(rows.sum(axis=1, dtype=np.int64)[:, None], 64, axis=1)
    assert (got.view(np.int64) == want).all()


def test_lane_rank():
    rng = np.random.default_rng(R.SEED + 12)
    masks = [0, R.U64, 0xFFFFFFFF, 0xFFFFFFFF00000000, 0x8000000080000000] + [1 << b for b in range(64)]
    masks += [int(x) for x in rng.integers(0, 1 << 64, 40, dtype=np.uint64)]
    a = np.repeat(np.array(masks, dtype=np.uint64)[:, None], 64, axis=1)
    got, _ = probe.lanes(probe.OP_LANE_RANK, a)
    want = np.array([[bin(m & ((1 << lane) - 1)).count("1") for lane in range(64)] for m in masks])
    assert (got == want).all()


def _f64_specials():
    pats = [0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,  # +-0, +-inf
            0x7FF8000000000000, 0xFFF8000000000001, 0x7FF0000000000001, 0x7FF4DEADBEEF1234,  # quiet / signalling NaNs
            0xFFF7FFFFFFFFFFFF, 0x0000000000000001, 0x800FFFFFFFFFFFFF, 0x3FF0000000000000]  # payloads, denormals, 1.0
    return np.array(pats, dtype=np.uint64)


def test_xor32():
    rng = np.random.default_rng(R.SEED + 13)
    rows = rng.integers(0, 1 << 64, (6, 64), dtype=np.uint64)
    sp = _f64_specials()
    rows[1, :len(sp)] = sp          # specials in the low half, random partners above
    rows[2, 64 - len(sp):] = sp     # and the other way round
    rows[3] = np.resize(sp, 64)     # specials against specials
    rows[4] = np.arange(64, dtype=np.uint64) * np.uint64(0x0101010101010101)
    swapped = np.concatenate([rows[:, 32:], rows[:, :32]], axis=1)  # lane l reads lane l ^ 32
    got, _ = probe.lanes(probe.OP_XOR32_U64, rows)
    assert (got == swapped).all()
    got, _ = probe.lanes(probe.OP_XOR32_F64, rows)
    assert (got == swapped).all()  # bit patterns: -0.0, infinities and NaN payloads survive
    got, _ = probe.lanes(probe.OP_XOR32_U32, rows)
    assert (got == swapped & np.uint64(0xFFFFFFFF)).all()


def test_lane_get_every_source_lane():
    rng = np.random.default_rng(R.SEED + 14)
    row = rng.integers(0, 1 << 64, 64, dtype=np.uint64)
    sp = _f64_specials()
    row[:len(sp)] = sp
    a = np.repeat(row[None, :], 64, axis=0)  # case i reads lane i
    b = np.repeat(np.arange(64, dtype=np.int32)[:, None], 64, axis=1)
    want = np.repeat(row[:, None], 64, axis=1)
    for op in (probe.OP_LANE_GET64, probe.OP_LANE_GETF):
        got, _ = probe.lanes(op, a, b)
        assert (got == want).all()


def _transpose_rows():
    rng = np.random.default_rng(R.SEED + 15)
    rows = [np.array([1 << j for j in range(64)], dtype=np.uint64),        # identity
            np.array([1 << (63 - j) for j in range(64)], dtype=np.uint64),  # anti-diagonal
            np.full(64, R.U64, dtype=np.uint64), np.zeros(64, dtype=np.uint64)]
    edges = (0, 1, 3, 4, 7, 8, 15, 16, 31, 32, 47, 48, 62, 63)  # corners and the butterfly's block-swap boundaries
    for j, t in itertools.product(edges, edges):
        r = np.zeros(64, dtype=np.uint64)
        r[j] = np.uint64(1 << t)
        rows.append(r)
    rows += [rng.integers(0, 1 << 64, 64, dtype=np.uint64) for _ in range(12)]
    rows.append(np.where(rng.integers(0, 8, 64) == 0, rng.integers(0, 1 << 64, 64, dtype=np.uint64), 0).astype(np.uint64))
    return np.stack(rows)


def test_wave_transpose64():
    rows = _transpose_rows()
    got, _ = probe.lanes(probe.OP_TRANSPOSE, rows)
    bad = R.check_transpose(rows, got)
    assert not bad, f"{len(bad)} lanes differ:\n" + "\n".join(bad[:20])
    twice, _ = probe.lanes(probe.OP_TRANSPOSE2, rows)
    assert (twice == rows).all()


def test_kth_bit():
    rng = np.random.default_rng(R.SEED + 16)
    masks = [R.U64, 0xFFFFFFFF00000000, 0xAAAAAAAAAAAAAAAA, 0x8000000000000001, 0x0001000100010001]
    masks += [1 << b for b in (0, 1, 31, 32, 62, 63)]
    masks += [int(x) for x in rng.integers(0, 1 << 64, 6, dtype=np.uint64)]
    masks += [int(x & y & z) for x, y, z in rng.integers(0, 1 << 64, (6, 3), dtype=np.uint64)]  # sparse
    a, b, want = [], [], []
    for m in masks:  # every k of every mask, padded to whole waves with k = 0
        pos = [i for i in range(64) if (m >> i) & 1]
        for k, p in enumerate(pos):
            a.append(m), b.append(k), want.append(p)
    pad = -len(a) % 64
    a += [1] * pad
    b += [0] * pad
    want += [0] * pad
    got, _ = probe.lanes(probe.OP_KTH_BIT, np.array(a, dtype=np.uint64), np.array(b, dtype=np.int32))
    assert (_i32(got).reshape(-1) == np.array(want)).all()


def test_item_sender():
    rng = np.random.default_rng(R.SEED + 17)
    counts = [rng.integers(0, 6, 64), np.ones(64), rng.integers(0, 2, 64) * rng.integers(1, 40, 64)]
    for zeros in (slice(0, 9), slice(20, 45), slice(50, 64), slice(0, 63), slice(1, 64)):
        c = rng.integers(1, 5, 64)
        c[zeros] = 0  # a run of senders without items at the front / in the middle / at the end
        counts.append(c)
    c = np.zeros(64)
    c[[0, 31, 63]] = (1, 200, 3)
    counts.append(c)
    counts = np.stack(counts).astype(np.int32)
    n_items = counts.sum(axis=1).astype(np.int32)
    s_it = (np.cumsum(counts, axis=1) - counts).astype(np.int32)  # exclusive prefix
    sender, within = probe.item_sender(s_it, n_items)
    for c in range(len(counts)):
        want_s = np.repeat(np.arange(64), counts[c])
        want_k = np.concatenate([np.arange(x) for x in counts[c]]) if n_items[c] else np.zeros(0)
        assert (sender[c, :n_items[c]] == want_s).all(), c
        assert (within[c, :n_items[c]] == want_k).all(), c


@pytest.mark.parametrize("narrow", [True, False], ids=["narrow", "wide"])
def test_dlt_round_trip(narrow):
    vals = (0, 1, 255) if narrow else (0, 1, 255, 256, 65535)
    q = np.array([f | (m << 16) for f, m in itertools.product(vals, vals)], dtype=np.uint32)
    assert (probe.dlt_round_trip(q, narrow) == q).all()
