"""The wave selects of csrc/gs_device.h launched alone through the probe
(tests/probe.py) on the case tables of tests/select_ref.py: select_k,
select_k_half and grp_select<true/false> against "the k smallest (key, lane)"
as ballot masks, select_kth and select_kth_est against "the k-th smallest
(key, id)", bit for bit.  tests/test_select_ref.py asserts on the CPU that
these tables reach every branch of the device code.  Domain: ids >= 0 and
distinct: every call site passes message ids, which gs_publish_ex hands out
as sequence numbers from 0, so no tie group with negative ids is included and
the signed / unsigned id compare of the two selects is not exercised below zero."""
import numpy as np
import pytest

import probe
import select_ref as R

pytestmark = pytest.mark.gpu


def _wave_arrays(cases, half):
    cand = np.stack([c[1] for c in cases]).astype(np.uint8)
    key = np.stack([c[2] for c in cases])
    if half:
        k = np.stack([np.repeat(np.array([c[3], c[4]], dtype=np.int32), 32) for c in cases])
    else:
        k = np.stack([np.full(64, c[3], dtype=np.int32) for c in cases])
    return cand, key, k


@pytest.mark.parametrize("mode", [probe.MODE_SELECT_K, probe.MODE_GRP_WAVE], ids=["select_k", "grp_select_wave"])
def test_select_k(mode):
    cases = R.select_k_cases()
    masks = probe.select_k(mode, *_wave_arrays(cases, False))
    bad = R.check_select_k(cases, masks)
    assert not bad, f"{len(bad)} of {len(cases)} cases differ:\n" + "\n".join(bad[:20])


@pytest.mark.parametrize("mode", [probe.MODE_HALF, probe.MODE_GRP_PAIR], ids=["select_k_half", "grp_select_pair"])
def test_select_k_half(mode):
    cases = R.select_k_half_cases()
    masks = probe.select_k(mode, *_wave_arrays(cases, True))
    bad = R.check_select_k(cases, masks, half="both")
    assert not bad, f"{len(bad)} of {len(cases)} cases differ:\n" + "\n".join(bad[:20])


def test_select_k_half_agrees_with_select_k_on_each_half():
    """A half-wave select equals the full-wave select of that half's candidates alone."""
    cases = R.select_k_half_cases()
    cand, key, k = _wave_arrays(cases, True)
    both = probe.select_k(probe.MODE_HALF, cand, key, k)
    for h, sh in ((0, 0), (1, 32)):
        only = cand.copy()
        only[:, 32 * (1 - h):32 * (1 - h) + 32] = 0
        kk = np.repeat(k[:, 32 * h:32 * h + 1], 64, axis=1)
        full = probe.select_k(probe.MODE_SELECT_K, only, key, kk)
        assert ((both >> np.uint64(sh)) & np.uint64(0xFFFFFFFF) == full >> np.uint64(sh)).all()


@pytest.mark.parametrize("mode,half", [(probe.MODE_HALF_IF_LO, "lo"), (probe.MODE_HALF_IF_HI, "hi")])
def test_select_k_half_under_divergence(mode, half):
    """Called inside `if (lane < 32)` / `if (lane >= 32)`: the executing half
    selects as in the full call, the idle half contributes nothing."""
    cases = R.select_k_half_cases()
    arrays = _wave_arrays(cases, True)
    masks = probe.select_k(mode, *arrays)
    bad = R.check_select_k(cases, masks, half=half)
    assert not bad, f"{len(bad)} of {len(cases)} cases differ:\n" + "\n".join(bad[:20])
    full = probe.select_k(probe.MODE_HALF, *arrays)
    keep = np.uint64(0xFFFFFFFF if half == "lo" else 0xFFFFFFFF00000000)
    assert (masks == full & keep).all()


def test_select_kth():
    cases = R.select_kth_cases()
    assert max(len(c["keys"]) for c in cases) == 8192 and min(len(c["keys"]) for c in cases) == 1
    K, M = probe.select_kth(cases)
    bad = R.check_select_kth(cases, K, M)
    assert not bad, f"{len(bad)} differences in {len(cases)} cases:\n" + "\n".join(bad[:20])


def test_select_kth_est():
    c = probe.consts()
    cases = R.select_kth_est_cases(c["GS_SEL_WIN"], c["GS_SEL_CAP"])
    K, M = probe.select_kth(cases, est=True)
    bad = R.check_select_kth(cases, K, M, est=True)
    assert not bad, f"{len(bad)} differences in {len(cases)} cases:\n" + "\n".join(bad[:20])


def test_select_kth_est_equals_select_kth_on_both_tables():
    """The estimate is an optimisation only: both selects give the same (K, M)
    on every case with k < n (at k >= n the estimate answers "everything"),
    whichever path the estimate takes."""
    c = probe.consts()
    cases = [x for x in R.select_kth_cases() + R.select_kth_est_cases(c["GS_SEL_WIN"], c["GS_SEL_CAP"])
             if x["k"] < len(x["keys"])]
    K0, M0 = probe.select_kth(cases)
    K1, M1 = probe.select_kth(cases, est=True)
    bad = [x["name"] for x, a, b, p, q in zip(cases, K0, K1, M0, M1) if (a, p) != (b, q)]
    assert not bad, bad
    assert not R.check_select_kth(cases, K1, M1, est=True)
