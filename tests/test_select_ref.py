"""tests/select_ref.py on the CPU: its references against an independent brute
force (sorted Python tuples), the case tables against the path models (every
branch of select_k, select_kth and select_kth_est is reached by construction;
the counts are printed), and each checker against a deliberately wrong answer."""
import collections

import numpy as np
import pytest

import probe
import select_ref as R


@pytest.fixture(scope="module")
def consts():
    return probe.consts()  # host-only call: needs the built probe library, no GPU


@pytest.fixture(scope="module")
def est_cases(consts):
    return R.select_kth_est_cases(consts["GS_SEL_WIN"], consts["GS_SEL_CAP"])


# ------------------------------------------------ references vs. brute force
def _brute_select_k(cand, key, k):
    lanes = sorted((int(key[l]), l) for l in range(len(cand)) if cand[l])
    if 0 < k < len(lanes):
        lanes = lanes[:k]
    return sum(1 << l for _, l in lanes)


def _brute_kth(keys, ids, k):
    pairs = sorted((int(a), int(b)) for a, b in zip(keys, ids))
    return pairs[k - 1] if 1 <= k <= len(pairs) else (R.U64, R.I64_MAX)


def test_select_k_reference_equals_brute_force():
    cases = R.select_k_cases()
    assert len(cases) > 500
    for name, cand, key, k in cases:
        assert R.ref_select_k(cand, key, k) == _brute_select_k(cand, key, k), name


def test_select_k_half_reference_equals_brute_force():
    for name, cand, key, k_lo, k_hi in R.select_k_half_cases():
        want = _brute_select_k(cand[:32], key[:32], k_lo) | (_brute_select_k(cand[32:], key[32:], k_hi) << 32)
        assert R.ref_select_k_half(cand, key, k_lo, k_hi) == want, name


def test_select_kth_reference_equals_brute_force(est_cases):
    for c in R.select_kth_cases() + est_cases:
        assert R.ref_select_kth(c["keys"], c["ids"], c["k"]) == _brute_kth(c["keys"], c["ids"], c["k"]), c["name"]


def test_case_tables_stay_in_the_domain(est_cases):
    """ids distinct and >= 0, every lane share inside its case, n as each() yields."""
    for c in R.select_kth_cases() + est_cases:
        assert len(set(c["ids"].tolist())) == len(c["ids"]) and (c["ids"] >= 0).all(), c["name"]
        lo = c["lane_off"]
        assert lo.shape == (65,) and lo[0] == 0 and lo[64] == len(c["keys"]) and (np.diff(lo) >= 0).all(), c["name"]
        assert c["n"] == len(c["keys"]) and c["k"] >= 1, c["name"]
    shares = np.concatenate([np.diff(c["lane_off"]) for c in R.select_kth_cases()])
    assert (shares == 0).any() and (shares > 1).any()


# ---------------------------------------------------------- coverage (models)
def test_select_kth_est_cases_cover_every_path(consts, est_cases):
    win, cap = consts["GS_SEL_WIN"], consts["GS_SEL_CAP"]
    models = [R.model_select_kth_est(c["keys"], c["k"], c["n"], win, cap) for c in est_cases]
    paths = collections.Counter(m["path"] for m in models)
    rest = [m for m in models if m["path"] != "all"]
    extra = {
        "overflow nc == cap + 1": sum(m["path"] == "overflow" and m["nc"] == cap + 1 for m in rest),
        "fast nc == cap": sum(m["path"] == "fast" and m["nc"] == cap for m in rest),
        "fast lo == 0 (clipped)": sum(m["path"] == "fast" and m["est"] - win < 0 for m in rest),
        "fast hi == 255 (clipped)": sum(m["path"] == "fast" and m["est"] + win > 255 for m in rest),
    }
    print("select_kth_est paths:", dict(paths), extra)
    for p in ("all", "fast", "miss_low", "miss_high", "overflow"):
        assert paths[p] >= 1, p
    for name, n in extra.items():
        assert n >= 1, name
    # what the fallbacks hand to select_kth is covered there too
    fb = collections.Counter(R.model_select_kth(c["keys"], c["k"])[0]
                             for c, m in zip(est_cases, models) if m["path"] in ("miss_low", "miss_high", "overflow"))
    print("select_kth_est fallbacks leave select_kth through:", dict(fb))


def test_select_kth_cases_cover_every_exit():
    exits = [R.model_select_kth(c["keys"], c["k"]) for c in R.select_kth_cases()]
    by_pass = collections.Counter(e[1] for e in exits if e[0] == "pass")
    ties = collections.Counter("tie loop of 1" if e[1] == 1 else "tie loop > 1" for e in exits if e[0] == "tie")
    above = sum(e[0] == "above" for e in exits)
    print("select_kth exits by pass:", dict(sorted(by_pass.items())), dict(ties), {"k above count": above},
          {"longest tie loop": max(e[1] for e in exits if e[0] == "tie")})
    for p in range(8):  # pass 7, every middle pass, pass 0
        assert by_pass[p] >= 1, p
    assert ties["tie loop of 1"] >= 1 and ties["tie loop > 1"] >= 1 and above >= 1
    assert max(e[1] for e in exits if e[0] == "tie") >= 200


def _select_k_coverage(models, label):
    live = [m for m in models if not m["early"]]
    count = {
        "early (k <= 0 or n <= k)": len(models) - len(live),
        "ends at bit 63": sum(m["end_bit"] == 63 for m in live),
        "ends at a middle bit": sum(m["end_bit"] is not None and 0 < m["end_bit"] < 63 for m in live),
        "ends at bit 0": sum(m["end_bit"] == 0 for m in live),
        "tie loop": sum(m["tie_len"] > 0 for m in live),
        "tie loop > 1": sum(m["tie_len"] > 1 for m in live),
        "n == need exit": sum(m["exit"] == "n_eq_need" for m in live),
    }
    print(f"{label} paths:", count)
    for name in ("early (k <= 0 or n <= k)", "ends at bit 63", "ends at a middle bit", "ends at bit 0", "tie loop",
                 "tie loop > 1"):
        assert count[name] >= 1, (label, name)
    return live, count


def test_select_k_cases_cover_every_path():
    live, count = _select_k_coverage([R.model_select_k(c, key, k) for _, c, key, k in R.select_k_cases()], "select_k")
    # The `n == need` exit cannot be taken by any input: the loop starts with
    # n > need (n > k), taking the zeros lowers both by nz, and narrowing to the
    # zeros happens only when nz > need; so n > need after every bit.  The model
    # checks that invariant on every case instead of a case that cannot exist.
    assert count["n == need exit"] == 0 and all(m["min_slack"] >= 1 for m in live)


def test_select_k_half_cases_cover_every_path_in_each_half():
    for h in (0, 1):
        models = [R.model_select_k(c[32 * h:32 * h + 32], key[32 * h:32 * h + 32], (k_lo, k_hi)[h])
                  for _, c, key, k_lo, k_hi in R.select_k_half_cases()]
        live, count = _select_k_coverage(models, f"select_k_half lanes {32 * h}..{32 * h + 31}")
        assert count["n == need exit"] == 0 and all(m["min_slack"] >= 1 for m in live)
    cases = R.select_k_half_cases()
    assert any(k_lo != k_hi for *_, k_lo, k_hi in cases)
    assert any(not c[:32].any() and c[32:].any() for _, c, *_ in cases)
    assert any(c[:32].any() and not c[32:].any() for _, c, *_ in cases)


# -------------------------------------------------------------- checker teeth
def _tied_case():
    keys = np.array([7, 7, 7, 3, 9], dtype=np.uint64)
    ids = np.array([40, 10, 30, 99, 5], dtype=np.int64)
    return {"name": "tied", "keys": keys, "ids": ids, "k": 3, "n": 5, "lane_off": np.zeros(65, dtype=np.int32)}


def test_kth_checker_rejects_a_rank_off_by_one_and_a_wrong_tied_id():
    c = _tied_case()  # sorted: (3,99) (7,10) (7,30) (7,40) (9,5): the 3rd is (7, 30)
    assert R.check_select_kth([c], [7], [30]) == []
    assert R.check_select_kth([c], [7], [10])  # one rank below
    assert R.check_select_kth([c], [7], [40])  # one rank above: the right K, the wrong tied id
    assert R.check_select_kth([c], [9], [5])
    big = R.select_kth_cases()[-3]
    assert R.check_select_kth([big], *[[v] for v in R.ref_select_kth(big["keys"], big["ids"], big["k"])]) == []
    assert R.check_select_kth([big], *[[v] for v in R.ref_select_kth(big["keys"], big["ids"], big["k"] - 1)])


def test_select_checker_rejects_the_highest_tied_lane():
    cand = np.zeros(64, dtype=bool)
    cand[[3, 17, 40, 41, 63]] = True
    key = np.full(64, 5, dtype=np.uint64)
    right = (1 << 3) | (1 << 17)
    assert R.check_select_k([("eq", cand, key, 2)], [right]) == []
    assert R.check_select_k([("eq", cand, key, 2)], [(1 << 3) | (1 << 63)])
    assert R.check_select_k([("eq", cand, key, 2)], [(1 << 41) | (1 << 63)])
    row = ("eq", cand, key, 1, 2)  # halves: lanes {3, 17} take 1, lanes {40, 41, 63} take 2
    want = (1 << 3) | (1 << 40) | (1 << 41)
    assert R.check_select_k([row], [want], half="both") == []
    assert R.check_select_k([row], [(1 << 3) | (1 << 41) | (1 << 63)], half="both")
    assert R.check_select_k([row], [want & 0xFFFFFFFF], half="lo") == []
    assert R.check_select_k([row], [want], half="lo")  # the idle half must read 0


@pytest.mark.parametrize("lane", [16, 32, 48])
def test_prefix_checker_rejects_one_off_at_a_row_boundary(lane):
    x = np.arange(64, dtype=np.int32).reshape(1, 64) + 1
    good = R.ref_incl_sum(x[0]).reshape(1, 64)
    assert R.check_incl_sum(x, good) == []
    bad = good.copy()
    bad[0, lane] += 1
    diff = R.check_incl_sum(x, bad)
    assert len(diff) == 1 and f"lane {lane}" in diff[0]


def test_transpose_checker_rejects_one_flipped_bit():
    rng = np.random.default_rng(5)
    x = rng.integers(0, 1 << 64, (1, 64), dtype=np.uint64)
    good = R.ref_transpose64(x[0]).reshape(1, 64)
    assert R.check_transpose(x, good) == []
    for t, j in ((0, 0), (31, 32), (63, 0), (20, 63)):
        assert (int(good[0, t]) >> j) & 1 == (int(x[0, j]) >> t) & 1  # the definition, bit by bit
        bad = good.copy()
        bad[0, t] ^= np.uint64(1 << j)
        assert len(R.check_transpose(x, bad)) == 1
    assert (R.ref_transpose64(good[0]) == x[0]).all()
