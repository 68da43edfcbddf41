"""CPU tests of tests/tables_ref.py: the case tables of the peertx rebuild
reach every path of the rebuild kernels with a non-zero count, counted from
the model alone, and the model, the checker and the cases agree with a
sequential emulation of the tables (no GPU: the GPU tests run the same cases
through the probe)."""
import collections

import numpy as np
import pytest

import tables_ref as T

CASES = T.rebuild_cases()
BY_NAME = {c["name"]: c for c in CASES}


def _model_stats(case):
    """The statistics of every rebuild of a case, from the model alone."""
    m = T.PtxModel(case["bits"], case["n_nodes"])
    out = []
    for step in case["steps"]:
        if step[0] == "incr":
            for r in step[1]:
                m.incr_round(r)
        else:
            out.append(m.rebuild(step[2][step[1]]))
    return out, m


STATS = {c["name"]: _model_stats(c)[0] for c in CASES}


def test_print_path_counts():
    """Every path is reached (run with -s for the counts per case)."""
    tot = collections.Counter()
    for name, sts in STATS.items():
        for i, st in enumerate(sts):
            print(f"{name} rebuild {i}: {st}")
            for k in ("leave_row", "leave_ovf", "home", "stay"):
                tot[k] += st[k]
    print("total:", dict(tot))
    assert tot["leave_row"] and tot["leave_ovf"] and tot["home"] and tot["stay"]


def test_the_model_decides_every_count():
    """Before every rebuild of every case the rules alone decide which table
    holds each entry, so the counts per path are facts of the case."""
    for name, sts in STATS.items():
        assert sts and all(st["exact"] for st in sts), name


def test_row_sizes_and_passes():
    rows = collections.defaultdict(set)
    for c in CASES:
        if c["kind"] == "full_rows":
            rows[1 << c["bits"]].add(c["roles"])
    assert set(rows) == {4, 16, 64, 128, 256, 512, 1024}
    for hn in (4, 16, 64, 128):  # below the wave's 256-entry read: neighbours on both sides
        assert rows[hn] == {T.FIVE}
    assert T.FIVE[1:4] == ("keep", "empty", "drop") and T.FIVE[0] == T.FIVE[4] == "half"
    passes = {1 << c["bits"]: STATS[c["name"]][0]["passes"] for c in CASES if c["kind"] == "full_rows"}
    assert [passes[hn] for hn in (256, 512, 1024)] == [1, 2, 4]
    for c in CASES:
        if c["kind"] != "full_rows":
            continue
        st, hn = STATS[c["name"]][0], 1 << c["bits"]
        # every row full (but the empty node's), the drop node loses all, the keep node none
        m = T.PtxModel(c["bits"], c["n_nodes"])
        for r in c["steps"][0][1]:
            m.incr_round(r)
        lastw = c["steps"][1][2][c["steps"][1][1]]
        for v, role in enumerate(c["roles"]):
            mine = [k for u, k in m.count if u == v]
            gone = sum(T.leaves(lastw, v, k) for k in mine)
            assert len(mine) == (0 if role == "empty" else hn)
            if role == "keep":
                assert gone == 0
            elif role == "drop":
                assert gone == hn
            elif role == "half":
                assert 0 < gone < hn
        assert st["skipped_nodes"] == c["roles"].count("empty") and st["leave_row"] > 0 and st["leave_ovf"] == 0
        # counts from 1 to the cap are in the tables when the rebuild runs
        assert set(m.count.values()) == set(range(1, T.GR + 2)) or hn == 4


def test_ring_rows():
    """R = 3 with last 0 and 2 (and a middle row), and every other ring row
    holds the opposite verdicts."""
    seen = set()
    for c in CASES:
        for step in c["steps"]:
            if step[0] == "rebuild":
                _, last, hist = step
                assert hist.shape == (c["r"], c["n_nodes"], c["w"])
                seen.add((c["r"], last))
                for r in range(c["r"]):
                    if r != last:
                        assert (hist[r] == ~hist[last]).all()
    assert {(3, 0), (3, 2), (3, 1), (1, 0)} <= seen


def test_spill_variants():
    s = {n: STATS[n][0] for n in ("spill_all_fit", "spill_some_fit", "spill_none_fit", "same_keys_three_nodes")}
    assert s["spill_all_fit"]["home"] == 6 and s["spill_all_fit"]["stay"] == 0
    assert s["spill_some_fit"]["home"] == 4 and s["spill_some_fit"]["stay"] == 8 and s["spill_some_fit"]["leave_ovf"] == 2
    assert s["spill_none_fit"]["home"] == 0 and s["spill_none_fit"]["stay"] == 8 and s["spill_none_fit"]["leave_ovf"] == 4
    assert s["spill_none_fit"]["leave_row"] == 0
    k = s["same_keys_three_nodes"]
    assert (k["leave_row"], k["leave_ovf"], k["home"], k["stay"]) == (1, 3, 1, 14)
    c = BY_NAME["same_keys_three_nodes"]
    keys = [collections.Counter(k for v, k in r) for r in c["steps"][0][1][:2]]
    assert all(set(cnt.values()) == {3} for cnt in keys)  # the same keys in all three nodes
    first, second = STATS["overflow_empties"]
    assert first["leave_ovf"] == 10 and first["stay"] == 0 and first["home"] == 0 and first["leave_row"] == 0
    assert second["leave_ovf"] == 0 and second["leave_row"] == 2 and second["home"] == second["stay"] == 0


def test_two_rebuilds_case():
    a, b = STATS["two_rebuilds"]
    assert a["leave_row"] and a["leave_ovf"] and a["home"] and a["stay"]
    assert b["leave_row"] and b["leave_ovf"] and b["home"] and b["stay"]
    steps = [s[0] for s in BY_NAME["two_rebuilds"]["steps"]]
    assert steps == ["incr", "rebuild", "incr", "rebuild", "incr"]


def test_top_slot_case():
    c = BY_NAME["w256_top_slot"]
    top = c["top_key"]
    assert c["w"] == 256 and top >> 14 == (1 << 14) - 1 and top >> 27 == 1
    _, last, hist = c["steps"][1]
    m = T.PtxModel(c["bits"], c["n_nodes"])
    for r in c["steps"][0][1]:
        m.incr_round(r)
    where = {v: ("ovf" if (v, top) in m.in_ovf else "row", T.leaves(hist[last], v, top)) for v in range(3)}
    # the top slot leaves from a row, survives in the overflow table and leaves from it
    assert where == {0: ("row", True), 1: ("ovf", False), 2: ("ovf", True)}
    assert int(hist[last][0][255]) >> 63 == 1


def test_one_home_slot_case():
    c = BY_NAME["one_home_slot_row64"]
    assert len(c["chain"]) >= 24 and len({T.ptx_hash(k, c["bits"]) for k in c["chain"]}) == 1
    assert STATS[c["name"]][0]["leave_row"] == 8


def test_no_case_fills_both_tables():
    """Every loop of the kernels under test stays bounded: no case asks for
    more overflow entries than half the overflow table."""
    for c in CASES:
        m = T.PtxModel(c["bits"], c["n_nodes"])
        for step in c["steps"]:
            if step[0] == "incr":
                for r in step[1]:
                    m.incr_round(r)
                    assert sum(m.ovfn) <= (1 << c["obits"]) // 2, c["name"]
                    assert all(k >> 14 < 64 * c["w"] for _, k in r)
            else:
                m.rebuild(step[2][step[1]])


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_cases_on_the_host_emulation(case):
    """The whole GPU procedure on the sequential emulation of the tables."""
    stats = T.run_case(case, T.HostTables(case["bits"], case["obits"], T.GR, case["n_nodes"]))
    assert stats == STATS[case["name"]]


@pytest.mark.parametrize("fault", ["stale", "lost", "ptxn", "kept_in_overflow"])
def test_the_checker_sees_a_wrong_rebuild(fault):
    """The four ways the issue names in which a rebuild can be wrong, made by
    hand on the emulation's tables after a right rebuild."""
    case = BY_NAME["spill_some_fit"]
    tx = T.HostTables(case["bits"], case["obits"], T.GR, case["n_nodes"])
    m = T.PtxModel(case["bits"], case["n_nodes"])
    for r in case["steps"][0][1]:
        m.incr_round(r)
    tx.run(rounds=case["steps"][0][1])
    _, last, hist = case["steps"][1]
    before = tx.rows.copy()
    m.rebuild(hist[last])
    tx.rebuild(hist, last)
    T.check_tables(m, tx.rows, tx.ovf, tx.ocnt, tx.ptxn)
    if fault == "stale":  # a departed entry still there
        gone = [int(w) for w in before if w and (0, int(w) & 0xFFFFFF00) in m.gone]
        tx.rows[int(np.flatnonzero(tx.rows[:4] != 0)[0])] = gone[0]
    elif fault == "lost":
        tx.rows[int(np.flatnonzero(tx.rows)[0])] = 0
    elif fault == "ptxn":
        tx.ptxn[0] = 0
    else:  # an overflow survivor kept although its row has a free slot
        i = int(np.flatnonzero(tx.rows[:4])[0])
        w = int(tx.rows[i])
        tx.rows[i] = 0
        tx.ovf[int(np.flatnonzero(tx.ovf == 0)[0])] = (1 << 32) | w
        tx.ocnt[0] += 1
        tx.ptxn[0] -= 1
    with pytest.raises(AssertionError):
        T.check_tables(m, tx.rows, tx.ovf, tx.ocnt, tx.ptxn)


def test_spam_model_packs_nibbles():
    m = T.SpamModel(2, 64, 13)
    for _ in range(20):
        assert m.incr(1, 9) <= 15
    assert m.incr(0, 7) == 1 and m.nib[1, 9] == 14
    w = m.words()
    assert w.shape == (2, 8) and w[1, 1] == 14 << 4 and w[0, 0] == 1 << 28 and int(w.sum()) == (14 << 4) + (1 << 28)
    m.retire([0, 1, 2], [1, -1], np.array([1 << 9], dtype=np.uint64), [0])
    assert m.nib[1, 9] == 0 and m.nib[0, 7] == 1
