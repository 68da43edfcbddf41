"""Message windows per topic (include/gs_window.h), the part that needs no GPU:

- the preconditions of the two workloads the feature exists for
  (tests/topic_windows_shapes.py), on the oracle: the ages tw_sparse reaches
  per topic and tail, the rate tw_hot puts on topic 0, and that no uniform
  layout within 16384 slots holds it;
- WithTopicWindows on the oracle (which has no window) changes nothing;
- csrc/gs_window_layout.h, the one statement of the layout and the two
  horizons: tests/topic_windows_check.cpp built with AddressSanitizer and
  UBSan and run directly.

tests/test_topic_windows_gpu.py runs the workloads on the engine."""
import os
import subprocess

import numpy as np
import pytest

import scenarios
import topic_windows_shapes as tw
from pubsub_amd import WithTopicWindows, _abi
from test_window import window

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- the sparse shape
@pytest.mark.parametrize("tail", sorted(tw.SPARSE_AGES))
def test_sparse_shape_ages(oracle_path, tail):
    r = tw.sparse_ran(oracle_path, tail)
    print("tail", tail, "N", r.e.N, "hops", r.hops, "max age", r.max_age(0), r.max_age(1))
    assert (r.max_age(0), r.max_age(1)) == tw.SPARSE_AGES[tail]
    assert r.all_delivered()
    # the tail's nodes take topic 1 only
    assert (r.hop[r.top == 0][:, scenarios.WIN_BODY:] < 0).all()


def test_sparse_shape_sits_on_the_default_limit(oracle_path):
    """Tail 28 reaches the policy's maxAge exactly, 29 is one past it, and 45
    needs 47; topic 1's retire horizon is then 117 hops, inside 128 slots at
    one message per hop."""
    max_age, retire = window()
    assert (max_age, retire) == (30, 100)
    assert tw.SPARSE_AGES[28][1] == max_age and tw.SPARSE_AGES[29][1] == max_age + 1
    assert 47 + (retire - max_age) == 117 <= 128
    r = tw.sparse_ran(oracle_path, 45)
    # the first hop with an age above 30 comes before the first with 47, and
    # both lie well inside the run
    assert tw.SPARSE_START + 31 <= r.first_hop_over(1, 30) < r.first_hop_over(1, 46) < r.hops


# ---------------------------------------------------------------- the hot shape
def test_hot_shape(oracle_path):
    r = tw.hot_ran(oracle_path)
    per = np.bincount(r.top, minlength=64)
    hops = r.e.sched_hops
    assert per[0] == tw.HOT_TOPIC0 and per[1:].max() == tw.HOT_OTHERS
    assert (int(hops.min()), int(hops.max())) == (5, 104)
    assert int(r.age.max()) == tw.HOT_MAX_AGE and r.counters["deliveries"] == tw.HOT_DELIVERIES
    assert r.all_delivered()


def test_no_uniform_layout_holds_the_hot_shape(oracle_path):
    """All of topic 0's messages fall within one retire horizon (100 hops), so
    its ring needs 1904 slots; 64 equal rings within 16384 slots have 256."""
    _, retire = window()
    hops = tw.hot_ran(oracle_path).e.sched_hops
    assert int(hops.max()) - int(hops.min()) < retire
    largest_uniform = 16384 // 64 // 64 * 64
    assert largest_uniform == 256 and tw.HOT_TOPIC0 > largest_uniform
    # sized by its own rate every topic fits: 2048 + 63 * 64 slots
    assert tw.HOT_SLOTS[0] >= tw.HOT_TOPIC0 and min(tw.HOT_SLOTS[1:]) >= tw.HOT_OTHERS
    assert sum(tw.HOT_SLOTS) == 6080 <= 16384 and all(s % 64 == 0 for s in tw.HOT_SLOTS)


# ---------------------------------------------------------------- the option on the oracle
def test_option_is_accepted_and_ignored_by_the_oracle(oracle_path):
    ref = tw.sparse_snap(oracle_path, 28)
    e, hops = tw.tw_sparse(oracle_path, 28, (WithTopicWindows([64, 192], [0, 47]),))
    e.step(hops)
    bad = scenarios.compare(ref, scenarios.snapshot(e, range(e.n_published)))
    assert bad == [], "\n".join(bad)
    with pytest.raises(ValueError, match="product library only"):
        e.topic_windows()
    e.close()


def test_abi_lists_the_window_calls():
    assert [n for n, _, _ in _abi.WINDOW_FUNCTIONS] == ["gs_set_topic_windows", "gs_read_topic_windows"]
    header = open(os.path.join(REPO, "include", "gs_window.h")).read()
    assert all(f"int {n}(" in header for n, _, _ in _abi.WINDOW_FUNCTIONS)


# ---------------------------------------------------------------- the layout header
def test_layout_header(tmp_path):
    exe = tmp_path / "topic_windows_check"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "go-libp2p-pubsub_amd", "csrc"),
                    os.path.join(REPO, "tests", "topic_windows_check.cpp"), "-o", str(exe)],
                   check=True, capture_output=True, timeout=180)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    word, checks = out.stdout.split()
    assert word == "ok" and int(checks) > 100000
