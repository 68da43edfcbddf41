"""Message windows per topic (include/gs_window.h) on the engine, against the
oracle, which has no window; every comparison is bit for bit
(scenarios.compare).  tests/test_topic_windows.py holds the workloads'
preconditions and the layout header's check.

1. a sparse topic's late deliveries run with an age limit of its own, and are
   refused without it, as before;
2. the limit is the topic's own and exact;
3. a hot topic among 64 runs with a ring of its own, and is refused by every
   uniform layout, as before;
4. results do not depend on how the window is cut among the topics: existing
   scenarios with uneven rings, on every kernel family that looks up a slot's
   topic or a topic's words;
5. the publish guard uses each topic's own retire horizon;
6. two ranks; 7. latency statistics; 8. the interface."""
import functools
import multiprocessing as mp
import os
import re
import sys

import numpy as np
import pytest

import scenarios
import topic_windows_shapes as tw
from pubsub_amd import (PRODUCT_LIB, GossipEngineError, WithEventTracer, WithFrontierBitmaps, WithFrontierLists,
                        WithLatencyStats, WithTopicWindows, _abi)
from test_partition_gpu import _free_port
from test_trace_rpc import RECV, SEND, TRACED

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TAIL = 45
AGE = tw.SPARSE_AGES[TAIL][1]  # 47
SPARSE_WINDOWS = WithTopicWindows(slots=[128, 128], max_age_hops=[0, AGE])


def _equals(ref, e, ids=None):
    bad = scenarios.compare(ref, scenarios.snapshot(e, ids if ids is not None else range(e.n_published)))
    assert bad == [], "\n".join(bad)


def _sparse_equals_oracle(oracle, extra=(SPARSE_WINDOWS,)):
    e, hops = tw.tw_sparse(PRODUCT_LIB, TAIL, extra)
    e.step(hops)
    _equals(tw.sparse_snap(oracle, TAIL), e)
    e.close()


def _refused_late(extra, at_hop):
    """The run stops with the late-delivery error at `at_hop`, twice in the
    same words."""
    e, hops = tw.tw_sparse(PRODUCT_LIB, TAIL, extra)
    said = []
    for n in (hops, 1):
        with pytest.raises(GossipEngineError) as ei:
            e.step(n)
        assert ei.value.code == _abi.GS_ECAPACITY
        said.append(str(ei.value))
    e.close()
    print(said[0])
    assert "later than" in said[0] and said[0] == said[1]
    assert int(re.search(r"hop (\d+):", said[0]).group(1)) == at_hop


# ---------------------------------------------------------------- 1. late on one topic
def test_sparse_topic_runs_with_its_own_age(oracle_path):
    _sparse_equals_oracle(oracle_path)


def test_sparse_topic_is_refused_without_the_option(oracle_path):
    _refused_late((), tw.sparse_ran(oracle_path, TAIL).first_hop_over(1, 30))


# ---------------------------------------------------------------- 2. the topic's own, and exact
@pytest.mark.parametrize("ages,over", [([0, AGE - 1], AGE - 1), ([AGE, 0], 30)],
                         ids=["one_short", "given_to_the_wrong_topic"])
def test_age_is_the_topics_own_and_exact(oracle_path, ages, over):
    r = tw.sparse_ran(oracle_path, TAIL)
    _refused_late((WithTopicWindows(slots=[128, 128], max_age_hops=ages),), r.first_hop_over(1, over))
    # the refusal leaves nothing behind: the run with the right ages follows in this process
    _sparse_equals_oracle(oracle_path)


# ---------------------------------------------------------------- 3. a hot topic
def test_hot_topic_runs_with_its_own_ring(oracle_path):
    r = tw.hot_ran(oracle_path)
    e, hops = tw.tw_hot(PRODUCT_LIB, (WithTopicWindows(slots=tw.HOT_SLOTS),))
    assert hops == r.hops
    e.step(hops)
    ids = e.snapshot_ids  # every ring holds its topic's messages of the ids read
    assert e.counters()["deliveries"] == tw.HOT_DELIVERIES
    _equals(scenarios.snapshot(r.e, ids), e, ids)
    e.close()


def test_hot_topic_is_refused_by_uniform_layouts():
    with pytest.raises(GossipEngineError) as ei:
        tw.tw_hot(PRODUCT_LIB, window=256)
    assert ei.value.code == _abi.GS_ECAPACITY and "message window too small" in str(ei.value)
    with pytest.raises(GossipEngineError) as ei:
        tw.tw_hot(PRODUCT_LIB, window=2048)
    assert ei.value.code == _abi.GS_EUNSUPPORTED and "must be <= 16384" in str(ei.value)


# ---------------------------------------------------------------- 4. the cut of the window
def _alt(n, a, b):
    return [a if t % 2 == 0 else b for t in range(n)]


# scenario: (rings, further options); no topic has fewer slots than the
# scenario's own window, except cut_spill_16t's 64s (37 messages per topic)
RECUT = {
    "gossipsub_slot_reuse_4t": ([128, 192, 256, 128], ()),
    "gossipsub_multitopic": ([1024, 2048, 1088], ()),
    # the same W as the scenario's 16 x 128: phase B's cut over uneven topic words
    "cut_spill_16t": (_alt(16, 64, 192), ()),
    "push_overflow": ([512, 1024, 576, 640], ()),
    "floodsub_multitopic/bitmaps": ([128, 256, 192], (WithFrontierBitmaps(),)),
    "floodsub_multitopic/lists": ([128, 256, 192], (WithFrontierLists(),)),
    # the adversarial instantiation, two topics (phantom ids, the IHAVE cuts)
    "spam_ihave_2t": ([4096, 8192], ()),
    # RPC byte accounting over three topics
    "acct_multitopic": ([1088, 1024, 2048], ()),
    # the 4-words-per-lane instantiation, every ring given explicitly (equal
    # rings: the multiply), and its table form on the window family of 64 topics
    # (two messages per topic: any ring holds them)
    "c4shape": ([256] * 64, ()),
    "win_gossip_64t_edge": (_alt(64, 192, 320), ()),
}


@functools.lru_cache(maxsize=None)
def _oracle_run(oracle, name):
    return scenarios.run(oracle, name)


@pytest.mark.parametrize("case", sorted(RECUT))
def test_results_do_not_depend_on_the_cut(oracle_path, case):
    name = case.split("/")[0]
    slots, more = RECUT[case]
    e, hops = scenarios.SCENARIOS[name](PRODUCT_LIB, (WithTopicWindows(slots=slots),) + more)
    assert e.topic_windows()[0].tolist() == slots
    e.step(hops)
    if more:
        assert e.frontier_dense == ("bitmaps" in case)
    _equals(_oracle_run(oracle_path, name), e, getattr(e, "snapshot_ids", range(e.n_published)))
    e.close()


def test_rpc_trace_does_not_depend_on_the_cut(oracle_path):
    name = "gossipsub_multitopic"
    eo, hops = scenarios.SCENARIOS[name](oracle_path, (WithEventTracer(TRACED, rpc=True),))
    eo.step(hops)
    want = eo.trace_events()
    e, _ = scenarios.SCENARIOS[name](PRODUCT_LIB, (WithEventTracer(TRACED, rpc=True),
                                                   WithTopicWindows(slots=[1024, 2048, 1088])))
    e.step(hops)
    got = e.trace_events()
    e.close()
    assert (got["type"] == SEND).any() and (got["type"] == RECV).any()
    assert len(got) == len(want) and np.array_equal(got, want)


# ---------------------------------------------------------------- 5. the publish guard per topic
GUARD_SLOTS = 64
GUARD_READABLE = range(2, 2 * GUARD_SLOTS + 2)


def _guard_run(lib, probe):
    """tw_sparse's network with two 64-slot rings: 64 messages per topic in hop
    25 (ids 2k: topic 0 by the body author; 2k + 1: topic 1 by the body author
    and the tip in turn), then one more on topic 0 at its retire horizon (100
    hops) and one on topic 1 at its own (117).  probe: ask for each slot one
    hop sooner first, after the engine has run 10 hops past the burst, and
    return what that raised."""
    e = tw.sparse_network(lib, TAIL, GUARD_SLOTS, (WithTopicWindows(max_age_hops=[0, AGE]),))
    s = tw.SPARSE_START
    src = np.full(2 * GUARD_SLOTS, scenarios.WIN_AUTHOR, np.int32)
    src[3::4] = e.tip
    top = np.tile(np.array([0, 1], np.int32), GUARD_SLOTS)
    ids = e.publish(src, top, np.full(2 * GUARD_SLOTS, s, np.int64))
    assert ids.tolist() == list(range(2 * GUARD_SLOTS))
    e.step(s + 10)
    raised = []
    if probe:
        for t, hop in ((0, s + 99), (1, s + 116)):
            with pytest.raises(GossipEngineError) as ei:
                e.publish([e.tip if t else scenarios.WIN_AUTHOR], [t], [hop])
            raised.append(ei.value)
    ids = e.publish([scenarios.WIN_AUTHOR, e.tip], [0, 1], [s + 100, s + 117])
    assert ids.tolist() == [2 * GUARD_SLOTS, 2 * GUARD_SLOTS + 1]
    e.step(117 + TAIL + 12 - 10)
    return e, raised


def test_publish_guard_uses_the_topics_own_horizon(oracle_path):
    eo, _ = _guard_run(oracle_path, False)
    ref = scenarios.snapshot(eo, GUARD_READABLE)
    # the oracle's ages stay inside the limits given (else the run below is refused as late)
    hop = np.stack([eo.deliveries(i)[0] for i in range(eo.n_published)])
    age = np.where(hop >= 0, hop - eo.msg_hop[:, None], -1)
    assert age[eo.msg_topic == 0].max() <= 30 and age[eo.msg_topic == 1].max() == AGE
    e, raised = _guard_run(PRODUCT_LIB, True)
    assert e.topic_windows()[2].tolist() == [100, 117]
    for ex, retire, t in zip(raised, (100, 117), (0, 1)):
        assert ex.code == _abi.GS_ECAPACITY and "message window too small" in str(ex)
        assert int(re.search(r"within (\d+) hops", str(ex)).group(1)) == retire
        assert f"topic {t}" in str(ex)
    _equals(ref, e, GUARD_READABLE)
    # the later messages took the burst's first slots and reached every subscriber as the oracle says
    for i in (2 * GUARD_SLOTS, 2 * GUARD_SLOTS + 1):
        hop, frm = e.deliveries(i)
        want_hop, want_frm = eo.deliveries(i)
        assert (want_hop[:None if i % 2 else scenarios.WIN_BODY] >= 0).all()  # (topic 0: the body)
        assert np.array_equal(hop, want_hop) and np.array_equal(frm, want_frm)
    e.close()
    eo.close()


# ---------------------------------------------------------------- 6. two ranks
def _rank_worker(rank, world, port, oracle, q):
    try:
        sys.path.insert(0, HERE)
        sys.path.insert(0, os.path.join(os.path.dirname(HERE), "go-libp2p-pubsub_amd"))
        import torch
        import torch.distributed as dist

        import scenarios
        import topic_windows_shapes as tw
        from pubsub_amd import PRODUCT_LIB, WithPartition, WithTopicWindows
        from pubsub_amd.transport import TorchTransport
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
        tr = TorchTransport(memory="device")
        e, hops = tw.tw_sparse(PRODUCT_LIB, TAIL, (WithPartition(rank, world, tr),
                                                   WithTopicWindows(slots=[128, 128], max_age_hops=[0, AGE])))
        e.step(hops)
        got = scenarios.snapshot(e, range(e.n_published))
        got["node_range"], got["edge_range"] = e.node_range, e.edge_range
        ref = dict(tw.sparse_snap(oracle, TAIL), node_range=e.node_range, edge_range=e.edge_range)
        bad = scenarios.compare(scenarios.restrict(ref, 2), scenarios.restrict(got, 2))
        keys = sorted(k for k in ref["counters"] if k not in ("hops", "heartbeats"))
        mine = torch.tensor([got["counters"][k] for k in keys], dtype=torch.int64)
        dist.all_reduce(mine)
        if dict(zip(keys, mine.tolist())) != {k: ref["counters"][k] for k in keys}:
            bad.append(f"summed counters {dict(zip(keys, mine.tolist()))} != oracle {ref['counters']}")
        if tr.calls == 0:
            bad.append("the transport was never called")
        q.put((rank, bad, e.node_range))
        dist.destroy_process_group()
    except Exception as ex:  # report instead of hanging the parent
        import traceback
        q.put((rank, [f"worker raised: {ex!r}\n{traceback.format_exc()}"], None))


def test_two_ranks(oracle_path):
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_rank_worker, args=(r, world, port, oracle_path, q)) for r in range(world)]
    for p in procs:
        p.start()
    try:
        res = sorted((q.get(timeout=240) for _ in range(world)), key=lambda r: r[0])
    finally:
        for p in procs:
            p.join(timeout=30)
            if p.is_alive():
                p.kill()
    assert all(r[1] == [] for r in res), res
    # the tail (nodes 24..68) lies on the second rank
    assert res[0][2][1] == res[1][2][0] <= scenarios.WIN_BODY and res[1][2][1] == scenarios.WIN_BODY + TAIL


# ---------------------------------------------------------------- 7. latency statistics
def test_latency_statistics_take_the_largest_age(oracle_path):
    r = tw.SparseRef(oracle_path, TAIL)
    e, hops = tw.tw_sparse(PRODUCT_LIB, TAIL, (SPARSE_WINDOWS, WithLatencyStats()))
    e.step(hops)
    bins = e.latency_bins()
    hist = e.latency_hist()
    deliveries = e.counters()["deliveries"]
    e.close()
    assert bins == AGE + 1 == 48
    want = r.hist(bins)
    assert np.array_equal(hist, want), f"first differences at {np.argwhere(hist != want)[:5].tolist()}"
    assert hist.sum() == deliveries == r.counters["deliveries"]
    assert not hist[0, 3:].any() and hist[0, 1:3].all() and hist[1, AGE] > 0


# ---------------------------------------------------------------- 8. the interface
def test_interface():
    e = tw.sparse_network(PRODUCT_LIB, TAIL, 128)
    # the policy's values before the call: 3 heartbeats, + (HistoryLength + 2) heartbeats
    assert [a.tolist() for a in e.topic_windows()] == [[128, 128], [30, 30], [100, 100]]
    assert all(a.dtype == np.int32 for a in e.topic_windows())
    e.close()
    e = tw.sparse_network(PRODUCT_LIB, TAIL, 128, (WithTopicWindows([64, 192], [7, 0]),))
    assert [a.tolist() for a in e.topic_windows()] == [[64, 192], [7, 30], [77, 100]]
    e.close()
    e = tw.sparse_network(PRODUCT_LIB, TAIL, 128, (WithTopicWindows(None, [0, AGE]),))
    assert [a.tolist() for a in e.topic_windows()] == [[128, 128], [30, AGE], [100, AGE + 70]]
    # after a publish the windows are fixed
    e.publish([0], [0], [3])
    rc = e.lib.gs_set_topic_windows(e.h, None, None)
    assert rc == _abi.GS_ESTATE and b"before the first publish" in e.lib.gs_last_error()
    assert [a.tolist() for a in e.topic_windows()] == [[128, 128], [30, AGE], [100, AGE + 70]]
    e.close()
    for slots, ages, code, word in (([64, 100], None, _abi.GS_EINVAL, "multiple of 64"),
                                    ([0, 64], None, _abi.GS_EINVAL, "multiple of 64"),
                                    ([8192, 8256], None, _abi.GS_EUNSUPPORTED, "must be <= 16384"),
                                    (None, [0, 30001], _abi.GS_EINVAL, "30000"),
                                    (None, [-1, 0], _abi.GS_EINVAL, "30000")):
        with pytest.raises(GossipEngineError) as ei:
            tw.sparse_network(PRODUCT_LIB, TAIL, 128, (WithTopicWindows(slots, ages),))
        assert ei.value.code == code and word in str(ei.value), str(ei.value)
    with pytest.raises(ValueError, match="one entry per topic"):
        tw.sparse_network(PRODUCT_LIB, TAIL, 128, (WithTopicWindows([64, 64, 64]),))
