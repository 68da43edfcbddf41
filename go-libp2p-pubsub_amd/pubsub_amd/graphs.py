"""Seeded peer-graph builders (the simulator's replacement for the reference
test harness's host dialing, floodsub_test.go:57-99).

All graphs are returned as symmetric CSR (rowptr int64[N+1], col int32[E],
outbound uint8[E]) with strictly ascending rows; `outbound[e]` marks the
side that dialed (the lower-index dialer is outbound for
random regular graphs; connectSome marks the dialing host).
"""
import numpy as np


def _to_csr(n, pairs_dialer):
    """pairs_dialer: array (M, 2) of (dialer, target), undirected, no dups."""
    a = pairs_dialer[:, 0].astype(np.int64)
    b = pairs_dialer[:, 1].astype(np.int64)
    src = np.concatenate([a, b])
    dst = np.concatenate([b, a])
    out = np.concatenate([np.ones(len(a), np.uint8), np.zeros(len(a), np.uint8)])
    order = np.lexsort((dst, src))
    src, dst, out = src[order], dst[order], out[order]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.add.at(rowptr, src + 1, 1)
    rowptr = np.cumsum(rowptr)
    return rowptr, dst.astype(np.int32), out


def random_regular(n, k, seed):
    """Random simple k-regular graph by the pairing model with rejection of
    self-loops / multi-edges (re-pair the rejected stubs a bounded number of
    times, then drop what is left; a few nodes may end with degree < k)."""
    rng = np.random.default_rng(seed)
    stubs = np.repeat(np.arange(n, dtype=np.int64), k)
    edges = set()
    for _ in range(200):
        rng.shuffle(stubs)
        if len(stubs) % 2:
            stubs = stubs[:-1]
        pairs = stubs.reshape(-1, 2)
        lo = np.minimum(pairs[:, 0], pairs[:, 1])
        hi = np.maximum(pairs[:, 0], pairs[:, 1])
        key = lo * n + hi
        ok = lo != hi
        # accept unseen, unique keys
        _, first = np.unique(key, return_index=True)
        uniq = np.zeros(len(key), bool)
        uniq[first] = True
        accept = ok & uniq
        if edges:
            existing = np.fromiter(edges, dtype=np.int64) if len(edges) < 5_000_000 else None
            if existing is not None:
                accept &= ~np.isin(key, existing)
        for kk in key[accept].tolist():
            edges.add(kk)
        rest = pairs[~accept].ravel()
        if len(rest) == 0:
            break
        stubs = rest
    keys = np.fromiter(edges, dtype=np.int64)
    lo, hi = keys // n, keys % n
    return _to_csr(n, np.stack([lo, hi], axis=1))


def random_regular_fast(n, k, seed):
    """Large-N k-regular-ish graph: union of k/2 random perfect matchings over
    a random cyclic ordering (each node gets exactly k distinct neighbours with
    overwhelming probability; duplicate pairs are dropped)."""
    rng = np.random.default_rng(seed)
    pairs = []
    for _ in range(k // 2):
        perm = rng.permutation(n)
        a = perm
        b = np.roll(perm, 1)
        pairs.append(np.stack([a, b], axis=1))
    p = np.concatenate(pairs)
    lo = np.minimum(p[:, 0], p[:, 1]).astype(np.int64)
    hi = np.maximum(p[:, 0], p[:, 1]).astype(np.int64)
    key = np.unique(lo * n + hi)
    lo, hi = key // n, key % n
    return _to_csr(n, np.stack([lo, hi], axis=1))


def connect_some(n, d, seed):
    """connectSome (floodsub_test.go:69-87): every host i dials d random other
    hosts (duplicate dials are no-ops); the dialer is outbound."""
    rng = np.random.default_rng(seed)
    seen = {}
    for i in range(n):
        j = 0
        while j < d:
            m = int(rng.integers(n))
            if m == i:
                continue
            key = (min(i, m), max(i, m))
            if key not in seen:
                seen[key] = i
            j += 1
    arr = np.array([[dialer, b if dialer == a else a] for (a, b), dialer in seen.items()], dtype=np.int64)
    return _to_csr(n, arr)


def dense_connect(n, seed):
    """denseConnect (floodsub_test.go:65-67)."""
    return connect_some(n, 10, seed)


def sparse_connect(n, seed):
    """sparseConnect (floodsub_test.go:61-63)."""
    return connect_some(n, 3, seed)


LADDER_HUBS = (64, 64, 63, 63, 62, 48, 33, 33, 32, 32, 31, 31)
LADDER32_HUBS = (32, 32, 31, 17, 16)


def degree_ladder(n, seed, hubs=LADDER_HUBS, pendant=4, isolated=2, body_dials=3, max_degree=None):
    """Every degree class of the one-wave-per-node kernels in one graph: nodes
    0..len(hubs)-1 are hubs with exactly the given degrees (hubs 0 and 1 are
    connected to each other, every other hub neighbour is a body node drawn
    without replacement), each body node dials `body_dials` random other body
    nodes (connectSome among the body), the last `isolated` nodes have no
    edges and the `pendant` nodes before them exactly one, to a body node.
    The dialer of every pair is drawn from the seeded generator.  Raises if
    the body is too small for a hub, or if `max_degree` is given and a node
    ends above it (LADDER32_HUBS with max_degree=32 keeps the graph inside
    the half-wave kernels)."""
    rng = np.random.default_rng(seed)
    nh = len(hubs)
    body = np.arange(nh, n - pendant - isolated)
    if len(body) < 2 or body_dials >= len(body):
        raise ValueError(f"degree_ladder: a body of {len(body)} nodes is too small")
    pairs = set()
    if nh >= 2:
        pairs.add((0, 1))
    for h, deg in enumerate(hubs):
        need = deg - (1 if h < 2 and nh >= 2 else 0)
        if need < 0 or need > len(body):
            raise ValueError(f"degree_ladder: hub {h} cannot reach degree {deg} with a body of {len(body)} nodes")
        for v in rng.choice(body, need, replace=False):
            pairs.add((h, int(v)))
    for u in body:
        others = body[body != u]
        for v in rng.choice(others, body_dials, replace=False):
            pairs.add((min(int(u), int(v)), max(int(u), int(v))))
    for p in range(n - pendant - isolated, n - isolated):
        pairs.add((int(rng.choice(body)), p))
    pairs = np.array(sorted(pairs), dtype=np.int64)
    flip = rng.random(len(pairs)) < 0.5
    pairs[flip] = pairs[flip][:, ::-1]
    g = _to_csr(n, pairs)
    deg = np.diff(g[0])
    if max_degree is not None and deg.max() > max_degree:
        raise ValueError(f"degree_ladder: node {int(deg.argmax())} has degree {int(deg.max())} > {max_degree}")
    return g


def tailed(n_body, k, tail, seed):
    """random_regular(n_body, k, seed) with a path of `tail` extra nodes hung on
    body node 0: node n_body is connected to node 0, node n_body + i to node
    n_body + i - 1, and the tip n_body + tail - 1 has degree 1.  A message
    authored in the body reaches tail node i exactly one hop after node i - 1,
    so the oldest first delivery of a run is set by `tail` (the message-window
    edge scenarios).  The body keeps random_regular's edges and dialers; the
    dialer of every tail pair is drawn from the seeded generator."""
    if tail < 1:
        raise ValueError("tailed: the tail needs at least one node")
    rowptr, col, outbound = random_regular(n_body, k, seed)
    src = np.repeat(np.arange(n_body, dtype=np.int64), np.diff(rowptr))
    dialed = outbound == 1
    body = np.stack([src[dialed], col[dialed].astype(np.int64)], axis=1)
    chain = np.concatenate([[0], n_body + np.arange(tail, dtype=np.int64)])
    path = np.stack([chain[:-1], chain[1:]], axis=1)
    flip = np.random.default_rng(seed + 7919).random(tail) < 0.5  # (a longer tail keeps the shorter one's draws)
    path[flip] = path[flip][:, ::-1]
    return _to_csr(n_body + tail, np.concatenate([body, path]))


def all_subscribed(n, topics):
    return np.full(n, (1 << topics) - 1 if topics < 64 else 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
