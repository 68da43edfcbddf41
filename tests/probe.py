"""ctypes loader of the test-only probe library (tests/probe/gs_probe.hip):
every entry point wrapped with numpy arrays.  A non-zero HIP error code of an
entry point raises ProbeError; a missing library raises it too, naming the
build command (the gpu tests then fail, they do not skip)."""
import ctypes as C
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROBE_LIB = os.path.join(REPO, "go-libp2p-pubsub_amd", "build", "libgs_probe.so")
BUILD_HINT = "make -C go-libp2p-pubsub_amd probe   (or: python __graft_entry__.py)"

# gsp_lanes ops (the enum of gs_probe.hip, same order)
(OP_INCL_SUM, OP_LANE_PREFIX, OP_WAVE_LAST, OP_SUM_INT, OP_SUM_LL, OP_LANE_RANK, OP_XOR32_U32, OP_XOR32_U64, OP_XOR32_F64,
 OP_LANE_GET64, OP_LANE_GETF, OP_TRANSPOSE, OP_TRANSPOSE2, OP_KTH_BIT, OP_COUNT) = range(15)
# gsp_select_k modes
MODE_SELECT_K, MODE_HALF, MODE_GRP_WAVE, MODE_GRP_PAIR, MODE_HALF_IF_LO, MODE_HALF_IF_HI = range(6)


class ProbeError(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(PROBE_LIB):
            raise ProbeError(f"{PROBE_LIB} is missing; build it with: {BUILD_HINT}")
        _lib = C.CDLL(PROBE_LIB, mode=C.RTLD_LOCAL)
        for name in ("gsp_consts", "gsp_select_k", "gsp_select_kth", "gsp_lanes", "gsp_item_sender", "gsp_dlt",
                     "gsp_philox", "gsp_keys", "gsp_quantum_div", "gsp_add_ones", "gsp_ptx_hash", "gsp_peertx",
                     "gsp_lds_limit", "gsp_ptx_rebuild", "gsp_spam", "gsp_pool_take"):
            getattr(_lib, name).restype = C.c_int
    return _lib


def _in(a, dtype, n=None):
    a = np.ascontiguousarray(a, dtype=dtype).reshape(-1)
    if n is not None and a.size != n:
        raise ValueError(f"expected {n} elements, got {a.size}")
    return a


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _call(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise ProbeError(f"{name} returned HIP error {rc}")


def consts():
    """{'GS_SEL_WIN', 'GS_SEL_CAP', 'E_PEERTX', 'E_POOL'} as the device code was built."""
    out = np.zeros(5, dtype=np.int32)
    _call("gsp_consts", _p(out))
    if int(out[3]) != OP_COUNT:
        raise ProbeError("tests/probe.py and gs_probe.hip disagree on the gsp_lanes ops")
    return {"GS_SEL_WIN": int(out[0]), "GS_SEL_CAP": int(out[1]), "E_PEERTX": int(out[2]), "E_POOL": int(out[4])}


def lds_limit():
    """hipDeviceAttributeMaxSharedMemoryPerBlock of the current device, in bytes."""
    out = np.zeros(1, dtype=np.int32)
    _call("gsp_lds_limit", _p(out))
    return int(out[0])


def select_k(mode, cand, key, k):
    """cand / key / k: [cases][64]; returns the ballot mask of every case."""
    cand = _in(cand, np.uint8)
    n = cand.size // 64
    key, k = _in(key, np.uint64, n * 64), _in(k, np.int32, n * 64)
    out = np.zeros(n, dtype=np.uint64)
    _call("gsp_select_k", C.c_int(mode), C.c_int(n), _p(cand), _p(key), _p(k), _p(out))
    return out


def select_kth(cases, est=False):
    """cases: the dicts of select_ref's tables; returns (K[cases], M[cases])."""
    n = len(cases)
    off = np.zeros(n + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(c["keys"]) for c in cases])
    keys = _in(np.concatenate([c["keys"] for c in cases]), np.uint64)
    ids = _in(np.concatenate([c["ids"] for c in cases]), np.int64)
    lane_off = _in(np.stack([c["lane_off"] for c in cases]), np.int32, 65 * n)
    k = _in([c["k"] for c in cases], np.int32)
    n_arg = _in([c["n"] for c in cases], np.int32)
    K, M = np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.int64)
    _call("gsp_select_kth", C.c_int(1 if est else 0), C.c_int(n), _p(off), _p(lane_off), _p(keys), _p(ids), _p(k),
          _p(n_arg), _p(K), _p(M))
    return K, M


def lanes(op, a, b=None):
    """a: [cases][64] uint64 operands (ints in the low 32 bits, doubles as bit
    patterns), b: [cases][64] int32 (source lane in lane 0 / k per lane).
    Returns (o1, o2), each [cases][64] uint64."""
    a = _in(a, np.uint64)
    n = a.size // 64
    b = np.zeros(n * 64, dtype=np.int32) if b is None else _in(b, np.int32, n * 64)
    o1, o2 = np.zeros(n * 64, dtype=np.uint64), np.zeros(n * 64, dtype=np.uint64)
    _call("gsp_lanes", C.c_int(op), C.c_int(n), _p(a), _p(b), _p(o1), _p(o2))
    return o1.reshape(n, 64), o2.reshape(n, 64)


def item_sender(s_it, n_items):
    """s_it: [cases][64] exclusive prefix tables, n_items[cases].  Returns
    (sender, within), each [cases][max items], 0 past a case's items."""
    s_it = _in(s_it, np.int32)
    n = s_it.size // 64
    n_items = _in(n_items, np.int32, n)
    mx = max(int(n_items.max()), 1)
    sender, within = np.zeros(n * mx, dtype=np.int32), np.zeros(n * mx, dtype=np.int32)
    _call("gsp_item_sender", C.c_int(n), _p(s_it), _p(n_items), C.c_int(mx), _p(sender), _p(within))
    return sender.reshape(n, mx), within.reshape(n, mx)


def dlt_round_trip(q, narrow):
    q = _in(q, np.uint32)
    got = np.zeros(q.size, dtype=np.uint32)
    _call("gsp_dlt", C.c_int(1 if narrow else 0), C.c_int(q.size), _p(q), _p(got))
    return got


def philox(ctr, key):
    ctr = _in(ctr, np.uint32)
    n = ctr.size // 4
    key = _in(key, np.uint32, 2 * n)
    out = np.zeros(4 * n, dtype=np.uint32)
    _call("gsp_philox", C.c_int(n), _p(ctr), _p(key), _p(out))
    return out.reshape(n, 4)


def keys(args):
    """args: [n][6] = seed, site, a, b, c, d.  Returns gs_key64, gs_key64_mid
    (c as the message id), gs_key64x2 [n][2], and the bits of gs_key_to_unit(key64)."""
    args = _in(args, np.uint32)
    n = args.size // 6
    k64, kmid, unit = (np.zeros(n, dtype=np.uint64) for _ in range(3))
    kx2 = np.zeros(2 * n, dtype=np.uint64)
    _call("gsp_keys", C.c_int(n), _p(args), _p(k64), _p(kmid), _p(kx2), _p(unit))
    return k64, kmid, kx2.reshape(n, 2), unit


def quantum_div(mt, q, magic):
    mt = _in(mt, np.int64)
    q, magic = _in(q, np.int64, mt.size), _in(magic, np.uint64, mt.size)
    out = np.zeros(mt.size, dtype=np.int64)
    _call("gsp_quantum_div", C.c_int(mt.size), _p(mt), _p(q), _p(magic), _p(out))
    return out


def add_ones(x, steps, cap):
    x = _in(x, np.float64)
    steps, cap = _in(steps, np.int64, x.size), _in(cap, np.float64, x.size)
    plain, capped = np.zeros(x.size, dtype=np.float64), np.zeros(x.size, dtype=np.float64)
    _call("gsp_add_ones", C.c_int(x.size), _p(x), _p(steps), _p(cap), _p(plain), _p(capped))
    return plain, capped


def ptx_hash(keys_, hbits):
    keys_ = _in(keys_, np.uint32)
    out = np.zeros(keys_.size, dtype=np.int32)
    _call("gsp_ptx_hash", C.c_int(keys_.size), _p(keys_), C.c_int(hbits), _p(out))
    return out


class PeerTx:
    """The peertx tables of n_nodes nodes (rows of 2^bits entries) and their
    overflow table (2^obits entries), kept on the host between calls."""

    def __init__(self, bits, obits, gr, n_nodes=1):
        self.bits, self.obits, self.gr, self.n_nodes = bits, obits, gr, n_nodes
        self.rows = np.zeros(n_nodes << bits, dtype=np.uint32)
        self.ovf = np.zeros(1 << obits, dtype=np.uint64)
        self.ocnt = np.zeros(3, dtype=np.uint32)
        self.ptxn = np.zeros(n_nodes, dtype=np.int32)  # Dev::ptxN, kept as the engine keeps it
        self.err = np.zeros(1, dtype=np.int32)

    def run(self, rounds=(), queries=()):
        """rounds: a list of rounds, each a list of (node, key) increments run
        concurrently (keys of a node distinct within a round); queries: (node,
        key) lookups afterwards.  Returns (ret, ins) per round and (ptx_count_g,
        ptxo_count) per query."""
        per = max((len(r) for r in rounds), default=0)
        node = np.full((len(rounds), max(per, 1)), -1, dtype=np.int32)
        key = np.zeros((len(rounds), max(per, 1)), dtype=np.uint32)
        for i, r in enumerate(rounds):
            for j, (v, k) in enumerate(r):
                node[i, j], key[i, j] = v, k
        ret = np.zeros(node.shape, dtype=np.int32)
        ins = np.zeros(node.shape, dtype=np.uint8)
        qn = _in([v for v, _ in queries], np.int32)
        qk = _in([k for _, k in queries], np.uint32)
        cg, co = np.zeros(qn.size, dtype=np.int32), np.zeros(qn.size, dtype=np.int32)
        _call("gsp_peertx", C.c_int(self.bits), C.c_int(self.obits), C.c_int(self.gr), C.c_int(self.n_nodes),
              _p(self.rows), _p(self.ovf), _p(self.ocnt), _p(self.err), C.c_int(len(rounds)), C.c_int(per if rounds else 0),
              _p(node), _p(key), _p(ret), _p(ins), C.c_int(qn.size), _p(qn), _p(qk), _p(cg), _p(co))
        out = [(ret[i, :len(r)].copy(), ins[i, :len(r)].astype(bool)) for i, r in enumerate(rounds)]
        for r, (_, inserted) in zip(rounds, out):  # handleIWant's pass: ptxN[v] += inserts (of either table)
            for (v, _), i in zip(r, inserted):
                self.ptxn[v] += int(i)
        return out, cg, co

    def rebuild(self, hist, last):
        """The heartbeat's rebuild, once: hist is the mcache ring [R][n_nodes][W]
        of uint64 words, `last` the ring row of the window leaving the cache."""
        hist = np.ascontiguousarray(hist, dtype=np.uint64)
        r, n, w = hist.shape
        if n != self.n_nodes:
            raise ValueError("hist is [R][n_nodes][W]")
        _call("gsp_ptx_rebuild", C.c_int(self.bits), C.c_int(self.obits), C.c_int(self.n_nodes), _p(self.rows),
              _p(self.ptxn), _p(self.ovf), _p(self.ocnt), C.c_int(r), C.c_int(w), C.c_int(last), _p(hist))


def spam(s, gr, cnt, rounds=(), retire=None):
    """cnt: spamCnt [rows][s / 8] uint32, updated in place.  rounds: lists of
    (row, slot) spam_incr calls run concurrently ((row, slot) distinct within a
    round); returns the returned count of every call, per round.  retire: None,
    or a dict for one launch of k_retire afterwards: cur, rowptr [nodes + 1],
    spam_row [edges] or None, pubmask [s / 64], words, pmask_row [nodes] or
    None, pmask [rows][s] uint64 (updated in place)."""
    if cnt.dtype != np.uint32 or not cnt.flags.c_contiguous or cnt.ndim != 2 or cnt.shape[1] != s // 8:
        raise ValueError("cnt is a contiguous uint32 array [rows][s / 8]")
    per = max((len(r) for r in rounds), default=0)
    row = np.full((len(rounds), max(per, 1)), -1, dtype=np.int32)
    slot = np.zeros(row.shape, dtype=np.int32)
    for i, r in enumerate(rounds):
        for j, (a, b) in enumerate(r):
            row[i, j], slot[i, j] = a, b
    ret = np.zeros(row.shape, dtype=np.int32)
    null = C.c_void_p(None)
    if retire is None:
        tail = (C.c_int(0), C.c_int(0), C.c_int(0), null, null, null, C.c_int(0), null, null, C.c_int(0), null)
    else:
        rowptr = _in(retire["rowptr"], np.int64)
        n_nodes = rowptr.size - 1
        spam_row = None if retire.get("spam_row") is None else _in(retire["spam_row"], np.int32, int(rowptr[-1]))
        pubmask = _in(retire["pubmask"], np.uint64, s // 64)
        words = _in(retire["words"], np.int32)
        pmask_row = None if retire.get("pmask_row") is None else _in(retire["pmask_row"], np.int32, n_nodes)
        pmask = retire.get("pmask")
        n_pm = 0
        if pmask_row is not None:
            if pmask.dtype != np.uint64 or not pmask.flags.c_contiguous or pmask.ndim != 2 or pmask.shape[1] != s:
                raise ValueError("pmask is a contiguous uint64 array [rows][s]")
            n_pm = pmask.shape[0]
        tail = (C.c_int(1), C.c_int(retire["cur"]), C.c_int(n_nodes), _p(rowptr), null if spam_row is None else _p(spam_row),
                _p(pubmask), C.c_int(words.size), _p(words), null if pmask_row is None else _p(pmask_row), C.c_int(n_pm),
                null if pmask_row is None else _p(pmask))
    _call("gsp_spam", C.c_int(s), C.c_int(gr), C.c_int(cnt.shape[0]), _p(cnt), C.c_int(len(rounds)),
          C.c_int(per if rounds else 0), _p(row), _p(slot), _p(ret), *tail)
    return [ret[i, :len(r)].copy() for i, r in enumerate(rounds)]


def pool_take(sub, s0_mask, sub_cap, base0, cur, n, cnt=None):
    """One launch of len(n) blocks, lane 0 of block b calling pool_take(d, cur,
    n[b]); a block with n[b] == 0 makes no call.  Returns (result per block as uint64, poolCnt [2][sub][16] after,
    err); cnt: poolCnt before (default zeros)."""
    n = _in(n, np.uint64)
    cnt = np.zeros(2 * sub * 16, dtype=np.uint64) if cnt is None else _in(cnt, np.uint64, 2 * sub * 16).copy()
    out = np.zeros(n.size, dtype=np.uint64)
    err = np.zeros(1, dtype=np.int32)
    _call("gsp_pool_take", C.c_int(sub), C.c_int(s0_mask), C.c_int64(sub_cap), C.c_int64(base0), C.c_int(cur),
          C.c_int(n.size), _p(n), _p(out), _p(cnt), _p(err))
    return out, cnt.reshape(2, sub, 16), int(err[0])
