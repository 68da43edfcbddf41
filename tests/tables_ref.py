"""Plain Python references, seeded case tables and checkers for the "counter
under atomics with a spill" tables of the device code:

  * the heartbeat's peertx rebuild (k_ptx_rebuild, k_ptxo_collect,
    k_ptxo_reinsert, k_ptxo_fin of csrc/gs_kernels_ctl.h),
  * the IWANT spammers' nibble counters (spam_incr of csrc/gs_device.h and
    their clear in k_retire of csrc/gs_kernels.h),
  * pool_take's hand-on across sub-arenas (csrc/gs_device.h).

The reference of the peertx tables is mcache.peertx itself: a dict (node, key)
-> count.  A rebuild drops the entries whose message slot has its bit set in
the node's bitmap hist[last][node]; everything else survives with its count.
Which slot an entry lands in depends on the race, so check_tables compares the
tables as multisets.  The model also follows which table holds each entry, as
far as the tables' rules decide it (a key goes to the overflow table exactly
when its node's row is full), so that the CPU test can count, from the model
alone, how many entries every rebuild of every case drops, moves home and
leaves in the overflow table (tests/test_tables_ref.py).  HostTables is a
sequential emulation of the same tables: the CPU test runs every case through
it to check the cases, the model and the checker against each other; the GPU
tests run the same cases through the probe (tests/probe.py)."""
import collections

import numpy as np

from select_ref import SEED

GR = 3
M32 = 0xFFFFFFFF


# ------------------------------------------------------------ peertx: layout
def ptx_key(slot, edge):
    """The 32-bit entry of (message slot < 2^14, in-edge < 64) with count 0."""
    return ((int(slot) << 14) | (int(edge) << 8)) & M32


def ptx_hash(key, bits):
    """ptx_hash of gs_kernels_ctl.h: the key's home slot in a row of 2^bits."""
    return ((int(key) * 0x9E3779B1) & M32) >> (32 - bits)


def ptxo_hash(tag, bits):
    x = int(tag) & ((1 << 64) - 1)
    x ^= x >> 29
    x = (x * 0xBF58476D1CE4E5B9) & ((1 << 64) - 1)
    x ^= x >> 32
    return x >> (64 - bits)


def leaves(lastw, v, key):
    """Does (node v, key) leave the cache: the bit of its slot in lastw [n][W]."""
    slot = int(key) >> 14
    return (int(lastw[v][slot >> 6]) >> (slot & 63)) & 1 == 1


# ------------------------------------------------------------- peertx: model
class PtxModel:
    """mcache.peertx of n nodes as a dict, plus which table holds each entry.
    `exact` says whether that placement is decided by the tables' rules alone;
    it is not after a round with more new keys of a node than its row has free
    slots (unless it has none), or after a rebuild in which only some of a
    node's overflow survivors fit at home: then the race picks which ones.  The
    counts per node stay exact either way."""

    def __init__(self, bits, n_nodes, gr=GR):
        self.bits, self.hn, self.n, self.gr = bits, 1 << bits, n_nodes, gr
        self.count = {}
        self.in_ovf = set()
        self.gone = set()  # dropped by a rebuild and not inserted since
        self.rown, self.ovfn = [0] * n_nodes, [0] * n_nodes
        self.exact = True

    def incr_round(self, round_):
        """One round of concurrent increments; the expected (ret, ins) of each."""
        assert len(set(round_)) == len(round_), "a round names a (node, key) once"
        new = collections.Counter(v for v, k in round_ if (v, k) not in self.count)
        for v, c in new.items():
            free = self.hn - self.rown[v]
            if free and c > free:
                self.exact = False
        exp = []
        for v, k in round_:
            old = self.count.get((v, k), 0)
            exp.append((min(old + 1, self.gr + 2), old == 0))
            self.count[(v, k)] = min(old + 1, self.gr + 1)
            if old == 0:
                self.gone.discard((v, k))
                if self.rown[v] < self.hn:
                    self.rown[v] += 1
                else:
                    self.ovfn[v] += 1
                    self.in_ovf.add((v, k))
        return exp

    def rebuild(self, lastw):
        """The heartbeat's rebuild.  Returns what it did: entries leaving from
        the rows / from the overflow table, overflow survivors going home /
        staying, the passes of k_ptx_rebuild's k0 loop, and whether the split
        between the tables was decided by the rules alone."""
        st = {"leave_row": 0, "leave_ovf": 0, "home": 0, "stay": 0, "passes": max(1, self.hn // 256),
              "exact": self.exact, "rebuilt_nodes": sum(1 for c in self.rown if c),
              "skipped_nodes": sum(1 for c in self.rown if not c)}
        surv = collections.defaultdict(list)
        for v, k in sorted(self.count):
            if leaves(lastw, v, k):
                if (v, k) in self.in_ovf:
                    st["leave_ovf"] += 1
                    self.in_ovf.discard((v, k))
                    self.ovfn[v] -= 1
                else:
                    st["leave_row"] += 1
                    self.rown[v] -= 1
                del self.count[(v, k)]
                self.gone.add((v, k))
            elif (v, k) in self.in_ovf:
                surv[v].append(k)
        for v, ks in surv.items():
            go = min(self.hn - self.rown[v], len(ks))
            if 0 < go < len(ks):
                self.exact = False
            for k in ks[:go]:
                self.in_ovf.discard((v, k))
            self.rown[v] += go
            self.ovfn[v] -= go
            st["home"] += go
            st["stay"] += len(ks) - go
        return st

    def place(self, in_ovf):
        """Take the placement from the tables themselves (after check_tables)."""
        self.in_ovf = set(in_ovf)
        self.ovfn = [0] * self.n
        for v, _ in self.in_ovf:
            self.ovfn[v] += 1
        per = collections.Counter(v for v, _ in self.count)
        self.rown = [per[v] - self.ovfn[v] for v in range(self.n)]
        self.exact = True


def check_round(exp, ret, ins):
    for i, ((r, n), gr, gi) in enumerate(zip(exp, ret, ins)):
        assert int(gr) == r and bool(gi) == n, f"increment {i}: returned {int(gr)} ins {bool(gi)}, expected {r} ins {n}"


def check_tables(m, rows, ovf, ocnt, ptxn=None):
    """Every entry of the model present exactly once across its node's row and
    the overflow table, with its count; no other non-zero word (a departed
    key, another node's key); ptxOCnt == [overflow entries, 0, 0]; a node with
    an overflow entry has no zero word in its row (ptx_count_g stops at one);
    with ptxn (right after a rebuild): ptxN[v] == non-zero words of row v.
    Returns the set of (node, key) in the overflow table."""
    rows = np.asarray(rows).reshape(m.n, m.hn)
    found = collections.Counter()
    row_nz = []
    for v in range(m.n):
        nz = 0
        for w in rows[v].tolist():
            if not w:
                continue
            nz += 1
            k = w & 0xFFFFFF00
            assert (v, k) in m.count, f"row {v} holds {w:#x}: not a live key of this node"
            assert w & 0xFF == m.count[(v, k)], f"row {v}: {w:#x} should count {m.count[(v, k)]}"
            found[(v, k)] += 1
        row_nz.append(nz)
        if ptxn is not None:
            assert int(ptxn[v]) == nz, f"ptxN[{v}] = {int(ptxn[v])}, row has {nz} entries"
    in_ovf = set()
    for w in np.asarray(ovf).tolist():
        if not w:
            continue
        v, k = (w >> 32) - 1, w & 0xFFFFFF00
        assert 0 <= v < m.n and (v, k) in m.count, f"overflow table holds {w:#x}: not a live key"
        assert w & 0xFF == m.count[(v, k)], f"overflow: {w:#x} should count {m.count[(v, k)]}"
        assert row_nz[v] == m.hn, f"node {v} has an overflow entry {w:#x} and {m.hn - row_nz[v]} free slots in its row"
        found[(v, k)] += 1
        in_ovf.add((v, k))
    missing = [f"({v}, {k:#x})" for v, k in m.count if found[(v, k)] == 0]
    twice = [f"({v}, {k:#x})" for (v, k), c in found.items() if c > 1]
    assert not missing and not twice, f"lost: {missing[:8]} twice: {twice[:8]}"
    assert [int(x) for x in ocnt] == [len(in_ovf), 0, 0], f"ptxOCnt {list(ocnt)} with {len(in_ovf)} overflow entries"
    assert [row_nz[v] for v in range(m.n)] == m.rown and len(in_ovf) == sum(m.ovfn)
    return in_ovf


# ------------------------------------------- peertx: a sequential emulation
class HostTables:
    """The tables of probe.PeerTx emulated one operation at a time: the same
    layout, hashes, probe sequences and rebuild rules, no race (a round runs in
    order).  For the CPU test of the cases; the GPU tests do not use it."""

    def __init__(self, bits, obits, gr, n_nodes=1):
        self.bits, self.obits, self.gr, self.n_nodes = bits, obits, gr, n_nodes
        self.rows = np.zeros(n_nodes << bits, dtype=np.uint32)
        self.ovf = np.zeros(1 << obits, dtype=np.uint64)
        self.ocnt = np.zeros(3, dtype=np.uint32)
        self.ptxn = np.zeros(n_nodes, dtype=np.int32)

    def _row_find(self, v, key, insert):
        """(index, found) of key in row v, probing from its home slot; with
        insert a free slot ends the probe; (-1, False) after a full circle."""
        hn = 1 << self.bits
        h = ptx_hash(key, self.bits)
        for p in range(hn):
            i = (v << self.bits) + ((h + p) & (hn - 1))
            w = int(self.rows[i])
            if w == 0:
                return (i, False) if insert else (-2, False)
            if w & 0xFFFFFF00 == key:
                return i, True
        return -1, False

    def _ovf_find(self, v, key):
        tag = ((v + 1) << 32) | key
        n = 1 << self.obits
        h = ptxo_hash(tag, self.obits)
        for p in range(n):
            i = (h + p) & (n - 1)
            w = int(self.ovf[i])
            if w == 0:
                return i, False, tag
            if w & ~0xFF == tag:
                return i, True, tag
        raise AssertionError("the cases never fill the overflow table")

    def _bump(self, tab, i):
        c = (int(tab[i]) & 0xFF) + 1
        if c <= self.gr + 1:
            tab[i] += 1
        return c

    def incr(self, v, key):
        i, hit = self._row_find(v, key, True)
        if i >= 0:
            if hit:
                return self._bump(self.rows, i), False
            self.rows[i] = key | 1
            self.ptxn[v] += 1
            return 1, True
        i, hit, tag = self._ovf_find(v, key)
        if hit:
            return self._bump(self.ovf, i), False
        self.ovf[i] = tag | 1
        self.ocnt[0] += 1
        self.ptxn[v] += 1
        return 1, True

    def run(self, rounds=(), queries=()):
        out = []
        for r in rounds:
            got = [self.incr(v, k) for v, k in r]
            out.append((np.array([g[0] for g in got], dtype=np.int32), np.array([g[1] for g in got], dtype=bool)))
        cg, co = [], []
        for v, k in queries:
            i, hit = self._row_find(v, k, False)
            j, ohit, _ = self._ovf_find(v, k)
            o = int(self.ovf[j]) & 0xFF if ohit else 0
            cg.append(int(self.rows[i]) & 0xFF if hit else (o if i == -1 else 0))  # -1: a full row, on to the overflow table
            co.append(o)
        return out, np.array(cg, dtype=np.int32), np.array(co, dtype=np.int32)

    def rebuild(self, hist, last):
        lastw = hist[last]
        hn = 1 << self.bits
        for v in range(self.n_nodes):
            if self.ptxn[v] == 0:
                continue
            old = self.rows[v << self.bits:(v + 1) << self.bits].copy()
            self.rows[v << self.bits:(v + 1) << self.bits] = 0
            kept = 0
            for w in old.tolist():
                if w and not leaves(lastw, v, w):
                    i, _ = self._row_find(v, w & 0xFFFFFF00, True)
                    self.rows[i] = w
                    kept += 1
            self.ptxn[v] = kept
        if self.ocnt[0] == 0:
            return
        stage = [w for w in self.ovf.tolist() if w and not leaves(lastw, (w >> 32) - 1, w & M32)]
        self.ovf[:] = 0
        kept = 0
        for w in stage:
            v, ent = (w >> 32) - 1, w & M32
            i, _ = self._row_find(v, ent & 0xFFFFFF00, True)
            if i >= 0:
                self.rows[i] = ent
                self.ptxn[v] += 1
                continue
            j, _, _ = self._ovf_find(v, ent & 0xFFFFFF00)
            self.ovf[j] = w
            kept += 1
        self.ocnt[:] = (kept, 0, 0)
        assert hn == self.rows.size // self.n_nodes


# ------------------------------------------------------- peertx: case tables
def _universe(rng, w):
    """Every key of the slots [0, 64 w) at every in-edge, shuffled."""
    u = rng.permutation(64 * w * 64)
    return [ptx_key(x >> 6, x & 63) for x in u.tolist()]


def _unique_slot_keys(rng, w, n):
    """n keys with n different slots (so a bitmap drops them one by one)."""
    slots = rng.permutation(64 * w)[:n].tolist()
    return [ptx_key(s, e) for s, e in zip(slots, rng.integers(0, 64, n).tolist())]


def _lastw(n, w, slots_of):
    """[n][w] bitmaps with the bits of slots_of[v] set ('all': every bit)."""
    out = np.zeros((n, w), dtype=np.uint64)
    for v in range(n):
        if isinstance(slots_of[v], str):
            out[v, :] = np.uint64((1 << 64) - 1)
            continue
        for s in slots_of[v]:
            out[v, s >> 6] |= np.uint64(1 << (s & 63))
    return out


def hist_ring(r, last, lastw):
    """The ring [r][n][w]: row `last` = lastw, every other row its complement,
    so a wrong ring row gives every entry the opposite verdict."""
    h = np.empty((r,) + lastw.shape, dtype=np.uint64)
    h[:] = ~lastw
    h[last] = lastw
    return h


def _slots(keys):
    return sorted({k >> 14 for k in keys})


def _count_rounds(keys_of, gr):
    """Rounds after the inserting one that spread the counts: every other key
    once more, then the first quarter of every node's keys up to gr + 1 and
    twice past it, the second quarter once more."""
    second = [(v, k) for v, ks in keys_of.items() for k in ks[::2]]
    quarter = [(v, k) for v, ks in keys_of.items() for k in ks[:max(1, len(ks) // 4)]]
    next_q = [(v, k) for v, ks in keys_of.items() for k in ks[max(1, len(ks) // 4):2 * max(1, len(ks) // 4)]]
    return [second] + [quarter] * (gr + 2) + [next_q]


def _case(name, bits, obits, n, w, r, steps, **tags):
    return dict(name=name, bits=bits, obits=obits, n_nodes=n, w=w, r=r, steps=steps, **tags)


FIVE = ("half", "keep", "empty", "drop", "half")
FOUR = ("half", "keep", "drop", "half")


def _full_rows_case(rng, bits, last, r, roles=FIVE):
    """Nodes side by side with different keys, every row full: a 'keep' node
    keeps everything (the rebuild fills its whole LDS table), a 'drop' node
    drops everything, a 'half' node drops about half of its keys;
    an 'empty' node has no entry (ptxN == 0, skipped) between full ones."""
    w, hn, n = 4, 1 << bits, len(roles)
    uni = _universe(rng, w)
    keys_of = {v: uni[v * hn:(v + 1) * hn] for v in range(n) if roles[v] != "empty"}
    first = [(v, k) for v, ks in keys_of.items() for k in ks]
    slots_of = []
    for v in range(n):
        if roles[v] == "keep":
            slots_of.append([])
        elif roles[v] == "drop":
            slots_of.append("all")
        elif roles[v] == "empty":
            slots_of.append(rng.permutation(64 * w)[:100].tolist())  # (no entries to drop)
        elif hn <= 16:
            ks = keys_of[v]
            slots_of.append(_slots([ks[i] for i in rng.permutation(len(ks))[:max(1, len(ks) // 2)].tolist()]))
        else:  # (many keys per slot: half of the slots)
            slots_of.append(rng.permutation(64 * w)[:32 * w].tolist())
    lastw = _lastw(n, w, slots_of)
    # afterwards every key again (the departed insert, the survivors go on) and
    # the empty node's first keys, then on to the cap
    keys_of2 = dict(keys_of)
    for v in range(n):
        if roles[v] == "empty":
            keys_of2[v] = uni[n * hn:n * hn + max(1, hn // 2)]
    again = [(v, k) for v, ks in keys_of2.items() for k in ks]
    steps = [("incr", [first] + _count_rounds(keys_of, GR)), ("rebuild", last, hist_ring(r, last, lastw)),
             ("incr", [again] + _count_rounds(keys_of2, GR))]
    return _case(f"rows{hn}_last{last}of{r}", bits, 6, n, w, r, steps, kind="full_rows", roles=roles)


def _same_home_keys(bits, n, w=4):
    """n keys of one home slot in a row of 2^bits (the fullest home slot)."""
    by = collections.defaultdict(list)
    for s in range(64 * w):
        for e in range(64):
            by[ptx_hash(ptx_key(s, e), bits)].append(ptx_key(s, e))
    keys = max(by.values(), key=len)
    # different slots, so that the bitmap can drop them one by one
    seen, out = set(), []
    for k in keys:
        if k >> 14 not in seen:
            seen.add(k >> 14)
            out.append(k)
    assert len(out) >= n
    return out[:n]


def _same_home_case(bits=6, n_keys=24):
    """One probe chain: n_keys keys of one home slot; the rebuild drops every
    third of them, and a lookup of a survivor must not stop at the hole a
    departed key would have left.  Two nodes hold the same chain; the second
    keeps it whole."""
    keys = _same_home_keys(bits, n_keys)
    first = [(v, k) for v in range(2) for k in keys]
    lastw = _lastw(2, 4, [_slots(keys[::3]), []])
    steps = [("incr", [first, first[::2]]), ("rebuild", 1, hist_ring(2, 1, lastw)), ("incr", [first, first])]
    return _case(f"one_home_slot_row{1 << bits}", bits, 6, 2, 4, 2, steps, kind="same_home", chain=keys)


def _top_slot_case(rng):
    """W = 256: slots up to 2^14 - 1 (the `slot >> 6` word index, the
    `x >> 14` decode of an entry's top bit, 27), in rows of 4 that spill, so the overflow
    table's decode sees them too."""
    w, top = 256, (1 << 14) - 1
    slots = [top, top - 1, top - 63, top - 64, 8192, 8191, 64, 63, 1, 0, 12345, 4242]
    keys = [ptx_key(s, e) for s, e in zip(slots, [63, 0, 17, 63, 1, 62, 5, 63, 0, 0, 33, 63])]
    order = {0: keys, 1: keys[::-1], 2: keys[3:] + keys[:3]}  # which four get the row differs by node
    rounds = [[(v, ks[i]) for v, ks in order.items()] for i in range(len(keys))]
    lastw = _lastw(3, w, [[top, 64, 8192, 12345], [top - 64, 0, 63, top - 1, 4242], [top]])
    steps = [("incr", rounds + [rounds[0] + rounds[5]]), ("rebuild", 1, hist_ring(2, 1, lastw)),
             ("incr", [[(v, k) for v in range(3) for k in keys]])]
    return _case("w256_top_slot", 2, 6, 3, w, 2, steps, kind="top_slot", top_key=ptx_key(top, 63))


def _spill_case(rng, name, n_row_leave, n_ovf, n_ovf_leave, n=2):
    """Rows of 4, full, with n_ovf more keys per node in the overflow table;
    the rebuild drops n_row_leave row keys and n_ovf_leave overflow keys of
    every node (each node has its own keys)."""
    w = 4
    steps, slots_of, fill, spill = [], [], [], []
    for v in range(n):
        ks = _unique_slot_keys(rng, w, 4 + n_ovf)
        fill += [(v, k) for k in ks[:4]]
        spill += [(v, k) for k in ks[4:]]
        slots_of.append(_slots(ks[:n_row_leave] + ks[4:4 + n_ovf_leave]))
    every = fill + spill
    steps = [("incr", [fill, spill, every[::2], every[::3]]), ("rebuild", 0, hist_ring(1, 0, _lastw(n, w, slots_of))),
             ("incr", [every[::2], every[1::2], every])]
    return _case(name, 2, 6, n, w, 1, steps, kind="spill")


def _same_keys_case(rng):
    """Three nodes with the same ten keys: four in the row, six in the overflow
    table, where only the node tag tells them apart; every node drops others."""
    w = 4
    ks = _unique_slot_keys(rng, w, 10)
    fill = [(v, k) for v in range(3) for k in ks[:4]]
    spill = [(v, k) for v in range(3) for k in ks[4:]]
    lastw = _lastw(3, w, [_slots(ks[4:6]), _slots([ks[0], ks[6]]), []])
    steps = [("incr", [fill, spill, spill[::2]]), ("rebuild", 2, hist_ring(3, 2, lastw)), ("incr", [fill + spill])]
    return _case("same_keys_three_nodes", 2, 6, 3, w, 3, steps, kind="same_keys")


def _ovf_empties_case(rng):
    """Every overflow entry leaves: ptxOCnt[0] returns to 0 and the next
    rebuild's overflow kernels return at once (its row kernel still runs)."""
    w = 4
    ks = {v: _unique_slot_keys(rng, w, 9) for v in range(2)}
    fill = [(v, k) for v in range(2) for k in ks[v][:4]]
    spill = [(v, k) for v in range(2) for k in ks[v][4:]]
    first = _lastw(2, w, [_slots(ks[v][4:]) for v in range(2)])
    second = _lastw(2, w, [_slots(ks[0][:2]), []])
    steps = [("incr", [fill, spill]), ("rebuild", 0, hist_ring(2, 0, first)), ("rebuild", 1, hist_ring(2, 1, second)),
             ("incr", [fill + spill])]
    return _case("overflow_empties", 2, 6, 2, w, 2, steps, kind="ovf_empties")


def _cadence_case(rng):
    """The heartbeat cadence: increments, a rebuild, increments on the rebuilt
    tables (new keys and old ones), a second rebuild, increments.  The rounds
    are cut so that the rules decide which table takes every key (the model
    stays exact through both rebuilds)."""
    w, n, bits = 4, 3, 2
    m = PtxModel(bits, n)
    pool = {v: _unique_slot_keys(rng, w, 40) for v in range(n)}
    used = {v: 0 for v in range(n)}

    def fresh(v, c):
        out = pool[v][used[v]:used[v] + c]
        used[v] += c
        return [(v, k) for k in out]

    def fill_then_spill(extra):
        """rounds that fill every row's free slots, then spill `extra` keys per node"""
        a = [x for v in range(n) for x in fresh(v, m.hn - m.rown[v])]
        b = [x for v in range(n) for x in fresh(v, extra[v])]
        rounds = [r for r in (a, b) if r]
        for r in rounds:
            m.incr_round(r)
        return rounds

    steps = []
    rounds = fill_then_spill([3, 0, 5])
    live = sorted(m.count)
    rounds.append(live[::2])
    m.incr_round(live[::2])
    steps.append(("incr", rounds))
    # rebuild 1: node 0 drops three row keys and keeps its three overflow keys
    # (all go home), node 1 drops one, node 2 keeps its row and drops two of
    # its five overflow keys (none goes home)
    row_keys = {v: [k for u, k in live if u == v and (u, k) not in m.in_ovf] for v in range(n)}
    ovf_keys = {v: [k for u, k in live if u == v and (u, k) in m.in_ovf] for v in range(n)}
    lastw = _lastw(n, w, [_slots(row_keys[0][:3]), _slots(row_keys[1][:1]), _slots(ovf_keys[2][:2])])
    m.rebuild(lastw)
    steps.append(("rebuild", 1, hist_ring(3, 1, lastw)))
    assert m.exact
    rounds = fill_then_spill([2, 4, 0])
    live = sorted(m.count)
    for r in (live, live[::3]):
        rounds.append(r)
        m.incr_round(r)
    steps.append(("incr", rounds))
    # rebuild 2: every node drops some of both tables
    drop = []
    for v in range(n):
        rk = [k for u, k in live if u == v and (u, k) not in m.in_ovf]
        ok = [k for u, k in live if u == v and (u, k) in m.in_ovf]
        drop.append(_slots(rk[:2] + ok[:1]))
    lastw = _lastw(n, w, drop)
    assert m.exact
    m.rebuild(lastw)
    steps.append(("rebuild", 0, hist_ring(3, 0, lastw)))
    gone = sorted(m.gone)
    steps.append(("incr", [sorted(m.count), gone[:1] + sorted(m.count)]))
    return _case("two_rebuilds", bits, 6, n, w, 3, steps, kind="cadence")


def rebuild_cases():
    """The case tables of the rebuild.  A case: the table sizes, the ring's
    shape and steps ('incr', rounds) / ('rebuild', last, hist [r][n][w])."""
    rng = np.random.default_rng(SEED + 100)
    cases = [
        # rows smaller than the wave's 256-entry read, neighbours on both sides
        _full_rows_case(rng, 2, 0, 3), _full_rows_case(rng, 4, 2, 3), _full_rows_case(rng, 6, 1, 3),
        _full_rows_case(rng, 7, 0, 1),
        # the k0 loop: 1, 2 and 4 passes
        _full_rows_case(rng, 8, 2, 3, FOUR), _full_rows_case(rng, 9, 0, 2, FOUR), _full_rows_case(rng, 10, 0, 3, FOUR),
        _same_home_case(),
        _top_slot_case(rng),
        _spill_case(rng, "spill_all_fit", n_row_leave=3, n_ovf=3, n_ovf_leave=0),
        _spill_case(rng, "spill_some_fit", n_row_leave=2, n_ovf=7, n_ovf_leave=1),
        _spill_case(rng, "spill_none_fit", n_row_leave=0, n_ovf=6, n_ovf_leave=2),
        _same_keys_case(rng),
        _ovf_empties_case(rng),
        _cadence_case(rng),
    ]
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


def absent_keys(case, model, n=300):
    """n (node, key) pairs the model has never held, colliding with its keys'
    home slots like any other (the same slots and in-edges)."""
    rng = np.random.default_rng(SEED + 101)
    slots = rng.integers(0, 64 * case["w"], 4 * n).tolist()
    edges = rng.integers(0, 64, 4 * n).tolist()
    out = []
    for i, (s, e) in enumerate(zip(slots, edges)):
        x = (i % case["n_nodes"], ptx_key(s, e))
        if x not in model.count and x not in model.gone and x not in out:
            out.append(x)
    assert len(out) >= n
    return out[:n]


def run_case(case, tx, on_rebuild=None):
    """Runs a case on `tx` (probe.PeerTx on the GPU, HostTables on the CPU)
    against the model, with every check after every step.  Returns the
    rebuilds' statistics.  A full circle of checks after a rebuild: the tables
    as multisets, ptxN, the counters, then ptx_count_g / ptxo_count of every
    survivor, every departed key and a few hundred absent ones."""
    m = PtxModel(case["bits"], case["n_nodes"], tx.gr)
    stats = []
    for step in case["steps"]:
        if step[0] == "incr":
            for r, (ret, ins) in zip(step[1], tx.run(rounds=step[1])[0]):
                check_round(m.incr_round(r), ret, ins)
            m.place(check_tables(m, tx.rows, tx.ovf, tx.ocnt))
            continue
        _, last, hist = step
        exact = m.exact
        st = m.rebuild(hist[last])
        tx.rebuild(hist, last)
        in_ovf = check_tables(m, tx.rows, tx.ovf, tx.ocnt, tx.ptxn)
        if exact and m.exact:
            assert in_ovf == m.in_ovf, "the rules decide which entries stay in the overflow table here"
        m.place(in_ovf)
        q = sorted(m.count) + sorted(m.gone) + absent_keys(case, m)
        _, cg, co = tx.run(queries=q)
        for (v, k), g, o in zip(q, cg, co):
            assert int(g) == m.count.get((v, k), 0), f"ptx_count_g({v}, {k:#x}) = {int(g)}, model {m.count.get((v, k), 0)}"
            assert int(o) == (m.count[(v, k)] if (v, k) in in_ovf else 0), f"ptxo_count({v}, {k:#x}) = {int(o)}"
        stats.append(st)
        if on_rebuild is not None:
            on_rebuild(st)
    return stats


# ------------------------------------------------------------ spam nibbles
class SpamModel:
    """spamCnt as an array of nibbles [rows][s]."""

    def __init__(self, rows, s, gr):
        self.nib = np.zeros((rows, s), dtype=np.int64)
        self.gr = gr

    def words(self):
        """The nibbles packed as spamCnt [rows][s / 8]."""
        sh = (4 * (np.arange(self.nib.shape[1]) & 7)).astype(np.uint64)
        w = self.nib.astype(np.uint64) << sh
        return np.bitwise_or.reduce(w.reshape(self.nib.shape[0], -1, 8), axis=2).astype(np.uint32)

    def incr(self, row, slot):
        """spam_incr: returns min(old + 1, gr + 2), stores min(old + 1, gr + 1)."""
        old = int(self.nib[row, slot])
        self.nib[row, slot] = min(old + 1, self.gr + 1)
        return min(old + 1, self.gr + 2)

    def retire(self, rowptr, spam_row, pubmask, words):
        """k_retire's spamCnt half: the nibbles of pubmask's bits in the listed
        words, in the rows of every node's spammer edges."""
        for v in range(len(rowptr) - 1):
            for e in range(rowptr[v], rowptr[v + 1]):
                if spam_row[e] < 0:
                    continue
                for w in words:
                    for b in range(64):
                        if (int(pubmask[w]) >> b) & 1:
                            self.nib[spam_row[e], 64 * w + b] = 0


# --------------------------------------------------------------- pool_take
def check_pool(sub, sub_cap, base0, n, out, cnt_cur, err, e_pool):
    """pool_take's contract for one launch on zeroed counters (sub_cap >= 1):
    the ranges handed out are disjoint and each lies inside one sub-arena of
    the segment [base0, base0 + sub * sub_cap); a request is refused (~0) only
    with E_POOL set, and err is E_POOL exactly when one was; a sub-arena's
    counter is at least what it handed out (it also counts the requests it
    passed on) and its padding words stay 0.  Returns (granted non-empty
    ranges, refused requests)."""
    none = (1 << 64) - 1
    taken = []
    refused = 0
    for b, (want, got) in enumerate(zip(np.asarray(n).tolist(), np.asarray(out).tolist())):
        if want == 0:  # (no call)
            continue
        if got == none:
            refused += 1
            continue
        assert base0 <= got and got + want <= base0 + sub * sub_cap, f"block {b}: [{got}, +{want}) outside the segment"
        s = (got - base0) // sub_cap if sub_cap else 0
        assert got + want <= base0 + (s + 1) * sub_cap, f"block {b}: [{got}, +{want}) straddles sub-arenas"
        taken.append((got, got + want, b))
    taken.sort()
    for (a0, a1, ba), (b0, b1, bb) in zip(taken, taken[1:]):
        assert a1 <= b0, f"blocks {ba} and {bb} share ids: [{a0}, {a1}) and [{b0}, {b1})"
    assert err == (e_pool if refused else 0), f"err {err} with {refused} refused requests"
    handed = collections.Counter()
    for a0, a1, _ in taken:
        handed[(a0 - base0) // sub_cap] += a1 - a0
    for s in range(sub):
        assert int(cnt_cur[s][0]) >= handed[s], f"sub-arena {s}: counter {int(cnt_cur[s][0])} < {handed[s]} handed out"
        assert not np.asarray(cnt_cur[s][1:]).any(), "the padding words of a counter stay 0"
    return len(taken), refused
