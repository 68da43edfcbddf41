"""Plain numpy / Python references, path models, seeded case tables and checkers
for the wave select and lane primitives of csrc/gs_device.h (select_k,
select_k_half, select_kth, select_kth_est, wave_incl_sum, wave_transpose64).

The references say WHAT the primitive computes (a sort); the path models
restate only the device code's branch conditions, so the CPU tests can assert
that the case tables reach every branch; the GPU tests run the same tables
through the probe (tests/probe.py) and hand the output to the checkers.

Domain: candidate ids are distinct and >= 0 (message ids; no call site
produces a negative one), keys are any uint64.  The constants GS_SEL_WIN and
GS_SEL_CAP are parameters everywhere: the tests read them from the probe."""
import numpy as np

U64 = (1 << 64) - 1
I64_MAX = (1 << 63) - 1
SEED = 20240611


# ---------------------------------------------------------------- references
def ref_select_k(cand, key, k):
    """Mask of the k smallest (key, lane) among the candidate lanes; k <= 0 or
    n <= k: every candidate."""
    lanes = [l for l in range(len(cand)) if cand[l]]
    if k <= 0 or len(lanes) <= k:
        take = lanes
    else:
        lanes = np.asarray(lanes)
        order = np.lexsort((lanes, np.asarray(key, dtype=np.uint64)[lanes]))
        take = lanes[order[:k]].tolist()
    return sum(1 << int(l) for l in take)


def ref_select_k_half(cand, key, k_lo, k_hi):
    """select_k within lanes 0..31 (k_lo) and within lanes 32..63 (k_hi)."""
    lo = ref_select_k(cand[:32], key[:32], k_lo)
    hi = ref_select_k(cand[32:], key[32:], k_hi)
    return lo | (hi << 32)


def ref_select_kth(keys, ids, k):
    """The k-th smallest (key, id), keys unsigned, ids signed; k above the
    candidate count (or an empty set): (2^64 - 1, INT64_MAX)."""
    keys = np.asarray(keys, dtype=np.uint64)
    ids = np.asarray(ids, dtype=np.int64)
    if k < 1 or k > len(keys):
        return U64, I64_MAX
    order = np.lexsort((ids, keys))
    j = order[k - 1]
    return int(keys[j]), int(ids[j])


def ref_select_kth_est(keys, ids, k):
    """select_kth_est answers "everything" (2^64 - 1, INT64_MAX) already at
    k == n; below that it is select_kth."""
    return (U64, I64_MAX) if k >= len(keys) else ref_select_kth(keys, ids, k)


def count_le(keys, ids, K, M):
    """Number of candidates with (key, id) <= (K, M): what the callers take."""
    keys = np.asarray(keys, dtype=np.uint64)
    ids = np.asarray(ids, dtype=np.int64)
    Ku = np.uint64(K)
    return int(np.count_nonzero((keys < Ku) | ((keys == Ku) & (ids <= np.int64(M)))))


def ref_transpose64(x):
    """Lane t gets column t of the 64 x 64 bit matrix whose row j is x[j]."""
    x = np.asarray(x, dtype="<u8")
    bits = np.unpackbits(x.view(np.uint8).reshape(64, 8), axis=1, bitorder="little")  # [row j][bit t]
    return np.packbits(bits.T.copy(), axis=1, bitorder="little").view("<u8").reshape(64)


def ref_incl_sum(x):
    """Inclusive prefix sum over the 64 lanes as int32 arithmetic does it."""
    return np.cumsum(np.asarray(x, dtype=np.int64)).astype(np.int32)


# --------------------------------------------------------------- path models
def model_select_k(cand, key, k):
    """The branches select_k takes: {'early': all candidates returned at once}
    or {'end_bit': the bit at which the loop breaks (None: it ran out), 'exit':
    'need0' | 'n_eq_need' | 'ran_out', 'tie_len': turns of the tie loop,
    'min_slack': the smallest n - need seen after a bit (the `n == need` exit
    needs 0)}."""
    act = [l for l in range(len(cand)) if cand[l]]
    n = len(act)
    if k <= 0 or n <= k:
        return {"early": True}
    need, end_bit, exit_, slack = k, None, "ran_out", n - k
    for b in range(63, -1, -1):
        z = [l for l in act if not (int(key[l]) >> b) & 1]
        if len(z) <= need:
            need -= len(z)
            act = [l for l in act if (int(key[l]) >> b) & 1]
        else:
            act = z
        n = len(act)
        slack = min(slack, n - need)
        if need == 0:
            end_bit, exit_ = b, "need0"
            break
        if n == need:
            end_bit, exit_ = b, "n_eq_need"
            break
    tie_len = min(need, len(act)) if exit_ == "ran_out" else 0
    return {"early": False, "end_bit": end_bit, "exit": exit_, "tie_len": tie_len, "min_slack": slack}


def model_select_kth(keys, k):
    """('above',) when k exceeds the count, ('pass', p) when the radix select
    leaves through its `inBin == 1` exit at pass p, ('tie', kk) when all 8
    passes ran and the tie loop makes kk turns."""
    keys = np.asarray(keys, dtype=np.uint64)
    prefix, kk = 0, k
    for p in range(7, -1, -1):
        sh = 8 * p
        hi_mask = 0 if p == 7 else (U64 << (sh + 8)) & U64
        m = keys[(keys & np.uint64(hi_mask)) == np.uint64(prefix & hi_mask)]
        hist = np.bincount(((m >> np.uint64(sh)) & np.uint64(255)).astype(np.int64), minlength=256)
        incl = np.cumsum(hist)
        if kk < 1 or kk > int(incl[-1]):
            return ("above",)
        digit = int(np.searchsorted(incl, kk))
        kk -= int(incl[digit] - hist[digit])
        prefix |= digit << sh
        if hist[digit] == 1:
            return ("pass", p)
    return ("tie", kk)


def model_select_kth_est(keys, k, n, win, cap):
    """Which way select_kth_est goes, from est, lo, hi, below, nc alone."""
    if k >= n:
        return {"path": "all"}
    est = (((k << 9) // n) + 1) >> 1
    lo, hi = max(0, est - win), min(255, est + win)
    top = (np.asarray(keys, dtype=np.uint64) >> np.uint64(56)).astype(np.int64)
    below = int(np.count_nonzero(top < lo))
    nc = int(np.count_nonzero((top >= lo) & (top <= hi)))
    if k <= below:
        path = "miss_low"
    elif k > below + nc:
        path = "miss_high"
    elif nc > cap:
        path = "overflow"
    else:
        path = "fast"
    return {"path": path, "est": est, "lo": lo, "hi": hi, "below": below, "nc": nc}


# --------------------------------------------------------------- case tables
def _key_sets(rng, n_lanes=64):
    """The key families of the wave selects, each a (name, keys[64]) pair."""
    base = int(rng.integers(0, 1 << 62)) << 1
    rnd = rng.integers(0, 1 << 64, n_lanes, dtype=np.uint64)
    bit0 = np.uint64(base & ~1) | rng.integers(0, 2, n_lanes, dtype=np.uint64)
    bit63 = np.uint64(base & ~(1 << 63)) | (rng.integers(0, 2, n_lanes, dtype=np.uint64) << np.uint64(63))
    equal = np.full(n_lanes, base | 1, dtype=np.uint64)
    return [("random", rnd), ("bit0", bit0), ("bit63", bit63), ("equal", equal)]


def _tie_groups(rng, cand, k):
    """Three key values over the candidates, in a random lane order, the middle
    value held by the candidates of rank k-2 .. k+1: the group straddles k."""
    v = np.sort(rng.integers(0, 1 << 64, 3, dtype=np.uint64))
    keys = np.full(64, v[2], dtype=np.uint64)
    lanes = rng.permutation(np.flatnonzero(cand))
    a = max(k - 2, 0)
    keys[lanes[:a]] = v[0]
    keys[lanes[a:a + 4]] = v[1]
    return keys


def _cand_masks(rng, n, lanes=64):
    """n candidates in the lowest lanes, and n at random (sparse) lanes."""
    dense = np.zeros(lanes, dtype=bool)
    dense[:n] = True
    sparse = np.zeros(lanes, dtype=bool)
    sparse[rng.permutation(lanes)[:n]] = True
    return [("dense", dense), ("sparse", sparse)]


def _exact_zeros(cand, bit, zeros, base):
    """Keys equal but for `bit`, which is 0 in the first `zeros` candidates."""
    keys = np.full(len(cand), np.uint64(base | (1 << bit)), dtype=np.uint64)
    keys[np.flatnonzero(cand)[:zeros]] = np.uint64(base & ~(1 << bit))
    return keys


def select_k_cases():
    """(name, cand[64], key[64], k) for select_k / grp_select<false>."""
    rng = np.random.default_rng(SEED)
    out = []
    for n in (0, 1, 2, 5, 6, 7, 31, 32, 33, 63, 64):
        for mname, cand in _cand_masks(rng, n):
            for k in sorted({-1, 0, 1, 6, n - 1, n, n + 1}):
                for kname, keys in _key_sets(rng):
                    out.append((f"{kname}-{mname}-n{n}-k{k}", cand, keys, k))
                if 1 <= k < n:
                    out.append((f"tiegroups-{mname}-n{n}-k{k}", cand, _tie_groups(rng, cand, k), k))
    # by construction: exactly k zeros at bit 63 / at bit 0 (the loop ends there
    # with need == 0), fewer zeros than k at bit 0 (the tie loop finishes)
    base = 0x5A5A5A5A5A5A5A5A & ~1 & ~(1 << 63)
    for mname, cand in _cand_masks(rng, 40):
        out.append((f"ends-bit63-{mname}", cand, _exact_zeros(cand, 63, 9, base), 9))
        out.append((f"ends-bit0-{mname}", cand, _exact_zeros(cand, 0, 9, base), 9))
        out.append((f"bit0-then-ties-{mname}", cand, _exact_zeros(cand, 0, 4, base), 9))
    return out


def select_k_half_cases():
    """(name, cand[64], key[64], k_lo, k_hi) for select_k_half / grp_select<true>."""
    rng = np.random.default_rng(SEED + 1)
    out = []
    for n_lo, n_hi in ((0, 0), (0, 20), (20, 0), (1, 32), (32, 1), (5, 7), (6, 6), (7, 5), (31, 32), (32, 32), (13, 29)):
        for mname in ("dense", "sparse"):
            pick = 0 if mname == "dense" else 1
            cand = np.concatenate([_cand_masks(rng, n_lo, 32)[pick][1], _cand_masks(rng, n_hi, 32)[pick][1]])
            for k_lo, k_hi in ((-1, 3), (0, 0), (1, 1), (6, 6), (n_lo, n_hi), (n_lo - 1, n_hi + 1), (n_lo + 1, n_hi - 1),
                               (3, 17), (17, 3)):
                for kname, keys in _key_sets(rng):
                    out.append((f"{kname}-{mname}-n{n_lo}+{n_hi}-k{k_lo}+{k_hi}", cand, keys, k_lo, k_hi))
                keys = np.empty(64, dtype=np.uint64)
                ok = True
                for h, (k, n) in enumerate(((k_lo, n_lo), (k_hi, n_hi))):
                    half = np.zeros(64, dtype=bool)
                    half[32 * h:32 * h + 32] = cand[32 * h:32 * h + 32]
                    ok = ok and 1 <= k < n
                    keys[32 * h:32 * h + 32] = _tie_groups(rng, half, max(k, 1))[32 * h:32 * h + 32] if half.any() else 0
                if ok:
                    out.append((f"tiegroups-{mname}-n{n_lo}+{n_hi}-k{k_lo}+{k_hi}", cand, keys, k_lo, k_hi))
    base = 0x3C3C3C3C3C3C3C3C & ~1 & ~(1 << 63)
    for mname in ("dense", "sparse"):
        pick = 0 if mname == "dense" else 1
        cand = np.concatenate([_cand_masks(rng, 20, 32)[pick][1], _cand_masks(rng, 24, 32)[pick][1]])
        lo = np.concatenate([cand[:32], np.zeros(32, dtype=bool)])
        hi = np.concatenate([np.zeros(32, dtype=bool), cand[32:]])
        for name, bit, z in (("ends-bit63", 63, 5), ("ends-bit0", 0, 5), ("bit0-then-ties", 0, 2)):
            keys = np.concatenate([_exact_zeros(lo, bit, z, base)[:32], _exact_zeros(hi, bit, z, base)[32:]])
            out.append((f"{name}-{mname}", cand, keys, 5, 5))
    return out


def _spread(rng, n):
    """Lane shares of n candidates: 65 ascending offsets, unequal, with empty
    lanes and lanes holding several."""
    style = int(rng.integers(0, 4))
    if style == 0:    # random cuts
        cuts = np.sort(rng.integers(0, n + 1, 63))
    elif style == 1:  # everything in a few lanes
        cuts = np.sort(rng.choice(np.array([0, n // 3, n]), 63))
    elif style == 2:  # even shares, the remainder on the last lane
        cuts = np.arange(1, 64) * (n // 64)
    else:             # one lane holds all
        cuts = np.full(63, n)
        cuts[:int(rng.integers(0, 63))] = 0
    return np.concatenate([[0], cuts, [n]]).astype(np.int32)


def _case(rng, name, keys, k, ids=None, n_arg=None):
    keys = np.asarray(keys, dtype=np.uint64)
    n = len(keys)
    if ids is None:  # distinct, non-negative, in no particular order
        ids = rng.permutation(n).astype(np.int64) * 3 + int(rng.integers(0, 1 << 40))
    order = rng.permutation(n)
    return {"name": name, "keys": keys[order], "ids": np.asarray(ids, dtype=np.int64)[order], "k": int(k),
            "n": n if n_arg is None else n_arg, "lane_off": _spread(rng, n)}


def _rand_keys(rng, n):
    return rng.integers(0, 1 << 64, n, dtype=np.uint64)


def _even_keys(rng, n):
    """Top bytes spread evenly over 0..255 (key i of n lies near i / n of the range)."""
    low = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    return np.array([((i << 64) // n) & ~((1 << 40) - 1) for i in range(n)], dtype=np.uint64) | low


def _top(byte, rng, n):
    """n keys with the given top byte and random lower bytes."""
    return (np.uint64(byte) << np.uint64(56)) | rng.integers(0, 1 << 56, n, dtype=np.uint64)


def select_kth_cases():
    """Cases of select_kth (each a dict: keys, ids, k, n, lane_off)."""
    rng = np.random.default_rng(SEED + 2)
    out = []
    for n in (1, 2, 3, 63, 64, 65, 257, 1000, 4097, 8192):
        keys = _rand_keys(rng, n)
        for k in sorted({1, 2, n // 2, n - 1, n} - {0}):
            if k <= n:
                out.append(_case(rng, f"random-n{n}-k{k}", keys, k))
    out.append(_case(rng, "config3-5000-of-6000", _rand_keys(rng, 6000), 5000))
    # exit at every pass p: the keys share every byte above p and differ at byte p
    for p in range(8):
        base = int(rng.integers(0, 1 << 64, dtype=np.uint64)) & ~(0xFF << (8 * p)) & U64
        keys = np.array([base | (i << (8 * p)) for i in range(200)], dtype=np.uint64)
        keys ^= rng.integers(0, 1 << (8 * p), 200, dtype=np.uint64) if p else np.uint64(0)
        out.append(_case(rng, f"exit-pass{p}", keys, 1 + 37 * p % 200))
    # the validation queue's keys: first deliverer << 56 | message id
    mids = rng.permutation(1 << 16)[:900].astype(np.uint64)
    ff = rng.integers(0, 6, 900, dtype=np.uint64)
    ff[::7] = 255
    for k in (1, 64, 450, 899, 900):
        out.append(_case(rng, f"valqueue-k{k}", (ff << np.uint64(56)) | mids, k, ids=mids.astype(np.int64)))
    # tie groups: equal keys with permuted ids
    for g, n_other in ((2, 0), (2, 50), (7, 300), (64, 64), (200, 0), (200, 1000)):
        tied = int(rng.integers(0, 1 << 64, dtype=np.uint64))
        keys = np.concatenate([np.full(g, tied, dtype=np.uint64), _rand_keys(rng, n_other)])
        first = int(np.count_nonzero(keys < np.uint64(tied))) + 1
        for j in sorted({0, 1, g // 2, g - 1}):
            out.append(_case(rng, f"ties-g{g}-of{g + n_other}-rank{j + 1}", keys, first + j))
    keys = np.repeat(_rand_keys(rng, 40), 5)  # every key five times
    for k in (1, 3, 5, 6, 100, 200):
        out.append(_case(rng, f"all-tied-x5-k{k}", keys, k))
    # a key equal to 2^64 - 1, selected and not
    keys = np.concatenate([_rand_keys(rng, 99), [np.uint64(U64)]])
    out.append(_case(rng, "maxkey-selected", keys, 100))
    out.append(_case(rng, "maxkey-not-selected", keys, 99))
    keys = np.concatenate([_rand_keys(rng, 97), np.full(3, U64, dtype=np.uint64)])
    for k in (98, 99, 100):
        out.append(_case(rng, f"maxkey-tied-k{k}", keys, k))
    # k above the candidate count
    out.append(_case(rng, "k-above-count-n10", _rand_keys(rng, 10), 11))
    out.append(_case(rng, "k-above-count-n300", _rand_keys(rng, 300), 1000))
    return out


def select_kth_est_cases(win, cap):
    """Cases of select_kth_est, built from the model so that each path is taken
    by construction (win = GS_SEL_WIN, cap = GS_SEL_CAP)."""
    rng = np.random.default_rng(SEED + 3)
    out = []
    for n in (2, 64, 1000, 4096):
        keys = _even_keys(rng, n)
        for k in sorted({1, n // 3, n // 2, n - 1} - {0}):
            out.append(_case(rng, f"fast-even-n{n}-k{k}", keys, k))
    for n, k in ((6000, 5000), (1000, 500), (8192, 4096), (8192, 100), (300, 299)):
        out.append(_case(rng, f"random-n{n}-k{k}", _rand_keys(rng, n), k))
    out.append(_case(rng, "miss-below-top0", _top(0, rng, 500), 250))
    out.append(_case(rng, "miss-above-top255", _top(255, rng, 500), 250))
    # est = 128: the window holds `inwin` keys, (inwin // 2) lie under it, the rest above
    for inwin, name in ((cap + 1, "overflow-cap+1"), (cap, "fast-cap-exactly"), (4 * cap, "overflow-4cap")):
        keys = np.concatenate([_top(128, rng, inwin), _top(5, rng, inwin // 2), _top(250, rng, inwin - inwin // 2)])
        out.append(_case(rng, name, keys, inwin))
    # the whole window full of one tied key: ranked by id in the fast path
    tied = (128 << 56) | 12345
    keys = np.concatenate([np.full(cap, tied, dtype=np.uint64), _top(5, rng, cap // 2), _top(250, rng, cap - cap // 2)])
    out.append(_case(rng, "fast-window-all-tied", keys, cap))
    keys = np.concatenate([np.full(2 * cap, tied, dtype=np.uint64), _top(5, rng, cap), _top(250, rng, cap)])
    out.append(_case(rng, "overflow-window-all-tied", keys, 2 * cap))  # the fallback ends in select_kth's tie loop
    # the window clipped at bin 0 and at bin 255
    even = _even_keys(rng, 1000)
    out.append(_case(rng, "clip-lo0-k2", even, 2))
    out.append(_case(rng, "clip-lo0-k1-top0", np.concatenate([_top(0, rng, 20), _top(200, rng, 480)]), 1))
    out.append(_case(rng, "clip-hi255-k999", even, 999))
    out.append(_case(rng, "clip-hi255-top255", np.concatenate([_top(3, rng, 480), _top(255, rng, 20)]), 495))
    # k >= n: everything is taken
    out.append(_case(rng, "k-eq-n", _rand_keys(rng, 77), 77))
    out.append(_case(rng, "k-above-n", _rand_keys(rng, 77), 500))
    out.append(_case(rng, "k-eq-n-1", _rand_keys(rng, 1), 1))
    # keys of the validation queue's form and a maximal key through the estimate
    mids = rng.permutation(1 << 16)[:600].astype(np.uint64)
    out.append(_case(rng, "valqueue-form", (rng.integers(0, 4, 600, dtype=np.uint64) << np.uint64(56)) | mids, 300,
                     ids=mids.astype(np.int64)))
    out.append(_case(rng, "maxkey-last", np.concatenate([_even_keys(rng, 499), [np.uint64(U64)]]), 499))
    return out


# ------------------------------------------------------------------ checkers
def check_select_k(cases, masks, half=None):
    """Differences between the device's ballot masks and the reference.  cases:
    select_k_cases() rows, or select_k_half_cases() rows with half = 'both' |
    'lo' | 'hi' (a call made under divergence by that half only: the other
    half's lanes made no call and read 0)."""
    bad = []
    for row, got in zip(cases, masks):
        if half is None:
            name, cand, key, k = row
            want = ref_select_k(cand, key, k)
        else:
            name, cand, key, k_lo, k_hi = row
            want = ref_select_k_half(cand, key, k_lo, k_hi)
            want &= {"both": U64, "lo": 0xFFFFFFFF, "hi": 0xFFFFFFFF << 32}[half]
        if int(got) != want:
            bad.append(f"{name}: mask {int(got):#018x}, reference {want:#018x}")
    return bad


def check_select_kth(cases, K, M, est=False):
    """Differences of the device's (K, M) from the reference (est: that of
    select_kth_est), and of the count of (key, id) <= (K, M) from min(k, n):
    the property the callers rely on."""
    bad = []
    for c, k_, m_ in zip(cases, K, M):
        got = (int(k_), int(m_))
        want = (ref_select_kth_est if est else ref_select_kth)(c["keys"], c["ids"], c["k"])
        if got != want:
            bad.append(f"{c['name']}: (K, M) = ({got[0]:#x}, {got[1]}), reference ({want[0]:#x}, {want[1]})")
        taken = count_le(c["keys"], c["ids"], got[0], got[1])
        if taken != min(c["k"], len(c["keys"])):
            bad.append(f"{c['name']}: (K, M) takes {taken} candidates, want {min(c['k'], len(c['keys']))}")
    return bad


def check_incl_sum(x, got):
    """x, got: [cases][64]; differences from the running sum, per lane."""
    bad = []
    for c, (row, g) in enumerate(zip(x, got)):
        want = ref_incl_sum(row)
        for lane in np.flatnonzero(want != np.asarray(g, dtype=np.int32)):
            bad.append(f"case {c} lane {lane}: {int(g[lane])}, reference {int(want[lane])}")
    return bad


def check_transpose(x, got):
    """x, got: [cases][64] uint64; differences from the bit-matrix transpose."""
    bad = []
    for c, (row, g) in enumerate(zip(x, got)):
        want = ref_transpose64(row)
        for lane in np.flatnonzero(want != np.asarray(g, dtype=np.uint64)):
            bad.append(f"case {c} lane {lane}: {int(g[lane]):#018x}, reference {int(want[lane]):#018x}")
    return bad
