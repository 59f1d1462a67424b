"""Inputs that hold the tiled class of the LZSS compress batch (csrc/lzss_tile.hip: k_lzss_tile_esc, _search, _chain, _emit) at its cuts, its
windows and its step cap: members whose greedy chain enters and leaves tiles in every way k_lzss_tile_chain tells apart, periods of the
window's length and one more at windows that are no multiple of a sub-tile, members just under and just over T_STEP_CAP, a list of more
bytes than a group's staging, and a seeded fuzz.  tests/test_lzss_tile_cases_host.py holds these builders against the models below on a
CPU, so that the GPU test (test_gpu_lzss_tile_limits.py) cannot quietly test something easier.  Nothing here needs a GPU or the library:
plain Python and numpy over oracle/oracle.py.

A case is (name, members, window, expect); `expect` says per member index what the host test proves and the GPU test asserts.

What the search counts (lzss_enc_body.h: chain_best).  Position i meets the candidates j of its two-byte chain with 2 <= d = i - j <= min(i, W).
One whose first eight bytes are i's is extended eight bytes at a time while off < lim = min(d, E - i), a step each, the step that finds the
mismatch included: a candidate with a common prefix of lcp bytes costs min(ceil((lim - 8) / 8), lcp // 8) steps -- IF it is extended.  It is
skipped when it cannot reach the best length so far, and the order of the walk is the chains': sub-tiles of 1024 positions from the
nearest to the farthest, inside one sub-tile any order.  So the sum over every candidate is an UPPER bound whatever the order.  The LOWER
bound leaves out the candidates that lie in i's own sub-tile and are shorter than another candidate of i; it takes the candidates of one
OLDER sub-tile as met nearest first, which is the order the waves of a workgroup link them in but not one the comment in lzss_enc_body.h
promises.  A thread's figure is the sum over its two positions of a tile, t0 + tid and t0 + 1024 + tid."""
import functools

import numpy as np

from oracle import oracle
from test_gpu_lzss_mid import _alpha, _csv, _text
from test_gpu_lzss_tile import PAD

TILE, SUB, STEP_CAP, W_MAX = 2048, 1024, 4096, 4096      # lzss_tile.hip: TILE, TT, T_STEP_CAP; lzss_tile_layout.h: LZT_W_MAX
GD_ENTRY, STATUS, GROUP_MEMBERS = 64, 16, 4096           # group_dev.hip: a SmallMember and a GatherEntry; group_layout.h; codecs.h: SMALL_GROUP_MAX
TAKEN, BACK, EITHER = "taken", "back", "either"


# ---------------------------------------------------------------- models
def escaped(d):
    return oracle.lzss_escape(d)


def digits(v):
    return len(str(v))


def item_size(L, d):
    """the bytes an item of the chain puts out: a token iff it is shorter than what it stands for (lzss.go:143)"""
    if L == 0:
        return 1
    el = 3 + digits(d) + digits(L)
    return el if el < L else L


def chain(esc, w):
    """the greedy chain's positions (r, L, d), r -> r + max(1, L); a match of one byte is a literal, as the kernels' keys have it"""
    off, size = oracle.lzss_matches(esc, w)
    items, r, E = [], 0, len(esc)
    while r < E:
        L, d = int(size[r]), int(off[r])
        if L < 2:
            L = d = 0
        items.append((r, L, d))
        r += max(1, L)
    return items


def tile_offsets(items, E):
    """off[t]: the first output byte of tile t's items; off[tiles]: the stream's length (lzss_tile_layout.h: ownership)"""
    T = (E + TILE - 1) // TILE
    off = [0] * (T + 1)
    for r, L, d in items:
        off[r // TILE + 1] += item_size(L, d)
    for t in range(T):
        off[t + 1] += off[t]
    return off


def events(items, E):
    """the names of what k_lzss_tile_chain and k_lzss_tile_emit tell apart, as far as this chain shows them"""
    seen = set()
    for r, L, d in items:
        nxt = r + max(1, L)
        if L and nxt < E and nxt // TILE != r // TILE:
            if nxt % TILE == 0 and item_size(L, d) < L:
                seen.add("entry 0 after a token that ends on an edge")
            if nxt % TILE == 1:
                seen.add("entry 1")
            if nxt % TILE == TILE - 1:
                seen.add("entry TILE - 1")
            if nxt == (r // TILE + 2) * TILE:
                seen.add("a landing exactly 2 tiles on")
        if r % TILE == TILE - 1 and L == 4096 and nxt // TILE == r // TILE + 2:
            seen.add("L = 4096 from position TILE - 1, the next tile skipped")
        if r % TILE == TILE - 1 and L == 2049 and nxt // TILE == r // TILE + 2:
            seen.add("L = 2049 from position TILE - 1, the next tile skipped")
    off = tile_offsets(items, E)
    for t in range(len(off) - 1):
        o0, o1 = off[t], off[t + 1]
        if o1 == o0:
            seen.add("a tile whose output is 0 bytes")
        elif 0 < o0 and o1 < off[-1] and o0 % 16 and o1 % 16 and o0 // 16 == o1 // 16:
            seen.add("a tile whose output shares one 16-byte unit with both neighbours")
    if E % TILE == 0:
        seen.add("E = 0 (mod TILE)")
    if E % TILE == 1:
        r, L, d = items[-1]
        seen.add("E = 1 (mod TILE), the chain lands on the last position" if r == E - 1 else "E = 1 (mod TILE), the chain steps over the last position")
    return seen


def e_cap(lz, n):
    m = min(n, lz.TILE_IN_MAX)
    return min(m + m // 2, lz.TILE_E_MAX)


def in_class(lz, d, w=4096):
    return lz.MID_IN_MAX < len(d) <= lz.TILE_IN_MAX and 1 <= w <= W_MAX


def group_cuts(lz, members, w=4096):
    """the groups [lo, hi) the device form makes of the members of the class, as indexes into `members` (group_layout.h: next_group over
    group_need with group_dev.hip's entry, lzss_tile_layout.h's slots and LZSS_TILE_GROUP_BYTES)"""
    idx = [i for i, d in enumerate(members) if in_class(lz, d, w)]
    need = [GD_ENTRY + ((len(members[i]) + 15) // 16 * 16 + 32) + ((e_cap(lz, len(members[i])) + 15) // 16 * 16 + 16) + STATUS for i in idx]
    cuts, lo = [], 0
    while lo < len(idx):
        k, used = lo, 0
        while k < len(idx) and k - lo < GROUP_MEMBERS and (k == lo or used + need[k] <= lz.TILE_GROUP_BYTES):
            used += need[k]
            k += 1
        cuts.append((idx[lo], idx[k - 1] + 1))
        lo = k
    return cuts


def groups(lz, members, w=4096):
    return len(group_cuts(lz, members, w))


def _keys(a):
    """the eight bytes from every position on as one number, zeros behind the stream (what the search's LDS image holds there)"""
    pad = np.concatenate((a, np.zeros(16, dtype=np.uint8)))
    return np.ascontiguousarray(np.lib.stride_tricks.sliding_window_view(pad, 8)[:len(a) + 8]).view("<u8").ravel()


def _pairs(key, E, w):
    """every (i, j), j < i, 2 <= i - j <= w, with the same eight bytes and lim = min(i - j, E - i) > 8"""
    order = np.argsort(key[:E], kind="stable")
    k = np.arange(E - 1)
    I, J = [], []
    for lag in range(1, E):
        k = k[k + lag < E]
        hi, lo = order[k + lag], order[k]
        ok = (key[hi] == key[lo]) & (hi - lo <= w)
        if not ok.any():
            break
        k, hi, lo = k[ok], hi[ok], lo[ok]
        use = (hi - lo >= 2) & (np.minimum(hi - lo, E - hi) > 8)
        I.append(hi[use])
        J.append(lo[use])
    if not I:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    return np.concatenate(I).astype(np.int64), np.concatenate(J).astype(np.int64)


def _lcp(a, key, I, J, lim):
    """the common prefix of positions I and J, exact below lim and at least lim where it is not"""
    E = len(a)
    lcp = np.zeros(len(I), dtype=np.int64)
    d = I - J
    ds, inv, cnt = np.unique(d, return_inverse=True, return_counts=True)
    many = cnt >= 128
    if many.sum() > 64:                                                       # (noise over a few letters: every distance, and short prefixes)
        many[:] = False
    big = many[inv]
    pad = np.concatenate((a, np.zeros(W_MAX + 16, dtype=np.uint8)))
    for dist in ds[many]:                                               # many pairs of one distance: the runs of fc[x] == fc[x - d]
        sel = np.flatnonzero(big & (d == dist))
        x = np.arange(dist, len(pad))
        stop = np.where(pad[dist:] != pad[:-dist], x, len(pad))
        nxt = np.minimum.accumulate(stop[::-1])[::-1]                         # the first x' >= x with a mismatch
        lcp[sel] = nxt[I[sel] - dist] - I[sel]
    act = np.flatnonzero(~big)                                                # the rest: eight bytes at a time, as the kernel does
    lcp[act] = 8
    k = 1
    while act.size:
        x = key[np.minimum(I[act] + 8 * k, E + 7)] ^ key[np.minimum(J[act] + 8 * k, E + 7)]
        eq = x == 0
        ne = act[~eq]
        low = x[~eq] & (~x[~eq] + np.uint64(1))
        lcp[ne] = 8 * k + (np.log2(low.astype(np.float64)).astype(np.int64) >> 3)
        lcp[act[eq]] = 8 * k + 8
        act = act[eq]
        act = act[8 * (k + 1) < lim[act]]
        k += 1
    return lcp


def steps_by_thread(esc, w):
    """-> (upper, lower): per tile and thread, the bounds of the module's docstring on the steps of k_lzss_tile_search"""
    a = np.frombuffer(bytes(esc), dtype=np.uint8)
    E = len(a)
    tiles = (E + TILE - 1) // TILE
    if E < 10:
        z = np.zeros((max(tiles, 1), SUB), dtype=np.int64)
        return z, z
    key = _keys(a)
    I, J = _pairs(key, E, w)
    lim = np.minimum(I - J, E - I)
    lcp = _lcp(a, key, I, J, lim)
    steps = np.minimum((lim - 8 + 7) // 8, lcp // 8)
    m = np.minimum(lcp, lim)
    longest = np.zeros(E, dtype=np.int64)
    np.maximum.at(longest, I, m)
    sure = ~((J // SUB == I // SUB) & (m < longest[I]))
    out = []
    for wt in (steps, steps * sure):
        pos = np.zeros(tiles * TILE, dtype=np.int64)
        pos[:E] = np.bincount(I, weights=wt, minlength=E).astype(np.int64)
        out.append(pos.reshape(tiles, 2, SUB).sum(axis=1))
    return out[0], out[1]


@functools.lru_cache(maxsize=None)
def steps_bound(esc, w):
    """-> (upper, lower) of the thread that spends most.  upper <= STEP_CAP: the member MUST be taken; lower > STEP_CAP: it MUST be handed back"""
    up, lo = steps_by_thread(esc, w)
    return int(up.max()), int(lo.max())


def classify(lz, d, w):
    """what the class does with a member of its lengths: TAKEN, BACK or EITHER"""
    esc = escaped(d)
    if len(esc) > e_cap(lz, len(d)):
        return BACK                                                           # (k_lzss_tile_esc)
    up, lo = steps_bound(esc, w)
    return TAKEN if up <= STEP_CAP else BACK if lo > STEP_CAP else EITHER


# ---------------------------------------------------------------- literal filler and planted copies
LETTERS = np.array([b for b in range(256) if b not in (0x00, 0x3C, 0x5C, 0xFF)], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def filler():
    """a cyclic de Bruijn sequence of order 2 over the 252 byte values that neither escape nor are zero: 63504 bytes, every bigram once, so
    a stretch of it has no match at any window and its chain steps by one.  (An Euler circuit of the complete graph with loops, every
    vertex's edges in a seeded random order: a bigram's neighbours in the sequence say nothing about where its letters recur.)"""
    k = len(LETTERS)
    rng = np.random.default_rng(62500)
    left = [list(rng.permutation(k)) for _ in range(k)]
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if left[v]:
            stack.append(left[v].pop())
        else:
            circuit.append(stack.pop())
    seq = LETTERS[np.array(circuit[:0:-1], dtype=np.int64)]
    assert len(seq) == k * k
    return seq


def _has(out, hi, a, b):
    """the bigram a b somewhere in the largest window in front of hi"""
    lo = max(0, hi - W_MAX - 2)
    return bool(((out[lo:hi - 1] == a) & (out[lo + 1:hi] == b)).any())


def planted(plants, n, start=0):
    """filler (from its byte `start` on) with copies: a plant (P, d, L) is a copy of [P - d, P - d + L) at P; behind it the filler goes on
    with its next byte that is not the source's continuation, so the match is L long and no longer"""
    f, out, at, used = filler(), np.empty(n, dtype=np.uint8), 0, start
    for P, d, L in sorted(plants):
        assert at <= P and 2 <= L <= d <= P and P + L <= n, (P, d, L)
        out[at:P] = f[(used + np.arange(P - at)) % len(f)]
        used += P - at
        # (the byte in front of the copy: with the copy's first byte it must be a bigram of its own, or the chain takes two bytes at P - 1)
        if P - at >= 2 and (_has(out, P, out[P - 1], out[P - d]) or _has(out, P - 1, out[P - 2], out[P - 1])):
            out[P - 1] = next(c for c in np.random.default_rng(P).permutation(LETTERS) if not (_has(out, P - 1, out[P - 2], c) or _has(out, P - 1, c, out[P - d])
                                                                                               or c in (out[P - 2], out[P - d])))
        out[P:P + L] = out[P - d:P - d + L]
        at = P + L
        while at < n and f[used % len(f)] == out[at - d]:
            used += 1
    out[at:] = f[(used + np.arange(n - at)) % len(f)]
    return out.tobytes()


def _pad(lz, members):
    have = sum(1 for d in members if in_class(lz, d))
    return list(members) + [PAD] * max(0, lz.TILE_GROUP_MIN - have)


# ---------------------------------------------------------------- cases
T = TILE
PLANTS_4096 = ((5 * T - 100, 4096, 100), (8 * T - 1, 4096, 4096), (11 * T, 4096, 4096), (16 * T - 1, 3000, 2), (20 * T - 1, 4096, 2049))
PLANTS_2049 = ((5 * T - 100, 2049, 100), (8 * T - 2, 2049, 2049), (11 * T - 1, 2049, 2049), (16 * T - 1, 2000, 2), (20 * T - 1, 2049, 2049), (21 * T, 2049, 2049))
EVENTS_4096 = {"entry 0 after a token that ends on an edge", "entry 1", "entry TILE - 1", "L = 4096 from position TILE - 1, the next tile skipped",
               "L = 2049 from position TILE - 1, the next tile skipped", "a landing exactly 2 tiles on", "a tile whose output is 0 bytes",
               "a tile whose output shares one 16-byte unit with both neighbours"}
EVENTS_2049 = EVENTS_4096 - {"L = 4096 from position TILE - 1, the next tile skipped"}
LANDED, OVER, FULL = "E = 1 (mod TILE), the chain lands on the last position", "E = 1 (mod TILE), the chain steps over the last position", "E = 0 (mod TILE)"


def _aligned(plants, n, w, start):
    """the plants and, in front of them, one more whose length moves every later output byte until the tile of one token shares its
    16-byte unit with both neighbours"""
    for k in range(16):
        d = planted(((2 * T + 10, 300, 20 + k),) + tuple(plants), n, start)
        if "a tile whose output shares one 16-byte unit with both neighbours" in events(chain(d, w), len(d)):
            return ((2 * T + 10, 300, 20 + k),) + tuple(plants)
    raise AssertionError("no length of the first plant puts the tile of one token inside one unit")


@functools.lru_cache(maxsize=None)
def landings(lz):
    cases = []
    for name, plants, w, want, start in (("landings", PLANTS_4096, 4096, EVENTS_4096, 0), ("landings at window 2049", PLANTS_2049, 2049, EVENTS_2049, 2000)):
        n = 33 * T + 1
        plants = _aligned(plants, n, w, start)
        members = [planted(plants, n, start), planted(plants, n - 1, start), planted(plants + ((n - 51, 1000, 51),), n, start)]
        expect = {0: want | {LANDED}, 1: want | {FULL}, 2: want | {OVER}}
        cases.append((name, tuple(_pad(lz, members)), w, expect))
    return tuple(cases)


WINDOWS = (1023, 1025, 2047, 2049, 3000, 4095)


@functools.lru_cache(maxsize=None)
def windows(lz):
    """a period of W - 1, W and W + 1 bytes of 20-letter noise at every W: the candidate exactly W back is the match, the one W + 1 back is
    none.  expect: the token every stream holds, None: the stream is the 70000 bytes"""
    block = _alpha(4040, 4200, b"abcdefghijklmnopqrst")
    cases = []
    for W in WINDOWS:
        members = [(block[:p] * (70000 // p + 1))[:70000] for p in (W - 1, W, W + 1)]
        expect = {0: b"<%d,%d>" % (W - 1, W - 1), 1: b"<%d,%d>" % (W, W), 2: None}
        cases.append(("window %d" % W, tuple(_pad(lz, members)), W, expect))
    return tuple(cases)


CAP_PERIODS = ((585, TAKEN), (513, TAKEN), (512, BACK))


@functools.lru_cache(maxsize=None)
def cap(lz):
    """periods whose candidates at every multiple within the window add up to just under and to over T_STEP_CAP; a list a period"""
    block = _alpha(4041, 600, b"abcdefghijklmnopqrst")
    return tuple(("period %d" % p, tuple(_pad(lz, [(block[:p] * (70000 // p + 1))[:70000]])), 4096, {0: what}) for p, what in CAP_PERIODS)


@functools.lru_cache(maxsize=None)
def two_groups(lz):
    """more staging than LZSS_TILE_GROUP_BYTES: two groups.  expect: the cut, the member of TILE_IN_MAX bytes (first group), the member
    that escapes to more than the class holds (second group)"""
    texts = [_text(4200 + i, 65537 + 115 * i) for i in range(5)]             # five distinct texts: the oracle runs five times
    members = [texts[i % 5] for i in range(420)]
    top, esc = 7, 415
    members[top] = _text(4210, lz.TILE_IN_MAX)
    table = bytes((0x5C, 0xFF)[c % 2] if c in b"abcdefghijklmnop " else c for c in range(256))
    members[esc] = _text(4211, 65800).translate(table)
    cut = group_cuts(lz, members)[0][1]
    return (("two groups", tuple(members), 4096, {"cut": cut, "top": top, "escaped": esc}),)


FUZZ_SEEDS = (1, 2, 3, 4)
FUZZ_WINDOWS = (1, 2, 17, 255, 1000, 1023, 1025, 2049, 3000, 4095, 4096)
FUZZ_WINDOW = {1: 4096, 2: 1025, 3: 255, 4: 2049}        # a seed's window: distinct, three of them no multiple of a sub-tile, one the largest


def _fuzz_member(seed, rng, n, kind=None):
    kind = int(rng.integers(0, 6)) if kind is None else kind
    if kind == 5:                                                             # a period of 520 to 600 bytes all through: at window 4096 seven candidates
        u = int(rng.integers(520, 601))                                       # a position, 3100 to 3700 steps a thread -- near the cap, under it
        a = np.tile(rng.integers(97, 117, size=u).astype(np.uint8), n // u + 1)[:n].copy()
    elif kind == 0:
        a = np.frombuffer(_text(seed, n), dtype=np.uint8).copy()
    elif kind == 1:
        a = np.frombuffer(_csv(seed, n), dtype=np.uint8).copy()
    elif kind == 2:
        letters = rng.permutation(256)[:int(rng.choice((2, 3, 4, 16, 20, 64, 256)))].astype(np.uint8)
        a = letters[rng.integers(0, len(letters), size=n)]
    else:                                                                     # stretches of units of 600 to 5000 bytes
        parts, have = [], 0
        while have < n:
            u = int(rng.integers(600, 5001))
            unit = rng.integers(32, 127, size=u).astype(np.uint8) if kind == 3 else np.frombuffer(_text(seed + have, u), dtype=np.uint8)
            part = np.tile(unit, int(rng.integers(1, 5)))[:int(rng.integers(u, 4 * u + 1))]
            parts.append(part)
            have += len(part)
        a = np.concatenate(parts)[:n].copy()
    for _ in range(int(rng.integers(0, 40))):                                 # copies from up to 4096 back
        d = int(rng.integers(2, 4097))
        L = int(rng.integers(2, d + 1))
        p = int(rng.integers(d, n - L + 1))
        a[p:p + L] = a[p - d:p - d + L].copy()
    share = float(rng.choice((0.0, 0.0, 0.002, 0.01, 0.03)))                  # bytes that escape: 3C to one byte, 5C and FF to two
    at = np.flatnonzero(rng.random(n) < share)
    a[at] = np.array((0x3C, 0x5C, 0xFF), dtype=np.uint8)[rng.integers(0, 3, size=len(at))]
    return a.tobytes()


@functools.lru_cache(maxsize=None)
def fuzz(lz, seed):
    """expect: TAKEN, BACK or EITHER per member index"""
    rng = np.random.default_rng(77000 + seed)
    w = FUZZ_WINDOW[seed]
    sizes = rng.integers(65537, 140001, size=lz.TILE_GROUP_MIN + 4)
    members = tuple(_fuzz_member(77000 + 100 * seed + i, rng, int(n), 5 if i in (3, 11) else None) for i, n in enumerate(sizes))   # (two of the long period in every list)
    return ("fuzz %d" % seed, members, w, {i: classify(lz, d, w) for i, d in enumerate(members)})
