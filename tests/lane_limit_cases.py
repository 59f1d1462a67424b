"""The inputs that hold the Huffman lane maps at their limits, built with the model of tests/lane_maps.py (no GPU; the library is not
imported): members that settle in the last round that is still taken beside members that need one more, lanes that end with exactly four
starts beside lanes that are offered a fifth, a tile whose 32 entries leave through five exits, flat codes of 1 to 7 bits in the tiled
class, and the members of the other suites whose hand-back depends on the data -- each with the model's verdict and reason.
tests/test_lane_maps_host.py asserts the figures on a CPU, tests/test_gpu_huffman_lane_limits.py runs the members on the GPU.

How a limit member is made.  A FILLER of fixed, well-separated counts fixes the code: the counts of the whole member are the same whatever
the stretch holds (the filler gives up what the stretch uses), so code lengths and codewords do not move.  The STRETCH is a short pattern
of symbols repeated: a periodic bit string, in which a wrong start can stay a wrong parse for as long as the stretch lasts.
  rounds   a pattern of 8 code bits over lengths {2,2,3,3,3,3} with a second parse that never meets the true one.  8 divides every lane
           width, so with the stretch's first bit at the right residue every lane's first guess lies in the second parse, all the lanes
           agree with each other from the first round on, and the true start walks down the stretch one lane a round.
  phases   a pattern whose period does not divide the lane width, with three or four parses that never meet: the lanes' first guesses
           fall on all of them in turn, and a lane collects one start a parse (and its own guess where that lies on none).
The verdicts and figures are read off the model, never assumed; the host test pins them."""
import collections
import functools

import numpy as np

import lane_maps as M
from oracle import oracle as O

TILE_BITS = M.SHAPES["tiled"].lanes * M.SHAPES["tiled"].s_max

# ---------------------------------------------------------------- the model's answers, once per member
_TAB, _ENC, _MODEL = {}, {}, {}


def enc(d):
    if d not in _ENC:
        _ENC[d] = O.huffman_compress(d)
    return _ENC[d]


def table(d):
    if d not in _TAB:
        _TAB[d] = O.huffman_table(d)
    return _TAB[d]


def lanes(d, cls, rounds_cap=M.DEC_ROUNDS):
    """the member's stream in the class's lanes -> (Lanes, taken, reason)"""
    key = (d, cls, rounds_cap)
    if key not in _MODEL:
        _MODEL[key] = M.model(enc(d), table(d), cls, rounds_cap=rounds_cap)
    return _MODEL[key]


def verdict(d, cls):
    """(taken, reason) of the member in the class"""
    return lanes(d, cls)[1:]


def class_of(d):
    """which grouped class a batch hands the member's stream to (codecs.h: the classes' cutoffs): a rune alphabet of up to 16384 bytes is
    the rune decoder's; a byte alphabet goes by its payload and its decoded size"""
    pay, out = len(M.split(enc(d))[0]), len(d)
    if max(d) >= 0x80:
        return "rune" if out <= M.SHAPES["rune"].out_max and pay <= M.SHAPES["rune"].pay_max else None
    for cls in ("small", "mid"):
        if pay <= M.SHAPES[cls].pay_max and out <= M.SHAPES[cls].out_max:
            return cls
    return "tiled" if M.SHAPES["mid"].out_max < out <= M.SHAPES["tiled"].out_max and pay <= M.SHAPES["tiled"].pay_max else None


# ---------------------------------------------------------------- filler and stretch
def with_counts(seed, counts, shuffled=True):
    a = np.concatenate([np.full(c, b, dtype=np.uint8) for b, c in sorted(counts.items())])
    if shuffled:
        np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


def scaled(base, u):
    return {b: c * u for b, c in base.items()}


# lengths {2,2,3,3,3,3}: 100 + 105 and 110 + 115 pair up, then the pairs, then 300 + 310
ROUNDS_BASE = {0x61: 300, 0x62: 310, 0x63: 100, 0x64: 105, 0x65: 110, 0x66: 115}
# lengths 2, 3, 3, four of 4, eight of 5: a dyadic distribution, the counts pulled apart so that no tie decides
PHASES_BASE = dict([(0x41, 800), (0x42, 400), (0x43, 405)] + [(0x44 + i, 200 + 3 * i) for i in range(4)] + [(0x48 + i, 100 + i) for i in range(8)])


@functools.lru_cache(maxsize=None)
def codes_of(items):
    """{byte: (code, length)} of the members with these counts (the oracle's table of one of them)"""
    return {r: (c, l) for r, _, c, l in O.huffman_table(with_counts(0, dict(items), False))}


def parses(codes, pattern):
    """The pattern repeated for ever: -> (period in bits, step) with step[r] = the length of the codeword that begins at residue r."""
    bits = "".join(format(codes[s][0], "0%db" % codes[s][1]) for s in pattern)
    P = len(bits)
    words = {format(c, "0%db" % l): l for c, l in codes.values()}
    step = []
    for r in range(P):
        rot = (bits * (64 // P + 2))[r:]
        step.append(next(l for w, l in words.items() if rot.startswith(w)))
    return P, step


def cycles(codes, pattern):
    """the parses that go on for ever: the cycles of r -> (r + step[r]) mod P, as sorted residue lists, the true one (through 0) first"""
    P, step = parses(codes, pattern)
    seen, out = {}, []
    for r0 in range(P):
        path, r = [], r0
        while r not in seen and r not in path:
            path.append(r)
            r = (r + step[r]) % P
        if r in path:
            out.append(sorted(path[path.index(r):]))
        for x in path:
            seen[x] = True
    out.sort(key=lambda c: (0 not in c, c))
    return P, out


def stretch_member(seed, counts, pattern, reps, q_target, ok=lambda q: True, pre_share=None):
    """A member with exactly `counts`: a shuffled prefix whose code bits end at the first q >= q_target with ok(q), the pattern `reps`
    times, the shuffled rest.  The prefix depends on the seed and the counts alone, so q does not move with reps.  -> (bytes, q)"""
    codes = codes_of(tuple(sorted(counts.items())))
    total_bits = sum(c * codes[b][1] for b, c in counts.items())
    share = pre_share if pre_share is not None else min(0.95, (q_target + 256) / total_bits)
    pre = np.frombuffer(with_counts(seed, {b: int(c * share) for b, c in counts.items()}), dtype=np.uint8)
    ends = np.cumsum(np.array([codes[b][1] if b in codes else 0 for b in range(256)])[pre])
    k = next(i + 1 for i, q in enumerate(ends.tolist()) if q >= q_target and ok(q))
    used = collections.Counter(pre[:k].tolist())
    for s in pattern:
        used[s] += reps
    rest = {b: c - used[b] for b, c in counts.items()}
    assert min(rest.values()) >= 0, rest
    d = pre[:k].tobytes() + bytes(pattern) * reps + with_counts(seed + 1, rest)
    assert collections.Counter(d) == collections.Counter(counts)
    return d, int(ends[k - 1])


# ---------------------------------------------------------------- rounds
def rounds_pattern(codes):
    """the first three-symbol pattern of 8 code bits with a second parse that never meets the true one -> (pattern, the second parse's residues)"""
    import itertools
    found = []
    for pat in itertools.product(sorted(codes), repeat=3):
        if sum(codes[s][1] for s in pat) == 8:
            P, cyc = cycles(codes, pat)
            if len(cyc) == 2:
                found.append((pat, cyc[1]))
    return found


ROUNDS_AT = {   # class -> (scale of ROUNDS_BASE, {place: the lane of the stream the stretch begins in front of})
    "tiled": (64, {"tile 0": 100, "tile 1": 960}),      # 66560 bytes, 167040 code bits: three tiles; "tile 1": the stretch begins in the last lane of tile 0, so that
    "mid": (32, {"block": 100}),                         #   tile 1's first lane lies in it and the true start arrives through the 32 entries
    "small": (6, {"block": 20}),
    "single": (32, {"block 0": 100, "block 1": 256}),    # the multi-block single call: five blocks of 256 lanes of 64 bits
}


def rounds_member(cls, place, n_lanes, seed=0):
    """the class's member whose stretch is n_lanes lanes long -> (bytes, the block the stretch lies in)"""
    u, at = ROUNDS_AT[cls]
    counts = scaled(ROUNDS_BASE, u)
    codes = codes_of(tuple(sorted(counts.items())))
    pattern, second = max(rounds_pattern(codes), key=lambda ps: min(counts[x] // ps[0].count(x) for x in ps[0]))   # (the one the filler can best afford)
    span = sum(c * codes[b][1] for b, c in counts.items())
    shape = M.SHAPES[cls]
    S, T, held = M.parse_lanes(span, shape.lanes * shape.blocks, shape.s_max)
    assert held and S % 8 == 0
    g0 = at[place]
    d, q = stretch_member(7000 + seed, counts, pattern, n_lanes * S // 8, g0 * S - 24, lambda q: (-q) % 8 in second)
    return d, (g0 + n_lanes // 2) // shape.lanes


def rounds_needed(cls, place, n_lanes):
    """the rounds the stretch's block needs to settle, the limit left aside"""
    d, b = rounds_member(cls, place, n_lanes)
    return lanes(d, cls, rounds_cap=1 << 30)[0].block(b).rounds


@functools.lru_cache(maxsize=None)
def rounds_lanes(cls, place):
    """the lanes of the stretch with which the block needs exactly DEC_ROUNDS rounds, read off the model (a lane more: a round more)"""
    return next(n for n in range(M.DEC_ROUNDS - 4, M.DEC_ROUNDS + 5) if rounds_needed(cls, place, n) == M.DEC_ROUNDS)


def rounds_pairs():
    """[(class, place, member that settles in the last round taken, member that needs one more, the block)]"""
    out = []
    for cls, (_, at) in ROUNDS_AT.items():
        for place in at:
            n = rounds_lanes(cls, place)
            (a, b), (c, _) = rounds_member(cls, place, n), rounds_member(cls, place, n + 1)
            out.append((cls, place, a, c, b))
    return out


# ---------------------------------------------------------------- phases
# class -> (scale of PHASES_BASE, lanes of the stretch, {place: lane it begins in front of}).  The scales are chosen so that the period of
# 10 bits does not divide the lane width (64, 192, 96) and the filler can afford the stretch.
PHASES_AT = {
    "tiled": (21, 24, {"tile 0": 50, "tile 1": 958}),
    "mid": (14, 24, {"block": 100}),
    "small": (2, 14, {"block": 60}),
    "single": (14, 24, {"block 0": 50, "block 1": 254}),
}
FOUR, FIVE, EXITS = b"MK", b"IO", b"OO"   # three parses that never meet and a guess beside them; four; five exits from a tile's 32 entries


def phases_member(cls, place, pattern):
    u, n_lanes, at = PHASES_AT[cls]
    counts = scaled(PHASES_BASE, u)
    codes = codes_of(tuple(sorted(counts.items())))
    span = sum(c * codes[b][1] for b, c in counts.items())
    shape = M.SHAPES[cls]
    S, T, held = M.parse_lanes(span, shape.lanes * shape.blocks, shape.s_max)
    P = sum(codes[s][1] for s in pattern)
    assert held and S % P
    return stretch_member(7100, counts, tuple(pattern), n_lanes * S // P, at[place] * S - 40)[0]


def phases_pairs():
    """[(class, place, member whose fullest lane ends with four starts, member in which a lane is offered a fifth)]"""
    return [(cls, place, phases_member(cls, place, FOUR), phases_member(cls, place, FIVE)) for cls, (_, _, at) in PHASES_AT.items() for place in at]


def five_exits():
    """the tiled member whose tile 1 is entered at 32 bits that leave its first lane through five exits"""
    return phases_member("tiled", "tile 1", EXITS)


# the natural one: the LZSS streams of the sixteen texts of tests/test_gpu_lzss_tile_dec.py::test_layered; the tiled class hands back one
LAYERED_SEEDS = range(6100, 6116)
LAYERED_BACK = 6111


def layered_text(seed):
    from test_gpu_lzss_mid import _text
    return _text(seed, 200000)


@functools.lru_cache(maxsize=None)
def layered_member(seed):
    return O.lzss_compress(layered_text(seed))


# ---------------------------------------------------------------- flat codes in the tiled class
def flat_member(bits):
    """Equal counts over 2^bits symbols, more than 65536 bytes in at least three tiles.  A tile is 61440 bits, a multiple of 2, 3, 4, 5 and
    6: there every tile is entered at its bit 0 and only the lanes' first boundaries move (64 is no multiple of 3, 5 or 6).  At 7 bits the
    tiles' entries move too, so that member is the long one: 17 tiles, entries 0 to 6, first output bytes on most residues mod 16."""
    k = 1 << bits
    per = 1100 if bits == 7 else max(65536 // k + 8, (2 * TILE_BITS // bits) // k + 8)
    return with_counts(7200 + bits, {0x30 + b if k <= 64 else b: per for b in range(k)})


FLAT_BITS = (2, 3, 4, 5, 6, 7)


# ---------------------------------------------------------------- the members other suites used to leave open
def either_members(samiam):
    """[(name, member, class)]: every member of the suite whose hand-back depends on the data and was expected "either way" """
    from test_gpu_huffman_big_dec import _skewed
    from test_gpu_huffman_mid import _alpha, _shape_tables, _with_counts
    from test_gpu_huffman_rune_dec_batch import _counter
    out = [("rune counter %d" % v, _counter(v), "rune") for v in range(16)]
    out.append(("big: periodic samiam", (samiam * (150000 // len(samiam) + 1))[:150000], "tiled"))
    out.append(("big: two symbols, 65537", np.random.default_rng(60).choice(np.frombuffer(b"xy", dtype=np.uint8), 65537).tobytes(), "tiled"))
    out.append(("big: two symbols, 262144", np.random.default_rng(80).choice(np.frombuffer(b"ab", dtype=np.uint8), 262144).tobytes(), "tiled"))
    out.append(("big: skewed", _skewed(81, 150000), "tiled"))
    block = _alpha(50, 4096, b"abcdefghijklmnopqrstuvwxyz ,.\n")
    per = [(samiam * (n // len(samiam) + 1))[:n] for n in (20000, 40000, 65536)] + [b"ab" * 16000, block * 12, block * 16]
    out += [("mid: periodic %d" % i, d, class_of(d)) for i, d in enumerate(per)]
    out += [("mid: sorted shape %d" % k, _with_counts(k, t, False), class_of(_with_counts(k, t, False))) for k, t in enumerate(_shape_tables())]
    return out


# name -> (class, taken, reason): the model's verdicts on them, pinned (tests/test_lane_maps_host.py holds the model to this table, the
# GPU suites hold the kernels to the model)
EITHER_WANT = dict(
    [("rune counter %d" % v, ("rune", v not in (0, 10), None if v not in (0, 10) else "phases")) for v in range(16)] +
    [("big: periodic samiam", ("tiled", True, None)), ("big: two symbols, 65537", ("tiled", False, "image")),
     ("big: two symbols, 262144", ("tiled", False, "image")), ("big: skewed", ("tiled", False, "image"))] +
    [("mid: periodic %d" % i, (cls, True, None)) for i, cls in enumerate(("small", "mid", "mid", "small", "mid", "mid"))] +
    [("mid: sorted shape %d" % k, (cls, k != 6, None if k != 6 else "phases")) for k, cls in enumerate(("mid", "mid", "mid", "mid", "small", "small", "mid"))])
