"""The model of the Huffman lane maps (tests/lane_maps.py) and the limit members built with it (tests/lane_limit_cases.py), held on a CPU:
wherever the model takes a member its composed maps are the encoder's own record of the stream -- the symbols of every lane and block,
every block's first output symbol, the total -- and wherever it hands one back it says why; the emit form of every tile of every taken
tiled member settles a subset of what the map form settled, no later, and arrives at the chain's count; the limit pairs have the
verdicts and the figures they were built for; the composed tile maps are the tile-level model's (tests/huff_big_dec_plan_test.cpp,
restated over the same array); and no member whose hand-back depends on the data is left with "either".  No GPU, no library."""
import os
import random
import re

import numpy as np
import pytest

import lane_limit_cases as C
import lane_maps as M
import long_codes
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")


def _constant(path, name):
    m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=\s*[^,;]+,\s*)*%s\s*=\s*([^;,]+)[;,]" % name, open(os.path.join(SRC, path)).read())
    assert m, name
    return m.group(1).strip()


def test_the_shapes_are_the_kernels():
    from raisin_amd import huffman
    body = lambda name: int(eval(_constant("huff_small_body.h", name).replace("u", "")))
    assert body("DEC_ROUNDS") == M.DEC_ROUNDS and body("OFF_BAD") == M.OFF_BAD
    assert len(re.findall(r"\b64\b", "".join(l for l in open(os.path.join(ROOT, "tests", "lane_maps.py")) if "DEC_ROUNDS" in l))) == 1   # stated once
    assert len(re.findall(r"^DEC_ROUNDS\s*=", open(os.path.join(ROOT, "tests", "lane_maps.py")).read(), re.M)) == 1
    s = M.SHAPES
    assert (s["single"].lanes, s["single"].blocks, s["single"].s_max, s["single"].cap) == (body("DL"), body("DEC_BLOCKS"), body("DEC_S_MAX"), body("DEC_OUT_CAP"))
    assert (s["small"].lanes, s["small"].s_max, s["small"].out_max) == (body("DL"), body("HB_S_MAX"), body("HB_OUT_MAX"))
    assert (s["small"].pay_max, s["small"].out_max) == (huffman.BATCH_GROUP_PAYLOAD_MAX, huffman.BATCH_GROUP_OUTPUT_MAX) and s["small"].pay_max == 256 * 512 // 8
    assert _constant("huff_mid.hip", "HM_T") == "1024" and _constant("huff_mid.hip", "HM_DL") == "HM_T - 64" and _constant("huff_mid.hip", "HM_S_MAX") == "480"
    assert (s["mid"].lanes, s["mid"].s_max, s["mid"].pay_max, s["mid"].out_max) == (960, 480, huffman.MID_PAY_MAX, huffman.MID_OUT_MAX)
    assert _constant("huff_parse_rune.h", "PARSE_RUNE_LANES") == "256" and _constant("huff_parse_rune.h", "PARSE_RUNE_S_MAX") == "576"
    assert (s["rune"].lanes, s["rune"].s_max, s["rune"].pay_max, s["rune"].out_max) == (256, 576, huffman.RUNE_PAY_MAX, huffman.RUNE_OUT_MAX)
    lay = lambda name: int(eval(_constant("huff_big_dec_layout.h", name).replace("u", "")))
    assert (s["tiled"].lanes, s["tiled"].s_max, s["tiled"].cap, s["tiled"].pay_max, s["tiled"].out_max) == (lay("BIGD_LANES"), lay("BIGD_S"), lay("BIGD_OUT_CAP"), lay("BIGD_PAY_MAX"), lay("BIGD_OUT_MAX"))
    assert (s["tiled"].lanes, s["tiled"].s_max, s["tiled"].cap, s["tiled"].pay_max, s["tiled"].out_max) == (huffman.BIG_DEC_LANES, huffman.BIG_DEC_LANE_BITS, huffman.BIG_DEC_OUT_CAP, huffman.BIG_PAY_MAX, huffman.BIG_OUT_MAX)
    assert s["tiled"].blocks == (8 * s["tiled"].pay_max + C.TILE_BITS - 1) // C.TILE_BITS == 30
    # the body the model restates keeps four starts a lane and answers 32 entries
    src = open(os.path.join(SRC, "huff_small_body.h")).read()
    assert "if (n_ent + n_fresh >= 4) { over = true; return; }" in src and "if (round >= DEC_ROUNDS) { lost = true; break; }" in src and "s_ex32[32]" in src
    assert (M.STARTS_MAX, M.ENTRIES) == (4, 32)


# ---------------------------------------------------------------- the members
@pytest.fixture(scope="module")
def samiam():
    return open(os.path.join(ROOT, "tests", "golden", "samiam.txt"), "rb").read()


@pytest.fixture(scope="module")
def cases(samiam):
    """[(name, member)]: the cases of lane_limit_cases.py"""
    out = []
    for cls, place, a, c, _ in C.rounds_pairs():
        out += [("rounds %s %s, %d rounds" % (cls, place, n), d) for n, d in zip((M.DEC_ROUNDS, M.DEC_ROUNDS + 1), (a, c))]
    for cls, place, a, c in C.phases_pairs():
        out += [("phases %s %s, four" % (cls, place), a), ("phases %s %s, five" % (cls, place), c)]
    out.append(("five exits", C.five_exits()))
    out += [("layered %d" % seed, C.layered_member(seed)) for seed in C.LAYERED_SEEDS]
    out += [("flat %d" % bits, C.flat_member(bits)) for bits in (1,) + C.FLAT_BITS]
    out += [(name, d) for name, d, _ in C.either_members(samiam)]
    return out


def _seeded(samiam):
    """[(name, member)]: text, alphabets of 2 to 64 symbols, skewed draws, Fibonacci counts (codes to 24 bits), periodic data, UTF-8 text"""
    from test_gpu_huffman_big_dec import _skewed
    from test_gpu_huffman_mid import _alpha, _text
    rng = random.Random(20261020)
    out = []
    for i in range(60):
        out.append(("text %d" % i, _text(4000 + i, rng.choice((rng.randint(40, 2000), rng.randint(2000, 40000), rng.randint(40000, 70000))))))
    for i in range(70):
        k = rng.randint(2, 64)
        alphabet = bytes(rng.sample(range(1, 128), k))
        out.append(("alphabet of %d, %d" % (k, i), _alpha(4100 + i, rng.choice((rng.randint(30, 3000), rng.randint(3000, 70000))), alphabet)))
    for i in range(25):
        out.append(("skewed %d" % i, _skewed(4200 + i, rng.randint(500, 70000))))
    for k in (8, 10, 12, 14, 16, 18, 20, 21, 22, 23, 24, 25):
        out.append(("fibonacci %d" % k, long_codes.fib_data(k, seed=4)))
    block = _alpha(50, 512, b"abcdefghijklmnopqrstuvwxyz ,.\n")
    for i in range(35):
        unit = (samiam, block[:rng.randint(3, 512)], bytes(rng.sample(range(32, 127), rng.randint(2, 40))))[i % 3]
        n = rng.randint(1000, 70000)
        out.append(("periodic %d" % i, (unit * (n // len(unit) + 1))[:n]))
    from test_gpu_huffman_rune_batch import _utf8
    out += [("runes %d" % i, _utf8(i, 150 + 290 * i)) for i in range(30)]
    return out


def _encoder_side(d):
    """the bit at which every symbol's codeword starts, and behind the last: the encoder's own record of the stream"""
    tab = C.table(d)
    syms = np.frombuffer(d, dtype=np.uint8).astype(np.int64) if max(d) < 0x80 else O.utf8_runes(d).astype(np.int64)
    lens = np.zeros(max(r for r, _, _, _ in tab) + 1, dtype=np.int64)
    for r, _, _, l in tab:
        lens[r] = l
    return np.concatenate(([0], np.cumsum(lens[syms])))


def _check_decode(name, ln, recs, starts):
    S, DLN, span, total = ln.S, ln.shape.lanes, ln.span, len(starts) - 1
    assert span == starts[-1], name
    at = starts[:-1]
    cnt = np.bincount(at // S, minlength=ln.T)
    first = at[np.minimum(np.searchsorted(at, np.arange(ln.T) * S), total - 1)] - np.arange(ln.T) * S
    assert len(recs) == ln.n_blocks and sum(n for _, _, n in recs) == total, name
    for b, (c, base, n) in enumerate(recs):
        lo = b * DLN * S
        i0 = int(np.searchsorted(at, lo))
        assert (base, n) == (i0, int(np.searchsorted(at, min(span, lo + DLN * S))) - i0) and c == (at[i0] if i0 < total else span) - lo, (name, b)
        path = ln.true_lanes(b, c)
        assert [t for t, _, _ in path] == list(range(min(DLN, ln.T - b * DLN))), (name, b)
        for t, st, k in path:
            assert k == cnt[b * DLN + t] and (k == 0 or st == first[b * DLN + t]), (name, b, t)


def test_where_the_model_takes_a_member_its_maps_are_the_decode(samiam, cases):
    members = _seeded(samiam) + cases
    assert len(members) >= 200 + len(cases) - 60
    seen = {cls: [0, 0] for cls in M.SHAPES}
    for name, d in members:
        s = C.enc(d)
        assert O.huffman_decompress(s) == d or len(set(d)) < 2, name
        tab = C.table(d)
        nxt, flat = M.code_ends(s, tab)
        starts = _encoder_side(d)
        for cls, shape in M.SHAPES.items():
            if shape.runes != (max(d) >= 0x80) or len(d) > shape.out_max or len(M.split(s)[0]) > shape.pay_max:
                continue
            ln = M.Lanes(nxt, flat, shape)
            if not ln.held:
                continue
            taken, why, recs = ln.verdict(len(starts) - 1)
            seen[cls][0 if taken else 1] += 1
            if taken:
                _check_decode(name + " in " + cls, ln, recs, starts)
            else:
                assert why in M.REASONS, (name, cls, why)
    print("taken / handed back by class: %r" % seen)
    assert all(t >= 20 for t, _ in seen.values()) and sum(t for t, _ in seen.values()) >= 400, seen


# ---------------------------------------------------------------- the emit launch's rule
def _tiled_taken(cases):
    return [(name, d) for name, d in cases if C.class_of(d) == "tiled" and C.verdict(d, "tiled")[0]]


def test_the_emit_form_settles_a_subset_of_the_map_form(cases):
    members = _tiled_taken(cases)
    assert len(members) >= 15 + 6 + 2 + 2 + 1                                 # layered, flat, rounds, four starts, the periodic samiam
    tight = {"four starts": 0, "last round": 0}
    for name, d in members:
        ln = C.lanes(d, "tiled")[0]
        for t, (entry, base, n) in enumerate(ln.records):
            full = ln.block(t)
            blk, count = ln.emit(t, entry)
            assert not blk.lost, "%s, tile %d: the emit form is lost (%s at lane %d, start %d)" % ((name, t, blk.why) + tuple(blk.where))
            for lane, (got, had) in enumerate(zip(blk.starts, full.starts)):
                at = {x[0]: x[3] for x in had}
                for st, _, _, rnd in got:
                    assert st in at and rnd <= at[st], "%s, tile %d, lane %d, start %d: round %d in the emit form, %s in the map form" % (name, t, lane, st, rnd, at.get(st, "never"))
            assert count == n, "%s, tile %d: the emit form arrives at %r symbols, the chain at %d" % (name, t, count, n)
            tight["four starts"] += blk.fullest == M.STARTS_MAX
            tight["last round"] += blk.rounds == M.DEC_ROUNDS
    print("tiles whose emit form is at a limit: %r" % tight)
    assert tight["four starts"] >= 2 and tight["last round"] >= 2, tight      # the rule is run where it is tight


# ---------------------------------------------------------------- the limit pairs
def test_the_rounds_grow_by_one_a_lane():
    for cls, (_, at) in C.ROUNDS_AT.items():
        for place in at:
            n = C.rounds_lanes(cls, place)
            got = [C.rounds_needed(cls, place, n + k) for k in range(-2, 4)]
            assert got == list(range(M.DEC_ROUNDS - 2, M.DEC_ROUNDS + 4)) and abs(n - M.DEC_ROUNDS) <= 1, (cls, place, n, got)


def test_the_limit_pairs_sit_at_their_limits():
    for cls, place, a, c, b in C.rounds_pairs():
        assert cls in (C.class_of(a), "single") and C.class_of(a) == C.class_of(c) and len(a) == len(c) <= 262144
        la, taken, why = C.lanes(a, cls)
        assert (taken, why, la.block(b).rounds, la.block(b).fullest) == (True, None, M.DEC_ROUNDS, 2), (cls, place)
        lc, taken, why = C.lanes(c, cls)
        assert (taken, why, lc.block(b).lost, lc.block(b).why) == (False, "rounds", True, "rounds"), (cls, place)
        assert C.lanes(c, cls, 1 << 30)[0].block(b).rounds == M.DEC_ROUNDS + 1, (cls, place)
        assert b == (1 if place in ("tile 1", "block 1") else 0)
        if b == 1:                                                 # the true start arrives through the 32 entries
            assert len(la.block(1).first) == M.ENTRIES and len(la.block(1).mask) == 2
    for cls, place, a, c in C.phases_pairs():
        assert cls in (C.class_of(a), "single") and C.class_of(a) == C.class_of(c)
        la, taken, why = C.lanes(a, cls)
        assert (taken, why, max(la.block(b).fullest for b in range(la.n_blocks))) == (True, None, M.STARTS_MAX), (cls, place)
        lc, taken, why = C.lanes(c, cls)
        lost = [lc.block(b) for b in range(lc.n_blocks) if b in lc._blocks and lc.block(b).lost]
        assert (taken, why) == (False, "phases") and len(lost) == 1 and lost[0].where[0] > 1, (cls, place)
        assert lost[0].b == (1 if place in ("tile 1", "block 1") else 0)
    ln, taken, why = C.lanes(C.five_exits(), "tiled")
    assert (taken, why, ln.block(1).lost, ln.block(1).where[0], len(ln.block(1).mask)) == (False, "phases", True, 1, 5)
    # the natural one
    back = [seed for seed in C.LAYERED_SEEDS if not C.verdict(C.layered_member(seed), "tiled")[0]]
    assert back == [C.LAYERED_BACK] and C.verdict(C.layered_member(C.LAYERED_BACK), "tiled") == (False, "phases")
    blk = C.lanes(C.layered_member(C.LAYERED_BACK), "tiled")[0].block(10)
    assert blk.lost and blk.where[0] == 1 and len(blk.mask) == 4             # tile 10: four exits and lane 1's own guess beside them
    # every member is small, and in the tiled class no tile is near the image's cap
    for cls, place, a, c in [(x[0], x[1], x[2], x[3]) for x in C.rounds_pairs()] + C.phases_pairs():
        if cls == "tiled":
            bits = C.lanes(a, cls)[0].span / len(a)
            assert len(a) > 65536 and bits >= 2, (cls, place, bits)


def test_the_flat_codes():
    bases, entries = set(), set()
    for bits in C.FLAT_BITS:
        d = C.flat_member(bits)
        ln, taken, why = C.lanes(d, "tiled")
        assert taken and ln.flat == bits and ln.n_blocks >= 3 and 65536 < len(d) <= 262144, bits
        assert [len(ln.block(t).first) for t in range(ln.n_blocks)] == [1] * ln.n_blocks
        assert max(ln.block(t).rounds for t in range(ln.n_blocks)) == 0        # the boundaries are where the arithmetic says: nothing to learn
        bases |= {base % 16 for _, base, _ in ln.records}
        entries |= {(bits, c) for c, _, _ in ln.records}
    # A tile is 61440 = 2^12 * 15 bits, a multiple of 2, 3, 4, 5 and 6: at those widths every tile is entered at bit 0 and begins at an
    # output byte that is a multiple of 16.  Only 7 bits move the entry, and tile t + 7 begins 61440 bytes behind tile t: seven residues
    # mod 16 are all that flat codes can reach, and the set reaches every one of them (tests/test_gpu_huffman_lane_limits.py asks the
    # members of the tiled class as a whole for all sixteen).
    assert {c for b, c in entries if b != 7} == {0} and {c for b, c in entries if b == 7} == set(range(7)), entries
    assert bases == {-(-61440 * t // 7) % 16 for t in range(7)} and len(bases) == 7, bases
    assert C.verdict(C.flat_member(1), "tiled") == (False, "image")


# ---------------------------------------------------------------- the tile-level model
def test_the_composed_tile_maps_are_the_tile_level_models(cases):
    members = _tiled_taken(cases)
    for name, d in members:
        ln = C.lanes(d, "tiled")[0]
        want = M.tile_model(ln.nxt, C.TILE_BITS, ln.flat)
        assert len(want) == ln.n_blocks
        for t in range(ln.n_blocks):
            got = ln.block_map(t)
            for c in ln.block(t).first:
                assert got[c] == want[t][c], (name, t, c, got[c], want[t][c])


# ---------------------------------------------------------------- no "either"
def test_no_member_is_left_with_either(samiam):
    got = {}
    for name, d, cls in C.either_members(samiam):
        assert cls == C.class_of(d) and cls is not None, name
        taken, why = C.verdict(d, cls)
        assert isinstance(taken, bool) and (why is None if taken else why in M.REASONS), name
        got[name] = (cls, taken, why)
    assert got == C.EITHER_WANT
