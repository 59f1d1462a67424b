"""GPU: every grouped Huffman decoder held to the CPU model of its lane maps (tests/lane_maps.py) at the model's limits -- the members of
tests/lane_limit_cases.py: a stretch that settles in round DEC_ROUNDS beside one that needs a round more, a lane that ends with four
starts beside one that is offered a fifth, a tile whose 32 entries leave through five exits, flat codes of 2 to 7 bits, the stream the
tiled class hands back among the sixteen layered texts, the rune counters.  Taken means taken: the model's taken members on their own
show exactly the class's launches.  Handed back means handed back: with the model's handed-back members mixed in, and each of them
alone among pads, the device form shows the single call's decoder beside the class's launches.  Every byte is the CPU oracle's and the
single call's; the streams lie back to back in one allocation with hostile bytes between them, out_cap exactly the result size wherever
the model says taken and the documented figure where it says handed back (tests/test_gpu_batch_dev.py's instruments).  The model and
the members are held on a CPU by tests/test_lane_maps_host.py."""
import pytest

import lane_limit_cases as C
from test_gpu_batch_dev import _prof, _ru16
from test_gpu_huffman_batch_dev import DEC, _run_slots

pytestmark = pytest.mark.gpu

TILED = ("huff_batch_big_dec_map", "huff_batch_big_dec_chain", "huff_batch_big_dec_emit")
RUNE, RUNE_PLAN = "huff_batch_rune_dec", "huff_dev_rune_plan"
SINGLE = "huff_small_dec"


def _staged(kernels):
    host = dict({k: 1 for k in kernels})
    return host, dict(host, huff_dev_plan=1, huff_dev_gather=1, huff_dev_scatter=1)


# class -> (its launches, the exact profile of a list it takes whole in the host form, ... in the device form)
PROFILES = {
    "tiled": (TILED, dict({k: 1 for k in TILED}, huff_dev_gather=1, huff_dev_scatter=1), dict({k: 1 for k in TILED}, huff_dev_plan=1, huff_dev_gather=1, huff_dev_scatter=1)),
    "mid": (("huff_batch_mid_dec",),) + _staged(("huff_batch_mid_dec",)),
    "small": (("huff_batch_dec",),) + _staged(("huff_batch_dec",)),
    "rune": ((RUNE,), {RUNE: 1}, {"huff_dev_plan": 1, RUNE_PLAN: 1, "group_gather": 1, RUNE: 1, "group_scatter": 1}),
}


def _general(prof):
    """the launches of the single call's decoders (huff_decode.hip: huff_dec_*; huff_small.hip: huff_small_dec)"""
    return {k for k in prof if k.startswith("huff_dec_") or k == SINGLE}


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman
    _lib.check(_lib.lib().rsn_device_set(0))
    return _lib, huffman


_CHECKED = set()


def _bytes_checked(huffman, oracle, d):
    """the member's stream against the oracle and the single call, once"""
    if d not in _CHECKED:
        s = C.enc(d)
        assert oracle.huffman_decompress(s) == d and huffman.Decompress(s) == d, (len(d), d[:24])
        _CHECKED.add(d)


def _pads(huffman, cls, k):
    """k members of the class that the model takes"""
    if cls == "tiled":
        from test_gpu_huffman_big import _text
        pads = [_text(700 + i, huffman.MID_OUT_MAX + 1 + 100 * i) for i in range(k)]
    elif cls == "rune":
        from test_gpu_huffman_rune_dec_batch import _texts
        pads = _texts(k)
    else:
        from test_gpu_huffman_mid import _text
        pads = [_text(900 + i, (40000 if cls == "mid" else 3000) + 100 * i) for i in range(k)]
    assert all(C.class_of(d) == cls and C.verdict(d, cls) == (True, None) for d in pads), cls
    return pads


def _run(mods, oracle, cls, members):
    """the list in both forms; what the profile must show follows from the model's verdicts"""
    _lib, huffman = mods
    kernels, host_prof, dev_prof = PROFILES[cls]
    assert all(C.class_of(d) == cls for d in members)
    taken = [C.verdict(d, cls)[0] for d in members]
    streams = [C.enc(d) for d in members]
    for d in members:
        _bytes_checked(huffman, oracle, d)
    got, prof, _ = _prof(_lib, lambda: huffman.DecompressBatch(streams))
    assert got == members
    assert all(prof.get(k) == 1 for k in kernels), prof
    if all(taken):
        assert prof == host_prof, prof                                        # no launch of the single call's decoder
    caps = [len(d) if t else _ru16(len(d)) + 16 for d, t in zip(members, taken)]
    got, prof, _ = _run_slots(_lib, DEC, streams, caps, behind=lambda i: b"\xac\xbf\x80", loose=[i for i, t in enumerate(taken) if not t])
    assert got == members
    assert all(prof.get(k) == 1 for k in kernels), prof
    if all(taken):
        assert prof == dev_prof, prof
    else:
        assert _general(prof), prof                                           # the handed-back members took the single call
    return taken


def _class_test(mods, oracle, cls, group_min, taken, pairs, back):
    """taken: members the model takes; pairs: limit pairs (taken, handed back); back: further members the model hands back"""
    _, huffman = mods
    pads = _pads(huffman, cls, group_min)
    assert all(C.verdict(d, cls) == (True, None) for d in taken + [a for a, _ in pairs])
    assert all(not C.verdict(d, cls)[0] for d in back + [c for _, c in pairs])
    # taken means taken
    alone = taken + [a for a, _ in pairs]
    assert all(_run(mods, oracle, cls, alone + pads[:max(0, group_min - len(alone))]))
    # handed back means handed back: the pairs side by side in both orders, the others between pads
    mixed = [x for a, c in pairs for x in (a, c, a)] + [x for c in back for x in (c, pads[0])] + pads[1:]
    assert _run(mods, oracle, cls, mixed).count(False) == len(pairs) + len(back)
    for c in [c for _, c in pairs] + back:
        assert _run(mods, oracle, cls, pads[:group_min // 2] + [c] + pads[group_min // 2:]).count(False) == 1


def _pairs(cls):
    rounds = [(a, c) for k, _, a, c, _ in C.rounds_pairs() if k == cls]
    phases = [(a, c) for k, _, a, c in C.phases_pairs() if k == cls]
    assert rounds and phases
    for a, c in rounds:
        assert C.verdict(c, cls) == (False, "rounds")
    for a, c in phases:
        assert C.verdict(c, cls) == (False, "phases")
    return rounds + phases


def test_tiled(mods, oracle):
    _, huffman = mods
    flats = [C.flat_member(bits) for bits in C.FLAT_BITS]
    natural = C.layered_member(C.LAYERED_BACK)
    exits = C.five_exits()
    assert C.verdict(natural, "tiled") == C.verdict(exits, "tiled") == (False, "phases") and C.verdict(C.flat_member(1), "tiled") == (False, "image")
    pairs = _pairs("tiled")
    assert len(pairs) == 4                                                    # rounds and phases, in tile 0 and through the 32 entries of tile 1
    # the tiles' first output bytes, from the model: the flat codes reach the seven residues mod 16 they can, the taken members all sixteen
    bases = {bits: {base % 16 for _, base, _ in C.lanes(d, "tiled")[0].records} for bits, d in zip(C.FLAT_BITS, flats)}
    assert len(set().union(*bases.values())) == 7 and bases[7] == {-(-61440 * t // 7) % 16 for t in range(7)}, bases
    every = flats + [a for a, _ in pairs] + _pads(huffman, "tiled", huffman.BIG_DEC_GROUP_MIN)
    assert {base % 16 for d in every for _, base, _ in C.lanes(d, "tiled")[0].records} == set(range(16))
    _class_test(mods, oracle, "tiled", huffman.BIG_DEC_GROUP_MIN, flats, pairs, [exits, natural, C.flat_member(1)])


def test_mid(mods, oracle):
    _, huffman = mods
    _class_test(mods, oracle, "mid", huffman.MID_GROUP_MIN, [], _pairs("mid"), [])


def test_small_batch(mods, oracle):
    _class_test(mods, oracle, "small", 4, [], _pairs("small"), [])


def test_rune(mods, oracle, samiam):
    _, huffman = mods
    counters = [(name, d) for name, d, cls in C.either_members(samiam) if cls == "rune"]
    assert len(counters) == 16 and all(C.EITHER_WANT[name] == (("rune",) + C.verdict(d, "rune")) for name, d in counters)
    back = [d for _, d in counters if not C.verdict(d, "rune")[0]]
    assert len(back) == 2 and all(C.verdict(d, "rune") == (False, "phases") for d in back)
    _class_test(mods, oracle, "rune", huffman.RUNE_DEC_GROUP_MIN, [d for _, d in counters if d not in back], [], back)


def test_the_multi_block_single_call(mods, oracle):
    """huffman.Decompress on its own: huff_small_dec alone where the model takes the stream in 256 lanes x up to 32 blocks, the general
    decoder's launches behind it where the model hands it back"""
    _lib, huffman = mods
    from test_gpu_huffman_mid import _text
    pairs = _pairs("single")
    assert len(pairs) == 4                                                    # rounds and phases, in block 0 and through the 32 entries of block 1
    members = [x for a, c in pairs for x in (a, c)] + [C.phases_member("single", "block 1", C.EXITS)] + [_text(930 + i, 20000 + 9000 * i) for i in range(4)]
    verdicts = [C.verdict(d, "single") for d in members]
    assert [t for t, _ in verdicts[:9]] == [True, False] * 4 + [False] and sum(t for t, _ in verdicts[9:]) >= 2   # (the model decides on the texts too)
    for d, (taken, why) in zip(members, verdicts):
        s = C.enc(d)
        got, prof, _ = _prof(_lib, lambda: huffman.Decompress(s))
        assert got == d == oracle.huffman_decompress(s)
        assert prof.get(SINGLE) == 1, prof
        assert (prof == {SINGLE: 1}) == taken and bool(_general(prof) - {SINGLE}) == (not taken), (len(d), why, prof)
