"""GPU: the tiled class of the Huffman decompress batch (csrc/huff_big_dec.hip) -- streams of a byte alphabet that promise more
than huffman.MID_OUT_MAX and at most huffman.BIG_OUT_MAX bytes are cut into tiles of their payload (BIG_DEC_LANES lanes of BIG_DEC_LANE_BITS
code bits) and a group of them is THREE launches (huff_batch_big_dec_map, huff_batch_big_dec_chain, huff_batch_big_dec_emit) between
huff_dev_gather and huff_dev_scatter, in the host form too.  Every result is compared byte for byte with the CPU oracle's huffman_decompress
AND with the library's single huffman.Decompress; what the chain hands back (a tile of more symbols than the emit image holds, malformed
streams) and what the wide plan refuses must come out of the single call with the same bytes or the same error.  Every list is padded to
BIG_DEC_GROUP_MIN members of the class with text of MID_OUT_MAX + 1 + 100 i bytes.

Which members are taken is not read off the library: _taken() is the verdict of the CPU model of the lane maps (tests/lane_maps.py, held
on a CPU by tests/test_lane_maps_host.py) -- phases, rounds, the emit image's cap -- on the member's stream, with its reason; _tiles()
restates the chain from the ENCODER's side -- the code lengths of the member's bytes, summed -- into every tile's first output byte and
symbol count, and the model's records must be those."""
import numpy as np
import pytest

import lane_limit_cases as C
import long_codes
from test_gpu_batch_dev import E_CAP, OK, SINGLE_WORDS, Pack, _batch, _fenced_call, _out_bytes, _prof, _ru16
from test_gpu_huffman_batch_dev import _run_slots
from test_gpu_huffman_big import _text, _with_counts
from test_gpu_huffman_mid import _outcome

pytestmark = pytest.mark.gpu

DEC = "rsn_huffman_decompress_batch_dev"
NEW = ("huff_batch_big_dec_map", "huff_batch_big_dec_chain", "huff_batch_big_dec_emit")


def _general(prof):
    """the launches of the single call's decoders (huff_decode.hip: huff_dec_*; huff_small.hip: huff_small_dec)"""
    return {k for k in prof if k.startswith("huff_dec_") or k == "huff_small_dec"}


HOST_PROF = dict({name: 1 for name in NEW}, huff_dev_gather=1, huff_dev_scatter=1)
DEV_PROF = dict(HOST_PROF, huff_dev_plan=1)
PLAN_UP, PLAN_DOWN, DEC_UP, DEC_DOWN = 16, 16, 64, 4   # huff_dev.hip: a candidate's plan entry up and summary down, a member's table entry up and answer down
LZ, HU = "lzss", "huffman"


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman
    _lib.check(_lib.lib().rsn_device_set(0))
    assert huffman.BIG_DEC_LANES * huffman.BIG_DEC_LANE_BITS == 61440 and huffman.BIG_OUT_MAX == huffman.BIG_IN_MAX
    return _lib, huffman


_ENC, _DEC, _SINGLE = {}, {}, {}


def _enc(oracle, d):
    if d not in _ENC:
        _ENC[d] = oracle.huffman_compress(d)
    return _ENC[d]


def _dec(oracle, s):
    """the oracle's answer, computed once per stream"""
    if s not in _DEC:
        _DEC[s] = oracle.huffman_decompress(s)
    return _DEC[s]


def _single_call(huffman, s):
    if s not in _SINGLE:
        _SINGLE[s] = huffman.Decompress(s)
    return _SINGLE[s]


def _payload(s):
    return len(s) - s.index(b"\\\n") - 3


def _in_class(huffman, d):
    """by the member the stream was written for (a byte alphabet: at most 7 bits a byte, so the payload bound holds)"""
    return huffman.MID_OUT_MAX < len(d) <= huffman.BIG_OUT_MAX and max(d) < 0x80 and len(set(d)) > 1


def _tiles(oracle, huffman, d):
    """[(first output byte, symbols)] of every tile of d's stream: a symbol belongs to the tile its codeword's first bit lies in"""
    lens = np.zeros(256, dtype=np.int64)
    for r, _, _, l in oracle.huffman_table(d):
        lens[r] = l
    starts = np.concatenate(([0], np.cumsum(lens[np.frombuffer(d, dtype=np.uint8)])))
    span, tile = int(starts[-1]), huffman.BIG_DEC_LANES * huffman.BIG_DEC_LANE_BITS
    bases = [int(np.searchsorted(starts[:-1], t * tile)) for t in range((span + tile - 1) // tile)] + [len(d)]
    return [(bases[t], bases[t + 1] - bases[t]) for t in range(len(bases) - 1)]


def _taken(oracle, huffman, d):
    """a member of the class that the model of the lane maps takes: no tile lost to phases or rounds, every tile within the emit image"""
    if not _in_class(huffman, d):
        return False
    ln, taken, why = C.lanes(d, "tiled")
    if taken:
        assert [(base, n) for _, base, n in ln.records] == _tiles(oracle, huffman, d)
    else:
        assert why != "image" or any(n + 16 > huffman.BIG_DEC_OUT_CAP for _, n in _tiles(oracle, huffman, d))
    return taken


def _pad(huffman, members, seed=700):
    have = sum(1 for d in members if _in_class(huffman, d))
    return list(members) + [_text(seed + i, huffman.MID_OUT_MAX + 1 + 100 * i) for i in range(max(0, huffman.BIG_DEC_GROUP_MIN - have))]


def _host(mods, oracle, members):
    """the host form over the members' streams -> prof; the bytes against the oracle and the single call"""
    _lib, huffman = mods
    streams = [_enc(oracle, d) for d in members]
    got, prof, _ = _prof(_lib, lambda: huffman.DecompressBatch(streams))
    for d, s, g in zip(members, streams, got):
        assert g == _dec(oracle, s) == d, (len(d), d[:24])
        assert g == _single_call(huffman, s), (len(d), d[:24])
    return prof


def _dev(mods, oracle, members, behind=None):
    """the device form: exact capacities for the members the class completes, the single call's need for the others -> (prof, copied)"""
    _lib, huffman = mods
    streams = [_enc(oracle, d) for d in members]
    grouped = sum(1 for d in members if _in_class(huffman, d)) >= huffman.BIG_DEC_GROUP_MIN
    exact = [grouped and _taken(oracle, huffman, d) for d in members]
    caps = [len(d) if e else _ru16(len(d)) + 16 for d, e in zip(members, exact)]
    got, prof, copied = _run_slots(_lib, DEC, streams, caps, behind=behind, loose=[i for i, e in enumerate(exact) if not e])
    for d, s, g in zip(members, streams, got):
        assert g == _dec(oracle, s) == d, (len(d), d[:24])
    return prof, copied


def _new_once(prof):
    return all(prof.get(name) == 1 for name in NEW)


# ---------------------------------------------------------------- 1: one group, the exact profile
def test_one_group_exact_profile(mods, oracle):
    _lib, huffman = mods
    sizes = [65537, 5 * 16384 - 1, 5 * 16384 + 1, 100000, 200000, 262144]
    members = [_text(10 + i, n) for i, n in enumerate(sizes)]
    assert all(_taken(oracle, huffman, d) for d in members) and len(members) >= huffman.BIG_DEC_GROUP_MIN
    assert max(len(_tiles(oracle, huffman, d)) for d in members) >= 15
    prof = _host(mods, oracle, members)
    assert prof == HOST_PROF, prof                                            # the three launches once, and no launch of a single call's decoder
    prof, _ = _dev(mods, oracle, members)
    assert prof == DEV_PROF, prof


# ---------------------------------------------------------------- 2: cutoffs
def test_cutoffs(mods, oracle):
    _lib, huffman = mods
    K = max(huffman.BIG_DEC_GROUP_MIN, huffman.MID_GROUP_MIN)
    two = np.random.default_rng(60).choice(np.frombuffer(b"xy", dtype=np.uint8), 65537).tobytes()
    s = _enc(oracle, two[:65536])
    assert _payload(s) == 8192
    dec, prof, _ = _prof(_lib, lambda: huffman.DecompressBatch([s] * K))
    assert prof == {"huff_batch_mid_dec": 1}, prof                            # 64 KiB out: the mid decoder's
    assert dec == [two[:65536]] * K
    s = _enc(oracle, two)
    dec, prof, _ = _prof(_lib, lambda: huffman.DecompressBatch([s] * K))
    assert _new_once(prof) and "huff_batch_mid_dec" not in prof, prof         # one byte more: this class's
    assert dec == [two] * K == [_single_call(huffman, s)] * K == [_dec(oracle, s)] * K
    assert not _taken(oracle, huffman, two) and C.verdict(two, "tiled") == (False, "image")   # (a bit a symbol: two tiles, the first of 61440 symbols)
    prof, _ = _dev(mods, oracle, [two] * K)                                   # (a handed-back member's single call is a batch worker's in the host form: not in this
    assert _new_once(prof) and _general(prof), prof                           #  thread's profile; in the device form it is this thread's)
    # the payload limit: 128 symbols of 7 bits each
    flat = _with_counts(61, {b: 2048 for b in range(128)}, True)
    s = _enc(oracle, flat)
    assert len(flat) == huffman.BIG_OUT_MAX and _payload(s) == huffman.BIG_PAY_MAX == 229376 and len(s) == 230148
    assert _taken(oracle, huffman, flat) and len(_tiles(oracle, huffman, flat)) == 30
    members = _pad(huffman, [flat])
    assert _host(mods, oracle, members) == HOST_PROF
    assert _dev(mods, oracle, members)[0] == DEV_PROF
    more = _with_counts(62, {b: 2049 if b == 65 else 2048 for b in range(128)}, True)
    assert len(more) == huffman.BIG_OUT_MAX + 1 and not _in_class(huffman, more)
    members = _pad(huffman, [more])
    prof = _host(mods, oracle, members)                                       # (the single call's launches are a batch worker's: not this thread's)
    assert _new_once(prof), prof
    prof, _ = _dev(mods, oracle, members)
    assert _new_once(prof) and _general(prof), prof                      # ... the single call's decoder for the one
    # fewer members than the minimum: no new launch
    few = [_text(70 + i, huffman.MID_OUT_MAX + 1 + 100 * i) for i in range(huffman.BIG_DEC_GROUP_MIN - 1)]
    for prof in (_host(mods, oracle, few), _dev(mods, oracle, few)[0]):
        assert not set(prof) & set(NEW), prof


# ---------------------------------------------------------------- 3: tile edges
def _skewed(seed, n):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(n) < 0.9, 0x61, rng.integers(0x62, 0x72, n)).astype(np.uint8).tobytes()


def test_tile_edges(mods, oracle):
    _lib, huffman = mods
    two = np.random.default_rng(80).choice(np.frombuffer(b"ab", dtype=np.uint8), 262144).tobytes()
    assert _payload(_enc(oracle, two)) == 32768                               # a payload tile that decodes to eight times what it holds
    fib = long_codes.fib_data(25, seed=4)
    assert len(fib) == 196417 and max(l for _, _, _, l in oracle.huffman_table(fib)) == 24
    skew = _skewed(81, 150000)
    bits = 8.0 * _payload(_enc(oracle, skew)) / len(skew)
    assert 1.2 < bits < 1.6, bits
    # the tiles' first output bytes on every residue mod 16: texts are added until the restated chain has seen them all, so that the list
    # cannot silently miss one
    texts, residues = [], {b % 16 for b, _ in _tiles(oracle, huffman, fib)}
    for i in range(12):
        d = _text(82 + i, 90001 + 7919 * i)
        new = {b % 16 for b, _ in _tiles(oracle, huffman, d)} - residues
        if new or len(texts) < 4:
            texts.append(d)
            residues |= new
    assert residues == set(range(16)) and 4 <= len(texts) <= 8, (residues, len(texts))
    verdicts = {"two symbols": _taken(oracle, huffman, two), "fibonacci": _taken(oracle, huffman, fib), "skewed": _taken(oracle, huffman, skew)}
    print("taken by the shape: %r" % verdicts)
    assert verdicts["fibonacci"]                                              # 24-bit codes that straddle tiles: taken, not handed back
    assert verdicts == {"two symbols": False, "fibonacci": True, "skewed": False}   # the cap: fewer than 1.875 bits a symbol over a tile is the single call's
    assert C.verdict(two, "tiled") == C.verdict(skew, "tiled") == (False, "image")
    assert _host(mods, oracle, texts + [fib]) == HOST_PROF
    assert _dev(mods, oracle, texts + [fib])[0] == DEV_PROF
    members = [two, texts[0], fib, skew] + texts[1:]
    prof = _host(mods, oracle, members)
    assert _new_once(prof), prof
    prof, _ = _dev(mods, oracle, members)
    assert _new_once(prof) and _general(prof), prof                      # the two handed back took the single call


# ---------------------------------------------------------------- 4: hand-backs word the single call's answer
def test_hand_backs_word_the_single_calls_answer(mods, oracle):
    _lib, huffman = mods
    good = _enc(oracle, _text(90, 100000))
    sep = good.index(b"\\\n")
    rng = np.random.default_rng(91)
    bad = {
        "a header naming a byte >= 0x80": good[:sep] + b"5|" + "é".encode() + good[sep:],
        "one distinct byte": _enc(oracle, b"z" * 70000),
        "cut inside its last codeword": good[:-1],
        "100 extra payload bytes": good + rng.integers(0, 256, 100, dtype=np.uint8).tobytes(),
        "a pad byte >= the payload bits": b"40000|a40000|b\\\n\x09\x80",
    }
    pads = [_enc(oracle, d) for d in _pad(huffman, [])]
    at = len(pads) // 2
    for what, s in bad.items():
        single = _outcome(lambda: huffman.Decompress(s))
        lst = pads[:at] + [s] + pads[at:]
        batch, prof, _ = _prof(_lib, lambda: _outcome(lambda: huffman.DecompressBatch(lst)))
        assert _new_once(prof), (what, prof)                                  # the other members of the list are still grouped
        if single[0] == "ok":
            assert batch[0] == "ok" and batch[1][at] == single[1] == _dec(oracle, s), what
            assert batch[1][:at] + batch[1][at + 1:] == [_dec(oracle, p) for p in pads], what
        else:
            assert batch[0] == "err" and batch[1] == single[1], (what, single, batch)
            msg = _lib.lib().rsn_last_error().decode()
            assert msg.startswith("member %d: " % at) and msg.split(": ", 1)[1] == single[2].split(": ", 1)[1], (what, msg, single)


# ---------------------------------------------------------------- 5: nothing depends on what the scratch held
def test_scratch_independence(mods, oracle):
    _lib, huffman = mods
    sizes = (65537, 81921, 100003, 150000)
    first = [_text(170 + i, n) for i, n in enumerate(sizes)]
    other = [_text(180 + i, n + 4001) for i, n in enumerate(sizes)] + [_text(186, 250000)]

    def mostly(seed, n):                                                      # two thirds of the bytes 0x7F, the rest over eight others: two bits a symbol, taken
        rng = np.random.default_rng(seed)
        return np.where(rng.random(n) < 0.65, 0x7F, rng.integers(0x30, 0x38, n)).astype(np.uint8).tobytes()
    sevens = [mostly(190 + i, n) for i, n in enumerate(sizes)]                # taken: the output slots mostly 0x7F
    high = [b"\x01" + b"\x7f" * (n - 1) for n in sizes]                       # the frequent byte codes as '1': streams of 0xFF in every input slot (handed back
    assert all(_taken(oracle, huffman, d) for d in sevens)                    # by the chain: a bit a symbol -- the gather and the map launch have run over them)
    assert all(_enc(oracle, d)[-40:] == b"\xff" * 40 and not _taken(oracle, huffman, d) for d in high)
    for run in (_host, lambda m, o, x: _dev(m, o, x, behind=lambda i: b"\xff")[0]):
        want = HOST_PROF if run is _host else DEV_PROF
        for between in (other, sevens, high):
            assert run(mods, oracle, first) == want
            run(mods, oracle, between)
        assert run(mods, oracle, first) == want


# ---------------------------------------------------------------- 6: the device form stays inside its buffers
def test_device_form_capacities_and_copies(mods, oracle):
    _lib, huffman = mods
    members = [_text(160 + i, n) for i, n in enumerate((65537, 81919, 81927, 100000, 131072, 200001))]
    assert all(_taken(oracle, huffman, d) for d in members) and len({len(d) % 16 for d in members}) >= 4
    streams = [_enc(oracle, d) for d in members]
    # exact capacities between fences
    rc, lens, msg, outs = _fenced_call(_lib, DEC, streams, [len(d) for d in members])
    assert rc == OK, msg
    assert lens == [len(d) for d in members] and [_out_bytes(o, k) for o, k in zip(outs, lens)] == members
    # one byte short, and the size query: the documented figure, every other member complete, the fences untouched
    tight = {1: "one byte short", 2: "null", 5: "one byte short"}
    figure = [_ru16(len(d)) + 16 for d in members]                            # rsn.h: what a decompress member that does not fit reports
    caps = [len(d) - 1 if i in tight else len(d) for i, d in enumerate(members)]
    rc, lens, msg, outs = _fenced_call(_lib, DEC, streams, caps, null_out=(2,))
    assert rc == E_CAP and msg.startswith("member 1: huffman: output needs %d bytes, buffer holds %d" % (len(members[1]), len(members[1]) - 1)), msg
    for i, d in enumerate(members):
        if i in tight:
            assert lens[i] == figure[i], (i, lens[i], figure[i])
        else:
            assert lens[i] == len(d) and _out_bytes(outs[i], lens[i]) == d, i
    # members back to back at 16-byte offsets; what crosses to the host is a member's plan entry and table entry up, its summary and answer down
    prof, copied = _dev(mods, oracle, members)
    assert prof == DEV_PROF, prof
    k = len(members)
    assert copied[0] <= k * (PLAN_UP + DEC_UP) + SINGLE_WORDS and copied[1] <= k * (PLAN_DOWN + DEC_DOWN) + SINGLE_WORDS, copied


# ---------------------------------------------------------------- 7: through the layers
def test_through_the_layers(mods, oracle):
    import torch
    _lib, huffman = mods
    from raisin_amd import layers
    members = [_text(190 + i, 200000) for i in range(max(4, huffman.BIG_DEC_GROUP_MIN))]
    moved = set(NEW) | {"huff_dev_plan", "huff_dev_gather", "huff_dev_scatter", "members_move"}
    for names in ([HU], [LZ, HU]):
        streams = [layers.Compress(d, names) for d in members]                # the chain of single calls
        assert [layers.Decompress(s, names) for s in streams] == members
        got, prof, _ = _prof(_lib, lambda: layers.DecompressBatch(streams, names))
        assert got == members
        if names == [HU]:
            assert streams == [_enc(oracle, d) for d in members]
            assert _new_once(prof) and set(prof) <= moved, prof               # the three launches once, no launch of a single call's decoder
        pack = Pack(streams)
        srcs = [pack.t[o:o + n] for o, n in zip(pack.offs, pack.lens)]
        got, prof, _ = _prof(_lib, lambda: [bytes(t.cpu().numpy()) for t in layers.decompress_tensors(srcs, names)])
        assert got == members
        if names == [HU]:
            assert _new_once(prof) and not _general(prof), prof
        res, prof, _ = _prof(_lib, lambda: layers.RoundTripBatch(members, names, hists=False))
        assert [(r.original_n, r.compressed_n, r.decompressed_n, r.lossless) for r in res] == [(len(d), len(s), len(d), True) for d, s in zip(members, streams)]
        if names == [HU]:
            assert _new_once(prof) and not _general(prof), prof


# ---------------------------------------------------------------- 8: closure
def test_the_decoder_takes_every_stream_the_big_encoder_writes(mods, oracle, samiam):
    _lib, huffman = mods
    flat = _with_counts(61, {b: 2048 for b in range(128)}, True)
    plain = [_text(10 + i, n) for i, n in enumerate([65537, 5 * 16384 - 1, 5 * 16384 + 1, 100000, 200000, 262144])] + [flat]   # tests 1 and 2: text and alphabets
    periodic = (samiam * (150000 // len(samiam) + 1))[:150000]
    two = np.random.default_rng(80).choice(np.frombuffer(b"ab", dtype=np.uint8), 262144).tobytes()
    named = [("periodic", periodic), ("two symbols", two), ("skewed", _skewed(81, 150000))]   # the model's verdicts on them: the lanes take the periodic one
    assert [C.verdict(d, "tiled") for _, d in named] == [(True, None), (False, "image"), (False, "image")]
    assert all(C.EITHER_WANT[k] == ("tiled",) + C.verdict(d, "tiled") for k, (_, d) in zip(("big: periodic samiam", "big: two symbols, 262144", "big: skewed"), named))
    members = plain + [d for _, d in named] + [long_codes.fib_data(25, seed=4)]
    assert all(huffman.MID_IN_MAX < len(d) <= huffman.BIG_IN_MAX for d in members)
    streams, prof, _ = _prof(_lib, lambda: huffman.CompressBatch(members))
    assert prof.get("huff_batch_big_emit") == 1 and streams == [_enc(oracle, d) for d in members]    # every one a taken member of the big encoder's class
    # ... and every such stream is one the decoder's takes() takes: a list of any BIG_DEC_GROUP_MIN of them launches the class
    for s in streams:
        assert _payload(s) <= huffman.BIG_PAY_MAX
        _, prof, _ = _prof(_lib, lambda: huffman.DecompressBatch([s] * huffman.BIG_DEC_GROUP_MIN))
        assert _new_once(prof), (len(s), prof)
    # the hand-backs are the model's: of the text and alphabet members none, the periodic one neither; the two-symbol and the skewed one
    assert _host(mods, oracle, plain + [periodic, members[-1]]) == HOST_PROF
    assert _dev(mods, oracle, plain + [periodic, members[-1]])[0] == DEV_PROF
    for name, d in named:                                                     # (the device form: a single call's launches are this thread's there)
        lst = _pad(huffman, [d])
        _host(mods, oracle, lst)
        prof, _ = _dev(mods, oracle, lst)                                     # (exact capacities wherever the model says taken)
        assert _new_once(prof) and (prof == DEV_PROF) == _taken(oracle, huffman, d) == (not _general(prof)), (name, prof)
