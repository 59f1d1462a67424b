"""GPU: the tiled class of the LZSS decompress batch (csrc/lzss_tile_dec.hip) -- the streams the small and the mid class leave,
longer than 2 KiB and at most lz.TILE_DEC_IN_MAX bytes, expanding to at most lz.TILE_DEC_OUT_MAX escaped bytes, are cut into tiles of
lz.TILE_POS bytes and a group of them is the launches lzss_batch_tile_dec_parse, _plan, _resolve and _finish between k_group_gather and
k_group_scatter -- in the host form too, which runs on device staging as the other tiled classes do.  Every result is compared byte for
byte with the CPU oracle AND with the library's single call; what the kernels hand back must come out of the single call with the same
bytes or the same error code.  The lists are padded to lz.TILE_DEC_GROUP_MIN candidates with copies of the stream of ONE text of 65537
bytes; hand-written streams are built here from literals and tokens, and the expected bytes always come from the oracle."""
import random

import pytest

from test_gpu_batch_dev import E_CAP, OK, Pack, _batch, _fenced_call, _out_bytes, _prof, _ru16, _run_slots
from test_gpu_lzss_mid import _text

pytestmark = pytest.mark.gpu

DEC = "rsn_lzss_decompress_batch_dev"
NEW = ("lzss_batch_tile_dec_parse", "lzss_batch_tile_dec_plan", "lzss_batch_tile_dec_resolve", "lzss_batch_tile_dec_finish")
ONLY = dict({name: 1 for name in NEW}, group_gather=1, group_scatter=1)     # one group of the class: every launch once and nothing else
MID = "lzss_batch_mid_dec"
P = 2048


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, lz
    _lib.check(_lib.lib().rsn_device_set(0))
    assert lz.TILE_POS == P
    return _lib, lz


_ENC, _WANT, _SINGLE = {}, {}, {}


def _enc(oracle, d, w=4096):
    if (d, w) not in _ENC:
        _ENC[d, w] = oracle.lzss_compress(d, w)
    return _ENC[d, w]


def _want(oracle, s):
    if s not in _WANT:
        _WANT[s] = oracle.lzss_decompress(s)
    return _WANT[s]


def _single(lz, s):
    if s not in _SINGLE:
        _SINGLE[s] = lz.Decompress(s)
    return _SINGLE[s]


def _candidate(lz, s):
    return P < len(s) <= lz.TILE_DEC_IN_MAX


def _pad(lz, oracle, streams, short=0):
    """at least TILE_DEC_GROUP_MIN - short candidates: copies of the stream of one text of 65537 bytes behind the ones the test is about"""
    have = sum(1 for s in streams if _candidate(lz, s))
    return list(streams) + [_enc(oracle, _text(4000, 65537))] * max(0, lz.TILE_DEC_GROUP_MIN - short - have)


def _host(mods, oracle, streams):
    _lib, lz = mods
    got, prof, _ = _prof(_lib, lambda: lz.DecompressBatch(streams))
    assert len(got) == len(streams)
    for i, (s, g) in enumerate(zip(streams, got)):
        assert g == _want(oracle, s), (i, len(s))
        assert g == _single(lz, s), (i, len(s))
    return prof


def _dev(mods, oracle, streams):
    """the device form: streams back to back at 16-byte offsets of one allocation, every output of exactly its result's size between guard
    bytes (test_gpu_batch_dev._run_slots checks them) -> prof"""
    _lib, lz = mods
    want = [_want(oracle, s) for s in streams]
    got, prof, _ = _run_slots(_lib, DEC, streams, [len(x) for x in want])
    for i, (g, x) in enumerate(zip(got, want)):
        assert g == x, (i, len(streams[i]))
    return prof


def _both(mods, oracle, streams, only=True):
    profs = [_host(mods, oracle, streams), _dev(mods, oracle, streams)]
    for prof in profs:
        if only:
            assert prof == ONLY, prof
    return profs


def tok(ptr, length, digits=0):
    return b"<%0*d,%0*d>" % (digits, ptr, digits, length)


def lit(seed, n):
    """n literal bytes of text: no '<', no 5C, no FF"""
    return _text(seed, n)


# ---------------------------------------------------------------- 1: the class runs, and only it
@pytest.mark.parametrize("window", [1, 255, 4096])
def test_the_class_runs_and_only_it(mods, oracle, window):
    _lib, lz = mods
    assert lz.TILE_DEC_GROUP_MIN >= 2 and lz.MID_IN_MAX + 1 == 65537
    streams = [_enc(oracle, _text(5001 + i, n), window) for i, n in enumerate((65537, 66000, 34 * P + 1, 70000))]
    streams = _pad(lz, oracle, streams)
    _both(mods, oracle, streams)                                              # fails on a build without the class: no such launch
    few = _pad(lz, oracle, streams[:4], short=1)
    assert sum(1 for s in few if _candidate(lz, s)) == lz.TILE_DEC_GROUP_MIN - 1
    for prof in _both(mods, oracle, few, only=False):
        assert not any(k in prof for k in NEW), prof


# ---------------------------------------------------------------- 2: short streams that expand past the mid class
def test_short_streams_that_expand_past_the_mid_class(mods, oracle):
    _lib, lz = mods
    def phrases(seed, n):                                                     # 100 phrases of 40 bytes in random order: long matches, a short stream
        rng, words = random.Random(seed), _text(seed, 4000)
        return b"".join(words[40 * k:40 * k + 40] for k in (rng.randrange(100) for _ in range(n // 40 + 1)))[:n]
    big = ([_enc(oracle, phrases(5020 + i, 128 * 1024 - 7 * i)) for i in range(4)] * lz.MID_GROUP_MIN)[:max(16, lz.TILE_DEC_GROUP_MIN)]
    assert 16 <= len(big) < lz.MID_GROUP_MIN and all(len(s) <= lz.MID_E_MAX for s in big)         # the mid class takes them by their length ...
    assert all(len(_want(oracle, s)) > lz.MID_E_MAX for s in big)             # ... and hands them back by their output
    small = [_enc(oracle, _text(5030 + i, 3000 + 211 * i)) for i in range(lz.MID_GROUP_MIN - len(big))]
    assert all(P < len(s) for s in small)
    streams = [s for pair in zip(big, small) for s in pair] + small[len(big):] + big[len(small):]
    assert len(streams) == lz.MID_GROUP_MIN
    for prof in _both(mods, oracle, streams, only=False):
        assert prof.get(MID) == 1 and all(prof.get(k) == 1 for k in NEW), prof
        assert set(prof) <= set(ONLY) | {MID}, prof                            # no kernel of a single call


# ---------------------------------------------------------------- 3: tokens across every stream cut
def test_tokens_across_every_stream_cut(mods, oracle):
    _lib, lz = mods
    streams = []
    for k in range(1, 23):
        for digits in (0, 10):
            s = bytearray(lit(5100 + k, P - k))
            s += tok(100 + k, 37 + k, digits) + b">,42>"                      # the '<' at 2048 - k; a literal '>', ',' and digits right behind the token
            s += lit(5200 + k, 2 * P - k - len(s))
            s += tok(2 * P - 300 - k, 512 + k, digits) + b",>7"               # the '<' at 4096 - k
            s += lit(5300 + k, 700)
            assert s[P - k] == 0x3C and s[2 * P - k] == 0x3C and s.count(b"<") == 2
            streams.append(bytes(s))
    assert any(len(tok(100 + k, 37 + k, 10)) == 23 for k in range(1, 23))
    # a literal '>', ',' and digits as the first bytes behind a cut, the token in front of them ending exactly at the cut
    for tail in (b">", b",", b"0123456789", b">,9<5,2>"):
        t = tok(999, 888)
        streams.append(lit(5400, P - len(t)) + t + tail + lit(5401, 900))
    _both(mods, oracle, _pad(lz, oracle, streams))


# ---------------------------------------------------------------- 4: output-tile edges and chain depth
def test_output_tile_edges_and_chain_depth(mods, oracle):
    _lib, lz = mods
    streams = [lit(5500, P) + tok(P, P) * 40 + lit(5501, 100),                # every output tile depends on the one before
               b"x" + tok(1, 1) * 3000 + lit(5502, 50),                       # chain depth 2047 inside a tile, and across a cut
               lit(5503, 3000) + tok(3000, 3000) + tok(6000, 6000) + lit(5504, 10)]   # a pointer equal to the whole data so far
    for d in (1, 2047, 2048, 4096, 70000):
        m = (d + 10 + P - 1) // P + 1
        pre = lit(5510 + d % 97, m * P - 10)                                  # the copy's destination begins ten bytes in front of an output cut
        body = tok(d, 20) if d >= 20 else tok(d, d) * (20 // d)
        streams.append(pre + body + lit(5520, 30))
    want = [_want(oracle, s) for s in streams]
    assert len(want[0]) == 41 * P + 100 and want[1][:3001] == b"x" * 3001 and len(want[2]) == 12010
    _both(mods, oracle, _pad(lz, oracle, streams))


# ---------------------------------------------------------------- 5: zero-length tokens
def test_zero_length_tokens(mods, oracle):
    _lib, lz = mods
    a = lit(5600, 3000)
    streams = [a[:1000] + tok(5, 0) + a[1000:2040] + tok(1, 0) + tok(2040, 0) + a[2040:],          # single ones, one across the cut
               a[:500] + tok(5, 0) * 500 + a[500:1500],                                             # a run longer than a stream tile
               a[:P] + tok(5, 0) * 900 + a[P:],                                                     # ... that covers whole stream tiles
               a[:10] + tok(5, 0, 10) * 200 + a[10:20] + tok(3, 3) + tok(0, 0) * 300 + a[20:400]]
    assert _want(oracle, streams[0]) == a and _want(oracle, streams[1]) == a[:1500] and _want(oracle, streams[2]) == a
    _both(mods, oracle, _pad(lz, oracle, streams))


# ---------------------------------------------------------------- 6: escapes
def test_escapes(mods, oracle):
    _lib, lz = mods
    streams = []
    for i, trio in enumerate((b"<\\\xff", b"\\<\\", b"\xff\xff<", b"\\\\\\", b"<<<")):
        d = bytearray(_text(5700 + i, 9000))
        d[2047:2050] = trio                                                   # '<', 5C and FF at 2047, 2048 and 2049 of the output
        d[4000:4003] = trio
        s = _enc(oracle, bytes(d))
        assert len(s) > P and _want(oracle, s) == bytes(d)
        streams.append(s)
    # hand-written, literals only: the escaped image is the stream itself, so the cuts of the output are known
    for run in (1, 2, 3, 4, 7, 8):
        streams.append(b"a" * (P - run) + b"\\" * run + b"bc" + lit(5710, 600))               # a 5C run that ends at the cut
        streams.append(b"a" * (P - run + 1) + b"\\" * run + b"\xffc" + lit(5711, 600))         # ... and one that straddles it
        streams.append(b"a" * (P - 1) + b"\\" * run + b"\\c"[run % 2:] + lit(5712, 600))       # begins on the cut's last byte
    for run in (2 * P + 404, 2 * P + 405):
        streams.append(b"ab" + b"\\" * run + b"\xffcd" + lit(5713, 300))                      # a 5C run longer than two tiles
    streams.append(b"\xff" * 3 + lit(5714, P - 5) + b"\xff\xff\xff" + b"\\\xff" + lit(5715, 500))   # FF -> '<' on the way out
    want = [_want(oracle, s) for s in streams]
    assert want[-1].startswith(b"<<<") and b"<<<\xff" in want[-1]
    _both(mods, oracle, _pad(lz, oracle, streams))


# ---------------------------------------------------------------- 7: the limits
def _raises(fn):
    from raisin_amd import _lib
    try:
        fn()
    except _lib.RsnError as e:
        return e.code
    return OK


def test_the_limits(mods, oracle):
    _lib, lz = mods
    top_e, top_n = lz.TILE_DEC_OUT_MAX, lz.TILE_DEC_IN_MAX
    assert top_e % P == 0
    exact = lit(5800, P) + tok(P, P) * (top_e // P - 1)                       # E = OUT_MAX exactly: taken
    over = exact + b"z"                                                       # E = OUT_MAX + 1: handed back
    longest = lit(5801, top_n)                                                # a stream of IN_MAX bytes: taken
    beyond = lit(5802, top_n + 1)                                             # IN_MAX + 1 bytes: no candidate
    assert len(_want(oracle, exact)) == top_e and len(_want(oracle, over)) == top_e + 1 and _want(oracle, longest) == longest
    pads = _pad(lz, oracle, [])
    profs = _both(mods, oracle, [exact, longest] + pads)
    for s in (over, beyond):                                                  # the single call's bytes, the other members still the class's
        for prof in _both(mods, oracle, pads[:3] + [s] + pads[3:], only=False):
            assert all(prof.get(k) == 1 for k in NEW) and set(prof) - set(ONLY), prof
    # ---- what the single call refuses: its error code, whatever the form, and the class has run for the others
    body = lit(5803, 3 * P)
    bad = {"a malformed token in the last tile": body + b"<12,>" + lit(5804, 40),
           "len > ptr": body[:P + 5] + tok(3, 5) + body[P + 5:],
           "a pointer before the data as a tile's first item": body[:P] + tok(3000, 1) + body[P:],
           "nothing but zero-length tokens": tok(0, 0) * 500}
    for what, s in bad.items():
        assert _candidate(lz, s), what
        code = _raises(lambda: lz.Decompress(s))
        streams = pads[:5] + [s] + pads[5:]
        if code == OK:                                                        # (the single call answers it: the same bytes then)
            for prof in _both(mods, oracle, streams, only=False):
                assert all(prof.get(k) == 1 for k in NEW), (what, prof)
            continue
        got, prof, _ = _prof(_lib, lambda: _raises(lambda: lz.DecompressBatch(streams)))
        assert got == code and all(prof.get(k) == 1 for k in NEW), (what, got, code, prof)
        pack = Pack(streams)
        import torch
        outs = [torch.empty(len(_want(oracle, p)) if p is not s else 4 * P, dtype=torch.uint8, device="cuda") for p in streams]
        members = [(pack.ptr(i), len(p), outs[i].data_ptr(), outs[i].numel()) for i, p in enumerate(streams)]
        (rc, _, msg), prof, _ = _prof(_lib, lambda: _batch(_lib, DEC, members))
        assert rc == code and msg.startswith("member 5: "), (what, rc, code, msg)
        assert all(prof.get(k) == 1 for k in NEW), (what, prof)
    assert profs


# ---------------------------------------------------------------- 8: scratch independence
def test_results_do_not_depend_on_what_earlier_calls_left(mods, oracle):
    _lib, lz = mods
    A = _pad(lz, oracle, [lit(5900, P) + tok(P, P) * 30, _enc(oracle, _text(5901, 100000)), b"x" + tok(1, 1) * 2500])
    B = _pad(lz, oracle, [_enc(oracle, _text(5902, 131072)), lit(5903, 5000) + tok(5000, 4000) * 20, lit(5904, 2100)] * 3)
    first = lz.DecompressBatch(A)
    _both(mods, oracle, B)
    again, prof, _ = _prof(_lib, lambda: lz.DecompressBatch(A))
    assert again == first == [_want(oracle, s) for s in A] and prof == ONLY


# ---------------------------------------------------------------- 9: the device form
def test_device_form_capacities(mods, oracle):
    _lib, lz = mods
    streams = _pad(lz, oracle, [_enc(oracle, _text(6000 + i, n)) for i, n in enumerate((65537, 34 * P - 1, 70001, 100003))] + [lit(6010, P) + tok(P, 1000) * 7])
    want = [_want(oracle, s) for s in streams]
    assert len({len(w) % 16 for w in want}) >= 4
    rc, lens, msg, outs = _fenced_call(_lib, DEC, streams, [len(w) for w in want])      # exact to the byte, between fences
    assert rc == OK, msg
    assert lens == [len(w) for w in want] and [_out_bytes(o, k) for o, k in zip(outs, lens)] == want
    # one byte short: the lowest such member is named with its exact need, out_lens is the capacity rsn.h documents for a member that does
    # not fit, every other member complete, the fences untouched -- and with those capacities the call succeeds (as lzss_tile.hip's class)
    tight = (1, 2, 4)
    caps = [len(w) - 1 if i in tight else len(w) for i, w in enumerate(want)]
    rc, lens, msg, outs = _fenced_call(_lib, DEC, streams, caps)
    assert rc == E_CAP and msg.startswith("member 1: lzss: output needs %d bytes, buffer holds %d" % (len(want[1]), len(want[1]) - 1)), msg
    for i, w in enumerate(want):
        if i in tight:
            assert lens[i] == _ru16(len(w)) + 16, (i, lens[i], len(w))
        else:
            assert lens[i] == len(w) and _out_bytes(outs[i], lens[i]) == w, i
    rc, lens2, msg, outs = _fenced_call(_lib, DEC, streams, [lens[i] if i in tight else caps[i] for i in range(len(want))])
    assert rc == OK, msg
    assert lens2 == [len(w) for w in want] and [_out_bytes(o, k) for o, k in zip(outs, lens2)] == want
    assert _dev(mods, oracle, streams) == ONLY
    pack = Pack(streams)
    got = lz.decompress_tensors([pack.t[o:o + n] for o, n in zip(pack.offs, pack.lens)])
    assert [bytes(t.cpu().numpy()) for t in got] == want


# ---------------------------------------------------------------- 10: layered
GROUPED = ("huff_batch_", "lzss_batch_", "group_", "huff_dev_", "members_move")


def test_layered(mods, oracle):
    _lib, lz = mods
    from raisin_amd import layers
    names = ["lzss", "huffman"]
    # the tiled HUFFMAN decoder hands back the LZSS stream of seed 6111: the model of its lane maps (tests/lane_maps.py) loses tile 10 to a
    # fifth start at lane 1 and takes the other fifteen -- so the members are those fifteen texts, repeated to the class's minimum, and
    # the check in front says that the kernels take them too: what the decode profile then shows of a single call would be the LZSS step's
    import lane_limit_cases as C
    from raisin_amd import huffman
    verdicts = {seed: C.verdict(C.layered_member(seed), "tiled") for seed in C.LAYERED_SEEDS}
    assert verdicts == {seed: (False, "phases") if seed == C.LAYERED_BACK else (True, None) for seed in range(6100, 6116)} and C.LAYERED_BACK == 6111
    distinct = [_text(seed, 200000) for seed in C.LAYERED_SEEDS if verdicts[seed][0]]
    members = (distinct * 3)[:max(16, lz.TILE_DEC_GROUP_MIN)]
    assert len(distinct) == 15 and len(members) >= lz.TILE_DEC_GROUP_MIN
    streams = layers.CompressBatch(members, names)
    assert streams[:15] == [C.enc(C.layered_member(seed)) for seed in C.LAYERED_SEEDS if verdicts[seed][0]]    # the streams the model judged
    _, prof, _ = _prof(_lib, lambda: huffman.DecompressBatch(streams))
    assert not [k for k in prof if not k.startswith(GROUPED)], sorted(prof)
    got, prof, _ = _prof(_lib, lambda: layers.DecompressBatch(streams, names))
    assert got == members
    assert all(prof.get(k) == 1 for k in NEW) and not [k for k in prof if not k.startswith(GROUPED)], sorted(prof)
    pack = Pack(streams)
    srcs = [pack.t[o:o + n] for o, n in zip(pack.offs, pack.lens)]
    got, prof, _ = _prof(_lib, lambda: [bytes(t.cpu().numpy()) for t in layers.decompress_tensors(srcs, names)])
    assert got == members
    assert all(prof.get(k) == 1 for k in NEW) and not [k for k in prof if not k.startswith(GROUPED)], sorted(prof)

    def row(r):
        return (r.original_n, r.compressed_n, r.decompressed_n, r.first_difference, r.lossless, r.hist_original, r.hist_decompressed)
    ones = [row(layers.RoundTripBatch([d], names)[0]) for d in members[:3]]
    res, prof, _ = _prof(_lib, lambda: layers.RoundTripBatch(members, names))
    assert [row(r) for r in res[:3]] == ones and all(r.lossless and r.compressed_n == len(s) for r, s in zip(res, streams))
    assert all(prof.get(k) == 1 for k in NEW), prof
    lists = [names, ["lzss"]]
    rows, best, errors = layers.SuiteBatch(members, lists)
    assert errors == [None, None] and [row(r) for r in rows[0]] == [row(r) for r in res]
    one_rows, _, one_errors = layers.SuiteBatch(members[:1], lists)
    assert one_errors == [None, None] and [row(rows[l][0]) for l in range(2)] == [row(one_rows[l][0]) for l in range(2)]


# ---------------------------------------------------------------- 11: seeded fuzz
def _fuzz_stream(rng, alphabet, n, e_lo, e_hi):
    """-> (a valid stream of about n bytes, random literals and random valid tokens; the escaped bytes it expands to, e_lo to e_hi)"""
    s, e = bytearray(), 0
    share = max(4.0, (e_lo + (e_hi - e_lo) * rng.random()) / n * 4)          # output bytes a token aims at
    while len(s) < n:
        if e and rng.random() < 0.3:
            ptr = min(e, rng.choice((1, 2, rng.randint(1, 300), rng.randint(1, e), e)))
            length = min(ptr, rng.choice((0, 1, rng.randint(0, int(share)), rng.randint(0, int(4 * share)))), max(0, e_hi - 64 - e - (n - len(s))))
            s += tok(ptr, length, rng.choice((0, 0, 0, rng.randint(1, 10))))
            e += length
        else:
            k = rng.randint(1, 12)
            s += bytes(rng.choices(alphabet, k=k))
            e += k
    while e < e_lo:                                                           # copies of up to the whole data so far, until it is long enough
        length = min(e, e_lo - e + rng.randint(0, 1000))
        s += tok(rng.randint(length, e), length)
        e += length
    assert e_lo <= e <= e_hi, (n, e, e_lo, e_hi)
    return bytes(s), e


def test_seeded_fuzz(mods, oracle):
    _lib, lz = mods
    rng = random.Random(2027)
    alphabets = [b"ab", b"ACGT", b"0123456789abcdef", bytes(b for b in range(256) if b != 0x3C)]   # test_gpu_lzss_mid.py's, without '<': it begins a token
    streams, escaped = [], []
    for i in range(200):
        n = rng.randint(P + 1, 40000)
        if i % 2:                                                             # half of them expand beyond what the mid class holds: the tiled class's
            st, e = _fuzz_stream(rng, alphabets[i % 4], n, lz.MID_E_MAX + 2000, lz.TILE_DEC_OUT_MAX - 2000)
        else:
            st, e = _fuzz_stream(rng, alphabets[i % 4], n, n, lz.MID_E_MAX - 2000)
        streams.append(st)
        escaped.append(e)
    assert all(P < len(s) <= 40000 + 128 for s in streams)
    # every stream is valid and expands to at most OUT_MAX escaped bytes: the oracle decodes it, to no more bytes than that
    assert all(len(_want(oracle, s)) <= e <= lz.TILE_DEC_OUT_MAX for s, e in zip(streams, escaped))
    assert sum(1 for e in escaped if e > lz.MID_E_MAX) == 100 >= lz.TILE_DEC_GROUP_MIN
    for prof in _both(mods, oracle, streams, only=False):
        assert set(prof) <= set(ONLY) | {MID}, prof                            # the class may hand back none: no kernel of a single call
        assert all(prof.get(k, 0) >= 1 for k in NEW), prof
