"""GPU: the mid-size class of the Huffman batch calls (csrc/huff_mid.hip) -- chunks above 16 KiB and up to huffman.MID_IN_MAX,
and streams beyond what one workgroup of huff_batch_dec holds (16 KiB of payload, 32 KiB of output) up to huffman.MID_PAY_MAX /
MID_OUT_MAX, go many to ONE launch of k_huff_mid_enc / k_huff_mid_dec, a workgroup each.  Every result is compared with the CPU oracle
AND with the library's single call; what the kernels hand back (runes, one distinct byte, more than four phases, malformed streams) must
come out of the single call with the same bytes or the same error.

One place where a list is narrower than "every stream": text of 17 KiB codes to about 9 KiB of payload and 17 KiB of output, which is the
small decoder's (huff_batch_dec), whatever wrote it -- no byte alphabet reaches 16 KiB of payload from 17 KiB.  So the one-launch and the
closure tests assert `{"huff_batch_mid_dec": groups}` for the streams of the mid class (payload above 16 KiB, or output above 32 KiB) and
the two grouped kernels, no single call, for the whole list.  The closure test's list holds the code shapes in shuffled order only: built in
sorted order they are runs of one codeword, periodic data that the decoder hands back where a lane is offered a fifth start.  Which of
those and of test_periodic_data's members it hands back is the verdict of the CPU model of the lane maps (tests/lane_maps.py;
tests/lane_limit_cases.py: EITHER_WANT pins it), and _held_to_the_model holds the kernels to it: of the sorted shapes the seventh, of
the periodic members none."""
import ctypes
import os
import random
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUP_BYTES, GROUP_MEMBERS = 16 << 20, 4096           # codecs.h: SMALL_GROUP_BYTES, SMALL_GROUP_MAX
HDR_MAX, DEC_ENTRY = 1100, 608                        # huff_small_body.h: HDR_MAX, sizeof(SmallDecArgs)


def _vocab(seed, k=300):
    rng = random.Random(seed)
    return [bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(rng.randint(2, 10))) for _ in range(k)]


VOCAB = _vocab(1)


def _text(seed, n):
    rng = random.Random(seed)
    t = bytearray()
    while len(t) < n:
        t += rng.choice(VOCAB) + rng.choice([b" ", b" ", b" ", b"\n", b", ", b". "])
    return bytes(t[:n])


def _alpha(seed, n, alphabet):
    a = np.frombuffer(bytes(alphabet), dtype=np.uint8)
    return a[np.random.default_rng(seed).integers(0, len(a), size=n)].tobytes()


def _with_counts(seed, table, shuffled):
    a = np.concatenate([np.full(c, b, dtype=np.uint8) for b, c in sorted(table.items())])
    if shuffled:
        np.random.default_rng(seed).shuffle(a)
    return a.tobytes()


def _payload(stream):
    return len(stream) - stream.index(b"\\\n") - 3


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman
    return _lib, huffman


@pytest.fixture(scope="module")
def K(mods):
    return max(mods[1].MID_GROUP_MIN, 8)


def _prof(_lib, fn):
    _lib.prof_enable(True)
    _lib.prof_reset()
    try:
        res = fn()
        return res, {k: v[0] for k, v in _lib.prof_get().items() if v[0]}
    finally:
        _lib.prof_enable(False)


def _pad(members, K, seed=900):
    """at least K members of the class: text of 20 KiB behind the ones the test is about"""
    return list(members) + [_text(seed + i, 20000 + 100 * i) for i in range(max(0, K - len(members)))]


def _mid_stream(huffman, s, out_len):
    """is the stream the mid decoder's: beyond one workgroup of huff_batch_dec, within the mid limits"""
    p = _payload(s)
    return (p > huffman.BATCH_GROUP_PAYLOAD_MAX or out_len > huffman.BATCH_GROUP_OUTPUT_MAX) and p <= huffman.MID_PAY_MAX and out_len <= huffman.MID_OUT_MAX


def _groups(needs):
    """how many launches the packing makes (codecs.h: a group's staging is at most SMALL_GROUP_BYTES, SMALL_GROUP_MAX members)"""
    groups, members, used = 0, 0, 0
    for need in needs:
        if members and (members == GROUP_MEMBERS or used + need > GROUP_BYTES):
            groups, members, used = groups + 1, 0, 0
        members, used = members + 1, used + need
    return groups + (1 if members else 0)


def _up(n):
    return (n + 15) // 16 * 16


def _enc_groups(members):
    return _groups(16 + _up(len(d)) + 16 + _up(HDR_MAX + (7 * len(d) + 7) // 8 + 3) + 16 for d in members)


def _dec_groups(pairs):
    """pairs: (stream, decoded length)"""
    def need(s, out_len):
        a0 = (s.index(b"\\\n") + 3) & ~3
        return DEC_ENTRY + _up(len(s) - a0) + 64 + _up(out_len) + 16 + 16
    return _groups(need(s, n) for s, n in pairs)


PRODUCED = []                                          # (member, stream): what the encoder tests produced on the mid path


def _check_compress(mods, oracle, members, record=True):
    """the batch's bytes against the oracle and the single call; returns (streams, prof)"""
    _lib, huffman = mods
    got, prof = _prof(_lib, lambda: huffman.CompressBatch(members))
    assert len(got) == len(members)
    for d, g in zip(members, got):
        assert g == oracle.huffman_compress(d), (len(d), d[:32])
        assert g == huffman.Compress(d), (len(d), d[:32])
        if record and huffman.BATCH_COMPRESS_INPUT_MAX < len(d) <= huffman.MID_IN_MAX and max(d) < 0x80 and len(set(d)) > 1:
            PRODUCED.append((d, g))
    return got, prof


def _check_decompress(mods, oracle, streams, members):
    _lib, huffman = mods
    dec, prof = _prof(_lib, lambda: huffman.DecompressBatch(streams))
    assert dec == list(members)
    for s, d in zip(streams, dec):
        assert d == huffman.Decompress(s) == oracle.huffman_decompress(s), len(s)
    return prof


def _held_to_the_model(mods, oracle, names, members, pads):
    """The device form over the members' streams, out_cap exactly the result size wherever the model of the lane maps takes the member
    and the single call's figure where it hands it back: the single call's decoder runs if and only if the model hands a member back,
    and not at all on the members it takes, run on their own.  names: the members' keys in lane_limit_cases.EITHER_WANT."""
    import lane_limit_cases as C
    from test_gpu_batch_dev import _ru16
    from test_gpu_huffman_batch_dev import DEC, _run_slots
    _lib, huffman = mods
    _lib.check(_lib.lib().rsn_device_set(0))
    verdicts = [(C.class_of(d),) + C.verdict(d, C.class_of(d)) for d in members]
    assert verdicts == [C.EITHER_WANT[k] for k in names], verdicts
    assert all(C.verdict(d, C.class_of(d)) == (True, None) for d in pads)
    taken = [v[1] for v in verdicts] + [True] * len(pads)
    lists = [(list(members) + list(pads), taken)]
    if not all(taken):
        lists.append(([d for d, t in zip(list(members) + list(pads), taken) if t], [True] * sum(taken)))
    for lst, took in lists:
        caps = [len(d) if t else _ru16(len(d)) + 16 for d, t in zip(lst, took)]
        got, prof, _ = _run_slots(_lib, DEC, [oracle.huffman_compress(d) for d in lst], caps, loose=[i for i, t in enumerate(took) if not t])
        assert got == lst
        general = {k for k in prof if k.startswith("huff_dec_") or k == "huff_small_dec"}
        assert prof.get("huff_batch_mid_dec") == 1 and bool(general) == (not all(took)), prof
    return taken


# ---------------------------------------------------------------- 1: sizes
def test_sizes(mods, oracle, K):
    _, huffman = mods
    sizes = [16383, 16384, 16385, 20000, 32767, 32768, 32769, 65535, 65536, 65537]
    members = _pad([_text(10 + i, n) for i, n in enumerate(sizes)], K + 3)   # (K of the class beside the three that are not)
    _, prof = _check_compress(mods, oracle, members)
    assert prof.get("huff_batch_mid_enc") == 1, prof
    assert set(prof) != {"huff_batch_mid_enc"}, prof                         # 65537 is not taken, up to 16384 is the small kernel's
    assert prof.get("huff_batch_enc") == 1, prof
    inside = [m for m in members if huffman.BATCH_COMPRESS_INPUT_MAX < len(m) <= huffman.MID_IN_MAX]
    assert len(inside) == len(members) - 3
    _, prof = _check_compress(mods, oracle, inside, record=False)
    assert prof == {"huff_batch_mid_enc": 1}, prof


# ---------------------------------------------------------------- 2: code shapes
def _fib_table():
    fib, f0, f1 = {}, 1, 1
    for k in range(22):                                                       # 1, 1, 2, 3, 5, ... 17711: 46367 bytes, the deepest codes
        fib[48 + k] = f0
        f0, f1 = f1, f0 + f1
    return fib


def _shape_tables():
    return [
        {b: 500 for b in range(128)},                                         # the flat 7-bit code, 64000 bytes
        {0: 1, 127: 65535},
        {65: 32768, 66: 32768},
        _fib_table(),
        {0x41: 5000, 0x42: 5000, 0x5C: 9000},                                 # '\\' the highest byte: its entry goes first
        {0x0A: 12000, 0x5C: 12000},
        {b: 60 * (3 + (b % 3)) for b in range(10, 100)},                      # many duplicate counts, newline among them
    ]


def test_code_shapes(mods, oracle, K):
    _, huffman = mods
    fib = _fib_table()
    assert sum(fib.values()) == 46367
    codes, _ = huffman.plan(fib)                                              # (the host's Go-exact tree: no device)
    assert max(l for _, _, l in codes) in (21, 22)
    assert max(l for _, _, _, l in oracle.huffman_table(_with_counts(0, fib, False))) in (21, 22)
    members = []
    for k, t in enumerate(_shape_tables()):
        members += [_with_counts(k, t, True), _with_counts(k, t, False)]
    assert all(huffman.BATCH_COMPRESS_INPUT_MAX < len(m) <= huffman.MID_IN_MAX for m in members)
    members = _pad(members, K)
    got, prof = _check_compress(mods, oracle, members, record=False)
    assert prof == {"huff_batch_mid_enc": 1}, prof
    # the closure test takes the shuffled ones: in sorted order a member is a few runs of one codeword thousands of symbols long, periodic
    # data with as many phases as the codeword has bits, of which the decoder hands back the seventh (below: the model's verdicts)
    PRODUCED.extend((d, g) for d, g in list(zip(members, got))[0:2 * len(_shape_tables()):2])
    # (the shapes of 19 to 24 KB are the small decoder's; K text streams of the mid class beside them, so that the class is grouped)
    more = [_text(100 + i, 40000) for i in range(K)]
    prof = _check_decompress(mods, oracle, got + [oracle.huffman_compress(d) for d in more], members + more)
    assert prof.get("huff_batch_mid_dec", 0) >= 1, prof
    # the sorted ones against the model of the lane maps: the runs of one codeword are taken, the seventh table's 90 runs are not
    n = len(_shape_tables())
    taken = _held_to_the_model(mods, oracle, ["mid: sorted shape %d" % k for k in range(n)], members[1:2 * n:2], more)
    assert taken[:n] == [True] * (n - 1) + [False]


# ---------------------------------------------------------------- 3: hand-backs
def test_hand_backs(mods, oracle, K):
    _, huffman = mods
    t = _text(40, 30000)
    back = [t[:12345] + "é".encode() + t[12345:], b"q" * 40000, _text(41, 16383), _text(42, 16384), _text(43, 65537)]
    members = _pad(back, K + len(back))
    got, prof = _check_compress(mods, oracle, members)
    assert prof.get("huff_batch_mid_enc") == 1 and len(prof) > 1, prof
    pad = members[len(back):]
    assert got[len(back):] == [oracle.huffman_compress(d) for d in pad]
    dec = huffman.DecompressBatch(got)                                        # (one distinct byte does not round-trip in the reference either)
    assert dec == [huffman.Decompress(s) for s in got] == [oracle.huffman_decompress(s) for s in got]
    assert [d for d, m in zip(dec, members) if len(set(m)) > 1] == [m for m in members if len(set(m)) > 1]


# ---------------------------------------------------------------- 4: one launch each way, no hand-back
def test_one_launch_each_way(mods, oracle):
    _lib, huffman = mods
    k = max(64, huffman.MID_GROUP_MIN)
    mid = [_text(200 + i, 17 * 1024 + (i * 761) % (47 * 1024 + 1)) for i in range(k)]
    mid[0], mid[1] = _text(200, 17 * 1024), _text(201, 64 * 1024)
    assert min(map(len, mid)) == 17 * 1024 and max(map(len, mid)) == 64 * 1024
    comp, prof = _check_compress(mods, oracle, mid)
    assert prof == {"huff_batch_mid_enc": _enc_groups(mid)}, prof
    above = [(s, len(d)) for s, d in zip(comp, mid) if _payload(s) > huffman.BATCH_GROUP_PAYLOAD_MAX]
    assert len(above) >= huffman.MID_GROUP_MIN and all(_payload(s) > 16384 for s, _ in above)
    dec, prof = _prof(_lib, lambda: huffman.DecompressBatch([s for s, _ in above]))
    assert prof == {"huff_batch_mid_dec": _dec_groups(above)}, prof
    assert dec == [oracle.huffman_decompress(s) for s, _ in above] == [huffman.Decompress(s) for s, _ in above]
    # the whole list: the streams of the class in the mid kernel, the shorter ones in the small kernel, no single call
    cls = [(s, len(d)) for s, d in zip(comp, mid) if _mid_stream(huffman, s, len(d))]
    dec, prof = _prof(_lib, lambda: huffman.DecompressBatch(comp))
    want = {"huff_batch_mid_dec": _dec_groups(cls)}
    if len(cls) < len(comp):
        want["huff_batch_dec"] = 1
    assert prof == want, prof
    assert dec == mid
    # small and mid members interleaved
    small = [_text(300 + i, 20 + (i * 37) % 16000) for i in range(k)]
    mixed = [x for pair in zip(small, mid) for x in pair]
    got, prof = _prof(_lib, lambda: huffman.CompressBatch(mixed))
    assert prof == {"huff_batch_enc": 1, "huff_batch_mid_enc": _enc_groups(mid)}, prof
    assert got == [oracle.huffman_compress(d) for d in mixed]
    # small members alone: the new kernels are not launched
    _, prof = _prof(_lib, lambda: huffman.DecompressBatch(huffman.CompressBatch(small)))
    assert prof and not [x for x in prof if "mid" in x], prof


# ---------------------------------------------------------------- 5: periodic and phase-rich data
def test_periodic_data(mods, oracle, samiam, K):
    _, huffman = mods
    block = _alpha(50, 4096, b"abcdefghijklmnopqrstuvwxyz ,.\n")
    per = [(samiam * (n // len(samiam) + 1))[:n] for n in (20000, 40000, 65536)] + [b"ab" * 16000, block * 12, block * 16]
    members = _pad(per, K)
    got, _ = _check_compress(mods, oracle, members, record=False)
    _check_decompress(mods, oracle, got, members)
    # two or three phases, never a fifth start: the model of the lane maps takes all six, and so do the kernels
    assert all(_held_to_the_model(mods, oracle, ["mid: periodic %d" % i for i in range(len(per))], per, [_text(960 + i, 40000) for i in range(4)]))


# ---------------------------------------------------------------- 6: the decoder's cutoffs from the host plan
def test_decoder_cutoffs(mods, oracle, K):
    _lib, huffman = mods
    two = _alpha(60, 65537, b"xy")
    s = oracle.huffman_compress(two[:65536])
    assert _payload(s) == 8192
    dec, prof = _prof(_lib, lambda: huffman.DecompressBatch([s] * K))
    assert prof == {"huff_batch_mid_dec": 1}, prof                            # 64 KiB out: beyond huff_batch_dec, the mid decoder's
    assert dec == [two[:65536]] * K == [huffman.Decompress(s)] * K
    s = oracle.huffman_compress(two)
    dec, prof = _prof(_lib, lambda: huffman.DecompressBatch([s] * K))
    assert prof and "huff_batch_dec" not in prof and "huff_batch_mid_dec" not in prof, prof
    assert dec == [two] * K == [huffman.Decompress(s)] * K
    # the payload limit: 128 symbols, near 7 bits each
    src = _alpha(61, 70000, bytes(range(128)))
    lo, hi = 1000, len(src)                                                   # the longest prefix whose payload is <= the limit
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if _payload(oracle.huffman_compress(src[:mid])) <= huffman.MID_PAY_MAX:
            lo = mid
        else:
            hi = mid - 1
    lo = min(lo, huffman.MID_OUT_MAX)                                         # (whichever bound refuses first)
    inside, outside = oracle.huffman_compress(src[:lo]), oracle.huffman_compress(src[:lo + 1])
    assert _payload(inside) <= huffman.MID_PAY_MAX and lo <= huffman.MID_OUT_MAX
    assert _payload(inside) == huffman.MID_PAY_MAX or lo == huffman.MID_OUT_MAX
    assert _payload(outside) > huffman.MID_PAY_MAX or lo + 1 > huffman.MID_OUT_MAX
    dec, prof = _prof(_lib, lambda: huffman.DecompressBatch([inside] * K))
    assert prof == {"huff_batch_mid_dec": 1}, prof
    assert dec == [src[:lo]] * K == [huffman.Decompress(inside)] * K
    dec, prof = _prof(_lib, lambda: huffman.DecompressBatch([outside] * K))
    assert prof and "huff_batch_dec" not in prof and "huff_batch_mid_dec" not in prof, prof
    assert dec == [src[:lo + 1]] * K == [huffman.Decompress(outside)] * K


# ---------------------------------------------------------------- 7: foreign and malformed streams
def _outcome(fn):
    from raisin_amd import RsnError
    try:
        return ("ok", fn())
    except RsnError as e:
        return ("err", e.code, str(e))


BAD_TINY = b"1|a1|b\\\n\x09\x80"                                               # the pad exceeds the payload


def _foreign(oracle):
    good = oracle.huffman_compress(_text(70, 40000))
    assert _payload(good) > 16384
    sep = good.index(b"\\\n")
    bar = good.index(b"|")
    more = str(int(good[:bar]) + 1).encode() + good[bar:]                     # the first count one higher than the payload holds
    less = str(int(good[:bar]) - 1).encode() + good[bar:]
    rune = good[:sep] + b"5|" + "é".encode() + good[sep:]
    cut = good[:sep] + b"7|" + good[sep:]                                     # the header ends after a '|'
    return good, [good[:-100], good[:-1], good[:-2], good[:-3], good[:sep + 3 + 16500], more, less, rune, cut]


def test_foreign_and_malformed_streams(mods, oracle, K):
    _lib, huffman = mods
    good, foreign = _foreign(oracle)
    for s in foreign:
        assert len(s) > 16384 + HDR_MAX + 8 or _payload(s) > 16384
        single = _outcome(lambda: huffman.Decompress(s))
        batch = _outcome(lambda: huffman.DecompressBatch([s] * K))
        if single[0] == "ok":
            assert batch == ("ok", [single[1]] * K), s[:40]
        else:
            assert batch[0] == "err" and batch[1] == single[1], (s[:40], single, batch)
            msg = _lib.lib().rsn_last_error().decode()
            assert msg.startswith("member 0: ") and msg[len("member 0: "):] == single[2].split(": ", 1)[1], (msg, single)
    # the tiny malformed stream among good mid streams
    single = _outcome(lambda: huffman.Decompress(BAD_TINY))
    assert single[0] == "err"
    lst = [good] * K
    lst[K // 2] = BAD_TINY
    batch = _outcome(lambda: huffman.DecompressBatch(lst))
    assert batch[0] == "err" and batch[1] == single[1], (single, batch)
    msg = _lib.lib().rsn_last_error().decode()
    assert msg.startswith("member %d: " % (K // 2)) and msg.split(": ", 1)[1] == single[2].split(": ", 1)[1], (msg, single)


def test_a_failing_mid_member_fails_the_batch(mods, oracle, K):
    _lib, huffman = mods
    from raisin_amd import RsnError
    good, foreign = _foreign(oracle)
    bad = next(s for s in foreign if _outcome(lambda: huffman.Decompress(s))[0] == "err")
    with pytest.raises(RsnError) as single:
        huffman.Decompress(bad)
    bufs = [oracle.huffman_compress(_text(800 + i, 40000)) for i in range(max(K, 6))]
    bufs[3] = bad
    bufs[5] = BAD_TINY                                                        # a later failure does not change the answer
    k = len(bufs)
    L = _lib.lib()
    ins = (ctypes.c_char_p * k)(*bufs)
    lens = (ctypes.c_size_t * k)(*[len(b) for b in bufs])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    assert L.rsn_huffman_decompress_batch(k, ins, lens, outs, olens) == single.value.code
    assert all(not outs[i] for i in range(k)) and all(olens[i] == 0 for i in range(k))
    msg = L.rsn_last_error().decode()
    assert msg.startswith("member 3: ") and msg[len("member 3: "):] == str(single.value).split(": ", 1)[1], msg
    bufs[3] = bufs[5] = bufs[0]
    assert huffman.DecompressBatch(bufs) == [oracle.huffman_decompress(b) for b in bufs]   # the thread goes on


# ---------------------------------------------------------------- 8: below the minimum
def test_below_the_minimum_group(mods, oracle):
    _lib, huffman = mods
    k = huffman.MID_GROUP_MIN - 1
    if k < 1:
        pytest.skip("every mid member is grouped")
    members = [_text(700 + i, 40000 + 500 * i) for i in range(k)]
    comp, prof = _check_compress(mods, oracle, members, record=False)
    assert not [x for x in prof if "mid" in x], prof                          # (the pipeline's launches are its workers': not this thread's)
    assert all(_payload(s) > 16384 for s in comp)
    dec, prof = _prof(_lib, lambda: huffman.DecompressBatch(comp))
    assert prof and not [x for x in prof if "mid" in x], prof
    assert dec == [huffman.Decompress(s) for s in comp] == [oracle.huffman_decompress(s) for s in comp]


# ---------------------------------------------------------------- 9: closure
def test_the_decoder_takes_every_stream_the_encoder_writes(mods, oracle, K):
    """(after the encoder tests of this file: they leave their streams in PRODUCED)"""
    _lib, huffman = mods
    if not PRODUCED:                                                          # run on its own: one encoder list
        members = [_text(950 + i, 36000 + 1800 * i) for i in range(K)]
        for d, g in zip(members, huffman.CompressBatch(members)):
            PRODUCED.append((d, g))
    assert all(_payload(s) <= huffman.MID_PAY_MAX and len(d) <= huffman.MID_OUT_MAX for d, s in PRODUCED)
    above = [(d, s) for d, s in PRODUCED if _payload(s) > 16384]
    assert len(above) >= K
    dec, prof = _prof(_lib, lambda: huffman.DecompressBatch([s for _, s in above]))
    assert prof == {"huff_batch_mid_dec": _dec_groups([(s, len(d)) for d, s in above])}, prof
    assert dec == [d for d, _ in above]
    dec, prof = _prof(_lib, lambda: huffman.DecompressBatch([s for _, s in PRODUCED]))
    assert set(prof) <= {"huff_batch_mid_dec", "huff_batch_dec"}, prof
    assert dec == [d for d, _ in PRODUCED]


# ---------------------------------------------------------------- 10: the callers
def _files(tmp_path, stem, datas):
    paths = []
    for i, d in enumerate(datas):
        p = tmp_path / ("%s%d.txt" % (stem, i))
        p.write_bytes(d)
        paths.append(str(p))
    return paths


def test_callers_pick_the_mid_kernels_up(mods, oracle, tmp_path, capsys):
    _lib, huffman = mods
    from raisin_amd import engine, lz
    n = max(16, huffman.MID_GROUP_MIN, lz.MID_GROUP_MIN)                       # (as many files as both codecs group)
    datas = [_text(1200 + i, 40 * 1024 + (i * 1531) % (24 * 1024 + 1)) for i in range(n)]
    paths = _files(tmp_path, "f", datas)
    layers = ["lzss", "huffman"]
    capsys.readouterr()
    for p in paths:
        engine.CompressFile(layers, p, p + ".loop")
    loop_lines = capsys.readouterr().out
    _, prof = _prof(_lib, lambda: engine.CompressFiles(layers, paths, ".pyl"))
    assert capsys.readouterr().out == loop_lines
    assert prof.get("lzss_batch_mid_enc", 0) >= 1 and prof.get("huff_batch_mid_enc", 0) >= 1, prof
    comp = [p + ".pyl" for p in paths]
    for p, d in zip(paths, datas):
        assert open(p + ".pyl", "rb").read() == open(p + ".loop", "rb").read() == oracle.huffman_compress(oracle.lzss_compress(d))
    for c in comp:
        engine.DecompressFile(layers, c, c + ".loop")
    loop_lines = capsys.readouterr().out
    _, prof = _prof(_lib, lambda: engine.DecompressFiles(layers, comp, ".py"))
    assert capsys.readouterr().out == loop_lines
    assert prof.get("huff_batch_mid_dec", 0) >= 1 and prof.get("lzss_batch_mid_dec", 0) >= 1, prof
    for c, d in zip(comp, datas):
        assert open(c + ".py", "rb").read() == open(c + ".loop", "rb").read() == d
    capsys.readouterr()
    # the C++ host: its default layer list
    exe = os.path.join(ROOT, "raisin_amd", "host", "rsn")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe)])
    out = subprocess.check_output([exe, "-compress", ",".join(paths), "-outext=cl"]).decode()
    assert out.count("Compressing...") == len(datas)
    for p, d in zip(paths, datas):
        assert open(p + ".cl", "rb").read() == engine.compress(d, layers)


# ---------------------------------------------------------------- 11: two threads
def test_two_threads_run_mid_batches_at_once(mods, oracle):
    _, huffman = mods
    lists = [[_text(1300 + 100 * t + i, 36000 + 1700 * i) for i in range(max(12, huffman.MID_GROUP_MIN))] for t in range(2)]
    want = [[oracle.huffman_compress(d) for d in l] for l in lists]
    errors = []

    def work(t):
        for r in range(5):
            c = huffman.CompressBatch(lists[t])
            if c != want[t] or huffman.DecompressBatch(c) != lists[t]:
                errors.append((t, r))
    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors


# ---------------------------------------------------------------- 12: seeded fuzz
def test_seeded_fuzz(mods, oracle):
    _, huffman = mods
    rng = random.Random(2026)
    alphabets = [b"ab", b"ACGT", b"0123456789abcdef", bytes(range(128))]
    members = []
    for i in range(120):
        n = rng.randint(16385, 65536)
        if i % 5 == 4:                                                        # a Zipf draw over 96 symbols
            w = 1.0 / np.arange(1, 97)
            members.append((32 + np.random.default_rng(1000 + i).choice(96, size=n, p=w / w.sum())).astype(np.uint8).tobytes())
        else:
            members.append(_alpha(1000 + i, n, alphabets[i % 5]))
    got = huffman.CompressBatch(members)
    for d, g in zip(members, got):
        assert g == oracle.huffman_compress(d), len(d)
    for d, g in zip(members[::10], got[::10]):
        assert g == huffman.Compress(d), len(d)
    for d, g in zip(members, got):
        PRODUCED.append((d, g))
    assert huffman.DecompressBatch(got) == members
