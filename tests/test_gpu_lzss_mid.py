"""GPU: the mid-size class of the LZSS batch calls (csrc/lzss_mid.hip) -- members above the small kernels' cutoffs (1 KiB of
input, 2 KiB of stream) and up to lz.MID_IN_MAX / lz.MID_E_MAX go many to ONE launch of k_lzss_mid_enc / k_lzss_mid_dec, a workgroup
each.  Every result is compared with the CPU oracle AND with the library's single call; what the kernels hand back (runs, short
periods, streams that expand beyond the limit, malformed tokens) must come out of the single call with the same bytes or the same error.

Two places where the list of a test is narrower than "every stream": a stream of at most 2 KiB belongs to the small decoder
(lzss_batch_dec), whatever wrote it, so the one-launch and the closure tests assert `{"lzss_batch_mid_dec": groups}` for the streams
above 2 KiB and `{"lzss_batch_dec", "lzss_batch_mid_dec"}` -- the two grouped kernels, no single call -- for the whole list."""
import ctypes
import os
import random
import subprocess
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_DEC_MAX = 2048                                  # lzss_small.hip's SL_DEC_IN_MAX: streams up to here are the small decoder's
GROUP_BYTES, GROUP_MEMBERS = 16 << 20, 4096           # codecs.h: SMALL_GROUP_BYTES, SMALL_GROUP_MAX


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


def _csv(seed, n):
    rng = random.Random(seed)
    t = bytearray()
    row = 0
    while len(t) < n:
        row += 1
        t += b"%d,2024-%02d-%02d,%s,%d.%02d,%s\n" % (row, rng.randint(1, 12), rng.randint(1, 28), rng.choice([b"INFO", b"WARN", b"ERROR", b"DEBUG"]),
                                                     rng.randint(0, 99999), rng.randint(0, 99), rng.choice(VOCAB))
    return bytes(t[:n])


def _longest_run(d):
    a = np.frombuffer(d, dtype=np.uint8)
    edges = np.flatnonzero(np.diff(a) != 0)
    return int(np.diff(np.concatenate(([-1], edges, [len(a) - 1]))).max())


FILLER = _alpha(77, 1100, b"0123456789 ")             # in front of the match-rule cases: on the mid path, across tile edges


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, lz
    return _lib, lz


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
    """at least K members: text of 3 KiB behind the ones the test is about"""
    return list(members) + [_text(seed + i, 3000 + 100 * i) for i in range(max(0, K - len(members)))]


def _dec_groups(lz, streams):
    """how many launches lzss_mid.hip's packing makes of these streams (codecs.h: a group's staging is at most SMALL_GROUP_BYTES)"""
    groups, members, used = 0, 0, 0
    for s in streams:
        need = 16 + (len(s) + 15) // 16 * 16 + 32 + lz.MID_E_MAX + 16 + 16
        if members and (members == GROUP_MEMBERS or used + need > GROUP_BYTES):
            groups, members, used = groups + 1, 0, 0
        members, used = members + 1, used + need
    return groups + (1 if members else 0)


PRODUCED = []                                          # (member, window, stream): what the encoder tests produced on the mid path


def _check_compress(mods, oracle, members, window, record=True):
    """the batch's bytes against the oracle and the single call; returns (streams, prof)"""
    _lib, lz = mods
    got, prof = _prof(_lib, lambda: lz.CompressAsyncBatch(members, window))
    assert len(got) == len(members)
    for d, g in zip(members, got):
        assert g == oracle.lzss_compress(d, window), (len(d), window, d[:32])
        assert g == lz.CompressAsync(d, False, window), (len(d), window, d[:32])
        if record and 1024 < len(d) <= lz.MID_IN_MAX:
            PRODUCED.append((d, window, g))
    return got, prof


# ---------------------------------------------------------------- 1: sizes and windows
def test_sizes_and_windows(mods, oracle, K):
    _, lz = mods
    sizes = [1025, 1500, 4095, 4096, 4097, 8191, 8193, 12345, lz.MID_IN_MAX - 1, lz.MID_IN_MAX, lz.MID_IN_MAX + 1]
    members = _pad([_text(10 + i, n) for i, n in enumerate(sizes)], K + 1)   # (K of the class beside the one that is not taken)
    for window in (4096, 50, 16, 1):
        _, prof = _check_compress(mods, oracle, members, window)
        assert prof.get("lzss_batch_mid_enc") == 1, (window, prof)
        assert "lzss_batch_enc" not in prof, (window, prof)
        assert set(prof) != {"lzss_batch_mid_enc"}, (window, prof)            # the member of MID_IN_MAX + 1 bytes is not taken
    for window in (0, 8192):                                                 # not the mid kernel's windows: today's path, the same bytes
        _, prof = _check_compress(mods, oracle, members, window, record=False)
        assert "lzss_batch_mid_enc" not in prof, (window, prof)


def test_members_up_to_the_limit_alone_are_one_launch(mods, oracle, K):
    _, lz = mods
    members = _pad([_text(30, lz.MID_IN_MAX - 1), _text(31, lz.MID_IN_MAX), _text(32, 1025)], K)
    _, prof = _check_compress(mods, oracle, members, 4096, record=False)
    assert prof == {"lzss_batch_mid_enc": 1}, prof


# ---------------------------------------------------------------- 2: the match rules
def _rule_members(known):
    known = known["survey"]
    rng = random.Random(5)
    uniq = bytes(range(128, 256))                                             # (0xFF: escaped to 5C FF -- still once each)
    pat = b"The-Pattern-0123"
    period = bytes(rng.choice(b"abcdefghijklmnopqrstuvwxyz") for _ in range(700))
    out = [FILLER + known["lzss_tiebreak"][0].encode(), FILLER + b"abcabcabcabcabcabcabcabc\n"]
    out += [FILLER + pair[0].encode() for pair in known["lzss_threshold"]]
    for gap in (4095, 4096, 4097):                                            # the far occurrence at exactly the window, one inside, one outside
        mid = _alpha(gap, gap - len(pat) - 2000, b"0123456789 ")
        out.append(FILLER + pat + mid + pat + _alpha(gap + 1, 2000 - len(pat), b"0123456789 ") + pat + b"!")
    out.append(FILLER + period * 8)                                           # matches longer than a tile's step
    out.append(FILLER + b"abc" * 1500)                                        # L capped by the distance
    out.append(FILLER + b"xyzzy-tail" + _alpha(9, 900, b"0123456789 ") + b"xyzzy-tail")   # a match that ends exactly at E
    out.append(FILLER + b"-tail" + _alpha(10, 3000, b"0123456789 ") + b"-tail")
    big = bytearray(FILLER)                                                   # isolated bigrams that recur once: L = 2 decides the chain
    for i in range(0, 126, 3):
        big += uniq[i:i + 2] + FILLER[i:i + 7] + uniq[i + 2:i + 3]
    for i in range(0, 126, 3):
        big += uniq[i:i + 2] + b"#"
    out.append(bytes(big))
    return out


def test_match_rules_behind_filler(mods, oracle, known, K):
    members = _pad(_rule_members(known), K)
    assert all(len(m) > 1024 for m in members)
    for window in (4096, 64):
        _check_compress(mods, oracle, members, window)
    # the golden strings themselves, behind the filler: the filler's stream, then the golden stream with its own distances
    _, lz = mods
    got = lz.CompressAsyncBatch(members, 4096)
    tie = known["survey"]["lzss_tiebreak"]
    assert got[0].endswith(tie[1].encode()[len("abcdefg1"):]), got[0][-40:]


# ---------------------------------------------------------------- 3: escapes
def test_escapes(mods, oracle, K):
    _lib, lz = mods
    esc = [_alpha(41, 3000, b"<\\\xffab"), _alpha(42, 40000, b"<\\\xffab")]
    for window in (4096, 16):
        _, prof = _check_compress(mods, oracle, _pad(esc, K), window)
        assert prof.get("lzss_batch_mid_enc") == 1, prof
    # every byte a 5C: E = 2 * MID_IN_MAX exceeds the limit -- handed back, the same bytes
    members = _pad([b"\\" * lz.MID_IN_MAX], K)
    got, prof = _check_compress(mods, oracle, members, 4096, record=False)
    assert prof.get("lzss_batch_mid_enc") == 1 and len(prof) > 1, prof
    assert lz.DecompressBatch(got) == members


# ---------------------------------------------------------------- 4: hard inputs
def test_hard_inputs(mods, oracle, K):
    _, lz = mods
    record = bytes(random.Random(8).choice(b"abcdefghij0123456789,") for _ in range(100))
    hard = [b"q" * 20000, b"ab" * 10000, b"\x00" * 65536, record * 300]
    members = _pad(hard, K)
    got, _ = _check_compress(mods, oracle, members, 4096, record=False)       # (no RsnError: RSN_OK, whichever path served them)
    dec = lz.DecompressBatch(got)
    assert dec == members
    assert dec == [lz.Decompress(s) for s in got]


# ---------------------------------------------------------------- 5: one launch, no hand-back
def test_one_launch_no_hand_back(mods, oracle):
    _lib, lz = mods
    mid = [_text(200 + i, 4096 + (i * 97) % 4097) for i in range(max(64, lz.MID_GROUP_MIN))]   # (from 4 KiB: every stream above the small decoder's 2 KiB)
    assert min(map(len, mid)) >= 2048 and max(map(len, mid)) <= 8192
    comp, prof = _check_compress(mods, oracle, mid, 4096)
    assert prof == {"lzss_batch_mid_enc": 1}, prof
    above = [s for s in comp if len(s) > SMALL_DEC_MAX]
    assert len(above) == len(comp)
    dec, prof = _prof(_lib, lambda: lz.DecompressBatch(above))
    assert prof == {"lzss_batch_mid_dec": 1}, prof
    assert dec == [oracle.lzss_decompress(s) for s in above] == [lz.Decompress(s) for s in above]
    dec, prof = _prof(_lib, lambda: lz.DecompressBatch(comp))
    assert prof == ({"lzss_batch_mid_dec": 1, "lzss_batch_dec": 1} if len(above) < len(comp) else {"lzss_batch_mid_dec": 1}), prof
    assert dec == mid
    small = [_text(300 + i, 20 + (i * 37) % 1000) for i in range(len(mid))]
    mixed = [x for pair in zip(small, mid) for x in pair]
    got, prof = _prof(_lib, lambda: lz.CompressAsyncBatch(mixed))
    assert prof == {"lzss_batch_enc": 1, "lzss_batch_mid_enc": 1}, prof
    assert got == [oracle.lzss_compress(d) for d in mixed]
    # small members alone: the new kernels are not launched
    _, prof = _prof(_lib, lambda: lz.DecompressBatch(lz.CompressAsyncBatch(small)))
    assert not [k for k in prof if "mid" in k], prof


def test_ordinary_data_is_never_handed_back(mods, oracle):
    _lib, lz = mods
    members = []
    for i in range((max(lz.MID_GROUP_MIN, 24) + 2) // 3):
        members += [_csv(400 + i, 4500 + 1100 * i), _alpha(500 + i, 3500 + 1200 * i, b"ACGT"), _alpha(600 + i, 2800 + 1000 * i, b"0123456789abcdef")]
    assert max(map(_longest_run, members)) <= 64
    comp, prof = _check_compress(mods, oracle, members, 4096)
    assert prof == {"lzss_batch_mid_enc": 1}, prof
    assert all(len(s) > SMALL_DEC_MAX for s in comp)
    dec, prof = _prof(_lib, lambda: lz.DecompressBatch(comp))
    assert prof == {"lzss_batch_mid_dec": 1}, prof
    assert dec == members


# ---------------------------------------------------------------- 6: below the minimum
def test_below_the_minimum_group(mods, oracle):
    _lib, lz = mods
    k = lz.MID_GROUP_MIN - 1
    if k < 1:
        return
    members = [_text(700 + i, 3000 + 500 * i) for i in range(k)]
    comp, prof = _check_compress(mods, oracle, members, 4096, record=False)
    assert not [x for x in prof if "mid" in x], prof
    comp = [s for s in comp if len(s) > SMALL_DEC_MAX]
    assert comp
    dec, prof = _prof(_lib, lambda: lz.DecompressBatch(comp))
    assert not [x for x in prof if "mid" in x], prof
    assert dec == [lz.Decompress(s) for s in comp] == [oracle.lzss_decompress(s) for s in comp]


# ---------------------------------------------------------------- 7: seeded fuzz
def test_seeded_fuzz(mods, oracle):
    _, lz = mods
    rng = random.Random(2026)
    alphabets = [b"ab", b"ACGT", b"0123456789abcdef", bytes(range(256))]
    members = [_alpha(1000 + i, rng.randint(1025, 12000), alphabets[i % 4]) for i in range(200)]
    for window in (4096, 16):
        got = lz.CompressAsyncBatch(members, window)
        for d, g in zip(members, got):
            assert g == oracle.lzss_compress(d, window), (len(d), window)
        if window == 4096:
            for d, g in zip(members[::10], got[::10]):
                assert g == lz.CompressAsync(d, False, window), len(d)
        for d, g in zip(members, got):
            if len(set(d)) > 2:                                                # (two letters: runs and short periods, maybe handed back)
                PRODUCED.append((d, window, g))
        assert lz.DecompressBatch(got) == members


# ---------------------------------------------------------------- 8: the decoder on foreign streams
def _outcome(fn):
    from raisin_amd import RsnError
    try:
        return ("ok", fn())
    except RsnError as e:
        return ("err", e.code, str(e))


def _foreign(lz):
    lit = _alpha(88, 2300, b"abcdefghij \n")
    return [lit + b"<0,0>" + lit[:50],
            lit + b"<3,5>tail",                                                # a length above its pointer
            b"abc<2400,3>" + lit,                                              # a pointer before the start of the data
            lit + b"<9999,3>tail",
            lit + b"<x,3>tail", lit + b"<3,y>", lit + b"<3,3", lit + b"<12<3,3>",   # non-numeric fields, an open token
            lit + b"<8,0>" * 300, b"<8,0>" * 500,
            lit[:100] + b"q" * 4000 + b"<4096,4096>" * (lz.MID_E_MAX // 4096 + 2),
            lit + b"<2300,2300><4600,4600><9200,9200>",                       # copies that chain through copies
            lit + b"\\\\\\a<1,1>\\" + lit[:20] + b"\\\xff\xff\\\\<3,2>\\"]     # 5C runs across token seams, a dangling escape


def test_decoder_on_foreign_streams(mods, oracle, K):
    _lib, lz = mods
    for s in _foreign(lz):
        assert len(s) > SMALL_DEC_MAX
        single = _outcome(lambda: lz.Decompress(s))
        batch = _outcome(lambda: lz.DecompressBatch([s] * K))
        if single[0] == "ok":
            assert batch == ("ok", [single[1]] * K), s[-40:]
            try:                                                           # (where the oracle takes the stream too)
                want = oracle.lzss_decompress(s)
            except oracle.OracleError:
                want = single[1]
            assert single[1] == want, s[-40:]
        else:
            assert batch[0] == "err" and batch[1] == single[1], (s[-40:], single, batch)
            msg = _lib.lib().rsn_last_error().decode()
            assert msg.startswith("member 0: ") and msg[len("member 0: "):] == single[2].split(": ", 1)[1], (msg, single)


def test_a_failing_mid_member_fails_the_batch(mods, oracle, K):
    _lib, lz = mods
    from raisin_amd import RsnError
    lit = _alpha(88, 2300, b"abcdefghij \n")
    bad = lit + b"<9999,3>tail"
    with pytest.raises(RsnError) as single:
        lz.Decompress(bad)
    bufs = [oracle.lzss_compress(_text(800 + i, 6000)) for i in range(max(K, 6))]
    bufs[3] = bad
    bufs[5] = lit + b"<x,1>"                                                   # a later failure does not change the answer
    k = len(bufs)
    L = _lib.lib()
    ins = (ctypes.c_char_p * k)(*bufs)
    lens = (ctypes.c_size_t * k)(*[len(b) for b in bufs])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    assert L.rsn_lzss_decompress_batch(k, ins, lens, outs, olens) == single.value.code
    assert all(not outs[i] for i in range(k)) and all(olens[i] == 0 for i in range(k))
    msg = L.rsn_last_error().decode()
    assert msg.startswith("member 3: ") and msg[len("member 3: "):] == str(single.value).split(": ", 1)[1], msg
    bufs[3] = bufs[5] = bufs[0]
    assert lz.DecompressBatch(bufs) == [oracle.lzss_decompress(b) for b in bufs]   # the thread goes on


# ---------------------------------------------------------------- 9: closure
def test_the_decoder_takes_every_stream_the_encoder_writes(mods, oracle, K):
    """(after the encoder tests of this file: they leave their streams in PRODUCED)"""
    _lib, lz = mods
    if not PRODUCED:                                                           # run on its own: one encoder list
        members = [_text(950 + i, 1025 + 4000 * i) for i in range(16)]
        for d, g in zip(members, lz.CompressAsyncBatch(members)):
            PRODUCED.append((d, 4096, g))
    assert all(len(s) <= lz.MID_E_MAX for _, _, s in PRODUCED)
    above = [(d, s) for d, _, s in PRODUCED if len(s) > SMALL_DEC_MAX]
    assert len(above) >= K
    dec, prof = _prof(_lib, lambda: lz.DecompressBatch([s for _, s in above]))
    assert prof == {"lzss_batch_mid_dec": _dec_groups(lz, [s for _, s in above])}, prof
    assert dec == [d for d, _ in above]
    dec, prof = _prof(_lib, lambda: lz.DecompressBatch([s for _, _, s in PRODUCED]))
    assert set(prof) <= {"lzss_batch_mid_dec", "lzss_batch_dec"}, prof
    assert dec == [d for d, _, _ in PRODUCED]


# ---------------------------------------------------------------- 10: the callers
def _files(tmp_path, stem, datas):
    paths = []
    for i, d in enumerate(datas):
        p = tmp_path / ("%s%d.txt" % (stem, i))
        p.write_bytes(d)
        paths.append(str(p))
    return paths


def test_callers_pick_the_mid_kernels_up(mods, oracle, tmp_path, capsys):
    _lib, lz = mods
    from raisin_amd import engine
    datas = [_text(1200 + i, 4096 + (i * 401) % 4097) for i in range(max(16, lz.MID_GROUP_MIN))]   # (16 files, or as many as are grouped)
    paths = _files(tmp_path, "f", datas)
    capsys.readouterr()
    for p in paths:
        engine.CompressFile(["lzss"], p, p + ".loop")
    loop_lines = capsys.readouterr().out
    _, prof = _prof(_lib, lambda: engine.CompressFiles(["lzss"], paths, ".pyl"))
    assert capsys.readouterr().out == loop_lines
    assert prof.get("lzss_batch_mid_enc", 0) >= 1 and "lzss_batch_enc" not in prof, prof
    comp = [p + ".pyl" for p in paths]
    for p, d in zip(paths, datas):
        assert open(p + ".pyl", "rb").read() == open(p + ".loop", "rb").read() == oracle.lzss_compress(d)
    for c in comp:
        engine.DecompressFile(["lzss"], c, c + ".loop")
    loop_lines = capsys.readouterr().out
    _, prof = _prof(_lib, lambda: engine.DecompressFiles(["lzss"], comp, ".py"))
    assert capsys.readouterr().out == loop_lines
    assert prof.get("lzss_batch_mid_dec", 0) >= 1, prof
    for c, d in zip(comp, datas):
        assert open(c + ".py", "rb").read() == open(c + ".loop", "rb").read() == d
    # two layers: each layer's batch call in turn
    engine.CompressFiles(["lzss", "huffman"], paths, ".lh")
    for p, d in zip(paths, datas):
        assert open(p + ".lh", "rb").read() == engine.compress(d, ["lzss", "huffman"])
    capsys.readouterr()
    # the C++ host
    exe = os.path.join(ROOT, "raisin_amd", "host", "rsn")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(exe)])
    out = subprocess.check_output([exe, "-compress", ",".join(paths), "-algorithm=lzss", "-outext=cl"]).decode()
    assert out.count("Compressing...") == len(datas)
    for p, d in zip(paths, datas):
        assert open(p + ".cl", "rb").read() == oracle.lzss_compress(d)


# ---------------------------------------------------------------- 11: two threads
def test_two_threads_run_mid_batches_at_once(mods, oracle):
    _, lz = mods
    lists = [[_text(1300 + 100 * t + i, 1500 + 97 * i) for i in range(max(12, lz.MID_GROUP_MIN))] for t in range(2)]
    want = [[lz.CompressAsync(d) for d in l] for l in lists]
    assert want == [[oracle.lzss_compress(d) for d in l] for l in lists]
    errors = []

    def work(t):
        for r in range(5):
            c = lz.CompressAsyncBatch(lists[t])
            if c != want[t] or lz.DecompressBatch(c) != lists[t]:
                errors.append((t, r))
    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
