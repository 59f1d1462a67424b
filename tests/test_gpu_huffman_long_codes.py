"""GPU parity for Huffman codes of 25 to 66 bits: every decoder and encoder against the oracle and against the runes the stream was built
from (tests/long_codes.py, itself checked on the CPU by test_long_codes_host.py).

Decode: trees built from headers alone (huffman.go:196-227) with longest codes L = 31 ... 64 in three alphabets -- past the 32-bit window
of the second-level tables (huff_decode.hip: decode_long's bit walk), past the 29 bits the other suites reach, with a long codeword in
every few symbols; the sliced decode above 32 MiB with 39-bit codewords across its cuts; periodic payloads (k_dec_phase); the switches;
counts past 2**32; truncated streams; and 65 / 66 bits, which the oracle decodes and this library refuses.
Encode: Fibonacci inputs on both sides of k_emit_ascii32's 24-bit limit and past 32 bits, byte and rune alphabets, sharded and batched,
and one input of 268 MB with 39-bit codes."""
import hashlib
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import long_codes as LC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (31, 32, 33, 40, 48, 63, 64)
SIZES = (3000, 1 << 20, 8 << 20)
RSN_ERR_FORMAT, RSN_ERR_LIMIT = -3, -6


@pytest.fixture(scope="module")
def huff():
    from raisin_amd import huffman
    return huffman


def _tensor_decode(huff, s):
    import torch
    src = torch.frombuffer(bytearray(s), dtype=torch.uint8).cuda()
    return bytes(huff.decompress_tensor(src).cpu().numpy())


def _tensor_encode(huff, data):
    import torch
    src = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    return bytes(huff.compress_tensor(src).cpu().numpy())


def _oracle_decode(oracle, s):
    return oracle.huffman_decompress_mt(s, oracle.host_cores()) if len(s) > (4 << 20) else oracle.huffman_decompress(s)


def _profiled(fn, *args):
    from raisin_amd import _lib
    _lib.prof_enable(True)
    _lib.prof_reset()
    try:
        out = fn(*args)
        return out, {k for k, (n, _) in _lib.prof_get().items() if n}
    finally:
        _lib.prof_enable(False)


def _child_hashes(streams, env):
    """sha256 of huffman.Decompress of each stream, in a process of its own under `env` (the switches are read once per process)."""
    code = ("import sys, hashlib, pickle; sys.path.insert(0, %r)\nfrom raisin_amd import huffman\n"
            "for s in pickle.load(open(sys.argv[1], 'rb')):\n"
            "    print(hashlib.sha256(huffman.Decompress(s)).hexdigest())\n" % ROOT)
    import pickle
    with tempfile.NamedTemporaryFile(suffix=".pkl") as f:
        pickle.dump(list(streams), f)
        f.flush()
        r = subprocess.run([sys.executable, "-c", code, f.name], capture_output=True, text=True, timeout=600, env=dict(os.environ, **env))
    assert r.returncode == 0, (env, r.stderr[-2000:])
    return r.stdout.split()


def _sha(b):
    return hashlib.sha256(b).hexdigest()


_STREAMS = {}


def _stream(alphabet, L, size, periodic=False):
    key = (alphabet, L, size, periodic)
    if key not in _STREAMS:
        counts = LC.layered_tree(L) if alphabet == "layered" else LC.tree(alphabet, L)
        pick, cs = LC.picker(counts)
        _STREAMS[key] = LC.block_stream(counts, pick, size, seed=L * 7 + size % 1000 + periodic, periodic=periodic, cs=cs)
    return _STREAMS[key]


# ------------------------------------------------------------------ decode: header-built trees
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("alphabet", LC.ALPHABET_NAMES)
def test_header_built_trees_decode(huff, oracle, alphabet, L):
    from oracle import literal
    for size in SIZES:
        s, want = _stream(alphabet, L, size)
        assert _oracle_decode(oracle, s) == want, (alphabet, L, size)
        if size < 4096:
            assert literal.huffman_decompress(s) == want
        assert huff.Decompress(s) == want, (alphabet, L, size)
        assert _tensor_decode(huff, s) == want, (alphabet, L, size)


def test_periodic_payloads_reach_the_phase_decoder(huff, oracle):
    """One block repeated: a stream that parses in more than one phase for as long as it lasts -- and with a code whose lengths are all
    multiples of 3 (long_codes.layered_tree), a lane that begins on the wrong residue never finds the boundaries.  The bytes are the
    oracle's; at least one of these streams must have been decoded from every entry (k_dec_phase), the path whose per-lane walk follows
    min(64, L) entries."""
    reached = []
    for alphabet, L in [("ascii", 40), ("ascii", 64), ("runes", 48), ("layered", 42), ("layered", 48), ("layered", 54)]:
        s, want = _stream(alphabet, L, 2 << 20, periodic=True)
        assert _oracle_decode(oracle, s) == want
        got, ran = _profiled(huff.Decompress, s)
        assert got == want, (alphabet, L)
        assert _tensor_decode(huff, s) == want, (alphabet, L)
        reached.append("huff_dec_phase" in ran)
    assert any(reached), "no periodic long-code stream reached k_dec_phase"


def test_long_code_streams_under_the_switches(oracle):
    """RSN_NO_MULTI=1 (one codeword per lookup), RSN_DEC_WARM=0 (no warm-up) and both: the same bytes, each in a process of its own."""
    keys = [(a, L, 1 << 20, False) for a in LC.ALPHABET_NAMES for L in (33, 48, 64)] + [("ascii", 64, 2 << 20, True), ("layered", 54, 2 << 20, True)]
    pairs = [_stream(*k) for k in keys]
    want = [_sha(d) for _, d in pairs]
    for env in ({}, {"RSN_NO_MULTI": "1"}, {"RSN_DEC_WARM": "0"}, {"RSN_DEC_WARM": "0", "RSN_NO_MULTI": "1"}):
        assert _child_hashes([s for s, _ in pairs], env) == want, env


def test_counts_past_2_to_the_32(huff, oracle):
    """The counts of an L <= 40 header times a power of two (the largest below 2**62): the same tree, built by the wide heap, the same
    bytes."""
    for alphabet in LC.ALPHABET_NAMES:
        for L in (33, 40):
            counts = LC.tree(alphabet, L)
            sh = 61 - max(counts.values()).bit_length()
            s, want = _stream(alphabet, L, 1 << 20)
            sep = s.index(LC.SEP)
            wide = {r: c << sh for r, c in counts.items()}
            assert max(wide.values()) < 1 << 62 and max(wide.values()) >= 1 << 32
            s2 = LC.header(wide) + s[sep:]
            assert oracle.huffman_decompress(s2) == want
            assert huff.Decompress(s2) == want, (alphabet, L)
            assert _tensor_decode(huff, s2) == want, (alphabet, L)


def test_a_payload_cut_inside_a_final_long_codeword(huff, oracle):
    """The last codeword is 64 or 48 bits; dropping 1..7 payload bytes ends the stream inside it (the pad is in front, huffman.go:245):
    RSN_ERR_FORMAT wherever the oracle raises, the oracle's bytes wherever it does not."""
    from raisin_amd import RsnError
    raised = 0
    for alphabet in LC.ALPHABET_NAMES:
        for L in (48, 64):
            counts = LC.tree(alphabet, L)
            pick, cs = LC.picker(counts)
            deep = max(cs, key=lambda r: (len(cs[r]), r))
            for n_syms in (200, 100000):
                syms = [int(x) for x in pick(np.random.default_rng(n_syms + L), n_syms)] + [deep]
                full = LC.stream(counts, syms, cs)
                assert huff.Decompress(full) == oracle.huffman_decompress(full)
                for drop in range(1, 8):
                    bad = full[:-drop]
                    try:
                        want = oracle.huffman_decompress(bad)
                    except oracle.OracleError:
                        want = None
                    for fn in (huff.Decompress, lambda b: _tensor_decode(huff, b)):
                        if want is None:
                            with pytest.raises(RsnError) as e:
                                fn(bad)
                            assert e.value.code == RSN_ERR_FORMAT, (alphabet, L, n_syms, drop)
                        else:
                            assert fn(bad) == want
                    raised += want is None
    assert raised >= 20


def test_codes_past_64_bits_are_refused_cleanly(huff, oracle):
    """L = 65 and 66: the oracle decodes these streams, this library returns RSN_ERR_LIMIT -- from Decompress below and
    above 32 MiB and from decompress_tensor -- and the next ordinary call on the same thread succeeds."""
    from raisin_amd import RsnError
    ok = oracle.huffman_compress(b"an ordinary call after a refused one\n" * 100)
    for alphabet in ("ascii", "runes"):
        for L in (65, 66):
            counts = LC.tree(alphabet, L)
            pick, cs = LC.picker(counts)
            for size in (3000, 1 << 20, 34 << 20):
                s, want = LC.block_stream(counts, pick, size, seed=L + size % 997, cs=cs)
                if size < (4 << 20):
                    assert oracle.huffman_decompress(s) == want
                calls = (huff.Decompress,) if size > (32 << 20) else (huff.Decompress, lambda b: _tensor_decode(huff, b))
                for fn in calls:
                    with pytest.raises(RsnError) as e:
                        fn(s)
                    assert e.value.code == RSN_ERR_LIMIT, (alphabet, L, size)
                    assert huff.Decompress(ok) == oracle.huffman_decompress(ok)


# ------------------------------------------------------------------ decode above 32 MiB: the sliced pipeline
SLICE_BITS = (64 << 20) * 8        # a pipelined decode cuts the payload every 64 MiB, counted from the 16-byte boundary at or before it


def _cut_bits(hdr_len):
    pay, a0 = LC.payload_start(hdr_len)
    return [k * SLICE_BITS - 8 * (pay - a0) for k in (1, 2)], [k * (SLICE_BITS // 2) - 8 * (pay - a0) for k in (1, 3)]   # (payload bits)


def test_sliced_decode_with_long_codewords_across_the_cuts(huff, oracle):
    """Above 32 MiB a decode runs in slices, each looking 4096 bits past its end for the codeword that begins inside it.  Two streams with
    39-bit codes (Fibonacci counts over 40 symbols: the deepest tree whose counts still fit the payload's bits, which the pipeline needs):
      * data-built, 268 MB of input: its stream is the oracle's (huffman_compress_mt), its two 39-bit codewords begin within 6 bits
        before the 64 MiB cut and a 32 MiB point -- then the same payload under counts doubled (the same tree; the pipeline) and counts
        halved (more symbols than announced: the serial retry);
      * header-built, 72 MiB of payload, a 39-bit codeword in every 8 symbols and one beginning 3 bits before the cut.
    Every result against the runes, the oracle, and the serial call (RSN_HOST_SERIAL=1) in a process of its own."""
    k = 40
    counts = LC.fib_counts(k)
    cs = LC.codes(counts)
    lens = np.zeros(256, dtype=np.uint8)
    for i in range(k):
        lens[i] = len(cs[LC.ALPHABETS["ascii"](i)])
    assert lens[0] == lens[1] == 39
    hdr = LC.header(counts)
    total = sum(f * int(lens[i]) for i, f in enumerate(LC.fib(k)))
    pad = (8 - total % 8) % 8
    cuts, halves = _cut_bits(len(hdr))
    idx = LC.move_to_bits(LC.fib_symbols(k, "shuffled", seed=40), lens, [0, 1], [halves[0] - pad, cuts[0] - pad])
    data = LC.encode_symbols(idx, k)
    del idx
    assert len(data) == LC.fib(k + 2)[-1] - 1
    c, ran = _profiled(huff.Compress, data)                            # (the 39-bit encode case: k_emit<ASCII_WIDE>)
    assert "huff_emit_wide" in ran
    assert c == oracle.huffman_compress_mt(data, oracle.host_cores())
    assert c.startswith(hdr + LC.SEP + bytes([pad])) and len(c) > (64 << 20) + (1 << 20)
    got, ran = _profiled(huff.Decompress, c)
    assert got == data
    assert "huff_dec_emit" in ran
    sep = c.index(LC.SEP)
    doubled = LC.header({r: 2 * f for r, f in counts.items()}) + c[sep:]
    halved = LC.header({r: f // 2 for r, f in counts.items()}) + c[sep:]
    assert huff.Decompress(doubled) == data == oracle.huffman_decompress_mt(doubled, oracle.host_cores())
    h = huff.Decompress(halved)
    assert h == oracle.huffman_decompress_mt(halved, oracle.host_cores())
    del got
    pick, _ = LC.picker(counts, deep=1 / 8)
    s, want = LC.block_stream(counts, pick, 72 << 20, seed=72, cs=cs, place=[(cuts[0] - 3, 33)])
    assert s.startswith(hdr + LC.SEP)
    assert huff.Decompress(s) == want == oracle.huffman_decompress_mt(s, oracle.host_cores())
    streams = [c, doubled, halved, s]
    assert _child_hashes(streams, {"RSN_HOST_SERIAL": "1"}) == [_sha(data), _sha(data), _sha(h), _sha(want)]


# ------------------------------------------------------------------ encode: data-built codes
@pytest.mark.parametrize("order", ["shuffled", "sorted"])
@pytest.mark.parametrize("k", [25, 26, 33, 34, 36])
def test_fibonacci_inputs_encode(huff, oracle, k, order):
    """k - 1 bit codes: 24 (the top of k_emit_ascii32, len << 24 | code), 25 (the bottom of k_emit<ASCII_WIDE>), 32, 33 and 35."""
    data = LC.fib_data(k, "ascii", order, seed=k)
    want = oracle.huffman_compress_mt(data, oracle.host_cores()) if len(data) > (4 << 20) else oracle.huffman_compress(data)
    got, ran = _profiled(huff.Compress, data)
    assert got == want, (k, order)
    assert ("huff_emit_wide" if k - 1 > 24 else "huff_emit") in ran, ran
    assert ("huff_emit" if k - 1 > 24 else "huff_emit_wide") not in ran, ran
    got, ran = _profiled(_tensor_encode, huff, data)
    assert got == want, (k, order)
    assert ("huff_emit_wide" if k - 1 > 24 else "huff_emit") in ran, ran
    assert huff.Decompress(want) == data


@pytest.mark.parametrize("alphabet", ["rune2", "rune4"])
def test_fibonacci_runes_encode(huff, oracle, alphabet):
    """33-bit codes over 2- and 4-byte runes: k_emit<MODE_RUNE>."""
    data = LC.fib_data(34, alphabet, "shuffled", seed=34)
    want = oracle.huffman_compress_mt(data, oracle.host_cores())
    got, ran = _profiled(huff.Compress, data)
    assert got == want
    assert "huff_emit_rune" in ran, ran
    assert _tensor_encode(huff, data) == want
    assert huff.Decompress(want) == data


def test_sharded_and_batched_encode_of_deep_codes(huff, oracle):
    deep = LC.fib_data(34, "ascii", "shuffled", seed=5)
    runes = LC.fib_data(33, "rune2", "sorted")
    for data in (deep, runes):
        want = huff.Compress(data)
        assert want == oracle.huffman_compress_mt(data, oracle.host_cores())
        for G in (2, 7, 33):
            assert huff.CompressSharded(data, G) == want, G
    chunks = [LC.fib_data(26, "ascii", "sorted"), np.random.default_rng(1).integers(0, 128, 3 << 20, dtype=np.uint8).tobytes(),
              LC.fib_data(33, "ascii", "shuffled", seed=9), runes[: 5 << 20], LC.fib_data(25, "rune4", "shuffled", seed=2)]
    assert huff.CompressBatch(chunks) == [huff.Compress(x) for x in chunks] == [oracle.huffman_compress(x) for x in chunks]
