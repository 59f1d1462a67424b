"""Every device-buffer call between fences: include/rsn.h promises that nothing is ever written outside [d_out, d_out + out_cap)
and that only the n bytes of the input are read as data.  GPU sanitizers are not to be had, so the instrument is a buffer with
64 KiB of seeded random bytes in front of it and behind it, compared after every call -- in front of d_out (where an aligned
store's head peel goes wrong), behind d_out + out_cap with out_cap exactly as passed (where a tail peel goes wrong), and on both
sides of the input, whose neighbours are filled with bytes that would change the answer if a kernel took them for data.

Expected bytes, exact sizes and the verdict on every damaged stream come from the CPU oracle, never from the library.  The only
refusals tolerated beyond the oracle's are DESIGN.md section 7's: a token that is not "<" 1-10 digits "," 1-10 digits ">"
(RSN_ERR_FORMAT) and a Huffman code above 64 bits (RSN_ERR_LIMIT); a case that may meet one says which.  Each path group brackets
one call with the library's own launch profile and asserts that the kernel it aims at ran, unless an A/B switch of
scripts/suite_under_switches.sh replaces that path.  An overrun lands in fence bytes this file allocated and is found by
comparison; nothing here can turn one into a fault."""
import ctypes
import os
import random

import numpy as np
import pytest

import long_codes as LC
from test_bounds_host import _distinct_runes
from test_gpu_fuzz import _token_stream
from test_gpu_lzss import long_copies, rnd, text

pytestmark = pytest.mark.gpu

OK, E_ARG, E_EMPTY, E_FORMAT, E_LIMIT, E_CAP = 0, -1, -2, -3, -6, -7
FENCE = 1 << 16                       # bytes of fence on either side: four 16 KiB tiles
RESIDUES = (0, 1, 7, 8, 15)
LZSS, HUFF = 1, 2
LOOSE = "a token spelling the reference's Atoi lets through (DESIGN 7)"
DEEP = "a code above 64 bits (DESIGN 7)"
_serial = [0]


def _ru16(x):
    return (x + 15) // 16 * 16


def _tiled(pat, k, right=False):
    """k bytes of `pat` repeated; right: the last repetition ENDS at the end (what lies before a buffer continues into it)."""
    reps = k // len(pat) + 2
    return (pat * reps)[len(pat) * reps - k:] if right else (pat * reps)[:k]


def fenced(cap, data=None, before=None, after=None):
    """(tensor, d_ptr, check): ONE uint8 allocation of FENCE + cap rounded up to 16 + FENCE seeded random bytes.  tensor is the
    cap bytes at d_ptr (16-byte aligned); check() synchronises and asserts that neither fence has changed -- the back fence
    begins at d_ptr + cap, not at the rounded size.  data: copied to d_ptr (an input); before / after: the bytes in front of it
    and behind it are these patterns repeated instead of random ones (hostile neighbours of an input)."""
    import torch
    _serial[0] += 1
    total = FENCE + _ru16(cap) + FENCE
    g = torch.Generator().manual_seed(0xFE2CE000 + _serial[0])
    host = torch.randint(0, 256, (total,), dtype=torch.uint8, generator=g)
    if before:
        host[:FENCE] = torch.frombuffer(bytearray(_tiled(before, FENCE, right=True)), dtype=torch.uint8)
    if after:
        host[FENCE + cap:] = torch.frombuffer(bytearray(_tiled(after, total - FENCE - cap)), dtype=torch.uint8)
    if data:
        assert len(data) == cap
        host[FENCE:FENCE + cap] = torch.frombuffer(bytearray(data), dtype=torch.uint8)
    whole = host.cuda()
    assert whole.data_ptr() % 16 == 0
    keep = (whole[:FENCE].clone(), whole[FENCE + cap:].clone())
    torch.cuda.synchronize()

    def check(what="buffer"):
        torch.cuda.synchronize()
        for now, was, base in ((whole[:FENCE], keep[0], -FENCE), (whole[FENCE + cap:], keep[1], cap)):
            if not torch.equal(now, was):
                first = int((now != was).nonzero()[0])
                raise AssertionError("%s of %d bytes: a byte outside it changed, first at offset %d from its start"
                                     % (what, cap, base + first))
    return whole[FENCE:FENCE + cap], whole.data_ptr() + FENCE, check


def _bytes(t, k):
    return bytes(t[:k].cpu().numpy())


@pytest.fixture(scope="module")
def L():
    from raisin_amd import _lib
    lib = _lib.lib()
    _lib.check(lib.rsn_device_set(0))
    return lib


class Op:
    """One *_dev entry point: how to call it, what the oracle says it returns, its compress bound (None for a decoder), and
    whether its last step is the Huffman encoder (the smallest buffer it takes is then the size rounded up to 16, plus 32)."""

    def __init__(self, name, fn, extra, want, bound=None, pad32=False):
        self.name, self.fn, self.extra, self.want, self.bound, self.pad32 = name, fn, extra, want, bound, pad32

    def call(self, d_in, n, d_out, cap):
        got = ctypes.c_size_t(0)
        rc = self.fn(d_in, n, *self.extra, d_out, cap, ctypes.byref(got), None)
        return rc, got.value

    def floor(self, E):
        return _ru16(E) + 32 if self.pad32 else E


def huff_c(L):
    return Op("huffman_compress_dev", L.rsn_huffman_compress_dev, (), lambda O, d: O.huffman_compress(d), L.rsn_huffman_compress_bound, True)


def huff_d(L):
    return Op("huffman_decompress_dev", L.rsn_huffman_decompress_dev, (), lambda O, d: O.huffman_decompress(d))


def lzss_c(L, w=4096):
    return Op("lzss_compress_dev(%d)" % w, L.rsn_lzss_compress_dev, (w,), lambda O, d: O.lzss_compress(d, w), L.rsn_lzss_compress_bound)


def lzss_d(L):
    return Op("lzss_decompress_dev", L.rsn_lzss_decompress_dev, (), lambda O, d: O.lzss_decompress(d))


def _layer_ids(ids):
    return (ctypes.c_int * max(len(ids), 1))(*ids), len(ids)


def layers_c(L, ids):
    def want(O, d):
        for i in ids:
            d = O.lzss_compress(d, 4096) if i == LZSS else O.huffman_compress(d)
        return d

    def bound(n):
        for i in ids:
            n = L.rsn_lzss_compress_bound(n) if i == LZSS else L.rsn_huffman_compress_bound(n)
        return n
    return Op("layers_compress_dev%r" % (ids,), L.rsn_layers_compress_dev, _layer_ids(ids), want, bound, bool(ids) and ids[-1] == HUFF)


def layers_d(L, ids):
    def want(O, d):
        for i in reversed(ids):
            d = O.lzss_decompress(d) if i == LZSS else O.huffman_decompress(d)
        return d
    return Op("layers_decompress_dev%r" % (ids,), L.rsn_layers_decompress_dev, _layer_ids(ids), want)


def _ran(fn):
    """fn() under the library's launch profile: (its result, the names of the kernels it launched)."""
    from raisin_amd import _lib
    _lib.prof_enable(True)
    _lib.prof_reset()
    try:
        out = fn()
        return out, {k for k, (n, _) in _lib.prof_get().items() if n}
    finally:
        _lib.prof_enable(False)


def _switched(*names):
    return any(os.environ.get(n) for n in names)


def matrix(O, op, data, expect=(), absent=(), unless=(), any_of=(), before=None, after=None, small=True):
    """The capacities of one input: the size query, a buffer of the size the query names, the smallest buffer the call takes
    (the exact size E; behind the Huffman encoder E rounded up to 16, plus 32 -- and E itself is then refused with that figure),
    the compress bound, and three buffers that are too small, each followed by a call with the size the refusal named.  Every
    call ends with all four fences compared.  expect / absent: kernels that must / must not have run in the first good call
    (any_of: at least one of these), unless one of the switches `unless` is set.  Returns the oracle's bytes."""
    want = op.want(O, data)
    E, n = len(want), len(data)
    src, d_in, chk_in = fenced(n, data, before, after)
    tag = "%s, %d bytes in, %d out" % (op.name, n, E)

    def run(cap):
        out, d_out, chk_out = fenced(cap)
        rc, got = op.call(d_in, n, d_out, cap)
        chk_out("%s: the output buffer" % tag)
        chk_in("%s: the input" % tag)
        return rc, got, out

    def good(cap, why):
        rc, got, out = run(cap)
        assert rc == OK, "%s: %s (%d bytes) was refused with %d" % (tag, why, cap, rc)
        assert got == E, (tag, why, cap, got)
        assert _bytes(out, E) == want, "%s: %s (%d bytes): not the oracle's bytes" % (tag, why, cap)

    rc, need = op.call(d_in, n, None, 0)
    chk_in("%s: the input, after the size query" % tag)
    assert rc == E_CAP and need >= E, (tag, "size query", rc, need)
    _, ran = _ran(lambda: good(need, "the size the query named"))
    if not _switched(*unless):
        assert set(expect) <= ran and not (set(absent) & ran), (tag, sorted(ran))
        assert not any_of or set(any_of) & ran, (tag, sorted(ran))
    floor = op.floor(E)
    good(floor, "the smallest buffer the call takes")
    if op.pad32:
        for cap in sorted({E, floor - 16}):
            rc, got, _ = run(cap)
            assert rc == E_CAP and got == floor, (tag, "the exact size behind the Huffman encoder", cap, rc, got)
    if op.bound:
        good(op.bound(n), "the compress bound")
    if small:
        for cap in sorted({16, E // 2 // 16 * 16, E // 16 * 16 - 16}):
            if not 0 < cap < floor:
                continue
            rc, got, _ = run(cap)
            assert rc == E_CAP and got >= E, (tag, "a buffer that is too small", cap, rc, got)
            good(got, "the size a refusal named")
    return want


def _residue_lengths(make, size_of, n0, span=400, lengths=None):
    """{r: n} with size_of(make(n)) % 16 == r for every r of RESIDUES, n from n0 up (or from `lengths`): input lengths chosen by
    the oracle's sizes."""
    found = {}
    for n in lengths or range(n0, n0 + span):
        r = size_of(make(n)) % 16
        if r in RESIDUES and r not in found:
            found[r] = n
            if len(found) == len(RESIDUES):
                return found
    raise AssertionError("no input length in [%d, %d) for every residue: %r" % (n0, n0 + span, found))


# ------------------------------------------------------------------------------------------------ inputs
def flat_bytes(Lbits, n, seed=0):
    """n bytes over exactly 2**Lbits symbols whose counts differ by one at most: every code Lbits long (the fixed-width kernels)."""
    k = 1 << Lbits
    lo = 0 if k == 128 else 40
    buf = bytearray(bytes(range(lo, lo + k)) * (n // k + 1))
    random.Random(Lbits * 1000 + n + seed).shuffle(buf)
    return bytes(buf[:n])


def skewed_bytes(n, seed=7):
    rng = np.random.default_rng(seed)
    return bytes((rng.geometric(0.25, size=n).clip(max=60) + 32).astype(np.uint8))


def rune_bytes(n, seed=3):
    """ASCII, valid 2-, 3- and 4-byte runes and invalid bytes mixed (each invalid byte is one U+FFFD, huffman.go:309)."""
    rng = random.Random(seed)
    good = [c.encode() for c in "abc déf ✓ λ 𝄞 世界 é€ 🙂\n"]
    bad = [b"\x80", b"\xbf", b"\xc0\x80", b"\xff", b"\xe2\x82", b"\xf0\x9f", b"\xed\xa0\x80", b"\xf4\x90\x80\x80"]
    out = bytearray()
    while len(out) < n:
        out += rng.choice(bad) if rng.random() < 0.03 else rng.choice(good)
    return bytes(out[:n])


def no_sync_bytes(n):
    """Code lengths {3 x 7, 6 x 8}: a parse that starts on the wrong residue mod 3 never finds the boundaries again."""
    rng = np.random.default_rng(77)
    w = np.array([8] * 7 + [1] * 8, dtype=np.float64)
    return np.arange(65, 80, dtype=np.uint8)[rng.choice(15, size=n, p=w / w.sum())].tobytes()


PLAIN = bytes(v for v in range(256) if v not in (0x5C, 0xFF, 0x3C))


def plain_text(seed, n):
    """Text without 5C and FF: nothing in it needs an escape, so its LZSS stream holds no 5C ('<' becomes one FF byte)."""
    return text(seed, n).replace(b"\\", b"/").replace(b"\xff", b"y")


# ------------------------------------------------------------------------------------------------ Huffman encode
@pytest.mark.parametrize("n", [4095, 4097, 2 << 20, (2 << 20) + 17])
def test_huffman_encode_flat(L, oracle, n):
    """The flat code (k_emit_flat: offsets by arithmetic) on both sides of a 4 KiB tile and of SMALL_INPUT (2 MiB: 64 KiB tiles)."""
    data = flat_bytes(7, n)
    assert {x[3] for x in oracle.huffman_table(data)} == {7}
    matrix(oracle, huff_c(L), data, expect=("huff_emit",), absent=("huff_emit_init",), unless=("RSN_NO_FLAT",))


@pytest.mark.parametrize("n", [4096, 65535, 65537, (2 << 20) + 1])
def test_huffman_encode_skewed(L, oracle, n):
    matrix(oracle, huff_c(L), skewed_bytes(n), expect=("huff_emit", "huff_emit_init", "huff_tile_bits"))


@pytest.mark.parametrize("n", [3000, 65536 + 5, 300001])
def test_huffman_encode_runes(L, oracle, n):
    matrix(oracle, huff_c(L), rune_bytes(n), expect=("huff_emit_rune", "huff_tile_bits_rune"))


def test_huffman_encode_single_symbol_and_wide_codes(L, oracle):
    for data in (b"a" * 5000, "é".encode() * 3001, b"z"):
        want = matrix(oracle, huff_c(L), data, absent=("huff_emit", "huff_emit_rune", "huff_emit_wide"))
        assert want.endswith(b"\\\n\x00")                                # the quirk: a header and a pad byte, no payload
    matrix(oracle, huff_c(L), LC.fib_data(30), expect=("huff_emit_wide",))


def test_huffman_encode_every_residue(L, oracle):
    base = skewed_bytes(21000, seed=11)
    sizes = _residue_lengths(lambda n: base[:n], lambda d: len(oracle.huffman_compress(d)), 20000)
    for r, n in sorted(sizes.items()):
        want = matrix(oracle, huff_c(L), base[:n], expect=("huff_emit",))
        assert len(want) % 16 == r
    base = rune_bytes(9000)
    for r, n in sorted(_residue_lengths(lambda n: base[:n], lambda d: len(oracle.huffman_compress(d)), 8000).items()):
        matrix(oracle, huff_c(L), base[:n], expect=("huff_emit_rune",), small=False)


# ------------------------------------------------------------------------------------------------ Huffman decode
@pytest.mark.parametrize("Lbits", [1, 2, 3, 4, 5, 6, 7])
def test_huffman_decode_flat_every_width(L, oracle, Lbits):
    """k_dec_flat<L>: 2**L equiprobable symbols.  Every width at a short and a long size; widths 3 and 7 at every residue of E."""
    k = 1 << Lbits
    sizes = [k * 37, k * 1000 + 3 + RESIDUES[Lbits % 5]]
    if Lbits in (3, 7):
        sizes += [k * 1000 + 16 + r for r in RESIDUES]
    for n in sizes:
        data = flat_bytes(Lbits, n)
        assert {x[3] for x in oracle.huffman_table(data)} == {Lbits}
        want = matrix(oracle, huff_d(L), oracle.huffman_compress(data), expect=("huff_dec_flat",), unless=("RSN_NO_FLAT",))
        assert want == data


def test_huffman_decode_general(L, oracle):
    """The multi-block decoder (k_dec_sync + k_dec_emit: LDS output images shifted to line up with memory) at every residue."""
    base = skewed_bytes((1 << 20) + 15)
    for n in [150000 + r for r in RESIDUES] + [(1 << 20) + 15]:
        want = matrix(oracle, huff_d(L), oracle.huffman_compress(base[:n]), expect=("huff_dec_sync", "huff_dec_emit"))
        assert want == base[:n]
    data = rune_bytes(200001)
    matrix(oracle, huff_d(L), oracle.huffman_compress(data), expect=("huff_dec_sync", "huff_dec_emit"))


@pytest.mark.parametrize("alphabet", LC.ALPHABET_NAMES)
def test_huffman_decode_long_codes(L, oracle, alphabet):
    """Second-level tables (LDS for byte alphabets, through L2 for 4096 CJK runes) and the bit walk below them: longest codes of
    25, 33, 48 and 64 bits, streams built from headers alone (tests/long_codes.py).  The launch profile has no name of its own for
    these paths -- they are template instances of k_dec_sync / k_dec_emit under the multi-block decoder's launch names -- so what
    shows that they ran is the names together with the stream itself: a quarter of its symbols carry codes of `bits` bits, past
    the 11 index bits of the first-level table (LUT_BITS_MAX), and from 33 up past the 32-bit window of the second level."""
    for bits in (25, 33, 48, 64):
        counts = LC.tree(alphabet, bits)
        pick, cs = LC.picker(counts)
        assert max(len(c) for c in cs.values()) == bits > 11
        stream, dec = LC.block_stream(counts, pick, 1 << 16, seed=bits, cs=cs)
        want = matrix(oracle, huff_d(L), stream, expect=("huff_dec_sync", "huff_dec_emit"), absent=("huff_dec_flat",), small=bits in (25, 64))
        assert want == dec


def test_huffman_decode_without_self_synchronisation(L, oracle):
    data = no_sync_bytes(300001)
    assert sorted(x[3] for x in oracle.huffman_table(data)) == [3] * 7 + [6] * 8
    # more than the one fixing pass: the passes go on (k_dec_sync's verify rounds) or every entry of every lane is walked (k_dec_phase)
    want = matrix(oracle, huff_d(L), oracle.huffman_compress(data), expect=("huff_dec_emit",), any_of=("huff_dec_phase", "huff_dec_sync_verify"))
    assert want == data


def test_huffman_decode_bare_leaf(L, oracle):
    for data in (b"aaaa", "ééé".encode(), "𝄞".encode() * 9):
        want = matrix(oracle, huff_d(L), oracle.huffman_compress(data), absent=("huff_dec_emit", "huff_dec_flat"))
        assert len(want) == len(data) // len(data.decode())               # the quirk: the symbol once (huffman.go:136-143)


# ------------------------------------------------------------------------------------------------ LZSS encode
@pytest.mark.parametrize("w", [4096, 1000, 8193, 0])
def test_lzss_encode_text_and_noise(L, oracle, w):
    """Text and noise over all 256 byte values (5C and FF: the escape writer; '<': the FF map) under every kind of window: the
    chain walk (4096, 1000) and lzss_big.hip (8193, unbounded)."""
    big = w == 0 or w > 8192
    n_text, n_noise = (30000, 20001) if big else (150001, 70000)
    expect = ("lzss_big_match", "lzss_big_emit") if big else ("lzss_tok_emit",)
    matrix(oracle, lzss_c(L, w), text(61, n_text), expect=expect + ("lzss_esc_write",))
    matrix(oracle, lzss_c(L, w), rnd(3, n_noise, bytes(range(256))), expect=expect + ("lzss_esc_write",))


def test_lzss_encode_escapes_only(L, oracle):
    """Nothing but 5C, FF and '<': the escape writer dominates and the stream is longer than the input."""
    for n in (4096, 40001):
        data = rnd(n, n, b"\\\xff<")
        want = matrix(oracle, lzss_c(L), data, expect=("lzss_esc_count", "lzss_esc_write"))
        assert len(want) > n
    data = b"\\\xff" * 3000 + b"<" * 17                                   # no match worth a token anywhere near the end
    matrix(oracle, lzss_c(L, 1), data, expect=("lzss_esc_write",))


def test_lzss_encode_periodic_tail(L, oracle):
    """W-periodic data: a short head through the encoder, the rest written by k_periodic_tail (16-byte units with a peeled head
    and tail) -- remainders chosen so that the stream's size takes every residue."""
    blk = rnd(77, 4096, PLAIN)

    def make(n):
        return (blk * (n // 4096 + 1))[:n]
    # (a period more adds one "<4096,4096>", 11 bytes; the last item adds its own length: both are varied)
    lengths = [4096 * (60 + j) + rem for j in range(16) for rem in (0, 1, 5, 9, 700)]
    sizes = _residue_lengths(make, lambda d: len(oracle.lzss_compress(d)), 0, lengths=lengths)
    for r, n in sorted(sizes.items()):
        matrix(oracle, lzss_c(L), make(n), expect=("lzss_periodic_tail",), unless=("RSN_LZSS_NO_PERIODIC_TAIL",))
    matrix(oracle, lzss_c(L), plain_text(5, 30001) + make(4096 * 70 + 9),
           expect=("lzss_periodic_tail",), unless=("RSN_LZSS_NO_PERIODIC_TAIL",))


def test_lzss_encode_runs_and_copies(L, oracle):
    matrix(oracle, lzss_c(L), b"\0" * 200000 + plain_text(8, 20000) + b"a" * 100001 + b"\xff" * 5000, expect=("lzss_tok_emit",))
    matrix(oracle, lzss_c(L), long_copies(4, 60000), expect=("lzss_tok_emit",))


def test_lzss_encode_every_residue(L, oracle):
    base = text(71, 21000)
    for w in (4096, 1000):
        sizes = _residue_lengths(lambda n: base[:n], lambda d: len(oracle.lzss_compress(d, w)), 20000)
        for r, n in sorted(sizes.items()):
            want = matrix(oracle, lzss_c(L, w), base[:n], expect=("lzss_tok_emit",), small=w == 4096)
            assert len(want) % 16 == r
    base = text(72, 12000)                                                # (an unbounded window is the stream's length: above 8192 it is lzss_big.hip's)
    for r, n in sorted(_residue_lengths(lambda n: base[:n], lambda d: len(oracle.lzss_compress(d, 0)), 10000).items()):
        matrix(oracle, lzss_c(L, 0), base[:n], expect=("lzss_big_emit",), small=False)


# ------------------------------------------------------------------------------------------------ LZSS decode
def test_lzss_decode_tile_path(L, oracle):
    """Without a 5C the emit kernel writes straight into d_out (`plain`); with one the separate unescape passes do."""
    base = plain_text(61, 200016)
    for r in RESIDUES:
        data = base[:200000 + r]
        want = matrix(oracle, lzss_d(L), oracle.lzss_compress(data), expect=("lzss_dec_emit",), absent=("lzss_une_write",))
        assert want == data
        data = data[:100000] + b"\\" + data[100001:]
        want = matrix(oracle, lzss_d(L), oracle.lzss_compress(data), expect=("lzss_dec_emit", "lzss_une_write"), small=r == 0)
        assert want == data
    noise = rnd(9, 70001, bytes(range(256)))
    assert matrix(oracle, lzss_d(L), oracle.lzss_compress(noise), expect=("lzss_une_write",)) == noise


def test_lzss_decode_run_tiles(L, oracle):
    blk = rnd(21, 4096, bytes(range(97, 123)))
    for data in (blk * 40 + blk[:7], blk[:1000] * 100 + b"x", blk[:37] * 3000, b"\x00" * 200001):
        want = matrix(oracle, lzss_d(L), oracle.lzss_compress(data), expect=("lzss_dec_runs",), unless=("RSN_LZSS_DEC_NO_RUNS",))
        assert want == data


@pytest.mark.parametrize("head,last", [(70001, b""), (70015, b""), (70001, b"<4096,14>"), (70015, b"xy"), (70000, b"<9,8>"),  (70007, b"\xffend")])
def test_lzss_decode_run_tail(L, oracle, head, last):
    """A stream of more than 1 MiB of output that ends in <P,P> repeated: the head by the ordinary decoder, the run by
    k_lzd_run_fill (16-byte stores between a peeled head and tail), the last item by a block of its own.  The head's length and
    the total take residues 1 and 15 (and others) mod 16; P = 4096 and, not a multiple of 16, 1000."""
    lit = rnd(head, head, bytes(range(97, 123)))
    for P, reps in ((4096, 300), (1000, 1300)):
        stream = lit + b"<%d,%d>" % (P, P) * reps + last
        want = matrix(oracle, lzss_d(L), stream, expect=("lzss_dec_run_fill",), unless=("RSN_LZSS_DEC_NO_RUN_TAIL",), small=P == 4096)
        assert len(want) >= 1 << 20 and (len(want) - reps * P - head) in (0, 2, 4, 8, 14), len(want)


def test_lzss_decode_general_path_and_zero_length_tokens(L, oracle):
    data = text(41, 70000)
    far = oracle.lzss_compress(data, 0)                                   # pointers beyond a tile: whole-stream pointer jumping
    assert matrix(oracle, lzss_d(L), far, expect=("lzss_dec_expand", "lzss_dec_jump", "lzss_dec_gather")) == data
    zero = b"abcdefgh" * 40 + b"<8,0>" * 6000 + b"xyz" * 9000 + b"<16000,27>" + b"<3,3>"
    # no pointer reaches beyond a tile, so the tile path runs; 30 KB of tokens that produce nothing do not fit a tile's input: the
    # emit kernel has written d_out when that turns out, and the general path then does the stream again
    matrix(oracle, lzss_d(L), zero, expect=("lzss_dec_emit", "lzss_dec_jump"))
    matrix(oracle, lzss_d(L), zero + b"\\\\" + b"<8,0>" * 5000 + b"q", expect=("lzss_dec_emit", "lzss_dec_jump", "lzss_une_write"))


def test_empty_inputs(L, oracle):
    """LZSS of nothing is nothing (CompressAsync(empty) == empty): RSN_OK and size 0, the size query included -- there is nothing to
    size (rsn.h); so is a chain of no layers.  Huffman of nothing is RSN_ERR_EMPTY, and nothing is not a Huffman stream."""
    assert oracle.lzss_compress(b"") == b"" == oracle.lzss_decompress(b"")
    src, d_in, chk_in = fenced(16)
    for op, code in ((lzss_c(L), OK), (lzss_c(L, 0), OK), (lzss_d(L), OK), (layers_c(L, ()), OK), (layers_d(L, ()), OK), (layers_c(L, (LZSS,)), OK),
                     (layers_d(L, (LZSS,)), OK), (huff_c(L), E_EMPTY), (huff_d(L), E_FORMAT), (layers_c(L, (LZSS, HUFF)), E_EMPTY)):
        out, d_out, chk_out = fenced(64)
        for dst, cap in ((d_out, 64), (d_out, 16), (None, 0)):
            rc, got = op.call(d_in, 0, dst, cap)
            assert (rc, got) == (code, 0), (op.name, cap, rc, got)
        chk_out(op.name), chk_in(op.name)


# ------------------------------------------------------------------------------------------------ layered calls
@pytest.mark.parametrize("ids", [(LZSS, HUFF), (HUFF, LZSS), (LZSS,), (HUFF,), ()])
def test_layers(L, oracle, ids):
    """rsn_layers_compress_dev / rsn_layers_decompress_dev: the same matrix; the stream between two layers lives in scratch."""
    for data in (plain_text(91, 150007), text(92, 40000), skewed_bytes(70001)):
        comp = matrix(oracle, layers_c(L, ids), data)
        back = matrix(oracle, layers_d(L, ids), comp)
        if HUFF not in ids:
            assert back == data
    base = plain_text(93, 5200)
    sizes = _residue_lengths(lambda n: base[:n], lambda d: len(layers_c(L, ids).want(oracle, d)), 5000, span=200)
    for r, n in sorted(sizes.items()):
        comp = matrix(oracle, layers_c(L, ids), base[:n], small=False)
        assert len(comp) % 16 == r
    for r in RESIDUES:
        data = base[:5100 + r]
        back = matrix(oracle, layers_d(L, ids), layers_c(L, ids).want(oracle, data), small=False)
        assert back == data or HUFF in ids                                # (the Huffman layer turns the stream's FF bytes, once '<', into U+FFFD)


# ------------------------------------------------------------------------------------------------ hostile streams
def _verdict(fn, stream):
    from oracle.oracle import OracleError
    try:
        return fn(stream)
    except OracleError:
        return None


def hostile(O, op, stream, prefix_E, allow=None, room=0):
    """A damaged stream between fences, at the capacity its well-formed part would need, at 4096 and at a generous one.  The
    oracle's verdict decides: bytes -> the library returns them (or asks for room and then returns them); an error -> the library
    returns an error code whatever the capacity, and at the generous one a verdict on the stream (FORMAT, LIMIT or EMPTY), not a
    request for room.  allow: the one documented refusal this stream may meet where the oracle accepts.  room: what the stream
    would expand to were its damage ignored, where that is more than its well-formed part -- the generous capacity covers it."""
    want = _verdict(lambda s: op.want(O, s), stream)
    n = len(stream)
    src, d_in, chk_in = fenced(n, stream)
    generous = _ru16(max(len(want) if want is not None else 0, prefix_E, room)) + 65536
    for cap in sorted({max(prefix_E, 16), 4096, generous}):
        tag = "%s, hostile stream of %d bytes, capacity %d" % (op.name, n, cap)
        out, d_out, chk_out = fenced(cap)
        rc, got = op.call(d_in, n, d_out, cap)
        chk_out(tag + ": the output buffer")
        chk_in(tag + ": the input")
        if want is None:
            assert rc != OK, tag + ": the oracle refuses this stream"
            if cap == generous:
                assert rc in (E_FORMAT, E_LIMIT, E_EMPTY), (tag, rc, got)
            continue
        if allow and rc == (E_LIMIT if allow == DEEP else E_FORMAT):
            continue                                                      # refusing is only allowed where documented
        if len(want) > cap:
            assert rc == E_CAP and got >= len(want), (tag, rc, got, len(want))
            out, d_out, chk_out = fenced(got)
            rc, got = op.call(d_in, n, d_out, got)
            chk_out(tag + ": the output buffer of the size the refusal named")
            chk_in(tag + ": the input")
        assert rc == OK and got == len(want), (tag, rc, got, len(want))
        assert _bytes(out, got) == want, tag + ": not the oracle's bytes"
    return want


def test_hostile_lzss_pointer_before_the_data(L, oracle):
    lit = rnd(1, (1 << 20) + 70000, bytes(range(97, 123)))
    for k in (1 << 20, (1 << 20) + 3 * 16384 + 5000):                     # at a 4 KiB block edge (and a tile's); inside a tile
        stream = lit[:k] + b"<%d,5>" % (k + 1) + lit[k:k + 1000]
        assert hostile(oracle, lzss_d(L), stream, k) is None
        stream = lit[:k] + b"<%d,5>" % k + lit[k:k + 1000]                # the farthest pointer that is still inside
        assert hostile(oracle, lzss_d(L), stream, k) is not None
    comp = oracle.lzss_compress(plain_text(7, 1 << 20))                  # (nothing escaped: a position of the output is one of the escaped stream)
    assert hostile(oracle, lzss_d(L), comp + b"<%d,9>" % ((1 << 20) + 1) + b"tail", 1 << 20) is None


def test_hostile_lzss_doubling_chains_and_token_runs(L, oracle):
    chain = b"a" * 16 + b"".join(b"<%d,%d>" % (16 << k, 16 << k) for k in range(18))   # 4 MiB out of 200 bytes
    assert len(hostile(oracle, lzss_d(L), chain, 16)) == 16 << 18
    assert hostile(oracle, lzss_d(L), chain + b"<%d,1>" % ((16 << 18) + 1), 16, room=(16 << 18) + 1) is None
    for lead in (100, 255):                                               # a token run whose first token points before the data
        stream = rnd(lead, lead, bytes(range(97, 123))) + b"<256,256>" * 7300   # (64 KiB of stream, 1.8 MiB of output: the run tail's sizes)
        assert hostile(oracle, lzss_d(L), stream, lead, room=lead + 7300 * 256) is None
    ok = rnd(5, 70000, bytes(range(97, 123))) + b"<4096,4096>" * 300
    assert hostile(oracle, lzss_d(L), ok + b"<8000000,2>", 70000 + 300 * 4096) is None   # the run's last item points before the data


def test_hostile_lzss_cut_tokens_and_long_numbers(L, oracle):
    base = plain_text(3, 30000)
    comp = oracle.lzss_compress(base)
    for tail in (b"<12", b"<12,", b"<12,3", b"<"):
        hostile(oracle, lzss_d(L), comp + tail, len(base), allow=LOOSE)
        hostile(oracle, lzss_d(L), base[:100] + tail, 100, allow=LOOSE)
    for stream in (comp + b"\\", rnd(4, 4095, bytes(range(97, 123))) + b"\\", b"\\", comp + b"\\\\" + b"\\"):   # a dangling escape as the last byte
        hostile(oracle, lzss_d(L), stream, len(base))
    for tok in (b"<0000000003,0000000003>", b"<4294967295,1>", b"<4294967296,1>", b"<9999999999,1>", b"<3,9999999999>",
                b"<3,4294967295>", b"<0000030000,0000030000>"):
        hostile(oracle, lzss_d(L), comp + tok + b"!", len(base))
        hostile(oracle, lzss_d(L), comp + tok * 40, len(base))
    for tok in (b"<00000000003,1>", b"<3,00000000001>"):                  # eleven digits
        hostile(oracle, lzss_d(L), comp + tok + b"!", len(base), allow=LOOSE)


@pytest.mark.parametrize("seed", range(12))
def test_hostile_lzss_token_streams(L, oracle, seed):
    rng = random.Random(5000 + seed)
    for _ in range(3):
        max_ptr = rng.choice((3, 40, 4096, 9000, 16384, 40000, 1 << 30))
        stream, loose = _token_stream(rng, rng.choice((60, 800, 6000)), max_ptr=max_ptr, bad=0.02)
        hostile(oracle, lzss_d(L), stream, len(stream), allow=LOOSE if loose else None)


def _huffman_bases(oracle):
    counts = LC.tree("ascii", 33)
    pick, cs = LC.picker(counts)
    deep = LC.tree("runes", 64)
    pick64, cs64 = LC.picker(deep)
    return [("flat", oracle.huffman_compress(flat_bytes(7, 5003)), None),
            ("general", oracle.huffman_compress(skewed_bytes(100001)), None),
            ("runes", oracle.huffman_compress(rune_bytes(30000)), None),
            ("codes of 33 bits", LC.block_stream(counts, pick, 1 << 15, seed=1, cs=cs)[0], None),
            ("codes of 64 bits", LC.block_stream(deep, pick64, 1 << 14, seed=2, cs=cs64)[0], DEEP),
            ("no self-synchronisation", oracle.huffman_compress(no_sync_bytes(60001)), None),
            ("bare leaf", oracle.huffman_compress(b"aaaa"), None)]


def _with_header(oracle, stream, edit):
    """The stream with its header's (count, symbol) entries passed through `edit`; a '\\' entry is never left last."""
    ents, rest = oracle.header_entries(stream)
    ents = list(edit(list(ents)))
    if len(ents) > 1 and ents[-1][1] == b"\\":
        ents.insert(0, ents.pop())
    return b"".join(f + b"|" + s for f, s in ents) + b"\\\n" + rest


@pytest.mark.parametrize("which", range(7))
def test_hostile_huffman(L, oracle, which):
    """Valid streams of every decode path, damaged: the counts only shape the tree (huffman.go:196-227), so the oracle decodes
    most of these to something -- and the library to the same bytes."""
    name, base, allow = _huffman_bases(oracle)[which]
    E0 = len(oracle.huffman_decompress(base))
    op = huff_d(L)
    rng = random.Random(which)
    sep = base.index(b"\\\n")
    # header counts multiplied or saturated: the header announces more, or less, than the payload holds
    hostile(oracle, op, _with_header(oracle, base, lambda e: [(b"%d" % (int(f) * 1000), s) for f, s in e]), E0, allow)
    hostile(oracle, op, _with_header(oracle, base, lambda e: [(b"%d" % max(1, int(f) // 3), s) for f, s in e]), E0, allow)
    hostile(oracle, op, _with_header(oracle, base, lambda e: [(b"18446744073709551615", e[0][1])] + e[1:]), E0, allow)
    hostile(oracle, op, _with_header(oracle, base, lambda e: e[:-1] + [(b"18446744073709551615", e[-1][1])]), E0, allow)
    hostile(oracle, op, _with_header(oracle, base, lambda e: [(b"18446744073709551615", s) for f, s in e]), E0, allow)
    for _ in range(2):                                                    # the entries permuted
        hostile(oracle, op, _with_header(oracle, base, lambda e: rng.sample(e, len(e))), E0, allow)
    if len(base) > sep + 3:
        pad = base[sep + 2]
        for extra in (1, 2):                                              # the pad byte raised by 8 and 16, zero bytes inserted
            hostile(oracle, op, base[:sep + 2] + bytes([pad + 8 * extra]) + b"\0" * extra + base[sep + 3:], E0, allow)
            hostile(oracle, op, base[:sep + 2] + bytes([pad + 8 * extra]) + base[sep + 3:], E0, allow)   # ... and not inserted
        for cut in range(1, min(20, len(base) - sep - 3) + 1):            # the payload cut at every one of its last 20 bytes
            hostile(oracle, op, base[:len(base) - cut], E0, allow)
        for _ in range(12):                                               # one bit of the payload flipped
            pos = rng.randrange(sep + 3, len(base))
            hostile(oracle, op, base[:pos] + bytes([base[pos] ^ (1 << rng.randrange(8))]) + base[pos + 1:], E0, allow)
        for _ in range(3):                                                # random payload bytes behind a valid header
            hostile(oracle, op, base[:sep + 3] + rng.randbytes(len(base) - sep - 3), E0, allow)
    else:
        hostile(oracle, op, base + b"\x80", E0, allow)                    # a bare leaf with a payload
    hostile(oracle, op, base[:sep], E0, allow)                            # no separator
    hostile(oracle, op, base[:sep + 2], E0, allow)                        # nothing behind it


def test_hostile_streams_through_the_layered_call(L, oracle):
    data = plain_text(17, 60000)
    good = oracle.huffman_compress(oracle.lzss_compress(data))
    op = layers_d(L, (LZSS, HUFF))
    assert hostile(oracle, op, good, len(data)) is not None
    for cut in (1, 2, 7):
        hostile(oracle, op, good[:-cut], len(data), allow=LOOSE)
    bad_inner = oracle.huffman_compress(oracle.lzss_compress(data) + b"<70000,3>")
    assert hostile(oracle, op, bad_inner, len(data)) is None


# ------------------------------------------------------------------------------------------------ slack: only n bytes are data
def slack(O, op, data, before, after, allow=None):
    """One call on an input whose neighbours are `before` / `after` (repeated over the whole fence): the oracle sees the n bytes
    alone, and the library's answer must be the oracle's."""
    want = _verdict(lambda s: op.want(O, s), data)
    n = len(data)
    src, d_in, chk_in = fenced(n, data, before, after)
    cap = _ru16(len(want) if want is not None else 4 * n) + 64
    out, d_out, chk_out = fenced(cap)
    rc, got = op.call(d_in, n, d_out, cap)
    tag = "%s on %d bytes with %r... behind them" % (op.name, n, after[:8])
    chk_out(tag + ": the output buffer")
    chk_in(tag + ": the input")
    if want is None:
        assert rc != OK, tag + ": the oracle refuses these n bytes"
    elif not (allow and rc == E_FORMAT):
        assert rc == OK and _bytes(out, got) == want, (tag, rc, got, len(want))
    return want


@pytest.mark.parametrize("r", [0, 1, 15])
def test_slack_lzss_decode(L, oracle, r):
    for n0 in (4096, 70000):
        lit = rnd(n0, n0 + r, bytes(range(97, 123)))
        assert slack(oracle, lzss_d(L), lit, b"<1,1>", b"<1,1>") == lit             # ends in literals; tokens lie behind it
        comp = oracle.lzss_compress(plain_text(n0, 3 * n0))
        pad = rnd(1, (r - len(comp)) % 16, b"xyz")
        slack(oracle, lzss_d(L), comp + pad, b"<1,1>", b"<1,1>")
        # the token's end lies behind the input.  (The reference drops a token that the stream cuts short -- the oracle returns the
        # bytes before it -- and this library refuses the spelling, DESIGN 7: those are the two answers; three more bytes are not.)
        cut = lit[:len(lit) - 5] + b"ab<12"
        assert slack(oracle, lzss_d(L), cut, b",3>", b",3>", allow=LOOSE) == cut[:-3]
        esc = lit[:len(lit) - 1] + b"\\"                                           # ... and so does the escaped byte
        slack(oracle, lzss_d(L), esc, b"\\", b"\\")
        slack(oracle, lzss_d(L), esc, b"\xff", b"\xff")


@pytest.mark.parametrize("r", [0, 1, 15])
def test_slack_lzss_encode(L, oracle, r):
    """The neighbours continue the input's own period on both sides: a match, a run or a periodic tail that looked past n -- or
    a candidate at a negative distance -- would find what it is looking for."""
    for period, w, n0 in ((4096, 4096, 4096 * 40), (37, 4096, 11104), (1000, 1000, 30000), (1, 4096, 70000), (5000, 8193, 5000 * 2 + 600)):
        blk = rnd(period, period, PLAIN)
        n = n0 + r
        data = _tiled(blk, n)
        after = _tiled(blk, 2 * period + n)[n:n + period * 2]             # in phase with the input's end
        before = blk
        slack(oracle, lzss_c(L, w), data, before, after)
    data = text(3, 20000 + r)
    for w in (4096, 0):
        slack(oracle, lzss_c(L, w), data, data, data[-300:])


@pytest.mark.parametrize("r", [0, 1, 15])
def test_slack_huffman_encode(L, oracle, r):
    for n0 in (4096, 65536, 200000):
        n = n0 + r
        cut = ("€" * (n // 3 + 1)).encode()[:n - 2 - (n - 2) % 3] + b"\xe2\x82"   # ends in a truncated rune; AC lies behind it
        cut = b"a" * (n - len(cut)) + cut
        assert len(cut) == n
        slack(oracle, huff_c(L), cut, b"\xac", b"\xac")
        slack(oracle, huff_c(L), cut, b"\xe2\x82\xac", b"\xac\xe2\x82")
        ascii_only = skewed_bytes(n, seed=r)                              # the ascii / rune classification must not flip
        slack(oracle, huff_c(L), ascii_only, b"\xe2\x82\xac", b"\xe2\x82\xac")
        slack(oracle, huff_c(L), flat_bytes(7, n), b"\xff", b"\xff")


def test_slack_huffman_decode(L, oracle):
    """All ones and all zeros behind the last payload byte: the bit reader's last words."""
    counts = LC.tree("ascii", 40)
    pick, cs = LC.picker(counts)
    makers = {"general": lambda n: oracle.huffman_compress(skewed_bytes(n)), "flat": lambda n: oracle.huffman_compress(flat_bytes(7, n)),
              "runes": lambda n: oracle.huffman_compress(rune_bytes(n)), "no self-synchronisation": lambda n: oracle.huffman_compress(no_sync_bytes(n))}
    for name, make in makers.items():
        found = {}
        for n in range(50000, 50400):
            s = make(n)
            if len(s) % 16 in (0, 1, 15) and len(s) % 16 not in found:
                found[len(s) % 16] = s
            if len(found) == 3:
                break
        assert len(found) == 3, name
        for s in found.values():
            a = slack(oracle, huff_d(L), s, b"\xff", b"\xff")
            b = slack(oracle, huff_d(L), s, b"\x00", b"\x00")
            assert a == b and a is not None
    for seed in range(3):
        s = LC.block_stream(counts, pick, (1 << 14) + seed, seed=seed, cs=cs)[0]
        assert slack(oracle, huff_d(L), s, b"\xff", b"\xff") == slack(oracle, huff_d(L), s, b"\x00", b"\x00")


@pytest.mark.parametrize("n", [13, 1024, 65535, 65536, 65537, 1 << 20])
def test_host_calls_read_their_slice_only(L, oracle, n):
    """The four host-buffer single calls on a slice in the middle of a larger buffer (the one-launch paths read pinned host
    memory in place): hostile neighbours on both sides, the oracle sees the slice alone."""
    u8p = ctypes.POINTER(ctypes.c_uint8)

    def host_call(fn, data, before, after, *extra):
        whole = _tiled(before, 4096, right=True) + data + _tiled(after, 4096)
        buf = ctypes.create_string_buffer(whole, len(whole))
        at = ctypes.cast(ctypes.addressof(buf) + 4096, ctypes.c_char_p)
        out, k = u8p(), ctypes.c_size_t(0)
        rc = fn(at, len(data), *extra, ctypes.byref(out), ctypes.byref(k))
        assert buf.raw == whole                                           # the input is borrowed, never modified
        if rc != OK:
            return None
        try:
            return ctypes.string_at(out, k.value)
        finally:
            L.rsn_free(out)

    blk = rnd(n, 37, PLAIN)
    periodic = _tiled(blk, n)
    cut = (b"a" * n + b"\xe2\x82")[-n:]
    txt = text(n, n)
    for data, before, after in ((periodic, blk, _tiled(blk, n + 74)[n:]), (txt, txt[-64:] or b"x", txt[:64]), (cut, b"\xe2\x82\xac", b"\xac")):
        assert host_call(L.rsn_lzss_compress, data, before, after, 4096) == oracle.lzss_compress(data, 4096), n
        assert host_call(L.rsn_huffman_compress, data, before, after) == oracle.huffman_compress(data), n
    for data in (periodic, txt, skewed_bytes(n)):
        lz_stream, hf_stream = oracle.lzss_compress(data), oracle.huffman_compress(data)
        for hostile_bytes in (b"<1,1>", b"\\", b"\xff", b"\x00"):
            assert host_call(L.rsn_lzss_decompress, lz_stream, hostile_bytes, hostile_bytes) == oracle.lzss_decompress(lz_stream), n
            assert host_call(L.rsn_huffman_decompress, hf_stream, hostile_bytes, hostile_bytes) == oracle.huffman_decompress(hf_stream), n
    if n >= 16:
        cut_tok = periodic[:n - 5] + b"ab<12"                              # ",3>" behind it must not complete the token
        assert host_call(L.rsn_lzss_decompress, cut_tok, b",3>", b",3>") in (None, oracle.lzss_decompress(cut_tok)), n


# ------------------------------------------------------------------------------------------------ the host calls' retry
def test_host_calls_retry_when_the_first_buffer_is_too_small(L, oracle):
    """A quarter of a million runes used once each: the stream outgrows the n + n / 8 + 64 KiB the host calls allocate first
    (test_bounds_host.py checks that on the CPU), so host_call -- and a layered call's layer_cap -- take their retry."""
    from raisin_amd import _lib
    n = 1 << 20
    data = _distinct_runes(n, "wide")
    want = oracle.huffman_compress(data)
    assert len(want) > n + n // 8 + 65536
    assert _lib.call_host(L.rsn_huffman_compress, data) == want
    for ids in ((HUFF,), (HUFF, LZSS)):
        arr, k = _layer_ids(ids)
        assert _lib.call_host(L.rsn_layers_compress, data, arr, k) == layers_c(L, ids).want(oracle, data), ids
    matrix(oracle, huff_c(L), data, expect=("huff_emit_rune",), small=False)


# ------------------------------------------------------------------------------------------------ argument refusals
def _all_ops(L):
    return [huff_c(L), huff_d(L), lzss_c(L), lzss_d(L)] + [f(L, ids) for f in (layers_c, layers_d) for ids in ((LZSS, HUFF), (HUFF,), (LZSS,), ())]


def test_misaligned_and_overlapping_buffers_are_refused(L, oracle):
    """Both device buffers must be 16-byte aligned and must not overlap: RSN_ERR_ARG before a byte is touched."""
    import torch
    data = plain_text(1, 4096)
    for op in _all_ops(L):
        src, d_in, chk_in = fenced(8192, data + data)
        out, d_out, chk_out = fenced(16384)
        was = out.clone()
        for off_in, off_out in ((1, 0), (8, 0), (0, 1), (0, 8), (8, 8)):
            rc, _ = op.call(d_in + off_in, 4096, d_out + off_out, 8192)
            assert rc == E_ARG, (op.name, off_in, off_out, rc)
        rc, _ = op.call(d_in + 1, 4096, None, 0)                          # the size query reads the input too
        assert rc == E_ARG, (op.name, "size query", rc)
        chk_in(op.name), chk_out(op.name)
        assert torch.equal(out, was), op.name
        # d_out inside [d_in, d_in + n), and d_in inside [d_out, d_out + out_cap)
        both, p, chk = fenced(16384, data * 4)
        was = both.clone()
        for a, na, b, nb in ((p, 4096, p + 2048, 8192), (p + 2048, 4096, p, 8192), (p, 8192, p + 8176, 16), (p + 4080, 4096, p, 4096 + 16)):
            rc, _ = op.call(a, na, b, nb)
            assert rc == E_ARG, (op.name, a - p, na, b - p, nb, rc)
        chk(op.name)
        assert torch.equal(both, was), op.name
