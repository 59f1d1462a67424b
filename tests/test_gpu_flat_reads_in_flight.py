"""The flat Huffman encoder's block in two barriers (k_emit_flat): the words of a chunk go to LDS unshifted behind the word in front of
the chunk, and the drain shifts two neighbouring words by the stream's phase o0 = base_bits % 32.  The word in front of a chunk is
rebuilt by one lane from the last 32 - floor(32 (L - 1) / L) symbols of the chunk before (5, 6, 7, 8, 11, 16, 32 for L = 7 .. 1), loaded
as 8, 16 or 32 bytes with the chunk's own loads; nothing is loaded in front of the first chunk or at phase 0.  Both kernels take one
chunk a block with no loop.  Through compress_tensor and decompress_tensor, byte for byte against the CPU oracle, and back.

Every input is flat by construction -- each of the 2**L symbols floor(n / 2**L) or ceil(n / 2**L) times -- and every case asserts the
payload of exactly ceil(L * n / 8) bytes that a flat code gives, so an input that is not flat fails and takes no other path.
Expected bytes are the oracle's, computed once per input and shared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHUNK = 8192
WIDTHS = (1, 2, 3, 4, 5, 6, 7)
LOOK_BACK_SIZES = [CHUNK * m + r for m in (1, 2, 3) for r in (0, 1, 31, 32, 33)]
# L = 7 only: the sizes above give headers of 4 k bytes, phases 0 .. 7.  With 99 * 128 + r symbols, r of the 128 counts are 100 and
# the others 99, so the header grows by a byte with every r: all four header lengths mod 4, the pad byte from 1 to 7 (counted on the
# CPU, see test_phases_that_the_look_back_cases_reach)
EXTRA_7 = [99 * 128 + r for r in range(1, 9)]
_cases = {}


def symbols_of(Lbits):
    k = 1 << Lbits
    lo = 0 if k == 128 else 40
    return np.arange(lo, lo + k, dtype=np.uint8)


def multiset(Lbits, n):
    """n bytes over 2**Lbits symbols, each floor(n / 2**Lbits) or ceil(n / 2**Lbits) times, in a seeded order."""
    syms = symbols_of(Lbits)
    rng = np.random.default_rng(Lbits * 7919 + n)
    buf = np.concatenate([np.tile(syms, n // syms.size), rng.permutation(syms)[:n % syms.size]])
    rng.shuffle(buf)
    return buf


def expect(oracle, key, data, Lbits):
    """(input, the oracle's stream, o0) of one case; asserts the flat code's payload length."""
    if key not in _cases:
        n = len(data)
        want = oracle.huffman_compress(data)
        pay = (Lbits * n + 7) // 8
        H = len(want) - pay
        assert H >= 3 and want[H - 3:H - 1] == b"\\\n", (key, "not a flat payload")
        pad = want[H - 1]
        assert pad == (-Lbits * n) % 8, (key, "not a flat payload", pad)
        _cases[key] = (data, want, (8 * H + pad) % 32)
    return _cases[key]


def look_back_case(oracle, Lbits, n, ones):
    """The multiset of (Lbits, n) with the 32 symbols in front of every chunk boundary set to the symbol whose code is all ones (or all
    zeros).  The code is the oracle's for this histogram; the order of the bytes does not change the tree."""
    key = ("lb", Lbits, n, ones)
    if key in _cases:
        return _cases[key]
    buf = multiset(Lbits, n)
    code = (1 << Lbits) - 1 if ones else 0
    sym = [r for r, _, c, ln in oracle.huffman_table(buf.tobytes()) if c == code and ln == Lbits]
    assert len(sym) == 1, (Lbits, n, "no symbol with that code")
    sym = sym[0]
    at = np.concatenate([np.arange(b - 32, b) for b in range(CHUNK, n + 1, CHUNK)])
    mine = np.flatnonzero(buf == sym)
    assert mine.size >= at.size
    # swap: the chosen symbol's first occurrences trade places with whatever stands at the boundary positions
    out = buf.copy()
    others = buf[at][buf[at] != sym]                       # the bytes that leave the boundary positions
    free = np.setdiff1d(mine, at)[:others.size]            # occurrences of the symbol elsewhere that take their place
    out[at] = sym
    out[free] = others
    assert np.array_equal(np.bincount(out, minlength=256), np.bincount(buf, minlength=256))
    assert (out[at] == sym).all()
    return expect(oracle, key, out.tobytes(), Lbits)


def rotated_case(oracle, Lbits):
    """Two chunks in which byte i is symbol (i + i // 32) % 2**L: every lane's 32 symbols are a run that starts one symbol later than
    the lane's before, so every symbol meets every lane position mod 32 and every table copy."""
    syms = symbols_of(Lbits)
    i = np.arange(2 * CHUNK)
    data = syms[(i + i // 32) % syms.size]
    for r in range(32):                                     # lanes r, r + 32, ...: their symbols together are the alphabet
        lanes = data.reshape(-1, 32)[r::32]
        assert np.unique(lanes).size == syms.size
    return expect(oracle, ("rot", Lbits), data.tobytes(), Lbits)


@pytest.fixture(scope="module")
def dev():
    import torch
    from raisin_amd import _lib, huffman
    _lib.check(_lib.lib().rsn_device_set(0))

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()

    def down(t):
        return bytes(t.cpu().numpy())
    return huffman, up, down


def round_trip(dev, data, want, tag):
    huffman, up, down = dev
    assert down(huffman.compress_tensor(up(data))) == want, (tag, "the stream is not the oracle's")
    assert down(huffman.decompress_tensor(up(want))) == data, (tag, "the decode is not the input")


def sizes_of(Lbits):
    return LOOK_BACK_SIZES + (EXTRA_7 if Lbits == 7 else [])


def test_phases_that_the_look_back_cases_reach(oracle):
    """On the CPU: the L = 7 cases reach phase 0 (no look-back at all) and a phase of 25 or more (the look-back's bits reach from the
    symbol that straddles into the word in front of the chunk)."""
    phases = {look_back_case(oracle, 7, n, ones)[2] for n in sizes_of(7) for ones in (True, False)}
    assert 0 in phases, sorted(phases)
    assert max(phases) >= 25, sorted(phases)


@pytest.mark.parametrize("Lbits", WIDTHS)
def test_narrowed_look_back(dev, oracle, Lbits):
    """One, two and three chunks with a tail of 0, 1, 31, 32 and 33 symbols; the 32 symbols in front of every chunk boundary carry the
    all-ones code in one variant and the all-zeros code in the other: a look-back that takes too few bytes, or the wrong ones, changes
    the first word of the chunk behind the boundary."""
    for n in sizes_of(Lbits):
        for ones in (True, False):
            data, want, o0 = look_back_case(oracle, Lbits, n, ones)
            assert oracle.huffman_decompress(want) == data
            round_trip(dev, data, want, (Lbits, n, ones, o0))


@pytest.mark.parametrize("Lbits", WIDTHS)
def test_every_symbol_at_every_lane_position(dev, oracle, Lbits):
    data, want, o0 = rotated_case(oracle, Lbits)
    round_trip(dev, data, want, (Lbits, o0))


@pytest.mark.parametrize("Lbits", (7, 3))
def test_sharded_slices_at_other_phases(oracle, Lbits):
    """Three slices of five chunks and a ragged tail: the later slices start at bit phases that the header alone does not give and
    write no header bytes; chunks inside a slice look back across a boundary at that phase."""
    from raisin_amd import huffman
    n = 5 * CHUNK + 33
    data, want, _ = expect(oracle, ("shard", Lbits), multiset(Lbits, n).tobytes(), Lbits)
    assert huffman.CompressSharded(data, 3) == want
    assert huffman.Decompress(want) == data
