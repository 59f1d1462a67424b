"""The flat Huffman kernels (k_emit_flat, k_dec_flat) at the edges of a wavefront's and a block's share of the stream: a lane takes 32
symbols, a wavefront 2048 (a unit: the last word of its last lane crosses to the next wavefront), a block a chunk of 8192 (four units:
the word in front of it is recomputed from the input), and the chunk that holds the stream's first or last word, or whose loads would
pass the end of the input, takes the careful path.  Through the device-buffer calls, because the host-buffer calls send inputs this
small to the one-launch kernels of huff_small.hip.

Every input is flat by construction -- each of the 2**L symbols floor(n / 2**L) or ceil(n / 2**L) times, shuffled by a seeded generator
-- and every case asserts the payload of exactly ceil(L * n / 8) bytes that a flat code gives, so an input that is not flat fails.
Expected bytes are the CPU oracle's, computed once per (L, n) and shared."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

UNIT, SPAN = 2048, 8192
WIDTHS = (1, 2, 3, 4, 5, 6, 7)
EDGES = ([2047, 2048, 2049]
         + [UNIT * k + d for k in (2, 3, 4) for d in (-1, 1, 31, 32, 33)]
         + [8191, 8192, 8193, SPAN + UNIT + 5, 3 * SPAN + 31, 3 * SPAN + 33]
         + [5 * SPAN + r for r in range(1, 34)])
# distinct bit phases o0 = (8 * H + pad) % 32 of the first code bit (H: the bytes in front of the payload, pad: the pad byte's value)
# that the sweep n = k * 2**L + r, k in {9, 99, 999}, r in 0 .. 2**L + 7 reaches: counted on the CPU with the oracle
PHASES_FLOOR = {1: 19, 2: 7, 3: 14, 4: 5, 5: 14, 6: 7, 7: 14}
ZERO_PHASE = (7,)                    # the widths of that sweep that reach o0 == 0 (L = 7: 51 of its cases, the first n = 1152 with H = 388 and pad 0)
_cases = {}


def flat_exact(Lbits, n):
    """n bytes over 2**Lbits symbols, each floor(n / 2**Lbits) or ceil(n / 2**Lbits) times, in a seeded order."""
    k = 1 << Lbits
    assert n >= 2 * k
    lo = 0 if k == 128 else 40
    rng = np.random.default_rng(Lbits * 1000003 + n)
    syms = np.arange(lo, lo + k, dtype=np.uint8)
    buf = np.concatenate([np.tile(syms, n // k), rng.permutation(syms)[:n % k]])
    rng.shuffle(buf)
    assert buf.size == n
    return buf.tobytes()


def case(oracle, Lbits, n):
    """(input, the oracle's stream, H, o0) of one case; asserts the flat code's payload length."""
    key = (Lbits, n)
    if key not in _cases:
        data = flat_exact(Lbits, n)
        want = oracle.huffman_compress(data)
        pay = (Lbits * n + 7) // 8
        H = len(want) - pay
        assert H >= 3 and want[H - 3:H - 1] == b"\\\n", (Lbits, n, "not a flat payload")
        pad = want[H - 1]
        assert pad == (-Lbits * n) % 8, (Lbits, n, "not a flat payload", pad)
        _cases[key] = (data, want, H, (8 * H + pad) % 32)
    return _cases[key]


def sweep_sizes(Lbits):
    return [k * (1 << Lbits) + r for k in (9, 99, 999) for r in range((1 << Lbits) + 8)]


@pytest.fixture(scope="module")
def dev():
    import torch
    from raisin_amd import _lib, huffman
    _lib.check(_lib.lib().rsn_device_set(0))

    def up(b):
        return torch.frombuffer(bytearray(b), dtype=torch.uint8).cuda()

    def down(t):
        return bytes(t.cpu().numpy())
    return torch, _lib, huffman, up, down


def round_trip(dev, data, want, tag):
    torch, _lib, huffman, up, down = dev
    c = huffman.compress_tensor(up(data))
    assert down(c) == want, (tag, "the stream is not the oracle's")
    assert down(huffman.decompress_tensor(up(want))) == data, (tag, "the decode is not the input")


def test_oracle_decodes_its_own_flat_streams(oracle):
    """The reference side of the file, without a kernel: a few cases of every width decode to their input on the CPU."""
    for Lbits in WIDTHS:
        for n in (2047, 5 * SPAN + 33, 9 * (1 << Lbits)):
            data, want, _, _ = case(oracle, Lbits, n)
            assert oracle.huffman_decompress(want) == data


@pytest.mark.parametrize("Lbits", WIDTHS)
def test_unit_and_span_edges(dev, oracle, Lbits):
    """One symbol short of a unit, a unit and one past it; the same around two, three and four units with the ragged tail before, on and
    behind a lane's 32 symbols; around a chunk; a chunk, a unit and five symbols; three chunks and a ragged lane; and five chunks with
    the tail at every place inside the last lane's group."""
    for n in EDGES:
        data, want, _, _ = case(oracle, Lbits, n)
        round_trip(dev, data, want, (Lbits, n))


@pytest.mark.parametrize("Lbits", WIDTHS)
def test_every_bit_phase_of_the_first_code_bit(dev, oracle, Lbits):
    """The header's length and the pad byte move the bit phase of the payload, the funnel shift of every lane: the sweep reaches at
    least the phases counted on the CPU, phase 0 (no shift, no bits from the word in front) among them where it occurs."""
    phases = set()
    for n in sweep_sizes(Lbits):
        data, want, _, o0 = case(oracle, Lbits, n)
        phases.add(o0)
        round_trip(dev, data, want, (Lbits, n, o0))
    assert len(phases) >= PHASES_FLOOR[Lbits], (Lbits, sorted(phases))
    if Lbits in ZERO_PHASE:
        assert 0 in phases, (Lbits, sorted(phases))


def test_the_flat_kernels_are_what_ran(dev, oracle):
    """The device-buffer calls send even a unit and a half to k_emit_flat and k_dec_flat (unless RSN_NO_FLAT switches them off)."""
    import os
    torch, _lib, huffman, up, down = dev
    data, want, _, _ = case(oracle, 7, UNIT + 1000)
    _lib.prof_enable(True)
    _lib.prof_reset()
    try:
        round_trip(dev, data, want, "profiled")
        ran = {k for k, (n, _) in _lib.prof_get().items() if n}
    finally:
        _lib.prof_enable(False)
    if not os.environ.get("RSN_NO_FLAT"):
        assert {"huff_emit", "huff_dec_flat"} <= ran, sorted(ran)


@pytest.mark.parametrize("Lbits,n", [(7, 5 * SPAN + 17), (7, 4 * UNIT), (3, 3 * SPAN + 33), (1, 2 * UNIT + 31)])
def test_out_cap_exactly_what_the_size_query_names(dev, oracle, Lbits, n):
    """Both directions into a buffer of exactly the size the size query names, with seeded bytes behind it that must not change: the
    last chunk's stores end with the buffer."""
    torch, _lib, huffman, up, down = dev
    data, want, _, _ = case(oracle, Lbits, n)
    lib = _lib.lib()
    for fn, src, expect in ((lib.rsn_huffman_compress_dev, data, want), (lib.rsn_huffman_decompress_dev, want, data)):
        d_src = up(src)
        try:
            need = _lib.call_dev(fn, d_src.data_ptr(), len(src), None, 0, _lib.own_stream(d_src))
        except _lib.RsnError as e:
            assert e.code == _lib.RSN_ERR_CAPACITY
            need = e.needed
        assert need >= len(expect)
        whole = torch.randint(0, 256, (need + 4096,), dtype=torch.uint8, generator=torch.Generator().manual_seed(n)).cuda()
        behind = whole[need:].clone()
        got = _lib.dev_tensor(fn, d_src, whole[:need], None, None, retry=False)
        assert down(got) == expect, (Lbits, n, need)
        torch.cuda.synchronize()
        assert torch.equal(whole[need:], behind), (Lbits, n, need, "a byte behind the buffer changed")


@pytest.mark.parametrize("Lbits,n", [(7, 5 * SPAN + 17), (7, 4 * UNIT), (4, SPAN + UNIT + 5), (1, 2 * UNIT + 31)])
def test_input_that_ends_with_its_allocation(dev, oracle, Lbits, n):
    """Both directions with the input as the last bytes of a tensor allocated at exactly that size: the chunk whose loads would pass the
    end takes the careful path.  The bytes in front of the input are seeded and are not data."""
    torch, _lib, huffman, up, down = dev
    data, want, _, _ = case(oracle, Lbits, n)
    for call, src, expect in ((huffman.compress_tensor, data, want), (huffman.decompress_tensor, want, data)):
        front = 1 << 16
        whole = torch.empty(front + len(src), dtype=torch.uint8, device="cuda")
        whole[:front] = torch.randint(0, 256, (front,), dtype=torch.uint8, generator=torch.Generator().manual_seed(n)).cuda()
        whole[front:] = up(src)
        assert whole[front:].data_ptr() % 16 == 0
        assert down(call(whole[front:])) == expect, (Lbits, n)
