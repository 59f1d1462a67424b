"""The mid-size class of the Huffman batch calls (csrc/huff_mid.hip) as far as it shows without a device: the cutoffs in
csrc/codecs.h and their mirrors in raisin_amd/huffman.py are the same numbers, the decoder's limits hold every stream the encoder can
write, the small kernels' cutoffs did not move, and a batch of mid-size members fails without a device the way every codec entry point
does.  Runs on any machine."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from raisin_amd import _lib
    return _lib


def _header_constants():
    src = open(os.path.join(ROOT, "raisin_amd", "csrc", "codecs.h")).read()
    out = {}
    for name in ("HUFF_MID_IN_MAX", "HUFF_MID_PAY_MAX", "HUFF_MID_OUT_MAX", "HUFF_MID_GROUP_MIN"):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert m, name
        out[name] = int(m.group(1))
    return out


def test_mirrored_constants_are_the_headers():
    from raisin_amd import huffman
    h = _header_constants()
    assert huffman.MID_IN_MAX == h["HUFF_MID_IN_MAX"]
    assert huffman.MID_PAY_MAX == h["HUFF_MID_PAY_MAX"]
    assert huffman.MID_OUT_MAX == h["HUFF_MID_OUT_MAX"]
    assert huffman.MID_GROUP_MIN == h["HUFF_MID_GROUP_MIN"]


def test_limits_hold_together():
    from raisin_amd import huffman
    assert huffman.MID_PAY_MAX * 8 >= huffman.MID_IN_MAX * 7          # a byte alphabet codes in at most 7 bits a byte
    assert huffman.MID_OUT_MAX >= huffman.MID_IN_MAX
    assert huffman.BATCH_COMPRESS_INPUT_MAX < huffman.MID_IN_MAX <= 65536
    assert huffman.MID_GROUP_MIN >= 1


def test_the_small_kernels_cutoffs_did_not_move():
    from raisin_amd import huffman
    assert huffman.BATCH_COMPRESS_INPUT_MAX == 16384
    assert huffman.BATCH_GROUP_PAYLOAD_MAX == 16384
    assert huffman.BATCH_GROUP_OUTPUT_MAX == 32768


def _batch(L, name, bufs):
    k = len(bufs)
    ins = (ctypes.c_char_p * k)(*bufs)
    lens = (ctypes.c_size_t * k)(*[len(b) for b in bufs])
    outs = (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = (ctypes.c_size_t * k)()
    for i in range(k):                                      # garbage the call must overwrite with NULL
        outs[i] = ctypes.cast(ctypes.c_void_p(0x1000 + 16 * i), ctypes.POINTER(ctypes.c_uint8))
    return getattr(L, name)(k, ins, lens, outs, olens), outs


def test_without_a_device_a_mid_batch_is_a_device_error(built, oracle):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from raisin_amd import huffman
    L = built.lib()
    k = max(huffman.MID_GROUP_MIN, 8)
    members = [(b"mid-size member %d, " % i) * (1800 + 80 * i) for i in range(k)]                # (above 32 KiB: mid-size to the decoder too)
    assert all(huffman.BATCH_COMPRESS_INPUT_MAX < len(b) <= huffman.MID_IN_MAX for b in members)
    streams = [oracle.huffman_compress(b) for b in members]
    for name, bufs in (("rsn_huffman_compress_batch", members), ("rsn_huffman_decompress_batch", streams)):
        rc, outs = _batch(L, name, bufs)
        assert rc == -4, name                                # RSN_ERR_DEVICE
        assert b"no CPU fallback" in L.rsn_last_error(), name
        assert all(not outs[i] for i in range(k)), name
