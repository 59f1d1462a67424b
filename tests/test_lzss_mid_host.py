"""The mid-size class of the LZSS batch calls (csrc/lzss_mid.hip) as far as it shows without a device: the cutoffs in
csrc/codecs.h and their mirrors in raisin_amd/lz.py are the same numbers, random bytes of the largest member fit the escaped limit, and
a batch of mid-size members fails without a device the way every codec entry point does.  Runs on any machine."""
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
    for name in ("LZSS_MID_IN_MAX", "LZSS_MID_E_MAX", "LZSS_MID_GROUP_MIN"):
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, src)
        assert m, name
        out[name] = int(m.group(1))
    return out


def test_mirrored_constants_are_the_headers():
    from raisin_amd import lz
    h = _header_constants()
    assert lz.MID_IN_MAX == h["LZSS_MID_IN_MAX"]
    assert lz.MID_E_MAX == h["LZSS_MID_E_MAX"]
    assert lz.MID_GROUP_MIN == h["LZSS_MID_GROUP_MIN"]


def test_limits_hold_together():
    from raisin_amd import lz
    assert 1024 < lz.MID_IN_MAX <= 65536
    assert lz.MID_E_MAX >= lz.MID_IN_MAX + lz.MID_IN_MAX // 64        # random bytes: one in 128 is a 5C or an FF
    assert lz.MID_GROUP_MIN >= 1


def _batch(L, name, bufs, window=4096, **missing):
    k = len(bufs)
    ins = None if missing.get("ins") else (ctypes.c_char_p * k)(*bufs)
    lens = None if missing.get("lens") else (ctypes.c_size_t * k)(*[len(b) for b in bufs])
    outs = None if missing.get("outs") else (ctypes.POINTER(ctypes.c_uint8) * k)()
    olens = None if missing.get("olens") else (ctypes.c_size_t * k)()
    if outs is not None:
        for i in range(k):                                  # garbage the call must overwrite with NULL
            outs[i] = ctypes.cast(ctypes.c_void_p(0x1000 + 16 * i), ctypes.POINTER(ctypes.c_uint8))
    extra = (window,) if name == "rsn_lzss_compress_batch" else ()
    return getattr(L, name)(k, ins, lens, *extra, outs, olens), outs


def _mid_members():
    from raisin_amd import lz
    k = max(lz.MID_GROUP_MIN, 8)
    return [(b"mid-size member %d, " % i) * (150 + 40 * i) for i in range(k)]


def test_null_arguments_are_refused_before_a_device_is_looked_for(built):
    L = built.lib()
    bufs = _mid_members()
    for name in ("rsn_lzss_compress_batch", "rsn_lzss_decompress_batch"):
        for arg in ("ins", "lens", "outs", "olens"):
            rc, _ = _batch(L, name, bufs, **{arg: True})
            assert rc == -1, (name, arg)                     # RSN_ERR_ARG
            assert b"no CPU fallback" not in L.rsn_last_error(), (name, arg)


def test_without_a_device_a_mid_batch_is_a_device_error(built):
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = built.lib()
    bufs = _mid_members()
    assert all(2048 < len(b) <= 65536 for b in bufs)
    for name in ("rsn_lzss_compress_batch", "rsn_lzss_decompress_batch"):
        rc, outs = _batch(L, name, bufs)
        assert rc == -4, name                                # RSN_ERR_DEVICE
        assert b"no CPU fallback" in L.rsn_last_error(), name
        assert all(not outs[i] for i in range(len(bufs))), name
