"""CPU tests of the batch round trip (include/rsn.h: rsn_layers_roundtrip_batch, rsn_layers_roundtrip_batch_dev): every
argument error answers RSN_ERR_ARG with its message before a device is looked for -- device pointers are integers where nothing can
dereference them -- with `res` zeroed, and the verify table's and the stats block's arithmetic (raisin_amd/csrc/roundtrip_batch_layout.h)
is held against a brute-force statement by a stand-alone g++ program.  A call that passes the checks ends at "no device" on a machine
without one; with one it gets real memory."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")
HOST, DEV = "rsn_layers_roundtrip_batch", "rsn_layers_roundtrip_batch_dev"
E_ARG, E_DEVICE = -1, -4
GARBAGE = 0x55
LZSS, HUFFMAN, LAYERS_MAX = 1, 2, 8
GOOD = (0x10000, 64, None, 0)
ZERO = (0, 0, 0, 0, 0)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from raisin_amd import _lib
    return _lib


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _ids(ids, null=False):
    return None if null else (ctypes.c_int * max(len(ids), 1))(*ids)


def _res(_lib, k):
    """k results full of garbage"""
    res = (_lib.RoundTripMember * max(k, 1))()
    ctypes.memset(res, GARBAGE, ctypes.sizeof(res))
    return res


def _fields(res, k):
    return [(res[i].original_n, res[i].compressed_n, res[i].decompressed_n, res[i].first_difference, res[i].lossless) for i in range(k)]


def _dev(_lib, members, ids=(LZSS, HUFFMAN), n=None, null_members=False, null_res=False, null_layers=False, n_layers=None, hists=False):
    """-> (rc, message, res as tuples), res full of garbage before the call"""
    k = len(members)
    arr = (_lib.DevMember * max(k, 1))(*[_lib.DevMember(*m) for m in members])
    res = _res(_lib, k)
    counts = (ctypes.c_uint32 * (512 * max(k, 1)))() if hists else None
    rc = getattr(_lib.lib(), DEV)(k if n is None else n, None if null_members else arr, _ids(ids, null_layers), len(ids) if n_layers is None else n_layers,
                                  None if null_res else res, counts, None)
    return rc, _lib.lib().rsn_last_error(), _fields(res, k)


def _host(_lib, datas, ids=(LZSS, HUFFMAN), n=None, null=(), null_layers=False, n_layers=None, lens=None, hists=False):
    """-> (rc, message, res as tuples), res full of garbage before the call; null: the names of the arrays passed as NULL"""
    k = len(datas)
    ins = (ctypes.c_char_p * max(k, 1))(*datas)
    ln = (ctypes.c_size_t * max(k, 1))(*(lens if lens is not None else [len(d) if d else 0 for d in datas]))
    res = _res(_lib, k)
    counts = (ctypes.c_uint32 * (512 * max(k, 1)))() if hists else None
    rc = getattr(_lib.lib(), HOST)(k if n is None else n, None if "ins" in null else ins, None if "lens" in null else ln, _ids(ids, null_layers),
                                   len(ids) if n_layers is None else n_layers, None if "res" in null else res, counts)
    return rc, _lib.lib().rsn_last_error(), _fields(res, k)


def test_the_two_calls_are_bound(built):
    for name in (HOST, DEV):
        assert name in built.SYMBOLS
        getattr(built.lib(), name)
    header = open(os.path.join(ROOT, "include", "rsn.h")).read()
    for name in (HOST, DEV):
        assert "RSN_API int %s(" % name in header
    assert "rsn_roundtrip_member;" in header
    assert ctypes.sizeof(built.RoundTripMember) == 40
    from raisin_amd import engine, layers
    for name in ("RoundTripBatch", "roundtrip_tensors"):
        assert callable(getattr(layers, name))
    assert callable(engine.BenchmarkFiles)


def test_a_batch_of_none_is_answered_before_anything_is_looked_at(built):
    garbage = [(0x5555555555555555,) * 4 + (0x55555555,)]
    rc, _, res = _dev(built, [], null_members=True, null_res=True, null_layers=True, n_layers=99)
    assert rc == 0
    rc, _, _ = _dev(built, [], ids=(7,))
    assert rc == 0
    rc, _, _ = _host(built, [], null=("ins", "lens", "res"), null_layers=True, n_layers=99)
    assert rc == 0
    rc, _, _ = _host(built, [], ids=(7,))
    assert rc == 0
    # ... and nothing is written: a result that is there stays as it was
    res = _res(built, 1)
    assert getattr(built.lib(), HOST)(0, None, None, None, 99, res, None) == 0 and _fields(res, 1) == garbage
    assert getattr(built.lib(), DEV)(0, None, None, 99, res, None, None) == 0 and _fields(res, 1) == garbage


def test_null_arrays(built):
    for kw in (dict(null_members=True), dict(null_res=True), dict(null_members=True, null_res=True)):
        rc, msg, _ = _dev(built, [GOOD], **kw)
        assert rc == E_ARG and msg == b"null argument"
    for which in ("ins", "lens", "res"):
        rc, msg, _ = _host(built, [b"abc"], null=(which,))
        assert rc == E_ARG and msg == b"null argument"
    # ... before the layer list is looked at
    rc, msg, _ = _host(built, [b"abc"], null=("lens",), ids=(7,))
    assert rc == E_ARG and msg == b"null argument"
    rc, msg, _ = _dev(built, [GOOD], null_res=True, ids=(7,))
    assert rc == E_ARG and msg == b"null argument"


def test_a_host_member_that_is_null_with_a_length(built):
    rc, msg, res = _host(built, [b"abc", None, b"de"], lens=[3, 7, 2])
    assert rc == E_ARG and msg == b"member 1: null argument" and res == [ZERO] * 3
    rc, msg, res = _host(built, [b"abc", None, b"de"], lens=[3, 7, 2], ids=(7,), hists=True)      # the members come before the layers
    assert rc == E_ARG and msg == b"member 1: null argument" and res == [ZERO] * 3


def test_a_device_member_s_input(built):
    rc, msg, res = _dev(built, [GOOD, (None, 7, None, 0)])
    assert rc == E_ARG and msg == b"member 1: null argument" and res == [ZERO] * 2
    for bad in ((0x10004, 64, None, 0), (0x10008, 64, None, 0), (0x10001, 0, None, 0)):
        rc, msg, res = _dev(built, [GOOD, GOOD, bad])
        assert rc == E_ARG and msg == b"member 2: layers: device buffers must be 16-byte aligned" and res == [ZERO] * 3
    rc, msg, _ = _dev(built, [GOOD, (None, 7, None, 0)], ids=(7,))                                 # the members come before the layers
    assert rc == E_ARG and msg == b"member 1: null argument"


def test_d_out_and_out_cap_are_reserved(built):
    for bad in ((0x10000, 64, 0x20000, 4096), (0x10000, 64, 0x20000, 0), (0x10000, 64, None, 16), (None, 0, 0x20000, 64)):
        rc, msg, res = _dev(built, [GOOD, bad, GOOD], hists=True)
        assert rc == E_ARG and msg == b"member 1: d_out and out_cap are reserved in a round trip: NULL and 0" and res == [ZERO] * 3
    rc, msg, _ = _dev(built, [(0x10000, 64, 0x20000, 4096)], ids=(7,))                             # ... before the layers
    assert rc == E_ARG and msg.startswith(b"member 0: d_out and out_cap are reserved")


def test_the_layer_list(built):
    def calls(**kw):
        yield _dev(built, [GOOD, (0x40000, 64, None, 0)], **kw)
        yield _host(built, [b"abc", b""], **kw)
    for rc, msg, res in calls(ids=(LZSS, 3)):                              # (3: the arithmetic codec is no layer)
        assert rc == E_ARG and msg == b"layer 1: unknown layer id 3" and res == [ZERO] * 2
    for rc, msg, res in calls(ids=(0,)):
        assert rc == E_ARG and msg == b"layer 0: unknown layer id 0" and res == [ZERO] * 2
    for rc, msg, res in calls(ids=(LZSS,) * (LAYERS_MAX + 1)):
        assert rc == E_ARG and msg == b"9 layers: at most 8 in one call" and res == [ZERO] * 2
    for rc, msg, res in calls(null_layers=True, n_layers=2):
        assert rc == E_ARG and msg == b"null layer list" and res == [ZERO] * 2


class _Mem:
    """addresses for members that pass the checks: integers without a device, one zeroed allocation with one"""

    def __init__(self):
        self.base = 0x100000
        if _has_gpu():
            import torch
            self.t = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            self.base = self.t.data_ptr()

    def at(self, off):
        return self.base + off


def _passes(rc, msg, res):
    if _has_gpu():
        assert rc != E_ARG, msg
    else:
        assert rc == E_DEVICE and b"no CPU fallback" in msg
        assert all(r == ZERO for r in res)                                 # res is zeroed on every failure


def test_what_passes_the_checks(built):
    mem = _Mem()
    for ids in ((LZSS, LZSS), (LZSS,), (), (LZSS,) * LAYERS_MAX):
        # one input handed in twice; members that touch end to start; a null input of length 0; an empty range inside another
        members = [(mem.at(0), 64, None, 0), (mem.at(0), 64, None, 0), (mem.at(64), 64, None, 0), (None, 0, None, 0), (mem.at(80), 0, None, 0)]
        for hists in (False, True):
            rc, msg, res = _dev(built, members, ids=ids, hists=hists)
            _passes(rc, msg, res)
    rc, msg, res = _dev(built, [(mem.at(0), 64, None, 0)], null_layers=True, n_layers=0)
    _passes(rc, msg, res)
    for ids in ((LZSS, LZSS), (LZSS,), ()):
        for hists in (False, True):
            rc, msg, res = _host(built, [b"abc", b"", None], ids=ids, hists=hists)
            _passes(rc, msg, res)
    rc, msg, res = _host(built, [b"abc"], null_layers=True, n_layers=0)
    _passes(rc, msg, res)


def test_the_wrappers_refuse_an_unknown_layer_name(built, monkeypatch):
    from raisin_amd import layers

    def no_library():
        raise AssertionError("the library is not to be loaded for a layer name nobody knows")
    monkeypatch.setattr(built, "lib", no_library)
    with pytest.raises(ValueError, match="unknown layer 'arithmetic'"):
        layers.RoundTripBatch([b"abc"], ["lzss", "arithmetic"])
    with pytest.raises(ValueError, match="unknown layer 'rle'"):
        layers.roundtrip_tensors([], ["rle"])
    assert layers.roundtrip_tensors([], ["lzss", "huffman"]) == []
    monkeypatch.undo()
    assert layers.RoundTripBatch([], ["lzss", "huffman"]) == [] and layers.RoundTripBatch([], [], hists=False) == []


@pytest.fixture(scope="module")
def gxx():
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the layout test")
    return "g++"


def _layout_test(gxx, tmp_path, *flags):
    exe = str(tmp_path / "roundtrip_batch_layout_test")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I" + SRC, os.path.join(ROOT, "tests", "roundtrip_batch_layout_test.cpp"),
                    "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe, "4000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "roundtrip batch layout:" in r.stdout and int(r.stdout.split()[-2]) > 100000, r.stdout


def test_the_layout_is_the_brute_force_statement(gxx, tmp_path):
    _layout_test(gxx, tmp_path)


def test_the_layout_under_the_sanitizers(gxx, tmp_path):
    # a stand-alone program of host code: AddressSanitizer and UBSan link into it directly
    _layout_test(gxx, tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def test_the_library_includes_the_header_under_test():
    # roundtrip_batch_layout.h includes nothing of HIP's (the program above compiled with g++ alone), and both units that lay out by it
    # include it
    includes = [line.split()[1] for line in open(os.path.join(SRC, "roundtrip_batch_layout.h")) if line.startswith("#include")]
    assert includes and all(i.startswith("<") or i == '"layers_batch_layout.h"' for i in includes), includes
    for unit in ("rsn_api.hip", "roundtrip_batch.hip"):
        assert '#include "roundtrip_batch_layout.h"' in open(os.path.join(SRC, unit)).read(), unit
