"""CPU tests of the layered batch calls (include/rsn.h: rsn_layers_*_batch, rsn_layers_*_batch_dev): every argument error
answers RSN_ERR_ARG with its message before a device is looked for -- device pointers are integers where nothing can dereference them --
and the run cuts and slot offsets (raisin_amd/csrc/layers_batch_layout.h) are held against a brute-force statement by a stand-alone g++
program.  A call that passes the checks ends at "no device" on a machine without one; with one it gets real memory."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")
HOST = ("rsn_layers_compress_batch", "rsn_layers_decompress_batch")
DEV = ("rsn_layers_compress_batch_dev", "rsn_layers_decompress_batch_dev")
E_ARG, E_DEVICE = -1, -4
GARBAGE = 5
LZSS, HUFFMAN, LAYERS_MAX = 1, 2, 8
GOOD = (0x10000, 64, 0x20000, 4096)


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


def _dev(_lib, name, members, ids=(LZSS, HUFFMAN), n=None, null_members=False, null_lens=False, null_layers=False, n_layers=None):
    """-> (rc, message, out_lens), out_lens full of garbage before the call"""
    k = len(members)
    arr = (_lib.DevMember * max(k, 1))(*[_lib.DevMember(*m) for m in members])
    olens = (ctypes.c_size_t * max(k, 1))(*[GARBAGE] * max(k, 1))
    rc = getattr(_lib.lib(), name)(k if n is None else n, None if null_members else arr, _ids(ids, null_layers), len(ids) if n_layers is None else n_layers,
                                   None if null_lens else olens, None)
    return rc, _lib.lib().rsn_last_error(), [olens[i] for i in range(k)]


def _host(_lib, name, datas, ids=(LZSS, HUFFMAN), n=None, null=(), null_layers=False, n_layers=None, lens=None):
    """-> (rc, message, outs as integers, out_lens), both full of garbage before the call; null: the names of the arrays passed as NULL"""
    k = len(datas)
    ins = (ctypes.c_char_p * max(k, 1))(*datas)
    ln = (ctypes.c_size_t * max(k, 1))(*(lens if lens is not None else [len(d) if d else 0 for d in datas]))
    outs = (ctypes.c_void_p * max(k, 1))(*[GARBAGE] * max(k, 1))
    olens = (ctypes.c_size_t * max(k, 1))(*[GARBAGE] * max(k, 1))
    fn = getattr(_lib.lib(), name)
    rc = fn(k if n is None else n, None if "ins" in null else ins, None if "lens" in null else ln, _ids(ids, null_layers), len(ids) if n_layers is None else n_layers,
            None if "outs" in null else ctypes.cast(outs, fn.argtypes[5]), None if "out_lens" in null else olens)
    got = [outs[i] for i in range(k)]
    if rc == 0:
        for p in got:
            _lib.lib().rsn_free(p)
    return rc, _lib.lib().rsn_last_error(), got, [olens[i] for i in range(k)]


def test_the_four_calls_are_bound(built):
    for name in HOST + DEV:
        assert name in built.SYMBOLS
        getattr(built.lib(), name)
    header = open(os.path.join(ROOT, "include", "rsn.h")).read()
    for name in HOST + DEV:
        assert "RSN_API int %s(" % name in header
    from raisin_amd import layers
    for name in ("CompressBatch", "DecompressBatch", "compress_tensors", "decompress_tensors"):
        assert callable(getattr(layers, name))
    assert layers.IDS == {"lzss": LZSS, "huffman": HUFFMAN}


def test_a_batch_of_none_is_answered_before_anything_is_looked_at(built):
    for name in DEV:
        rc, _, _ = _dev(built, name, [], null_members=True, null_lens=True, null_layers=True, n_layers=99)
        assert rc == 0
        rc, _, _ = _dev(built, name, [], ids=(7,))
        assert rc == 0
    for name in HOST:
        rc, _, _, _ = _host(built, name, [], null=("ins", "lens", "outs", "out_lens"), null_layers=True, n_layers=99)
        assert rc == 0
        rc, _, _, _ = _host(built, name, [], ids=(7,))
        assert rc == 0


def test_null_arrays(built):
    for name in DEV:
        for kw in (dict(null_members=True), dict(null_lens=True), dict(null_members=True, null_lens=True)):
            rc, msg, _ = _dev(built, name, [GOOD], **kw)
            assert rc == E_ARG and msg == b"null argument"
    for name in HOST:
        for which in ("ins", "lens", "outs", "out_lens"):
            rc, msg, _, _ = _host(built, name, [b"abc"], null=(which,))
            assert rc == E_ARG and msg == b"null argument"
        # ... before the layer list is looked at
        rc, msg, _, _ = _host(built, name, [b"abc"], null=("outs",), ids=(7,))
        assert rc == E_ARG and msg == b"null argument"


def test_a_host_member_that_is_null_with_a_length(built):
    for name in HOST:
        rc, msg, outs, lens = _host(built, name, [b"abc", None, b"de"], lens=[3, 7, 2])
        assert rc == E_ARG and msg == b"member 1: null argument" and outs == [None] * 3 and lens == [0] * 3
        rc, msg, outs, lens = _host(built, name, [b"abc", None, b"de"], lens=[3, 7, 2], ids=(7,))     # the members come before the layers
        assert rc == E_ARG and msg == b"member 1: null argument"


def test_a_device_member_s_pointers(built):
    for name in DEV:
        rc, msg, lens = _dev(built, name, [GOOD, (None, 7, 0x30000, 64)])
        assert rc == E_ARG and msg == b"member 1: null argument" and lens == [0, 0]
        for bad in ((0x10004, 64, 0x20000, 4096), (0x10000, 64, 0x20008, 4096), (0x10001, 0, 0x20000, 4096)):
            rc, msg, lens = _dev(built, name, [GOOD, GOOD, bad])
            assert rc == E_ARG and msg == b"member 2: layers: device buffers must be 16-byte aligned" and lens == [0, 0, 0]
        rc, msg, lens = _dev(built, name, [(0x10000, 64, None, 16)])
        assert rc == E_ARG and msg.startswith(b"member 0: a null d_out with an out_cap of 16") and lens == [0]
        rc, msg, lens = _dev(built, name, [GOOD, (None, 7, 0x30000, 64)], ids=(7,))               # the members come before the layers
        assert rc == E_ARG and msg == b"member 1: null argument"


def test_overlapping_ranges_of_the_caller(built):
    for name in DEV:
        for ids in ((LZSS, HUFFMAN), (LZSS,), ()):                         # whatever runs between them, the caller's ranges are checked
            rc, msg, lens = _dev(built, name, [(0x10000, 64, 0x20000, 64), (0x30000, 64, 0x10030, 64)], ids=ids)
            assert rc == E_ARG and msg == b"member 1: its output range and member 0's input range overlap" and lens == [0, 0]
            rc, msg, _ = _dev(built, name, [GOOD, (0x30000, 64, 0x30020, 64)], ids=ids)
            assert rc == E_ARG and msg == b"member 1: its output range and member 1's input range overlap"
            rc, msg, lens = _dev(built, name, [(0x10000, 64, 0x20000, 64), GOOD, (0x30000, 64, 0x20030, 64)], ids=ids)
            assert rc == E_ARG and b"output range overlap" in msg and b"member 0: " in msg and b"member 1's" in msg and lens == [0, 0, 0]


def test_the_layer_list(built):
    for name in HOST + DEV:
        def call(**kw):
            if name in DEV:
                rc, msg, lens = _dev(built, name, [GOOD, (0x40000, 64, 0x50000, 4096)], **kw)
                return rc, msg, lens
            rc, msg, outs, lens = _host(built, name, [b"abc", b""], **kw)
            assert outs == [None, None]
            return rc, msg, lens
        rc, msg, lens = call(ids=(LZSS, 3))
        assert rc == E_ARG and msg == b"layer 1: unknown layer id 3" and lens == [0, 0]
        rc, msg, lens = call(ids=(0,))
        assert rc == E_ARG and msg == b"layer 0: unknown layer id 0"
        rc, msg, lens = call(ids=(LZSS,) * (LAYERS_MAX + 1))
        assert rc == E_ARG and msg == b"9 layers: at most 8 in one call"
        rc, msg, lens = call(null_layers=True, n_layers=2)
        assert rc == E_ARG and msg == b"null layer list" and lens == [0, 0]


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


def _passes(rc, msg):
    if _has_gpu():
        assert rc != E_ARG, msg
    else:
        assert rc == E_DEVICE and b"no CPU fallback" in msg


def test_what_passes_the_checks(built):
    mem = _Mem()
    for name in DEV:
        for ids in ((LZSS, LZSS), (LZSS,), (), (LZSS,) * LAYERS_MAX):
            # ranges that touch end to start; one input handed in twice; a size query; a null input of length 0; empty ranges inside others
            members = [(mem.at(0), 64, mem.at(64), 4032), (mem.at(0), 64, mem.at(4096), 4096), (mem.at(0), 64, None, 0),
                       (None, 0, mem.at(8192), 4096), (mem.at(80), 0, mem.at(12288), 4096), (mem.at(0), 64, mem.at(16), 0)]
            rc, msg, _ = _dev(built, name, members, ids=ids)
            _passes(rc, msg)
        rc, msg, _ = _dev(built, name, [(mem.at(0), 64, mem.at(4096), 4096)], null_layers=True, n_layers=0)
        _passes(rc, msg)
    for name in HOST:
        for ids in ((LZSS, LZSS), (LZSS,), ()):
            rc, msg, _, _ = _host(built, name, [b"abc", b"", None], ids=ids)
            _passes(rc, msg)
        rc, msg, _, _ = _host(built, name, [b"abc"], null_layers=True, n_layers=0)
        _passes(rc, msg)


def test_the_wrappers_refuse_an_unknown_layer_name(built):
    from raisin_amd import layers
    for fn in (layers.CompressBatch, layers.DecompressBatch):
        with pytest.raises(ValueError, match="unknown layer 'arithmetic'"):
            fn([b"abc"], ["lzss", "arithmetic"])
    for fn in (layers.compress_tensors, layers.decompress_tensors):
        with pytest.raises(ValueError, match="unknown layer 'rle'"):
            fn([], ["rle"])
    assert layers.CompressBatch([], ["lzss", "huffman"]) == [] and layers.DecompressBatch([], []) == []


@pytest.fixture(scope="module")
def gxx():
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the layout test")
    return "g++"


def _layout_test(gxx, tmp_path, *flags):
    exe = str(tmp_path / "layers_batch_layout_test")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I" + SRC, os.path.join(ROOT, "tests", "layers_batch_layout_test.cpp"),
                    "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe, "4000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "layers batch layout:" in r.stdout and int(r.stdout.split()[-2]) > 100000, r.stdout


def test_the_layout_is_the_brute_force_statement(gxx, tmp_path):
    _layout_test(gxx, tmp_path)


def test_the_layout_under_the_sanitizers(gxx, tmp_path):
    # a stand-alone program of host code: AddressSanitizer and UBSan link into it directly
    _layout_test(gxx, tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def test_the_api_lays_out_by_the_header_under_test():
    # layers_batch_layout.h includes nothing of HIP's (the program above compiled with g++ alone), and the API unit cuts its runs and
    # places its slots through it; the step is layer_batch_dev's body, factored, not copied
    includes = [line for line in open(os.path.join(SRC, "layers_batch_layout.h")) if line.startswith("#include")]
    assert includes and all(line.split()[1].startswith("<") for line in includes), includes
    api = open(os.path.join(SRC, "rsn_api.hip")).read()
    assert '#include "layers_batch_layout.h"' in api and "lb_runs(" in api and "lb_arena(" in api and "lb_packed(" in api
    assert api.count("run_dev(c, s, per[r]") == 1 and api.count("layer_batch_run(c, s,") >= 3
