"""CPU tests of the batch calls on device buffers (include/rsn.h: rsn_*_batch_dev): every argument error answers RSN_ERR_ARG with its
message before a device is looked for -- device pointers are integers where nothing can dereference them -- and the overlap check
(raisin_amd/csrc/dev_ranges.h) is held against the quadratic comparison by a stand-alone g++ program.  A call that passes the checks ends
at "no device" on a machine without one; with one it gets real memory."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")
NAMES = ("rsn_lzss_compress_batch_dev", "rsn_lzss_decompress_batch_dev", "rsn_arithmetic_compress_batch_dev", "rsn_arithmetic_decompress_batch_dev")
E_ARG, E_DEVICE = -1, -4
GARBAGE = 5


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from raisin_amd import _lib
    return _lib


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _calls(_lib):
    L = _lib.lib()
    return [(name, getattr(L, name), (4096,) if name == "rsn_lzss_compress_batch_dev" else ()) for name in NAMES]


def _call(_lib, fn, extra, members, n=None, null_members=False, null_lens=False):
    """-> (rc, message, out_lens), out_lens full of garbage before the call"""
    k = len(members)
    arr = (_lib.DevMember * max(k, 1))(*[_lib.DevMember(*m) for m in members])
    olens = (ctypes.c_size_t * max(k, 1))(*[GARBAGE] * max(k, 1))
    rc = fn(k if n is None else n, None if null_members else arr, *extra, None if null_lens else olens, None)
    return rc, _lib.lib().rsn_last_error(), [olens[i] for i in range(k)]


GOOD = (0x10000, 64, 0x20000, 4096)


def test_the_four_calls_are_bound(built):
    for name in NAMES:
        assert name in built.SYMBOLS
        getattr(built.lib(), name)
    assert ctypes.sizeof(built.DevMember) == 4 * ctypes.sizeof(ctypes.c_void_p)


def test_a_batch_of_none_is_answered_before_the_arrays_are_looked_at(built):
    for _name, fn, extra in _calls(built):
        rc, _, _ = _call(built, fn, extra, [], null_members=True, null_lens=True)
        assert rc == 0


def test_null_arrays(built):
    for _name, fn, extra in _calls(built):
        for kw in (dict(null_members=True), dict(null_lens=True), dict(null_members=True, null_lens=True)):
            rc, msg, _ = _call(built, fn, extra, [GOOD], **kw)
            assert rc == E_ARG and msg == b"null argument"


def test_a_member_s_pointers(built):
    for name, fn, extra in _calls(built):
        word = b"lzss" if "lzss" in name else b"arithmetic"
        rc, msg, lens = _call(built, fn, extra, [GOOD, (None, 7, 0x30000, 64)])
        assert rc == E_ARG and msg == b"member 1: null argument" and lens == [0, 0]
        for bad in ((0x10004, 64, 0x20000, 4096), (0x10000, 64, 0x20008, 4096), (0x10001, 0, 0x20000, 4096)):
            rc, msg, lens = _call(built, fn, extra, [GOOD, GOOD, bad])
            assert rc == E_ARG and msg == b"member 2: " + word + b": device buffers must be 16-byte aligned" and lens == [0, 0, 0]
        rc, msg, lens = _call(built, fn, extra, [(0x10000, 64, None, 16)])
        assert rc == E_ARG and msg.startswith(b"member 0: a null d_out with an out_cap of 16") and lens == [0]


def test_overlapping_ranges(built):
    for _name, fn, extra in _calls(built):
        # member 1's output over member 0's input
        rc, msg, lens = _call(built, fn, extra, [(0x10000, 64, 0x20000, 64), (0x30000, 64, 0x10030, 64)])
        assert rc == E_ARG and msg == b"member 1: its output range and member 0's input range overlap" and lens == [0, 0]
        # a member's output over its own input, as the single calls refuse it
        rc, msg, _ = _call(built, fn, extra, [GOOD, (0x30000, 64, 0x30020, 64)])
        assert rc == E_ARG and msg == b"member 1: its output range and member 1's input range overlap"
        # two outputs
        rc, msg, lens = _call(built, fn, extra, [(0x10000, 64, 0x20000, 64), GOOD, (0x30000, 64, 0x20030, 64)])
        assert rc == E_ARG and b"output range overlap" in msg and b"member 0: " in msg and b"member 1's" in msg and lens == [0, 0, 0]


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
    for _name, fn, extra in _calls(built):
        # ranges that touch end to start; one input handed in twice; a size query (null d_out, out_cap 0); a null input of length 0;
        # an EMPTY input that lies inside another member's output, and an empty output inside an input: empty ranges overlap nothing
        members = [(mem.at(0), 64, mem.at(64), 4032), (mem.at(0), 64, mem.at(4096), 4096), (mem.at(0), 64, None, 0),
                   (None, 0, mem.at(8192), 4096), (mem.at(80), 0, mem.at(12288), 4096), (mem.at(0), 64, mem.at(16), 0)]
        rc, msg, _ = _call(built, fn, extra, members)
        _passes(rc, msg)
        rc, msg, _ = _call(built, fn, extra, [(mem.at(0), 64, mem.at(4096), 4096)])
        _passes(rc, msg)


@pytest.fixture(scope="module")
def gxx():
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the range test")
    return "g++"


def _range_test(gxx, tmp_path, *flags):
    exe = str(tmp_path / "dev_ranges_test")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I" + SRC, os.path.join(ROOT, "tests", "dev_ranges_test.cpp"),
                    "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe, "20000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "dev ranges:" in r.stdout and int(r.stdout.split()[-2]) > 20000, r.stdout


def test_the_sorted_check_is_the_quadratic_one(gxx, tmp_path):
    _range_test(gxx, tmp_path)


def test_the_sorted_check_under_the_sanitizers(gxx, tmp_path):
    # a stand-alone program of host code: AddressSanitizer and UBSan link into it directly
    _range_test(gxx, tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def test_the_api_checks_by_the_header_under_test():
    # dev_ranges.h includes nothing of HIP's (the program above compiled with g++ alone), and the API unit takes its verdict from it
    includes = [line for line in open(os.path.join(SRC, "dev_ranges.h")) if line.startswith("#include")]
    assert includes and all(line.split()[1].startswith("<") for line in includes), includes
    api = open(os.path.join(SRC, "rsn_api.hip")).read()
    assert '#include "dev_ranges.h"' in api and "dev_ranges_clash(" in api
