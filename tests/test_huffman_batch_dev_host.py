"""CPU tests of the Huffman batch calls on device buffers (include/rsn.h: rsn_huffman_compress_batch_dev, rsn_huffman_decompress_batch_dev):
the argument errors of tests/test_batch_dev_host.py for the two new calls -- RSN_ERR_ARG with its message before a device is looked for,
device pointers being integers where nothing can dereference them -- the empty member of the compress call, and "no device" for what passes."""
import ctypes

import pytest

from test_batch_dev_host import E_ARG, E_DEVICE, GOOD, _Mem, _call, _has_gpu

NAMES = ("rsn_huffman_compress_batch_dev", "rsn_huffman_decompress_batch_dev")
E_EMPTY = -2


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from raisin_amd import _lib
    return _lib


def _calls(_lib):
    return [(name, getattr(_lib.lib(), name), ()) for name in NAMES]


def test_the_two_calls_are_bound_and_declared(built):
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rsn.h")).read()
    for name in NAMES:
        assert name in built.SYMBOLS
        getattr(built.lib(), name)
        assert "RSN_API int %s(size_t n, const rsn_dev_member *members, size_t *out_lens, void *stream);" % name in header
    assert "Huffman is not offered in this form" not in header
    assert built.lib().rsn_huffman_compress_batch_dev.argtypes[1]._type_ is built.DevMember


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
    for _name, fn, extra in _calls(built):
        rc, msg, lens = _call(built, fn, extra, [GOOD, (None, 7, 0x30000, 64)])
        assert rc == E_ARG and msg == b"member 1: null argument" and lens == [0, 0]
        for bad in ((0x10004, 64, 0x20000, 4096), (0x10000, 64, 0x20008, 4096), (0x10001, 0, 0x20000, 4096)):
            rc, msg, lens = _call(built, fn, extra, [GOOD, GOOD, bad])
            assert rc == E_ARG and msg == b"member 2: huffman: device buffers must be 16-byte aligned" and lens == [0, 0, 0]
        rc, msg, lens = _call(built, fn, extra, [(0x10000, 64, None, 16)])
        assert rc == E_ARG and msg.startswith(b"member 0: a null d_out with an out_cap of 16") and lens == [0]


def test_overlapping_ranges(built):
    for _name, fn, extra in _calls(built):
        rc, msg, lens = _call(built, fn, extra, [(0x10000, 64, 0x20000, 64), (0x30000, 64, 0x10030, 64)])
        assert rc == E_ARG and msg == b"member 1: its output range and member 0's input range overlap" and lens == [0, 0]
        rc, msg, _ = _call(built, fn, extra, [GOOD, (0x30000, 64, 0x30020, 64)])
        assert rc == E_ARG and msg == b"member 1: its output range and member 1's input range overlap"
        rc, msg, lens = _call(built, fn, extra, [(0x10000, 64, 0x20000, 64), GOOD, (0x30000, 64, 0x20030, 64)])
        assert rc == E_ARG and b"output range overlap" in msg and b"member 0: " in msg and b"member 1's" in msg and lens == [0, 0, 0]


def test_an_empty_member_fails_the_compress_call_as_the_single_call_words_it(built):
    fn = built.lib().rsn_huffman_compress_batch_dev
    # before a device is looked for, the lowest such member named, behind the argument checks of every member
    rc, msg, lens = _call(built, fn, (), [GOOD, (None, 0, 0x30000, 4096), (0x40000, 0, 0x50000, 64)])
    assert rc == E_EMPTY and msg.startswith(b"member 1: huffman: empty input") and lens == [0, 0, 0]
    rc, msg, lens = _call(built, fn, (), [(None, 0, 0x30000, 4096), (0x10004, 64, 0x20000, 4096)])
    assert rc == E_ARG and msg.startswith(b"member 1: huffman: device buffers") and lens == [0, 0]


def _passes(rc, msg):
    if _has_gpu():
        assert rc != E_ARG, msg
    else:
        assert rc == E_DEVICE and b"no CPU fallback" in msg


def test_what_passes_the_checks(built):
    mem = _Mem()
    for name, fn, extra in _calls(built):
        # ranges that touch end to start; one input handed in twice; a size query (null d_out, out_cap 0); an empty output inside an input;
        # for the decompress call also a null input of length 0 and an EMPTY input inside another member's output
        members = [(mem.at(0), 64, mem.at(64), 4032), (mem.at(0), 64, mem.at(4096), 4096), (mem.at(0), 64, None, 0), (mem.at(0), 64, mem.at(16), 0)]
        if "decompress" in name:
            members += [(None, 0, mem.at(8192), 4096), (mem.at(80), 0, mem.at(12288), 4096)]
        rc, msg, _ = _call(built, fn, extra, members)
        _passes(rc, msg)
        rc, msg, _ = _call(built, fn, extra, [(mem.at(0), 64, mem.at(4096), 4096)])
        _passes(rc, msg)
