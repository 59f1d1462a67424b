"""CPU tests of the batch suite (include/rsn.h: rsn_layers_suite_batch, rsn_layers_suite_batch_dev): every argument error
answers RSN_ERR_ARG with its message before a device is looked for -- device pointers are integers where nothing can dereference them --
in the order rsn.h states, with every row zeroed; a call that passes the checks ends at "no device" on a machine without one."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST, DEV = "rsn_layers_suite_batch", "rsn_layers_suite_batch_dev"
E_ARG, E_DEVICE = -1, -4
GARBAGE = 0x55
LZSS, HUFFMAN, LAYERS_MAX, LISTS_MAX = 1, 2, 8, 16
GOOD = (0x10000, 64, None, 0)
ZERO = (0, 0, 0, 0, 0)
GARBAGE_ROW = (0x5555555555555555,) * 4 + (0x55555555,)
SUITE = ((HUFFMAN,), (LZSS,), (LZSS, HUFFMAN))
NOT_WRITTEN = 77


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from raisin_amd import _lib
    return _lib


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def _lists(_lib, lists, null_layers=()):
    """-> (the rsn_layer_list array, what keeps its layer arrays alive); null_layers: {list index: n_layers} of lists with a null array"""
    keep = [(ctypes.c_int * max(len(l), 1))(*l) for l in lists]
    arr = (_lib.LayerList * max(len(lists), 1))()
    for k, l in enumerate(lists):
        if k in null_layers:
            arr[k] = _lib.LayerList(None, null_layers[k])
        else:
            arr[k] = _lib.LayerList(ctypes.cast(keep[k], ctypes.POINTER(ctypes.c_int)), len(l))
    return arr, keep


def _res(_lib, rows):
    res = (_lib.RoundTripMember * max(rows, 1))()
    ctypes.memset(res, GARBAGE, ctypes.sizeof(res))
    return res


def _fields(res, rows):
    return [(res[i].original_n, res[i].compressed_n, res[i].decompressed_n, res[i].first_difference, res[i].lossless) for i in range(rows)]


def _call(_lib, form, members, lists=SUITE, n=None, n_lists=None, null=(), null_layers=(), lens=None, hists=False):
    """one call of `form` -> (rc, message, the n_lists * n rows as tuples, list_rc, best); every output full of garbage before the call.
    members: bytes (the host form) or rsn_dev_member tuples; null: the names of the arguments passed as NULL"""
    k, nl = len(members), len(lists)
    arr, keep = _lists(_lib, lists, dict(null_layers))
    rows = k * nl
    res = _res(_lib, k * max(nl, n_lists or 0))                            # (what the call is told it holds)
    codes = (ctypes.c_int * max(nl, 1))(*([NOT_WRITTEN] * max(nl, 1)))
    best = (ctypes.c_uint32 * max(k, 1))(*([NOT_WRITTEN] * max(k, 1)))
    ho = (ctypes.c_uint32 * (256 * max(k, 1)))() if hists else None
    hd = (ctypes.c_uint32 * (256 * max(rows, 1)))() if hists else None
    tail = (nl if n_lists is None else n_lists, None if "lists" in null else arr, None if "res" in null else res, None if "list_rc" in null else codes, ho, hd,
            None if "best" in null else best)
    if form == HOST:
        ins = (ctypes.c_char_p * max(k, 1))(*members)
        ln = (ctypes.c_size_t * max(k, 1))(*(lens if lens is not None else [len(d) if d else 0 for d in members]))
        rc = getattr(_lib.lib(), HOST)(k if n is None else n, None if "ins" in null else ins, None if "lens" in null else ln, *tail)
    else:
        mem = (_lib.DevMember * max(k, 1))(*[_lib.DevMember(*m) for m in members])
        rc = getattr(_lib.lib(), DEV)(k if n is None else n, None if "members" in null else mem, *tail, None)
    del keep
    return rc, _lib.lib().rsn_last_error(), _fields(res, rows), list(codes)[:nl], list(best)[:k]


def _both(_lib, mem=None, **kw):
    """the same call in both forms over two good members; mem: where the device form's lie when the call passes the checks"""
    yield _call(_lib, HOST, [b"abc", b""], **kw)
    yield _call(_lib, DEV, [GOOD, (0x40000, 64, None, 0)] if mem is None else [(mem.at(0), 64, None, 0), (mem.at(4096), 64, None, 0)], **kw)


def test_the_two_calls_are_bound(built):
    header = open(os.path.join(ROOT, "include", "rsn.h")).read()
    for name in (HOST, DEV):
        assert name in built.SYMBOLS
        getattr(built.lib(), name)
        assert "RSN_API int %s(" % name in header
    assert "#define RSN_SUITE_LISTS_MAX 16" in header and "} rsn_layer_list;" in header
    assert ctypes.sizeof(built.LayerList) == 16
    for doc in ("INTEGRATION.md",):
        text = open(os.path.join(ROOT, doc)).read()
        assert HOST in text and DEV in text, doc
    from raisin_amd import engine, layers
    for name in ("SuiteBatch", "suite_tensors"):
        assert callable(getattr(layers, name))
    assert callable(engine.BenchmarkFilesSuite) and layers.SUITE_LISTS_MAX == LISTS_MAX


def test_the_abi_is_the_header(built):
    """exported symbols == include/rsn.h == _lib.SYMBOLS, with the two new calls in it"""
    import subprocess
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rsn.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(rsn_[a-z0-9_]+)\s*\(", hdr))
    assert {HOST, DEV} <= declared and declared == set(built.SYMBOLS)
    out = subprocess.check_output(["nm", "-D", "--defined-only", os.path.join(ROOT, "raisin_amd", "librsn.so")], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert declared <= exported and not {x for x in exported - declared if not x.startswith("__hip_")}


def test_a_batch_of_none_is_answered_before_anything_is_looked_at(built):
    for form, null in ((HOST, ("ins", "lens", "lists", "res", "list_rc", "best")), (DEV, ("members", "lists", "res", "list_rc", "best"))):
        rc, _, _, _, _ = _call(built, form, [], n_lists=99, null=null)
        assert rc == 0
        rc, _, _, _, _ = _call(built, form, [], lists=((7,),))
        assert rc == 0
    # ... and nothing is written: what is there stays as it was
    res = _res(built, 3)
    codes = (ctypes.c_int * 3)(NOT_WRITTEN, NOT_WRITTEN, NOT_WRITTEN)
    assert getattr(built.lib(), HOST)(0, None, None, 3, None, res, codes, None, None, None) == 0
    assert _fields(res, 3) == [GARBAGE_ROW] * 3 and list(codes) == [NOT_WRITTEN] * 3
    assert getattr(built.lib(), DEV)(0, None, 3, None, res, codes, None, None, None, None) == 0
    assert _fields(res, 3) == [GARBAGE_ROW] * 3 and list(codes) == [NOT_WRITTEN] * 3


def test_the_arrays_and_members_come_first(built):
    # null arrays, in front of every fault of the lists: a null `lists`, too many of them, an unknown layer
    for later in (dict(), dict(null=("lists",)), dict(n_lists=LISTS_MAX + 1), dict(lists=((LZSS,), (LZSS, 3)))):
        for which in ("ins", "lens"):
            kw = dict(later)
            kw["null"] = tuple(kw.get("null", ())) + (which,)
            rc, msg, rows, _, _ = _call(built, HOST, [b"abc", b"de"], **kw)
            assert rc == E_ARG and msg == b"null argument" and all(r == ZERO for r in rows)
        kw = dict(later)
        kw["null"] = tuple(kw.get("null", ())) + ("members",)
        rc, msg, rows, _, _ = _call(built, DEV, [GOOD, GOOD], **kw)
        assert rc == E_ARG and msg == b"null argument" and all(r == ZERO for r in rows)
    # a host member that is null with a length
    for kw in (dict(), dict(lists=((7,),)), dict(null=("lists",))):
        rc, msg, rows, codes, best = _call(built, HOST, [b"abc", None, b"de"], lens=[3, 7, 2], hists=True, **kw)
        assert rc == E_ARG and msg == b"member 1: null argument" and all(r == ZERO for r in rows)
        assert codes == [NOT_WRITTEN] * len(codes) and best == [NOT_WRITTEN] * 3      # a failure of the call as a whole writes neither
    # a device member's input, its alignment, and the reserved fields
    rc, msg, rows, _, _ = _call(built, DEV, [GOOD, (None, 7, None, 0)], lists=((7,),))
    assert rc == E_ARG and msg == b"member 1: null argument" and all(r == ZERO for r in rows)
    for bad in ((0x10004, 64, None, 0), (0x10008, 64, None, 0), (0x10001, 0, None, 0)):
        rc, msg, rows, _, _ = _call(built, DEV, [GOOD, GOOD, bad])
        assert rc == E_ARG and msg == b"member 2: layers: device buffers must be 16-byte aligned" and rows == [ZERO] * 9
    for bad in ((0x10000, 64, 0x20000, 4096), (0x10000, 64, 0x20000, 0), (0x10000, 64, None, 16), (None, 0, 0x20000, 64)):
        rc, msg, rows, _, _ = _call(built, DEV, [GOOD, bad, GOOD], hists=True, lists=SUITE * 5 + ((LZSS,), (7,)))   # (in front of the seventeen lists)
        assert rc == E_ARG and msg == b"member 1: d_out and out_cap are reserved in a round trip: NULL and 0" and all(r == ZERO for r in rows)


def test_no_lists_is_answered_behind_the_members_with_nothing_written(built):
    for form, members, null in ((HOST, [b"abc", b"de"], ("lists", "res", "list_rc", "best")), (DEV, [GOOD, GOOD], ("lists", "res", "list_rc", "best"))):
        rc, _, _, _, _ = _call(built, form, members, lists=(), null=null)
        assert rc == 0
        rc, _, _, codes, best = _call(built, form, members, lists=())
        assert rc == 0 and best == [NOT_WRITTEN] * 2
    # ... a result that is there stays as it was
    res = _res(built, 2)
    ins = (ctypes.c_char_p * 2)(b"abc", b"de")
    lens = (ctypes.c_size_t * 2)(3, 2)
    assert getattr(built.lib(), HOST)(2, ins, lens, 0, None, res, None, None, None, None) == 0 and _fields(res, 2) == [GARBAGE_ROW] * 2
    # ... but the members are looked at first
    rc, msg, _, _, _ = _call(built, HOST, [b"abc", None], lens=[3, 7], lists=())
    assert rc == E_ARG and msg == b"member 1: null argument"
    rc, msg, _, _, _ = _call(built, DEV, [GOOD, (0x10004, 64, None, 0)], lists=())
    assert rc == E_ARG and msg == b"member 1: layers: device buffers must be 16-byte aligned"


def test_null_lists_or_rows(built):
    for which in ("lists", "res"):
        for later in (dict(), dict(n_lists=LISTS_MAX + 1), dict(lists=((LZSS,), (LZSS, 3)))):
            for rc, msg, rows, _, _ in _both(built, null=(which,), **later):
                assert rc == E_ARG and msg == b"null argument"
                if which != "res":
                    assert all(r == ZERO for r in rows)
    for rc, msg, _, _, _ in _both(built, mem=_Mem(), null=("list_rc", "best")):       # both are optional
        assert rc != E_ARG, msg


def test_seventeen_lists_are_rejected(built):
    for rc, msg, rows, _, _ in _both(built, lists=SUITE * 5 + ((LZSS,), (7,))):
        assert rc == E_ARG and msg == b"17 layer lists: at most 16 in one call" and rows == [ZERO] * 34
    for rc, msg, rows, _, _ in _both(built, mem=_Mem(), lists=SUITE * 5 + ((LZSS,),)):      # sixteen pass
        assert rc != E_ARG, msg


def test_every_list_is_checked_as_a_layer_list(built):
    for rc, msg, rows, codes, _ in _both(built, lists=((LZSS,), (LZSS, 3))):                   # (3: the arithmetic codec is no layer)
        assert rc == E_ARG and msg == b"list 1: layer 1: unknown layer id 3" and rows == [ZERO] * 4 and codes == [NOT_WRITTEN] * 2
    for rc, msg, rows, _, _ in _both(built, lists=((0,), (7,))):                               # the lowest list's fault
        assert rc == E_ARG and msg == b"list 0: layer 0: unknown layer id 0" and rows == [ZERO] * 4
    for rc, msg, rows, _, _ in _both(built, lists=((LZSS,), (), (LZSS,) * (LAYERS_MAX + 1))):
        assert rc == E_ARG and msg == b"list 2: 9 layers: at most 8 in one call" and rows == [ZERO] * 6
    for rc, msg, rows, _, _ in _both(built, lists=((LZSS,), (LZSS, LZSS)), null_layers={1: 2}.items()):
        assert rc == E_ARG and msg == b"list 1: null layer list" and rows == [ZERO] * 4


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


def _passes(rc, msg, rows, codes, best):
    if _has_gpu():
        assert rc != E_ARG, msg
    else:
        assert rc == E_DEVICE and b"no CPU fallback" in msg
        assert all(r == ZERO for r in rows)                                # every row is zeroed on a failure of the call as a whole ...
        assert all(c == NOT_WRITTEN for c in codes) and all(b == NOT_WRITTEN for b in best)   # ... which writes neither list_rc nor best


def test_what_passes_the_checks_ends_at_the_device(built):
    mem = _Mem()
    members = [(mem.at(0), 64, None, 0), (mem.at(0), 64, None, 0), (mem.at(64), 64, None, 0), (None, 0, None, 0), (mem.at(80), 0, None, 0)]
    for lists in (((LZSS,), (LZSS, LZSS)), ((LZSS,),), ((),), ((LZSS,) * LAYERS_MAX, (LZSS,), (LZSS,)), ((LZSS,),) * LISTS_MAX):
        for hists in (False, True):
            _passes(*_call(built, DEV, members, lists=lists, hists=hists))
            _passes(*_call(built, HOST, [b"abc", b"", None], lists=lists, hists=hists))
    _passes(*_call(built, DEV, members[:1], lists=((), (LZSS,)), null_layers={0: 0}.items()))   # a null array of no layers is the empty list
    _passes(*_call(built, HOST, [b"abc"], lists=((), (LZSS,)), null_layers={0: 0}.items()))


def test_the_wrappers_refuse_an_unknown_layer_name(built, monkeypatch, tmp_path):
    from raisin_amd import engine, layers

    def no_library():
        raise AssertionError("the library is not to be loaded for a layer name nobody knows")
    monkeypatch.setattr(built, "lib", no_library)
    with pytest.raises(ValueError, match="unknown layer 'arithmetic'"):
        layers.SuiteBatch([b"abc"], [["lzss"], ["lzss", "arithmetic"]])
    with pytest.raises(ValueError, match="unknown layer 'rle'"):
        layers.suite_tensors([], [["huffman"], ["rle"]])
    assert layers.suite_tensors([], [["lzss"], ["lzss", "huffman"]]) == ([[], []], [], [None, None])
    monkeypatch.undo()
    assert layers.SuiteBatch([], [["lzss"], ["lzss", "huffman"]]) == ([[], []], [], [None, None])
    assert layers.SuiteBatch([b"abc"], [], hists=False) == ([], [None], [])
    # the engine: a name that neither the layered calls nor the engine's own writers know, before a file is read
    monkeypatch.setattr(built, "lib", no_library)
    with pytest.raises(ValueError, match="unknown layer 'arithmetic'"):
        engine.BenchmarkFilesSuite([str(tmp_path / "not_there_0"), str(tmp_path / "not_there_1")], [["lzss"], ["lzss", "arithmetic"]])
    monkeypatch.undo()
    assert engine.BenchmarkFilesSuite([], [["lzss"], ["huffman"]]) == []
