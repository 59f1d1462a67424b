"""GPU: the batch suite (include/rsn.h: rsn_layers_suite_batch, rsn_layers_suite_batch_dev) -- many members under several
layer lists in one call.  Every list's rows and both histogram blocks are held against the one-list call (layers.RoundTripBatch /
roundtrip_tensors, computed once per list and shared), the compressed sizes against the CPU oracle's chain.  The instruments are
tests/test_gpu_batch_dev.py's: members packed back to back in ONE allocation with hostile bytes between them, the library's launch
profile (names and counts) and its count of copied bytes."""
import ctypes

import numpy as np
import pytest

from test_gpu_batch_dev import Pack, _prof
from test_gpu_layered_batch import _files, _text
from test_gpu_layers_batch import _chain

pytestmark = pytest.mark.gpu

OK, E_EMPTY = 0, -2
LZ, HU = "lzss", "huffman"
LISTS = ([LZ], [HU], [LZ, HU], [HU, LZ], [LZ, LZ], [], [LZ, HU])              # (the last: a duplicate of the third)
NONE = (1 << 64) - 1
NO_BEST = 0xFFFFFFFF
TILE = 65536
ZERO = (0, 0, 0, 0, 0)
NOT_WRITTEN = 77

NOT_UTF8 = bytes([0xFF, 0xFE, 65, 66, 0xC3, 67]) * 50
TILE_AND_ONE = _text(7, TILE) + b"\xff"                                      # 64 KiB + 1: two tiles, and Huffman brings it back two bytes longer
EDGES = [_text(n, n) for n in (1, 2, 15, 16, 17)] + [_text(3, 1024), b"zzzz", NOT_UTF8, TILE_AND_ONE]
MID = [_text(300 + k, 2048 + 48 * k) for k in range(64)]                     # 2 to 5 KiB: the LZSS mid class forms
MEMBERS = EDGES + MID
WITH_EMPTY = EDGES[:3] + [b""] + EDGES[3:] + MID[:6] + [b""]
TILE_EDGES = [_text(n, n) for n in (1, 15, 16, 17, 255, TILE - 1, TILE, TILE + 1, TILE + 16, 2 * TILE, 2 * TILE + 4097)]


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, layers
    _lib.check(_lib.lib().rsn_device_set(0))
    return _lib, layers


def _hostile(datas):
    """members back to back in one allocation; behind a member either bytes that read as the start of an LZSS token or a copy of its own
    first bytes -- bytes that would change a histogram or hide a difference if they were counted or compared"""
    return Pack(datas, behind=lambda i: b"<1,1>\xa5\\\n" if i % 3 else datas[i][:48] or b"\xa5")


def _tensors(pack):
    return [pack.t[o:o + n] for o, n in zip(pack.offs, pack.lens)]


def _row(r):
    return (r.original_n, r.compressed_n, r.decompressed_n, r.first_difference, int(r.lossless))


# ---------------------------------------------------------------- the one-list call's answers, every (form, members, list) computed once
_REF = {}


def _ref(_lib, layers, form, datas, names):
    """-> ("ok", fields, hists of 512) of the one-list call, or ("failed", code, message)"""
    key = (form, id(datas), tuple(names))
    if key not in _REF:
        try:
            rows = layers.RoundTripBatch(datas, names) if form == "host" else layers.roundtrip_tensors(_tensors(_hostile(datas)), names)
            _REF[key] = ("ok", [_row(r) for r in rows], [r.hist_original + r.hist_decompressed for r in rows])
        except _lib.RsnError as e:
            _REF[key] = ("failed", e.code, str(e).split(": ", 1)[1])
    return _REF[key]


# ---------------------------------------------------------------- the calls, raw: every output full of garbage going in
def _suite(_lib, form, datas, lists, hists=True, want_codes=True, want_best=True):
    """-> (rc, rows[l][i] as tuples, hists_original[i], hists_decompressed[l][i], list_rc, best, message)"""
    import torch
    from raisin_amd import layers
    n, k = len(datas), len(lists)
    keep = [layers.ids(a) for a in lists]
    arr = (_lib.LayerList * max(k, 1))(*[_lib.LayerList(ctypes.cast(a, ctypes.POINTER(ctypes.c_int)), c) for a, c in keep])
    res = (_lib.RoundTripMember * max(k * n, 1))()
    ctypes.memset(res, 0x5A, ctypes.sizeof(res))
    codes = (ctypes.c_int * max(k, 1))(*([NOT_WRITTEN] * max(k, 1)))
    best = np.full(max(n, 1), NOT_WRITTEN, dtype=np.uint32)
    ho = np.full(256 * max(n, 1), 0xDEADBEEF, dtype=np.uint32) if hists else None
    hd = np.full(256 * max(k * n, 1), 0xDEADBEEF, dtype=np.uint32) if hists else None
    u32 = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)) if a is not None else None      # noqa: E731
    tail = (k, arr, res, codes if want_codes else None, u32(ho), u32(hd), u32(best) if want_best else None)
    if form == "host":
        ins = (ctypes.c_char_p * max(n, 1))(*datas)
        lens = (ctypes.c_size_t * max(n, 1))(*[len(d) for d in datas])
        rc = _lib.lib().rsn_layers_suite_batch(n, ins, lens, *tail)
    else:
        pack = _hostile(datas)
        before = pack.t.cpu().numpy().copy()
        mem = (_lib.DevMember * max(n, 1))(*[_lib.DevMember(pack.ptr(i) if d else None, len(d), None, 0) for i, d in enumerate(datas)])
        rc = _lib.lib().rsn_layers_suite_batch_dev(n, mem, *tail, None)
        torch.cuda.synchronize()
        assert np.array_equal(pack.t.cpu().numpy(), before), "the call wrote into the caller's members"
    msg = _lib.lib().rsn_last_error().decode("utf-8", "replace")
    rows = [[(int(r.original_n), int(r.compressed_n), int(r.decompressed_n), int(r.first_difference), int(r.lossless)) for r in res[l * n:(l + 1) * n]] for l in range(k)]
    h_o = [ho[256 * i:256 * i + 256].tolist() for i in range(n)] if hists else None
    h_d = [[hd[256 * (l * n + i):256 * (l * n + i) + 256].tolist() for i in range(n)] for l in range(k)] if hists else None
    return rc, rows, h_o, h_d, list(codes)[:k], best[:n].tolist(), msg


def _argmin(rows, ok, i):
    """the list with the smallest compressed size of member i among the lists `ok`, the lowest index among equals"""
    best = None
    for l in ok:
        if best is None or rows[l][i][1] < rows[best][i][1]:
            best = l
    return NO_BEST if best is None else best


def _holds(_lib, layers, form, datas, lists, got, oracle=None):
    """a suite call's answer against the one-list calls: every row and both histogram blocks of every list that succeeds, the code and
    the message of every list that fails, the call's own code and message, and best"""
    rc, rows, h_o, h_d, codes, best, msg = got
    refs = [_ref(_lib, layers, form, datas, names) for names in lists]
    ok = [l for l, r in enumerate(refs) if r[0] == "ok"]
    for l, (names, ref) in enumerate(zip(lists, refs)):
        if ref[0] == "ok":
            assert codes[l] == OK and rows[l] == ref[1], (form, names, [i for i in range(len(datas)) if rows[l][i] != ref[1][i]])
            if h_d is not None:
                assert [a + b for a, b in zip(h_o, h_d[l])] == ref[2], (form, names)
            if oracle is not None:
                assert [r[1] for r in rows[l]] == [len(_chain(oracle, d, names)[-1]) for d in datas], (form, names)
        else:
            assert codes[l] == ref[1] and rows[l] == [ZERO] * len(datas), (form, names, codes[l])
    failed = [l for l, r in enumerate(refs) if r[0] == "failed"]
    if failed:
        assert rc == refs[failed[0]][1] and msg == "list %d: %s" % (failed[0], refs[failed[0]][2]), (form, rc, msg)
    else:
        assert rc == OK, msg
    assert best == [_argmin(rows, ok, i) for i in range(len(datas))], form
    return ok, failed


# ---------------------------------------------------------------- the figures the members were chosen for
def test_the_members_are_the_ones_meant(oracle):
    from raisin_amd import lz
    assert [len(d) for d in EDGES] == [1, 2, 15, 16, 17, 1024, 4, 300, TILE + 1]
    assert len(MID) >= lz.MID_GROUP_MIN and all(2048 <= len(d) <= 5120 and 1024 < len(d) <= lz.MID_IN_MAX for d in MID)
    assert [len(d) for d in WITH_EMPTY].count(0) == 2
    back = oracle.huffman_decompress(oracle.huffman_compress(NOT_UTF8))
    assert len(back) > len(NOT_UTF8)                                       # bytes that are not UTF-8: Huffman comes back longer
    back = oracle.huffman_decompress(oracle.huffman_compress(TILE_AND_ONE))
    assert len(back) == TILE + 3 and back[:TILE] == TILE_AND_ONE[:TILE]    # the first difference is the first byte of the second tile
    assert oracle.huffman_decompress(oracle.huffman_compress(b"zzzz")) != b"zzzz"   # a single distinct byte


# ---------------------------------------------------------------- equality: every list, both forms
@pytest.mark.parametrize("form", ["host", "dev"])
def test_every_row_equals_the_one_list_call(mods, oracle, form):
    _lib, layers = mods
    got = _suite(_lib, form, MEMBERS, LISTS)
    ok, failed = _holds(_lib, layers, form, MEMBERS, LISTS, got, oracle)
    assert ok == list(range(len(LISTS))) and not failed
    rc, rows, h_o, h_d, codes, best, msg = got
    lossy = [i for i, r in enumerate(rows[1]) if not r[4]]
    assert [i for i in lossy if i >= 5] == [6, 7, 8] and rows[1][7][2] > rows[1][7][0] and rows[1][8][2:4] == (TILE + 3, TILE)
    assert rows[6] == rows[2] and h_d[6] == h_d[2]                         # the duplicate: the rows of the list it repeats ...
    assert 6 not in best                                                   # ... which win every tie with it
    # the tie rule is checked (in _holds, against the argmin) on members where two lists tie: one byte is one byte under [lzss], [lzss, lzss]
    # and [] alike, and the first of them wins
    ties = [i for i in range(len(MEMBERS)) if [rows[l][i][1] for l in range(len(LISTS))].count(rows[best[i]][i][1]) > 1]
    assert 0 in ties and rows[0][0][1] == rows[4][0][1] == rows[5][0][1] == 1 and best[0] == 0, (ties, best[:3])
    # without histograms, without list_rc, without best: the same rows
    rc2, rows2, _, _, codes2, best2, msg2 = _suite(_lib, form, MEMBERS, LISTS, hists=False, want_codes=False, want_best=False)
    assert rc2 == OK and rows2 == rows and codes2 == [NOT_WRITTEN] * len(LISTS) and best2 == [NOT_WRITTEN] * len(MEMBERS), msg2


def test_the_wrappers(mods):
    _lib, layers = mods
    datas = EDGES[:8] + MID[:4]
    lists = [[HU], [LZ], [LZ, HU]]
    for form, (rows, best, errors) in (("host", layers.SuiteBatch(datas, lists)), ("dev", layers.suite_tensors(_tensors(_hostile(datas)), lists))):
        assert errors == [None] * 3
        for l, names in enumerate(lists):
            want = layers.RoundTripBatch(datas, names)
            assert [_row(r) for r in rows[l]] == [_row(r) for r in want], (form, names)
            assert [r.hist_original + r.hist_decompressed for r in rows[l]] == [r.hist_original + r.hist_decompressed for r in want], (form, names)
        assert best == [_argmin([[_row(r) for r in rows[l]] for l in range(3)], range(3), i) for i in range(len(datas))]
    rows, best, errors = layers.SuiteBatch(datas[:3], lists, hists=False)
    assert rows[0][0].hist_original is None and errors == [None] * 3
    # an empty member: the Huffman lists fail and say so, the others answer
    rows, best, errors = layers.SuiteBatch(datas + [b""], lists)
    assert rows[0] is None and rows[2] is None and errors[1] is None and [e.code for e in (errors[0], errors[2])] == [E_EMPTY, E_EMPTY]
    assert "list 0: member %d: layer 0 (huffman): huffman: empty input" % len(datas) in str(errors[0])
    assert best == [1] * (len(datas) + 1) and rows[1][-1].compressed_n == 0


# ---------------------------------------------------------------- the second instance of the verify kernel at the tile's edges
def test_tile_edges_through_the_second_instance(mods):
    """{[], [lzss]}: the empty list is verified first, through the instance that counts both sides; [lzss] goes through the instance that
    counts the decompressed side alone -- a member against its own round trip, at lengths around 16 and around the tile"""
    _lib, layers = mods
    datas, lists = TILE_EDGES, [[], [LZ]]
    for form in ("host", "dev"):
        got, prof, _ = _prof(_lib, lambda: _suite(_lib, form, datas, lists))
        ok, failed = _holds(_lib, layers, form, datas, lists, got)
        assert ok == [0, 1] and not failed
        assert prof.get("members_verify") == 1 and prof.get("members_verify_dec") == 1, prof
        assert got[3][1] == got[2]                                        # lossless: the decompressed side's counts are the original's


# ---------------------------------------------------------------- per-list failure
@pytest.mark.parametrize("budget", [None, "1"], ids=["one_run", "a_run_a_member"])
def test_a_list_that_fails_zeroes_only_its_own_rows(mods, monkeypatch, budget):
    _lib, layers = mods
    refs = {form: [_ref(_lib, layers, form, WITH_EMPTY, names) for names in LISTS] for form in ("host", "dev")}   # (under the default budget)
    if budget:
        monkeypatch.setenv("RSN_LAYERS_BATCH_BUDGET", budget)
    for form in ("host", "dev"):
        got = _suite(_lib, form, WITH_EMPTY, LISTS)
        ok, failed = _holds(_lib, layers, form, WITH_EMPTY, LISTS, got)
        assert failed == [1, 2, 3, 6] and ok == [0, 4, 5]                  # every list that holds Huffman
        rc, rows, _, _, codes, best, msg = got
        assert [codes[l] for l in failed] == [E_EMPTY] * 4 and rc == E_EMPTY
        assert msg == "list 1: member 3: layer 0 (huffman): huffman: empty input (reference panics in heap.Pop, huffman.go:102)"
        assert refs[form][2][2].startswith("member 3: layer 1 (huffman): huffman: empty input")
        assert set(best) <= {0, 4, 5} and rows[0][3] == (0, 0, 0, NONE, 1)   # best ignores the failed lists; the empty member's row under [lzss]
    # the lowest failing list is not the first: its message is the one read
    got = _suite(_lib, "host", WITH_EMPTY, [[LZ], [LZ, HU], [HU]])
    assert got[0] == E_EMPTY and got[4] == [OK, E_EMPTY, E_EMPTY] and got[6].startswith("list 1: member 3: layer 1 (huffman): huffman: empty input")
    # every list fails: every row zeroed, no best
    got = _suite(_lib, "dev", WITH_EMPTY, [[HU], [HU, LZ]])
    assert got[0] == E_EMPTY and got[4] == [E_EMPTY] * 2 and got[5] == [NO_BEST] * len(WITH_EMPTY)
    assert got[1] == [[ZERO] * len(WITH_EMPTY)] * 2


# ---------------------------------------------------------------- sharing, by the library's own profile
def test_a_shared_prefix_is_compressed_once(mods):
    """{[lzss], [lzss, huffman]}: for every kernel an LZSS batch compress of the members launches, the suite launches what the two one-list
    calls launch less ONE such compress.  K is taken from layers.CompressBatch(datas, [lzss]) without "members_move": that launch is the
    host form's packing of its results for the way down, no step of the compress, and no round trip has one to take away -- the suite must
    not launch it at all (a kept output is written where it stays, not copied there)."""
    _lib, layers = mods
    lists = [[LZ], [LZ, HU]]
    _, prof_c, _ = _prof(_lib, lambda: layers.CompressBatch(MEMBERS, [LZ]))
    K = set(prof_c) - {"members_move"}
    assert "members_move" in prof_c and len(K) >= 2, prof_c                  # (the mid class and the single calls' kernels at least)
    rt, up_rt = {}, 0
    for names in lists:
        _, rt[tuple(names)], (up, _) = _prof(_lib, lambda: layers.RoundTripBatch(MEMBERS, names))
        up_rt += up
    got, prof, (up, _) = _prof(_lib, lambda: _suite(_lib, "host", MEMBERS, lists))
    assert got[0] == OK, got[6]
    for name in sorted(K):
        assert prof.get(name, 0) == rt[(LZ,)].get(name, 0) + rt[(LZ, HU)].get(name, 0) - prof_c[name], (name, prof, rt, prof_c)
    assert "members_move" not in prof, prof
    assert prof.get("members_verify") == 1 and prof.get("members_verify_dec") == 1, prof
    # every launch of the suite is one of the two calls' (the second verify under its own name), and none more often
    both = {name: rt[(LZ,)].get(name, 0) + rt[(LZ, HU)].get(name, 0) for name in set(rt[(LZ,)]) | set(rt[(LZ, HU)])}
    assert both.pop("members_verify") == 2
    less = {name: count - (prof_c[name] if name in K else 0) for name, count in both.items()}
    assert {k: v for k, v in prof.items() if not k.startswith("members_verify")} == {k: v for k, v in less.items() if v}, (prof, both)
    # the members go up once: the two calls' uploads less the packed input bytes, once
    packed = sum((len(d) + 15) // 16 * 16 for d in MEMBERS)
    print("upload bytes: suite %d, the two calls %d, the packed members %d" % (up, up_rt, packed))
    assert up <= up_rt - packed, (up, up_rt, packed)
    # the device form launches the same
    got_d, prof_d, _ = _prof(_lib, lambda: _suite(_lib, "dev", MEMBERS, lists))
    assert got_d[0] == OK and got_d[1] == got[1] and prof_d == prof, (prof_d, prof)


# ---------------------------------------------------------------- more than one run
def test_forced_run_cuts_give_the_same_answers(mods, monkeypatch):
    _lib, layers = mods
    refs = [_ref(_lib, layers, form, MEMBERS, names) for form in ("host", "dev") for names in LISTS]                # (under the default budget)
    assert all(r[0] == "ok" for r in refs)
    monkeypatch.setenv("RSN_LAYERS_BATCH_BUDGET", "3000000")
    for form in ("host", "dev"):
        got, prof, _ = _prof(_lib, lambda: _suite(_lib, form, MEMBERS, LISTS))
        ok, failed = _holds(_lib, layers, form, MEMBERS, LISTS, got)
        assert len(ok) == len(LISTS) and not failed
        runs = prof.get("members_verify")
        assert 3 <= runs < len(MEMBERS), prof                               # several members to a run, at least three runs
        assert prof.get("members_verify_dec") == runs * 5, prof           # a run: the first list through the first instance, the five other distinct lists through the second


# ---------------------------------------------------------------- the one-list call runs the suite's flow: calls in turn, one process
SEQ_LISTS = [[LZ], [LZ, HU], [HU]]                                           # the lzss node is kept: LB_KEEP is live in the suite calls
SEQ_MEMBERS = [_text(20 + k, 500 + 100 * k) for k in range(5)] + [_text(1, 1), _text(9, TILE + 1)]   # the last: two verify tiles, rows that add


@pytest.mark.parametrize("budget", [None, "1"], ids=["one_run", "a_run_a_member"])
def test_a_one_list_call_between_two_suite_calls(mods, oracle, monkeypatch, budget):
    """suite, one list, suite again: every answer is the oracle's, whatever the call before left in the slots the two share (the arenas,
    the verify slot) and in the one only the suite has; the one-list call launches the first instance of the verify kernel once a run
    and never the second"""
    from test_gpu_roundtrip_batch import _dev as one_dev, _host as one_host, _wants
    _lib, _ = mods
    assert [len(d) for d in SEQ_MEMBERS] == [500, 600, 700, 800, 900, 1, TILE + 1]
    want = [_wants(oracle, SEQ_MEMBERS, names) for names in SEQ_LISTS]
    if budget:
        monkeypatch.setenv("RSN_LAYERS_BATCH_BUDGET", budget)
    runs = len(SEQ_MEMBERS) if budget else 1
    for form, one in (("host", one_host), ("dev", one_dev)):
        first = _suite(_lib, form, SEQ_MEMBERS, SEQ_LISTS)
        (rc, got, hists, msg), prof, _ = _prof(_lib, lambda: one(_lib, SEQ_MEMBERS, SEQ_LISTS[1]))
        second = _suite(_lib, form, SEQ_MEMBERS, SEQ_LISTS)
        for s_rc, rows, h_o, h_d, codes, best, s_msg in (first, second):
            assert s_rc == OK and codes == [OK] * 3, (form, s_msg)
            for l, (fields, counts) in enumerate(want):
                assert rows[l] == fields, (form, l, [i for i in range(len(fields)) if rows[l][i] != fields[i]])
                assert [a + b for a, b in zip(h_o, h_d[l])] == counts, (form, l)
            assert best == [_argmin(rows, range(3), i) for i in range(len(SEQ_MEMBERS))], form
        assert first == second, form
        assert rc == OK and got == want[1][0] and hists == want[1][1], (form, msg)
        assert prof.get("members_verify") == runs and "members_verify_dec" not in prof, (form, prof)


# ---------------------------------------------------------------- the engine
def test_benchmark_files_suite_is_the_loop_of_benchmark_files(mods, tmp_path):
    from raisin_amd import engine
    _lib, _ = mods
    algorithms = [[HU], [LZ], [LZ, HU]]
    datas = [_text(k, 13 + 97 * k) for k in range(12)] + [NOT_UTF8, b"zzzz"]
    paths = _files(tmp_path, "s", datas)

    def row(r):
        return (r.CompressionEngine, r.Ratio, r.Entropy, r.ActualEntropy, r.Lossless, r.Failed)
    want = [[row(r) for r in engine.BenchmarkFiles(a, paths)] for a in algorithms]
    got, prof, _ = _prof(_lib, lambda: engine.BenchmarkFilesSuite(paths, algorithms))
    assert len(got) == len(paths)
    for i, (results, best) in enumerate(got):
        assert [row(r) for r in results] == [want[l][i] for l in range(3)], i    # exact: both sum the same integer counts in the same order
        ratios = [r.Ratio for r in results]
        assert best is results[ratios.index(min(ratios))]                 # the first of the smallest, lossless or not
    assert prof.get("members_verify") == 1 and prof.get("members_verify_dec") == 2, prof
    # one empty file among them: the Huffman lists go file by file and that file's rows are `failed`; [lzss] stays in the call
    empty = tmp_path / "empty.txt"
    empty.write_bytes(b"")
    mixed = paths[:5] + [str(empty)] + paths[5:]
    got = engine.BenchmarkFilesSuite(mixed, algorithms)
    assert [r.Failed for r in got[5][0]] == [True, False, True] and got[5][1] is got[5][0][1]
    others = got[:5] + got[6:]
    assert [[row(r) for r in results] for results, _ in others] == [[want[l][i] for l in range(3)] for i in range(len(paths))]
