"""GPU: the layered batch calls (include/rsn.h: rsn_layers_*_batch, rsn_layers_*_batch_dev).  Expected bytes come from the
CPU oracle's chain, never from the library, and the single rsn_layers_* call is held against the same bytes -- members that are not UTF-8
included, which the Huffman layer treats lossily.  The instruments are tests/test_gpu_batch_dev.py's: members packed back to back in ONE
allocation with hostile bytes between them, outputs between the fences of tests/test_gpu_dev_fences.py at exactly the capacity the last
step takes, the library's launch profile and its count of copied bytes."""
import ctypes

import pytest

from test_gpu_batch_dev import TABLE_DOWN, TABLE_UP, Pack, _batch, _out_bytes, _prof, _ru16
from test_gpu_dev_fences import fenced
from test_gpu_huffman_batch_dev import PLAN_DOWN, PLAN_UP
from test_gpu_layered_batch import _text

pytestmark = pytest.mark.gpu

OK, E_EMPTY, E_FORMAT, E_CAP = 0, -2, -3, -7
LZ, HU = "lzss", "huffman"
LISTS = ([LZ, HU], [HU, LZ], [LZ, LZ], [LZ, HU, LZ], [LZ], [])
LZSS_SMALL_MAX = 1024                                   # codecs.h: what the small LZSS encoder takes
HUFF_SMALL_MAX = 16384                                  # huffman.BATCH_COMPRESS_INPUT_MAX
MOVE_ENTRY, TILE = 24, 65536                            # codecs.h: MoveEntry; layers_batch_layout.h: LB_TILE
C_HOST, D_HOST, C_DEV, D_DEV = "rsn_layers_compress_batch", "rsn_layers_decompress_batch", "rsn_layers_compress_batch_dev", "rsn_layers_decompress_batch_dev"


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman, layers, lz
    _lib.check(_lib.lib().rsn_device_set(0))
    return _lib, layers, lz, huffman


# ---------------------------------------------------------------- the oracle's chain, every step computed once
_STEP = {}


def _step(oracle, layer, enc, d):
    key = (layer, enc, d)
    if key not in _STEP:
        if layer == LZ:
            _STEP[key] = oracle.lzss_compress(d, 4096) if enc else oracle.lzss_decompress(d)
        else:
            _STEP[key] = oracle.huffman_compress(d) if enc else oracle.huffman_decompress(d)
    return _STEP[key]


def _chain(oracle, d, names):
    """[d, after layer 0, after layer 1, ...]"""
    out = [d]
    for a in names:
        out.append(_step(oracle, a, True, out[-1]))
    return out


def _unchain(oracle, s, names):
    """[s, after undoing the last layer, ...]"""
    out = [s]
    for a in reversed(names):
        out.append(_step(oracle, a, False, out[-1]))
    return out


SMALL = [_text(k, 13 + (1011 * k) // 63) for k in range(64)]                 # 13 B ... 1 KiB
MID = [_text(100 + k, 4096 if k == 32 else 2048 + 48 * k) for k in range(64)]   # 2 to 5 KiB
LARGE = [_text(200 + k, 40000) for k in range(4)]
VERY = [_text(300, 300000)]
ODD = [b"z", b"zzzz", "héllo wörld, naïve café. ".encode() * 20, bytes([0xFF, 0xFE, 65, 66, 0xC3, 67]) * 50]
MEMBERS = SMALL + MID + LARGE + VERY + ODD
ABC, ABC_BIG = b"abc" * 20000, b"abc" * 120000


def test_the_members_land_in_the_classes_meant(mods, oracle):
    """from the oracle's lengths alone: which class of each layer a member of [lzss, huffman] meets"""
    _lib, layers, lz, huffman = mods
    assert (len(SMALL[0]), len(SMALL[-1]), len(MID[32])) == (13, 1024, 4096)
    assert [len(x) for x in _chain(oracle, _text(1024, 1024), [LZ, HU])] == [1024, 945, 772]
    assert [len(x) for x in _chain(oracle, _text(4096, 4096), [LZ, HU])] == [4096, 3565, 2443]
    assert [len(x) for x in _chain(oracle, _text(40000, 40000), [LZ, HU])] == [40000, 33234, 20821]
    assert len(_step(oracle, LZ, True, _text(300000, 300000))) == 249746
    for d in SMALL:                                                       # the small classes of both layers
        assert len(d) <= LZSS_SMALL_MAX and 2 <= len(_step(oracle, LZ, True, d)) <= HUFF_SMALL_MAX
    for d in MID:                                                         # LZSS mid class, then Huffman small class
        assert LZSS_SMALL_MAX < len(d) <= lz.MID_IN_MAX and 2 <= len(_step(oracle, LZ, True, d)) <= HUFF_SMALL_MAX
    assert len(MID) + len(LARGE) >= lz.MID_GROUP_MIN
    for d in LARGE:                                                       # LZSS mid class, then Huffman mid class
        assert LZSS_SMALL_MAX < len(d) <= lz.MID_IN_MAX and HUFF_SMALL_MAX < len(_step(oracle, LZ, True, d)) <= huffman.MID_IN_MAX
    assert len(LARGE) >= huffman.MID_GROUP_MIN
    for d in VERY:                                                        # the single path in both layers
        assert len(d) > lz.MID_IN_MAX and len(_step(oracle, LZ, True, d)) > huffman.MID_IN_MAX
    for d in ODD[:2]:
        assert len(set(d)) == 1                                           # a single distinct byte: the grouped Huffman encoder hands it back
    for d in ODD[2:]:
        assert max(d) >= 0x80
    try:
        ODD[3].decode()
        raise AssertionError("meant not to be UTF-8")
    except UnicodeDecodeError:
        pass


# ---------------------------------------------------------------- the calls
def _host(_lib, name, datas, names):
    """the host form, raw -> (rc, results or None each, out_lens, message); outs and out_lens full of garbage going in"""
    from raisin_amd import layers
    L = _lib.lib()
    arr, k = layers.ids(names)
    n = len(datas)
    ins = (ctypes.c_char_p * max(n, 1))(*datas)
    lens = (ctypes.c_size_t * max(n, 1))(*[len(d) for d in datas])
    outs = (ctypes.POINTER(ctypes.c_uint8) * max(n, 1))()
    olens = (ctypes.c_size_t * max(n, 1))(*[77] * max(n, 1))
    rc = getattr(L, name)(n, ins, lens, arr, k, outs, olens)
    msg = L.rsn_last_error().decode("utf-8", "replace")
    res = [ctypes.string_at(outs[i], olens[i]) if outs[i] else None for i in range(n)]
    for i in range(n):
        L.rsn_free(outs[i])
    return rc, res, [int(olens[i]) for i in range(n)], msg


def _dev(_lib, name, members, names):
    from raisin_amd import layers
    arr, k = layers.ids(names)
    return _batch(_lib, name, members, arr, k)


def _tensors(datas):
    import torch
    ts = [torch.frombuffer(bytearray(d) + bytearray(16), dtype=torch.uint8).cuda()[:len(d)] for d in datas]
    torch.cuda.synchronize()
    return ts


def _tbytes(ts):
    return [bytes(t.cpu().numpy()) for t in ts]


@pytest.mark.parametrize("names", LISTS, ids=lambda v: "+".join(v) or "none")
def test_every_list_both_directions_both_forms(mods, oracle, names):
    _lib, layers, _, _ = mods
    want = [_chain(oracle, d, names)[-1] for d in MEMBERS]
    back = [_unchain(oracle, s, names)[-1] for s in want]
    for d, b in zip(MEMBERS[:-len(ODD)], back):
        assert b == d                                                     # (text comes back; what the reference's Huffman codec does to a
    if HU not in names:                                                   #  single distinct byte and to bytes that are not UTF-8 is the oracle's to say)
        assert back == MEMBERS
    else:
        assert back[-1] != MEMBERS[-1] and back[-2] == MEMBERS[-2]
    for i in (0, 63, 64, 128, 132, 133, 134, 135, 136):                   # the single layered call, host and device, says the same
        assert layers.Compress(MEMBERS[i], names) == want[i], i
        assert layers.Decompress(want[i], names) == back[i], i
    one = _tbytes([layers.compress_tensor(t, names) for t in _tensors(MEMBERS[-2:])])
    assert one == want[-2:]
    # host form
    assert layers.CompressBatch(MEMBERS, names) == want
    assert layers.DecompressBatch(want, names) == back
    # device form, tensors through the wrappers
    assert _tbytes(layers.compress_tensors(_tensors(MEMBERS), names)) == want
    assert _tbytes(layers.decompress_tensors(_tensors(want), names)) == back


def test_empty_members_where_no_layer_refuses_them(mods, oracle):
    _lib, layers, _, _ = mods
    datas = [b"", _text(5, 100), b"", b""]
    for names in ([LZ], [LZ, LZ], []):
        want = [_chain(oracle, d, names)[-1] for d in datas]
        assert want[0] == b"" and want[2] == b""
        assert layers.CompressBatch(datas, names) == want
        assert layers.DecompressBatch(want, names) == datas
        assert _tbytes(layers.compress_tensors(_tensors(datas), names)) == want
        assert _tbytes(layers.decompress_tensors(_tensors(want), names)) == datas
    assert layers.CompressBatch([], [LZ, HU]) == [] and layers.compress_tensors([], [LZ, HU]) == []


# ---------------------------------------------------------------- a step that outgrows its first slot
def test_a_step_that_outgrows_its_first_slot(mods, oracle):
    """A decompress slot is the single chain's first guess: 8 n + 64 KiB for an LZSS stream of n bytes (rsn_api.hip: codec().cap).  Under
    [huffman, lzss] decompress runs LZSS first, mid-chain, on an LZSS stream of a Huffman stream of period 5 that expands many tens of
    times.  For b"abc" * 20000 the oracle gives 133 -> 12524 bytes: ninety-four times, yet inside the guess of 66600, whose constant term
    decides at that size -- so that member shows nothing, and stays only as a case.  For b"abc" * 120000 the oracle gives 309 -> 75027
    against a guess of 8 * 309 + 65536 = 68008: the step reports its need, and the member is run again alone while its neighbours are
    complete.  Under [lzss, lzss] the same happens in the last step (1045 bytes -> 360000 against 73896)."""
    _lib, layers, _, _ = mods
    assert [len(x) for x in _chain(oracle, ABC, [LZ, LZ])] == [60000, 241, 130]
    c = _chain(oracle, ABC, [HU, LZ])
    assert len(c[2]) == 133 and len(c[1]) == 12524 and len(c[1]) <= 8 * len(c[2]) + 65536
    c = _chain(oracle, ABC_BIG, [HU, LZ])
    assert len(c[1]) > 8 * len(c[2]) + 65536, "the mid-chain LZSS step must exceed its first guess"
    c2 = _chain(oracle, ABC_BIG, [LZ, LZ])
    assert len(c2[0]) > 8 * len(c2[1]) + 65536, "the last LZSS step must exceed its first guess"
    datas = [_text(7, 900), ABC, _text(8, 5000), ABC_BIG, _text(9, 30)]
    for names in ([HU, LZ], [LZ, LZ]):
        want = [_chain(oracle, d, names)[-1] for d in datas]
        assert layers.CompressBatch(datas, names) == want
        assert layers.DecompressBatch(want, names) == datas
        assert _tbytes(layers.compress_tensors(_tensors(datas), names)) == want
        assert _tbytes(layers.decompress_tensors(_tensors(want), names)) == datas
        assert layers.Decompress(want[3], names) == ABC_BIG


# ---------------------------------------------------------------- device form: fences and capacity
def _grouped_huffman(x):
    return 2 <= len(x) <= 65536 and max(x) < 0x80 and len(set(x)) > 1


def _last_caps(enc, names, into_last, results):
    """the smallest capacity the last step takes (rsn.h): the exact size -- but behind a last Huffman compress layer, for a member that
    takes the single call, the size rounded up to 16, plus 32.  into_last: what the last layer reads, from the oracle."""
    if not (enc and names and names[-1] == HU):
        return [len(r) for r in results]
    small = sum(1 for x in into_last if _grouped_huffman(x) and len(x) <= HUFF_SMALL_MAX)
    mid = sum(1 for x in into_last if _grouped_huffman(x) and len(x) > HUFF_SMALL_MAX)
    caps = []
    for x, r in zip(into_last, results):
        grouped = _grouped_huffman(x) and (small >= 2 if len(x) <= HUFF_SMALL_MAX else mid >= 4)
        caps.append(len(r) if grouped else _ru16(len(r)) + 32)
    return caps


def _fenced_layers(_lib, name, datas, caps, names, null_out=()):
    pack = Pack(datas, behind=lambda i: b"<1,1>\xa5\\\n" if i % 3 else datas[i][:48] or b"\xa5")
    outs = [None if i in null_out else fenced(c) for i, c in enumerate(caps)]
    members = [(pack.ptr(i), len(d), outs[i][1] if outs[i] else None, caps[i] if outs[i] else 0) for i, d in enumerate(datas)]
    rc, lens, msg = _dev(_lib, name, members, names)
    for i, o in enumerate(outs):
        if o:
            o[2]("member %d's output" % i)
    return rc, lens, msg, outs


FENCE_MEMBERS = SMALL[::7] + MID[::9] + LARGE + VERY + ODD


@pytest.mark.parametrize("names", ([LZ, HU], [HU, LZ], [LZ], []), ids=lambda v: "+".join(v) or "none")
def test_fences_at_exactly_the_capacity_the_last_step_takes(mods, oracle, names):
    _lib = mods[0]
    datas = FENCE_MEMBERS
    chains = [_chain(oracle, d, names) for d in datas]
    want = [c[-1] for c in chains]
    caps = _last_caps(True, names, [c[-2] for c in chains] if names else datas, want)
    rc, lens, msg, outs = _fenced_layers(_lib, C_DEV, datas, caps, names)
    assert rc == OK, msg
    assert lens == [len(w) for w in want]
    assert [_out_bytes(o, k) for o, k in zip(outs, lens)] == want
    back = [_unchain(oracle, s, names)[-1] for s in want]
    rc, lens, msg, outs = _fenced_layers(_lib, D_DEV, want, [len(b) for b in back], names)
    assert rc == OK, msg
    assert [_out_bytes(o, k) for o, k in zip(outs, lens)] == back


@pytest.mark.parametrize("names", ([LZ, HU], [HU, LZ], []), ids=lambda v: "+".join(v) or "none")
def test_one_member_a_byte_short_and_one_a_size_query(mods, oracle, names):
    _lib = mods[0]
    short, query = 3, 5
    for enc in (True, False):
        if enc:
            datas = FENCE_MEMBERS
            chains = [_chain(oracle, d, names) for d in datas]
        else:
            datas = [_chain(oracle, d, names)[-1] for d in FENCE_MEMBERS]
            chains = [_unchain(oracle, s, names) for s in datas]
        want = [c[-1] for c in chains]
        caps = _last_caps(enc, names, [c[-2] for c in chains] if names else datas, want)
        caps[short] -= 1
        rc, lens, msg, outs = _fenced_layers(_lib, C_DEV if enc else D_DEV, datas, caps, names, null_out=(query,))
        assert rc == E_CAP, msg
        last = (len(names) - 1 if enc else 0) if names else None
        assert msg.startswith("member %d: " % short + ("layer %d (%s): " % (last, names[last]) if names else "layers: ")), msg
        assert "buffer holds %d" % caps[short] in msg, msg
        for i, (o, w) in enumerate(zip(outs, want)):
            if i in (short, query):
                assert lens[i] > (caps[i] if i == short else 0) and lens[i] >= len(w), (i, lens[i])
            else:
                assert lens[i] == len(w) and _out_bytes(o, lens[i]) == w, i
        caps[short], caps[query] = lens[short], lens[query]                # a second call with the reported figures
        rc, lens, msg, outs = _fenced_layers(_lib, C_DEV if enc else D_DEV, datas, caps, names)
        assert rc == OK, msg
        assert [_out_bytes(o, k) for o, k in zip(outs, lens)] == want


# ---------------------------------------------------------------- the profile and the copied bytes
def _allowance(members, plan=False):
    """what one layer's batch call on device buffers may copy for `members` grouped members: test_gpu_batch_dev.py's, and the Huffman
    decoders' plan entries on top"""
    return members * (TABLE_UP + TABLE_DOWN + (PLAN_UP + PLAN_DOWN if plan else 0)) + 32


def test_device_form_profile_and_copied_bytes(mods, oracle):
    """64 small members under [lzss, huffman]: one launch a layer, and per layer only 4.10's tables and answers cross -- far less than the
    intermediates, which therefore did not"""
    _lib = mods[0]
    names = [LZ, HU]
    chains = [_chain(oracle, d, names) for d in SMALL]
    want = [c[-1] for c in chains]
    rc_lens, prof, copied = _prof(_lib, lambda: _fenced_layers(_lib, C_DEV, SMALL, [len(w) for w in want], names))
    rc, lens, msg, outs = rc_lens
    assert rc == OK, msg
    assert [_out_bytes(o, k) for o, k in zip(outs, lens)] == want
    assert prof == {"group_gather": 2, "lzss_batch_enc": 1, "huff_batch_enc": 1, "group_scatter": 2}, prof
    bound = 2 * _allowance(len(SMALL))
    assert sum(copied) <= bound < sum(len(c[1]) for c in chains) // 2, (copied, bound)
    rc_lens, prof, copied = _prof(_lib, lambda: _fenced_layers(_lib, D_DEV, want, [len(d) for d in SMALL], names))
    rc, lens, msg, outs = rc_lens
    assert rc == OK, msg
    assert [_out_bytes(o, k) for o, k in zip(outs, lens)] == SMALL
    assert prof.get("huff_batch_dec") == 1 and prof.get("lzss_batch_dec") == 1 and prof.get("huff_dev_plan") == 1, prof
    assert set(prof) == {"huff_dev_plan", "huff_dev_gather", "huff_batch_dec", "huff_dev_scatter", "group_gather", "lzss_batch_dec", "group_scatter"}, prof
    bound = _allowance(len(SMALL), plan=True) + _allowance(len(SMALL))
    assert sum(copied) <= bound < sum(len(c[1]) for c in chains) // 2, (copied, bound)


def test_host_form_profile_and_copied_bytes(mods, oracle):
    """one copy up, one copy down, one members_move launch a run; between them the device form's traffic and the move table"""
    _lib, layers, _, _ = mods
    names = [LZ, HU]
    want = [_chain(oracle, d, names)[-1] for d in SMALL]
    tiles = len(SMALL)
    assert all(0 < len(w) <= TILE for w in want + SMALL)
    got, prof, (up, down) = _prof(_lib, lambda: layers.CompressBatch(SMALL, names))
    assert got == want
    assert prof == {"group_gather": 2, "lzss_batch_enc": 1, "huff_batch_enc": 1, "group_scatter": 2, "members_move": 1}, prof
    assert up <= sum(_ru16(len(d)) for d in SMALL) + 2 * (len(SMALL) * TABLE_UP + 32) + tiles * MOVE_ENTRY, up
    assert down <= sum(_ru16(len(w)) for w in want) + 2 * (len(SMALL) * TABLE_DOWN + 32), down
    got, prof, (up, down) = _prof(_lib, lambda: layers.DecompressBatch(want, names))
    assert got == SMALL
    assert prof.get("members_move") == 1 and prof.get("huff_batch_dec") == 1 and prof.get("lzss_batch_dec") == 1, prof
    assert up <= sum(_ru16(len(w)) for w in want) + len(SMALL) * (2 * TABLE_UP + PLAN_UP) + 64 + tiles * MOVE_ENTRY, up
    assert down <= sum(_ru16(len(d)) for d in SMALL) + len(SMALL) * (2 * TABLE_DOWN + PLAN_DOWN) + 64, down


def test_the_move_kernel_cuts_a_large_member_into_tiles(mods):
    """the device form without layers is k_members_move alone: lengths around the tile and around 16, fenced at the exact size"""
    _lib = mods[0]
    datas = [_text(n, n) for n in (1, 15, 16, 17, 255, 4096, TILE - 1, TILE, TILE + 1, 4 * TILE + 4097, 300000)]
    (rc, lens, msg, outs), prof, (up, down) = _prof(_lib, lambda: _fenced_layers(_lib, C_DEV, datas, [len(d) for d in datas], []))
    assert rc == OK, msg
    assert [_out_bytes(o, k) for o, k in zip(outs, lens)] == datas
    assert prof == {"members_move": 1}, prof
    assert (up, down) == (MOVE_ENTRY * sum((len(d) + TILE - 1) // TILE for d in datas), 0)


# ---------------------------------------------------------------- run cuts
def test_forced_run_cuts_give_the_same_bytes(mods, oracle, monkeypatch):
    _lib, layers, _, _ = mods
    names = [LZ, HU]
    datas = SMALL[40:] + MID[:6] + LARGE[:1] + SMALL[:8]
    want = [_chain(oracle, d, names)[-1] for d in datas]
    monkeypatch.setenv("RSN_LAYERS_BATCH_BUDGET", "400000")
    got, prof, _ = _prof(_lib, lambda: layers.CompressBatch(datas, names))
    assert got == want
    runs = prof.get("members_move")
    assert 3 < runs < len(datas), prof                                    # several members to a run, several runs; the 40000-byte member exceeds the budget alone
    back, prof, _ = _prof(_lib, lambda: layers.DecompressBatch(want, names))
    assert back == datas and prof.get("members_move") > 1, prof
    assert _tbytes(layers.compress_tensors(_tensors(datas), names)) == want
    assert _tbytes(layers.decompress_tensors(_tensors(want), names)) == datas
    monkeypatch.setenv("RSN_LAYERS_BATCH_BUDGET", "1")                    # every member a run of its own
    got, prof, _ = _prof(_lib, lambda: layers.CompressBatch(datas[:9], names))
    assert got == want[:9] and prof.get("members_move") == 9, prof
    monkeypatch.delenv("RSN_LAYERS_BATCH_BUDGET")
    got, prof, _ = _prof(_lib, lambda: layers.CompressBatch(datas, names))
    assert got == want and prof.get("members_move") == 1, prof


# ---------------------------------------------------------------- errors
def _dev_members(datas, cap=1 << 17):
    import torch
    pack = Pack(datas)
    out = torch.zeros(len(datas) * cap + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return (pack, out), [(pack.ptr(i), len(d), out.data_ptr() + i * cap, cap) for i, d in enumerate(datas)]


def test_an_empty_member_fails_in_the_huffman_layer(mods, monkeypatch):
    _lib, layers, _, _ = mods
    L = _lib.lib()
    datas = [_text(1, 500), _text(2, 900), b"", _text(3, 700), b""]
    with pytest.raises(_lib.RsnError) as single:
        layers.Compress(b"", [LZ, HU])
    assert single.value.code == E_EMPTY and str(single.value).split(": ", 1)[1].startswith("layer 1 (huffman): huffman: empty input")
    text = "layer 1 (huffman): huffman: empty input (reference panics in heap.Pop, huffman.go:102)"      # the batch calls' wording of it
    for budget in (None, "1"):                                            # one run, and a run a member
        if budget:
            monkeypatch.setenv("RSN_LAYERS_BATCH_BUDGET", budget)
        rc, res, lens, msg = _host(_lib, C_HOST, datas, [LZ, HU])
        assert rc == E_EMPTY and msg == "member 2: " + text and res == [None] * 5 and lens == [0] * 5
        keep, members = _dev_members(datas)
        rc, lens, msg = _dev(_lib, C_DEV, members, [LZ, HU])
        assert rc == E_EMPTY and msg == "member 2: " + text and lens == [0] * 5
        # [huffman, lzss]: the same member fails in layer 0, and with both kinds of failure in one call the earlier layer's is the call's
        rc, res, lens, msg = _host(_lib, C_HOST, datas, [HU, LZ])
        assert rc == E_EMPTY and msg.startswith("member 2: layer 0 (huffman): huffman: empty input") and res == [None] * 5 and lens == [0] * 5
    assert L.rsn_last_error() is not None


def test_a_third_stream_that_is_not_one(mods, oracle, monkeypatch):
    _lib, layers, _, _ = mods
    names = [LZ, HU]
    datas = [_text(1, 500), _text(2, 900), b"x" * 9, _text(3, 700)]
    streams = [_chain(oracle, d, names)[-1] for d in datas]
    streams[2] = b"1|a1|b"
    with pytest.raises(_lib.RsnError) as single:                         # (the single call on a device buffer: the codec the batch runs)
        layers.decompress_tensor(_tensors([streams[2]])[0], names)
    code, text = single.value.code, str(single.value).split(": ", 1)[1]
    with pytest.raises(_lib.RsnError) as on_host:
        layers.Decompress(streams[2], names)
    assert on_host.value.code == code
    assert code == E_FORMAT and text.startswith("layer 1 (huffman): ")
    for budget in (None, "1"):
        if budget:
            monkeypatch.setenv("RSN_LAYERS_BATCH_BUDGET", budget)
        rc, res, lens, msg = _host(_lib, D_HOST, streams, names)
        assert rc == code and msg == "member 2: " + text and res == [None] * 4 and lens == [0] * 4
        keep, members = _dev_members(streams)
        rc, lens, msg = _dev(_lib, D_DEV, members, names)
        assert rc == code and msg == "member 2: " + text and lens == [0] * 4
    # a later layer's failure in a LOWER member loses to an earlier layer's in a higher one, whatever the runs: member 1 is a Huffman
    # stream of bytes that are no LZSS stream (layer 0 fails, second in run order), member 3 no Huffman stream (layer 1, first in run order)
    bad_lzss = _step(oracle, HU, True, b"<9,9>" + _text(4, 40))
    with pytest.raises(_lib.RsnError) as inner:
        layers.Decompress(bad_lzss, names)
    assert str(inner.value).split(": ", 1)[1].startswith("layer 0 (lzss): ")
    mixed = [streams[0], bad_lzss, streams[1], b"1|a1|b"]
    for budget in ("1", None):
        if budget:
            monkeypatch.setenv("RSN_LAYERS_BATCH_BUDGET", budget)
        else:
            monkeypatch.delenv("RSN_LAYERS_BATCH_BUDGET")
        rc, res, lens, msg = _host(_lib, D_HOST, mixed, names)
        assert rc == code and msg == "member 3: " + text and res == [None] * 4 and lens == [0] * 4, msg


# ---------------------------------------------------------------- independence from earlier calls
def test_the_same_call_before_and_after_a_different_batch(mods, oracle):
    _lib, layers, _, _ = mods
    names = [LZ, HU]
    datas = SMALL[::5] + MID[::16] + [ABC]
    want = [_chain(oracle, d, names)[-1] for d in datas]
    first = layers.CompressBatch(datas, names)
    first_back = layers.DecompressBatch(first, names)
    other = [bytes([0x41 + (i * 7 + k) % 23 for k in range(200 + 300 * i)]) for i in range(40)] + [_text(77, 150000)]
    assert layers.DecompressBatch(layers.CompressBatch(other, [HU, LZ]), [HU, LZ]) == other
    assert _tbytes(layers.decompress_tensors(layers.compress_tensors(_tensors(other), [LZ, LZ]), [LZ, LZ])) == other
    assert layers.CompressBatch(datas, names) == first == want
    assert layers.DecompressBatch(first, names) == first_back == datas
