"""GPU: the tiled class of the LZSS compress batch (csrc/lzss_tile.hip) on the cases of tests/lzss_tile_cases.py -- where the greedy chain
enters and leaves a tile, windows that are no multiple of a sub-tile with the match exactly at the window's edge, members just under and
over the step cap, more bytes than a group's staging, a seeded fuzz, every LZSS class in one call, two threads at once.  Every result is
compared byte for byte with the CPU oracle and with the single call (test_gpu_lzss_tile's _host and _dev), in the host form and in the
device form with exact capacities between guard bytes.  Which members the kernels handed back is read from the call's contract -- with
every capacity exact, a member whose single call asks for its bound is answered E_CAP -- and from the profile, which shows the single
call's kernels also where that call completed at the exact capacity.
tests/test_lzss_tile_cases_host.py proves on a CPU that the cases are what they claim."""
import threading

import pytest

import lzss_tile_cases as C
from test_gpu_batch_dev import E_CAP, OK, _fenced_call, _out_bytes, _prof
from test_gpu_batch_dev import _single as _single_dev
from test_gpu_lzss_mid import _text
from test_gpu_lzss_tile import ENC, ONLY, TILE, _dev, _host, _single, _want, mods  # noqa: F401  (mods: the fixture)

pytestmark = pytest.mark.gpu

GROUP = TILE + ("group_gather", "group_scatter")
ONCE = "lzss_tok_emit"                                   # lzss_encode.hip: the single call's last launch


def _by_contract(mods, oracle, members, w):
    """the device form with every capacity exact -> (the members handed back, the first call's profile); the bytes against the oracle"""
    _lib, lz = mods
    want = [_want(oracle, d, w) for d in members]
    caps = [len(x) for x in want]
    (rc, lens, msg, outs), prof, _ = _prof(_lib, lambda: _fenced_call(_lib, ENC, members, caps, w))
    assert rc in (OK, E_CAP), msg
    back = {i for i in range(len(members)) if lens[i] > caps[i]}
    assert (rc == E_CAP) == bool(back), (rc, msg, back)
    for i, x in enumerate(want):
        if i not in back:
            assert lens[i] == len(x) and _out_bytes(outs[i], lens[i]) == x, (i, len(members[i]), w)
    if back:
        rc, lens, msg, outs = _fenced_call(_lib, ENC, members, [max(a, b) for a, b in zip(lens, caps)], w)
        assert rc == OK, msg
        assert lens == caps and [_out_bytes(o, k) for o, k in zip(outs, lens)] == want
    return back, prof


# ---------------------------------------------------------------- 1: where the chain enters and leaves a tile
@pytest.mark.parametrize("k", (0, 1))
def test_landings(mods, oracle, k):
    name, members, w, expect = C.landings(mods[1])[k]
    members = list(members)
    assert _host(mods, oracle, members, w) == ONLY, name
    prof, _ = _dev(mods, oracle, members, w)
    assert prof == ONLY, (name, prof)


# ---------------------------------------------------------------- 2: the match exactly at the window's edge
@pytest.mark.parametrize("k", range(len(C.WINDOWS)))
def test_windows(mods, oracle, k):
    name, members, w, expect = C.windows(mods[1])[k]
    members = list(members)
    assert _host(mods, oracle, members, w) == ONLY, name
    prof, _ = _dev(mods, oracle, members, w)
    assert prof == ONLY, (name, prof)


# ---------------------------------------------------------------- 3: the step cap from both sides
@pytest.mark.parametrize("k", range(len(C.CAP_PERIODS)))
def test_cap(mods, oracle, k):
    """Every member but the first is PAD, which the model says must be taken, so the profile alone tells whether the first was handed
    back.  On an MI355X the lists of period 585 (4088 steps at most) and 513 (3584) are the class's launches and nothing else; the list of
    period 512 (4592) adds the single call's kernels, and that call completes at the exact capacity, so the contract does not name it."""
    name, members, w, expect = C.cap(mods[1])[k]
    members = list(members)
    predicted = {i for i, what in expect.items() if what == C.BACK}
    assert all(what != C.EITHER for what in expect.values())
    back, prof = _by_contract(mods, oracle, members, w)
    print(name, "handed back:", sorted(back), prof)
    assert back <= predicted, (name, back)                                    # (a member the single call completes at the exact capacity does not show here)
    assert all(prof.get(x) == 1 for x in GROUP), prof
    assert (prof == ONLY) == (not predicted), (name, prof)                    # the single call's kernels appear for a member handed back, and only then
    prof = _host(mods, oracle, members, w)
    assert all(prof.get(x) == 1 for x in TILE), prof
    if not predicted:
        assert prof == ONLY, (name, prof)


# ---------------------------------------------------------------- 4: more bytes than a group
def _rest(prof):
    """what a profile holds beside the class's launches and the group's two"""
    return {x: v for x, v in prof.items() if x not in GROUP}


def test_two_groups(mods, oracle):
    """Every launch of the class and of the group exactly groups(...) times; beside them exactly the launches of ONE single call, the
    escaped member's, count for count -- in the device form the device single call's, in the host form (which hands the member to the
    host single call as well) CompressAsync's.  A second member handed back, by a give-up word left in the re-laid scratch for instance,
    would double a count."""
    _lib, lz = mods
    (name, members, w, expect), = C.two_groups(lz)
    members = list(members)
    g = C.groups(lz, members, w)
    assert g == 2
    esc = expect["escaped"]
    want = _want(oracle, members[esc], w)
    got, alone_dev, _ = _prof(_lib, lambda: _single_dev(_lib, "rsn_lzss_compress_dev", members[esc], lz.compress_bound(len(members[esc])), w))
    assert got == want
    got, alone_host, _ = _prof(_lib, lambda: lz.CompressAsync(members[esc], False, w))
    assert got == want
    assert alone_dev and alone_host and not (set(alone_dev) | set(alone_host)) & set(GROUP)
    prof, _ = _dev(mods, oracle, members, w, loose=(esc,))
    print(name, "device form:", prof, "single:", alone_dev)
    assert {x: prof.get(x) for x in GROUP} == {x: g for x in GROUP}, prof
    assert _rest(prof) == alone_dev, (prof, alone_dev)
    prof = _host(mods, oracle, members, w)
    print(name, "host form:", prof, "single:", alone_host)
    assert {x: prof.get(x) for x in GROUP} == {x: g for x in GROUP}, prof
    assert _rest(prof) == alone_host, (prof, alone_host)


# ---------------------------------------------------------------- 5: a seeded fuzz
@pytest.mark.parametrize("seed", C.FUZZ_SEEDS)
def test_fuzz(mods, oracle, seed):
    """The contract names the members whose single call asked for its bound; a single call that completes at the exact capacity shows only
    in the profile.  ONCE counts the single calls of a list: a launch every single call of a member of these lengths makes exactly once."""
    _lib, lz = mods
    name, members, w, expect = C.fuzz(lz, seed)
    members = list(members)
    _, alone, _ = _prof(_lib, lambda: _single(lz, C.PAD + b"!", w))
    assert alone.get(ONCE) == 1, alone
    back, prof = _by_contract(mods, oracle, members, w)
    singles = prof.get(ONCE, 0)
    print(name, w, "handed back by the contract:", sorted(back), "single calls:", singles, sorted(expect.values()))
    free = sum(1 for what in expect.values() if what != C.TAKEN)
    must = sum(1 for what in expect.values() if what == C.BACK)
    for i in back:
        assert expect[i] != C.TAKEN, (name, i, "handed back without need")
    assert len(back) <= singles, (name, back, prof)
    assert singles <= free, (name, singles, free, "a member the class must take went to the single call")
    assert singles >= must, (name, singles, must, "a member beyond the cap was taken")
    if not free:
        assert prof == ONLY, (name, prof)
    _host(mods, oracle, members, w)
    # the members taken once more behind a list of hand-backs: nothing left in scratch matters
    taken = [d for i, d in enumerate(members) if i not in back]
    if len(taken) >= lz.TILE_GROUP_MIN:
        others = [b"<" * n for n in (66001, 69999)] + [C.PAD] * lz.TILE_GROUP_MIN
        _dev(mods, oracle, others, w, loose=(0, 1))
        prof, _ = _dev(mods, oracle, taken, w)
        assert prof == ONLY, (name, prof)


# ---------------------------------------------------------------- 6: every LZSS class in one call
@pytest.mark.parametrize("short", (False, True))
def test_every_lzss_class_in_one_call(mods, oracle, short):
    _lib, lz = mods
    mid = [_text(5000 + i, 2048 + (i * 929) % 59000) for i in range(lz.MID_GROUP_MIN)]
    small = [_text(5100 + i, 1 + 199 * i) for i in range(6)]
    tiles = [_text(5200 + i % 2, 65537) for i in range(lz.TILE_GROUP_MIN - (1 if short else 0))]
    above = [_text(5300, lz.TILE_IN_MAX + 1)]
    rest = small + tiles + above
    members = []
    for i, d in enumerate(mid):                                               # in index order, the classes interleaved
        members.append(d)
        if i % 3 == 0 and rest:
            members.append(rest.pop(0))
    members += rest
    assert all(2048 <= len(d) <= 61440 for d in mid) and all(len(d) <= 1024 for d in small)
    loose = tuple(i for i, d in enumerate(members) if len(d) > lz.MID_IN_MAX and (short or len(d) > lz.TILE_IN_MAX))
    for prof in (_host(mods, oracle, members), _dev(mods, oracle, members, loose=loose)[0]):
        assert prof.get("lzss_batch_enc") == 1 and prof.get("lzss_batch_mid_enc") == 1, prof
        if short:
            assert not any(x.startswith("lzss_batch_tile_") for x in prof), prof
        else:
            assert all(prof.get(x) == 1 for x in TILE), prof
    got = lz.CompressAsyncBatch(members)
    assert got == [_want(oracle, d, 4096) for d in members]
    assert lz.DecompressBatch(got) == members                                 # the batch's own results, back


# ---------------------------------------------------------------- 7: two threads
def test_two_threads_run_tile_batches_at_once(mods, oracle):
    _, lz = mods
    lists = [list(case[1]) for case in C.landings(lz)]
    ws = [case[2] for case in C.landings(lz)]
    assert lists[0][0] != lists[1][0]
    want = [[_want(oracle, d, w) for d in l] for l, w in zip(lists, ws)]
    errors = []

    def work(t):
        for r in range(3):
            if lz.CompressAsyncBatch(lists[t], ws[t]) != want[t]:
                errors.append((t, r))
    ts = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
