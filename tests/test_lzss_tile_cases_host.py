"""The cases of tests/lzss_tile_cases.py are what they claim, decided by the CPU oracle and the module's models alone: every landing event
is in the oracle's chain, the window cases hold the tokens they promise, the step-cap cases sit where their figures say, the long list is
two groups with its special members on the stated sides of the cut, and the fuzz lists are mostly members the class must take.  The
constants the models restate are held against the sources.  Runs on any machine."""
import os
import re

import pytest

import lzss_tile_cases as C

SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "raisin_amd", "csrc")


@pytest.fixture(scope="module")
def lz():
    from raisin_amd import lz
    return lz


def _constant(path, name):
    m = re.search(r"constexpr\s+[\w:]+\s+%s\s*=\s*([^;]+);" % name, open(os.path.join(SRC, path)).read())
    assert m, name
    return m.group(1).strip()


def test_the_models_restate_the_sources(lz):
    assert int(_constant("lzss_tile.hip", "TT")) == C.SUB and int(_constant("lzss_tile.hip", "T_STEP_CAP")) == C.STEP_CAP
    assert int(_constant("lzss_tile_layout.h", "LZT_TILE")) == C.TILE == lz.TILE_POS == 2 * C.SUB and int(_constant("lzss_tile_layout.h", "LZT_W_MAX")) == C.W_MAX
    assert int(_constant("codecs.h", "SMALL_GROUP_MAX")) == C.GROUP_MEMBERS and int(_constant("group_layout.h", "GROUP_STATUS_BYTES")) == C.STATUS
    src = open(os.path.join(SRC, "group_dev.hip")).read()
    assert "sizeof(GatherEntry) == 48" in src and "struct SmallMember { uint32_t in_off, n, out_off, status_off; }" in open(os.path.join(SRC, "codecs.h")).read()
    assert C.GD_ENTRY == 16 + 48
    f = C.filler()
    assert len(f) == 252 * 252 and len({(int(a), int(b)) for a, b in zip(f, list(f[1:]) + [f[0]])}) == len(f)   # every bigram once
    assert not set(f.tobytes()) & {0x00, 0x3C, 0x5C, 0xFF}


def test_every_landing_event_is_in_the_chain(lz):
    cases = C.landings(lz)
    assert [w for _, _, w, _ in cases] == [4096, 2049]
    for name, members, w, expect in cases:
        assert len(members) >= lz.TILE_GROUP_MIN and all(C.in_class(lz, d, w) for d in members)
        for i, want in expect.items():
            esc = C.escaped(members[i])
            assert esc == members[i]                                           # (nothing of the filler escapes: positions are raw offsets)
            items = C.chain(esc, w)
            seen = C.events(items, len(esc))
            for event in sorted(want):
                assert event in seen, (name, i, event)
            assert max(d for _, _, d in items) <= w
            assert C.steps_bound(esc, w)[0] <= C.STEP_CAP, (name, i)
    assert len(cases[0][3][0]) == 9 and len(cases[1][3][0]) == 8


def test_window_cases_hold_their_tokens(lz, oracle):
    cases = C.windows(lz)
    assert tuple(w for _, _, w, _ in cases) == (1023, 1025, 2047, 2049, 3000, 4095)
    for name, members, w, expect in cases:
        for i, token in expect.items():
            assert len(members[i]) == 70000
            stream = oracle.lzss_compress(members[i], w)
            if token is None:
                assert stream == members[i], (name, i, "a period of W + 1: no token")
            else:
                assert token == b"<%d,%d>" % ((w - 1, w - 1) if i == 0 else (w, w)) and token in stream and len(stream) < 8192, (name, i)
            assert C.steps_bound(members[i], w)[0] <= C.STEP_CAP // 4, (name, i)


def test_cap_cases_sit_where_their_figures_say(lz):
    got = {name: (C.steps_bound(members[0], w), expect[0]) for name, members, w, expect in C.cap(lz)}
    (up, lo), what = got["period 585"]
    assert up == 4088 and what == C.TAKEN, "period 585: 8 steps under the cap"
    (up, lo), what = got["period 513"]
    assert up == 3584 and what == C.TAKEN, "period 513"
    (up, lo), what = got["period 512"]
    assert lo >= 4466 and up == 4592 and what == C.BACK, "period 512: over the cap whatever the order inside the position's own sub-tile"
    for name, members, w, expect in C.cap(lz):
        assert w == 4096 and C.classify(lz, members[0], w) == expect[0], name
    assert C.classify(lz, C.PAD, 4096) == C.TAKEN                             # the member every list is padded with


def test_the_long_list_is_two_groups(lz):
    (name, members, w, expect), = C.two_groups(lz)
    cuts = C.group_cuts(lz, members, w)
    assert C.groups(lz, members, w) == 2 and cuts == [(0, expect["cut"]), (expect["cut"], len(members))], cuts
    cut, top, esc = expect["cut"], expect["top"], expect["escaped"]
    assert top < cut <= esc and len(members[top]) == lz.TILE_IN_MAX and max(len(d) for i, d in enumerate(members) if i != top) <= 66000
    assert len(C.escaped(members[esc])) > C.e_cap(lz, len(members[esc])) and all(len(C.escaped(d)) == len(d) for d in members[:5])
    assert all(65537 <= len(d) for d in members) and len(set(members)) >= 5
    assert all(members[i] != members[i + 1] for i in range(cut - 3, cut + 2))  # distinct on both sides of the cut
    assert len(members[cut - 1]) != len(members[cut])


def test_fuzz_lists_are_mostly_members_the_class_must_take(lz):
    total = free = 0
    assert len({C.FUZZ_WINDOW[seed] for seed in C.FUZZ_SEEDS}) == len(C.FUZZ_SEEDS) == 4 and sum(1 for w in C.FUZZ_WINDOW.values() if w % C.SUB) == 3
    reach = max(C.steps_bound(C.escaped(d), w)[0] for _, members, w, _ in (C.fuzz(lz, seed) for seed in C.FUZZ_SEEDS) for d in members)
    assert 3000 <= reach <= C.STEP_CAP, "the fuzz comes near the step cap, from below: %d" % reach
    for seed in C.FUZZ_SEEDS:
        name, members, w, expect = C.fuzz(lz, seed)
        assert w == C.FUZZ_WINDOW[seed] and w in C.FUZZ_WINDOWS and len(members) == lz.TILE_GROUP_MIN + 4 and all(C.in_class(lz, d, w) and len(d) <= 140000 for d in members)
        total += len(members)
        free += sum(1 for what in expect.values() if what != C.TAKEN)
    assert 4 * free <= total, "more than a quarter of the fuzz members may be handed back: %d of %d" % (free, total)
