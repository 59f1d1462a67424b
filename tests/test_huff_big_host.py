"""The big class of the Huffman compress batch (csrc/huff_big.hip) as far as it shows without a device: the planner at the
class's counts against the host's Go-exact tree, codes and header; what the plan refuses (a code beyond 24 bits, a header beyond its
derived bound); the tiles, the scratch, the slots and the tiles' bit offsets against naive loops; a member coded tile by tile against the
serial stream (tests/huff_big_plan_test.cpp, also under the address and undefined-behaviour sanitizers as a plain program); and the
constants of csrc/huff_big_layout.h, their one home, and of csrc/codecs.h against their mirrors in raisin_amd/huffman.py.  Runs on any machine."""
import os
import re
import shutil
import subprocess

import pytest

import long_codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")


def _build(tmp_path_factory, name, extra):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner test")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + SRC] + extra + [os.path.join(ROOT, "tests", "huff_big_plan_test.cpp"),
                    os.path.join(SRC, "huff_host.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def plan_test(tmp_path_factory):
    return _build(tmp_path_factory, "huff_big_plan_test", ["-O2"])


def _texts(path, names):
    src = open(os.path.join(SRC, path)).read()
    out = {}
    for name in names:
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, src)
        assert m, name
        out[name] = m.group(1).strip()
    return out


def _constants(path, names):
    return {k: int(eval(v.replace("u", ""), {})) for k, v in _texts(path, names).items()}   # (a number, or 1u << 20)


def test_plan_layout_and_tiled_members(plan_test):
    r = subprocess.run([plan_test, "20000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    word, tables, members = r.stdout.split()
    assert word == "ok" and int(tables) >= 20000 + 127 * 7 and int(members) >= 37, r.stdout


def test_the_same_under_the_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "huff_big_plan_test_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    r = subprocess.run([exe, "2000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok "), r.stdout


def _table(plan_test, counts):
    r = subprocess.run([plan_test, "table"] + ["%d:%d" % kv for kv in sorted(counts.items())], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    f = r.stdout.split()
    return {"max_len": int(f[1]), "header": int(f[3]), "refused": bool(int(f[5]))}


def test_a_code_of_24_bits_is_taken_and_one_of_25_refused(plan_test):
    from raisin_amd import huffman
    # a code of d bits needs fib(d + 2) bytes at least -- 196418 for 25 -- and F1..F26, 317810 bytes, where no tie decides: the plan refuses
    # it whatever the class's upper limit is, and F1..F25, a member of the class, is taken
    for k, deepest in ((25, 24), (26, 25)):
        counts = long_codes.fib_counts(k)
        assert sum(counts.values()) == (196417, 317810)[k - 25] > huffman.MID_IN_MAX
        assert max(len(c) for c in long_codes.codes(counts).values()) == deepest
        got = _table(plan_test, counts)
        assert got["max_len"] == deepest and got["refused"] == (deepest > 24), got
    assert sum(long_codes.fib_counts(25).values()) <= huffman.BIG_IN_MAX


def _header_bound(n):
    """huff_big_layout.h's big_hdr_bound, worked out again: the most digits of at most 128 counts that sum to at most n, bought cheapest first"""
    best = 0
    for a in range(2, 129):
        left, digits, step = n - a, a, 9
        while step <= left:
            k = min(left // step, a)
            digits, left, step = digits + k, left - k * step, step * 10
            if k < a:
                break
        best = max(best, digits + 2 * a + 1 + 3)
    return best


def test_the_header_bound_is_reached_and_not_exceeded(plan_test):
    from raisin_amd import huffman
    src = open(os.path.join(SRC, "huff_big_layout.h")).read()
    bound = int(re.search(r"static_assert\(HUFF_BIG_HDR_MAX == (\d+),", src).group(1))
    assert bound == _header_bound(huffman.BIG_IN_MAX) and _header_bound(1 << 20) == 874
    five = (huffman.BIG_IN_MAX - 128 * 1000) // 9000                          # counts of five digits that the largest member buys beside counts of four
    assert 0 < five < 128
    longest = {b: 10000 if b < five else 1000 for b in range(128)}
    assert sum(longest.values()) <= huffman.BIG_IN_MAX < sum(longest.values()) + 9000
    got = _table(plan_test, longest)
    assert got == {"max_len": got["max_len"], "header": bound, "refused": False}
    assert len(long_codes.header(longest)) + 3 == bound
    beyond = dict(longest)
    beyond[five] = 10000                                                      # one digit more: only a member beyond the class has it
    assert sum(beyond.values()) > huffman.BIG_IN_MAX
    got = _table(plan_test, beyond)
    assert got["header"] == bound + 1 and got["refused"]
    assert bound <= 1100                                                      # HUFF_HDR_MAX stays what it was


def test_mirrored_constants_are_the_headers():
    from raisin_amd import huffman
    # the class's limits are stated in the layout header alone; codecs.h names them
    assert _texts("codecs.h", ["HUFF_BIG_IN_MAX", "HUFF_BIG_TILE"]) == {"HUFF_BIG_IN_MAX": "BIGL_IN_MAX", "HUFF_BIG_TILE": "BIGL_TILE"}
    h = _constants("codecs.h", ["HUFF_BIG_GROUP_MIN", "HUFF_BIG_GROUP_BYTES", "HUFF_MID_IN_MAX"])
    h.update({"HUFF_BIG_" + k[5:]: v for k, v in _constants("huff_big_layout.h", ["BIGL_IN_MAX", "BIGL_TILE"]).items()})
    assert huffman.BIG_IN_MAX == h["HUFF_BIG_IN_MAX"]
    assert huffman.BIG_TILE == h["HUFF_BIG_TILE"]
    assert huffman.BIG_GROUP_MIN == h["HUFF_BIG_GROUP_MIN"]
    assert huffman.BIG_GROUP_BYTES == h["HUFF_BIG_GROUP_BYTES"]
    assert huffman.MID_IN_MAX == h["HUFF_MID_IN_MAX"] < huffman.BIG_IN_MAX
    assert huffman.BIG_IN_MAX % huffman.BIG_TILE == 0 and huffman.BIG_GROUP_MIN >= 4
    assert (huffman.BIG_IN_MAX << 8) < 1 << 32                                # a count and a node id in one word


def test_the_other_classes_cutoffs_did_not_move():
    from raisin_amd import huffman
    assert (huffman.BATCH_COMPRESS_INPUT_MAX, huffman.MID_IN_MAX, huffman.MID_GROUP_MIN) == (16384, 65536, 4)
    src = open(os.path.join(SRC, "huff_plan_small.h")).read() + open(os.path.join(SRC, "huff_parse_small.h")).read() + open(os.path.join(SRC, "group_layout.h")).read()
    assert re.search(r"PLAN_COUNT_LIMIT\s*=\s*1u << 16;", src) and re.search(r"PARSE_HDR_MAX\s*=\s*1100;", src) and re.search(r"HUFF_HDR_MAX\s*=\s*1100;", src)
