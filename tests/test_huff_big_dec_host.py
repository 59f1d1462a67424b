"""The tiled class of the Huffman decompress batch (csrc/huff_big_dec.hip) as far as it shows without a device: the layout
header against naive loops; the wide form of the stream plan against the host's parse_header / build_tree at counts of 65535, 65536 and
262143 and sums of 262144 and 262145, the narrow form refusing what it refused; a model of the three phases -- every tile's map from all
32 entries, the maps chained, every tile emitted from its entry -- byte for byte against the serial decoder on whole members
(tests/huff_big_dec_plan_test.cpp, also under the address and undefined-behaviour sanitizers as a plain program); and the constants of
csrc/huff_big_dec_layout.h, their one home, and of csrc/codecs.h against their mirrors in raisin_amd/huffman.py.  Runs on any machine."""
import os
import re
import shutil
import subprocess

import pytest

import long_codes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")
SAMIAM = os.path.join(ROOT, "tests", "golden", "samiam.txt")


def _build(tmp_path_factory, name, extra):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the plan test")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + SRC] + extra + [os.path.join(ROOT, "tests", "huff_big_dec_plan_test.cpp"),
                    os.path.join(SRC, "huff_host.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def _run(exe):
    r = subprocess.run([exe, SAMIAM], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    word, layout, headers, members, _, periodic = r.stdout.split()
    assert word == "ok" and periodic == "taken", r.stdout                   # (no phases to lose here; the lane model takes it too: test_lane_maps_host.py)
    return int(layout), int(headers), int(members), periodic


def test_layout_wide_plan_and_the_three_phases(tmp_path_factory):
    layout, headers, members, periodic = _run(_build(tmp_path_factory, "huff_big_dec_plan_test", ["-O2"]))
    # text at four sizes, two symbols, 128 symbols, the flat code, F1..F25, samiam repeated
    assert layout >= 2000 and headers >= 17 and members == 9, (layout, headers, members)
    assert periodic == "taken"                                                # the tile-level model has no phases to lose; the lanes' model (tests/lane_maps.py) agrees


def test_the_same_under_the_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "huff_big_dec_plan_test_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert _run(exe)[2] == 9


def _texts(path, names):
    src = open(os.path.join(SRC, path)).read()
    out = {}
    for name in names:
        m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, src)
        assert m, name
        out[name] = m.group(1).strip()
    return out


def _constants(path, names):
    return {k: int(eval(v.replace("u", ""), {})) for k, v in _texts(path, names).items()}


def test_mirrored_constants_are_the_headers():
    from raisin_amd import huffman
    # the classes' limits are stated in the layout headers alone; codecs.h names them
    assert _texts("codecs.h", ["HUFF_BIG_OUT_MAX", "HUFF_BIG_PAY_MAX", "HUFF_BIG_IN_MAX"]) == {"HUFF_BIG_OUT_MAX": "BIGD_OUT_MAX", "HUFF_BIG_PAY_MAX": "BIGD_PAY_MAX", "HUFF_BIG_IN_MAX": "BIGL_IN_MAX"}
    h = _constants("codecs.h", ["HUFF_BIG_DEC_GROUP_MIN", "HUFF_MID_OUT_MAX", "HUFF_BIG_GROUP_BYTES"])
    h.update({"HUFF_BIG_" + k[5:]: v for k, v in _constants("huff_big_dec_layout.h", ["BIGD_OUT_MAX", "BIGD_PAY_MAX"]).items()})
    h["HUFF_BIG_IN_MAX"] = _constants("huff_big_layout.h", ["BIGL_IN_MAX"])["BIGL_IN_MAX"]
    assert (huffman.BIG_OUT_MAX, huffman.BIG_PAY_MAX, huffman.BIG_DEC_GROUP_MIN) == (h["HUFF_BIG_OUT_MAX"], h["HUFF_BIG_PAY_MAX"], h["HUFF_BIG_DEC_GROUP_MIN"])
    assert huffman.MID_OUT_MAX == h["HUFF_MID_OUT_MAX"] < huffman.BIG_OUT_MAX and huffman.BIG_GROUP_BYTES == h["HUFF_BIG_GROUP_BYTES"]
    lay = _constants("huff_big_dec_layout.h", ["BIGD_OUT_MAX", "BIGD_PAY_MAX", "BIGD_LANES", "BIGD_S", "BIGD_OUT_CAP"])
    assert (lay["BIGD_OUT_MAX"], lay["BIGD_PAY_MAX"]) == (h["HUFF_BIG_OUT_MAX"], h["HUFF_BIG_PAY_MAX"])
    assert (huffman.BIG_DEC_LANES, huffman.BIG_DEC_LANE_BITS, huffman.BIG_DEC_OUT_CAP) == (lay["BIGD_LANES"], lay["BIGD_S"], lay["BIGD_OUT_CAP"])
    par = _constants("huff_parse_small.h", ["PARSE_OUT_MAX_WIDE", "PARSE_PAY_MAX_WIDE"])
    assert (par["PARSE_OUT_MAX_WIDE"], par["PARSE_PAY_MAX_WIDE"]) == (h["HUFF_BIG_OUT_MAX"], h["HUFF_BIG_PAY_MAX"])
    # the decoder takes every stream the encoder writes: at most 7 bits a byte of a byte alphabet
    assert huffman.BIG_OUT_MAX >= huffman.BIG_IN_MAX == h["HUFF_BIG_IN_MAX"] and 8 * huffman.BIG_PAY_MAX >= 7 * huffman.BIG_IN_MAX
    assert huffman.BIG_DEC_GROUP_MIN >= 2 and (huffman.BIG_OUT_MAX << 8) < 1 << 32


def test_the_fibonacci_member_is_of_the_class():
    from raisin_amd import huffman
    counts = long_codes.fib_counts(25)
    assert huffman.MID_OUT_MAX < sum(counts.values()) == 196417 <= huffman.BIG_OUT_MAX
    assert max(len(c) for c in long_codes.codes(counts).values()) == 24


def test_the_narrow_limits_did_not_move():
    src = open(os.path.join(SRC, "huff_parse_small.h")).read()
    assert re.search(r"PARSE_STREAM_MAX\s*=\s*65536 \+ 2048;", src) and re.search(r"PARSE_OUT_MAX\s*=\s*65536;", src)
    assert re.search(r"PLAN_COUNT_LIMIT\s*=\s*1u << 16;", open(os.path.join(SRC, "huff_plan_small.h")).read())
