"""The host side of the mid-size rune class of the Huffman compress batch (raisin_amd/csrc/huff_rune_mid.hip), on any machine:
which members it takes out of the RUNES pool and what the 16 KiB class makes of the rest (huff_rune_mid_select.h, compiled alone with g++
against a brute-force statement of the rules, and once more under the address and undefined-behaviour sanitizers), the rune planner at
counts up to 65535 (huff_plan_rune.h with huff_host.cpp), and the constants the Python package mirrors."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")
SANITIZERS = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _build(tmp_path, name, *flags, extra=()):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the host tests")
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I" + SRC, os.path.join(ROOT, "tests", name + ".cpp"), *extra, "-o", exe],
                   check=True, capture_output=True)
    return exe


@pytest.mark.parametrize("flags", [(), SANITIZERS], ids=["plain", "sanitizers"])
def test_selection_against_the_brute_force_statement(tmp_path, flags):
    # a stand-alone program of host code: AddressSanitizer and UBSan link into it directly
    r = subprocess.run([_build(tmp_path, "rune_mid_select_test", *flags)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("rune mid select:") and int(r.stdout.split()[-2]) >= 2000, r.stdout


def test_planner_at_the_larger_counts_equals_host(tmp_path):
    # 65534 beside 1 and 2, the digit boundaries, 256 x 256, Fibonacci counts to 21 and 22 bits, ties across the widths, 400 random alphabets
    exe = _build(tmp_path, "huff_rune_mid_plan_test", *SANITIZERS, extra=(os.path.join(SRC, "huff_host.cpp"),))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(r.stdout.split()[-1]) >= 400 + 20, r.stdout


def _constant(path, name):
    m = re.search(r"constexpr\s+\w+\s+(?:\w+\s*=\s*[^,;]+,\s*)*%s\s*=\s*([^;,]+)[;,]" % name, open(os.path.join(SRC, path)).read())
    assert m, name
    return int(m.group(1).strip())


def test_mirrored_constants_are_the_headers():
    from raisin_amd import huffman
    assert huffman.RUNE_MID_IN_MAX == _constant("huff_rune_mid_select.h", "HUFF_RUNE_MID_IN_MAX")
    assert huffman.RUNE_MID_GROUP_MIN == _constant("huff_rune_mid_select.h", "HUFF_RUNE_MID_GROUP_MIN")
    assert huffman.RUNE_MID_IN_MAX == huffman.MID_IN_MAX == 65536 and huffman.RUNE_MID_GROUP_MIN >= 16
    assert huffman.BATCH_COMPRESS_INPUT_MAX == _constant("huff_rune_select.h", "HUFF_RUNE_IN_MAX") == 16384     # where the class begins
    assert _constant("huff_plan_rune.h", "PLAN_RUNE_MID_COUNT_MAX") == huffman.RUNE_MID_IN_MAX and _constant("huff_plan_rune.h", "PLAN_RUNE_COUNT_MAX") == 16384
    # the values the other rune tests pin stay
    assert (huffman.RUNE_GROUP_MIN, huffman.RUNE_SYMS_MAX, huffman.RUNE_OUT_MAX, huffman.RUNE_PAY_MAX, huffman.RUNE_DEC_GROUP_MIN) == (16, 256, 16384, 18432, 16)


def test_the_class_is_wired_through_the_shared_pieces():
    # plain host selection; both offers choose through it; listed ahead of the 16 KiB class; the API unit names no class
    assert [ln.split()[1] for ln in open(os.path.join(SRC, "huff_rune_mid_select.h")) if ln.startswith("#include")] == ['"huff_rune_select.h"']
    unit = open(os.path.join(SRC, "huff_rune_mid.hip")).read()
    assert unit.count("rune_mid_class_members(") == 2 and "class_run<RuneMidEncClass>" in unit and "class_run_dev<RuneMidEncClass>" in unit
    assert '"huff_batch_rune_mid_enc"' in unit and "func_dyn_lds(" in unit and "asm" not in unit
    # the kernel is the one body of both rune encoders: each unit instantiates it and holds no count loop of its own, and the body holds
    # the tree of the rune alphabet, through the one wavefront helper (huff_small_body.h)
    small = open(os.path.join(SRC, "huff_rune.hip")).read()
    for text in (unit, small):
        assert '#include "huff_rune_body.h"' in text and text.count("huff_rune_enc_body<") == 1 and "atomicCAS(" not in text and "plan_tree" not in text
    body = open(os.path.join(SRC, "huff_rune_body.h")).read()
    assert body.count("atomicCAS(") == 1 and body.count("wave_tree<PLAN_RUNE_IDB>(") == 1 and "asm" not in body
    shared = open(os.path.join(SRC, "huff_small_body.h")).read()
    assert '#include "huff_small_body.h"' in body and shared.count("plan_tree<IDB>(") == 1 and "asm" not in shared
    rows = open(os.path.join(SRC, "codecs.h")).read()
    assert "{&huff_rune_mid_class(), &huff_rune_class()}" in rows
    api = open(os.path.join(SRC, "rsn_api.hip")).read()
    assert "rune_mid" not in api
    make = open(os.path.join(SRC, "Makefile")).read()
    assert "huff_rune_mid.hip" in make and "huff_rune_mid_select.h" in make and "huff_rune_body.h" in make
