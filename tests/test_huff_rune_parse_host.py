"""The grouped rune decoder's plan of a stream (raisin_amd/csrc/huff_parse_rune.h: the code k_huff_batch_rune_dec runs per member, the
light scan k_huff_dev_rune_plan and the host's classifier run) against the host's parse_header, build_tree and assign_codes
(huff_host.cpp), compiled together with g++ and the address and undefined-behaviour sanitizers.  Runs on any machine."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")


@pytest.fixture(scope="module")
def parse_test(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the parse test")
    exe = str(tmp_path_factory.mktemp("rune_parse") / "huff_rune_parse_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + SRC, os.path.join(ROOT, "tests", "huff_rune_parse_test.cpp"), os.path.join(SRC, "huff_host.cpp"), "-o", exe],
                   check=True, capture_output=True)
    return exe


def test_rune_parse_equals_host(parse_test):
    # the library's own headers of 2 to 257 runes, foreign orders, duplicates, zero counts, the header's special bytes, invalid forms,
    # a rune the separator cuts, every refusal, the scan limit's three positions, tails behind n, 3000 random alphabets and headers
    r = subprocess.run([parse_test, "3000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) >= 6000 and int(words[3]) >= 3000, r.stdout


def test_rune_parse_is_the_code_the_kernels_run():
    # one header for the host test and both kernels, the tree and the ranks shared with the rune encoder, the payload's decoder shared
    # with the byte decoders
    text = open(os.path.join(SRC, "huff_parse_rune.h")).read()
    assert '#include "huff_plan_rune.h"' in text and '#include "huff_parse_small.h"' in text and "parse_rune_plan_serial" in text
    # (the kernel's text is the one body of both rune decoders; the unit is its LDS and one call of it)
    kernel = open(os.path.join(SRC, "huff_rune_dec_body.h")).read()
    assert '#include "huff_parse_rune.h"' in kernel and '#include "huff_small_body.h"' in kernel and kernel.count("wave_tree<PLAN_RUNE_IDB>(") == 1
    assert "rune_light_plan<T, L>(" in kernel and kernel.count("plan_rune_ranks(") == 1 and kernel.count("lane_dec_body<") == 1
    assert "parse_rune_scan<L>(" in open(os.path.join(SRC, "huff_rune_dec_plan.h")).read()
    unit = open(os.path.join(SRC, "huff_rune_dec.hip")).read()
    assert '#include "huff_rune_dec_body.h"' in unit and "rune_dec_body<RS>(" in unit and "rune_plan_body<RS>(" in unit and "using RS = ParseRuneSmall;" in unit
    assert "void k_huff_batch_rune_dec(" in unit and "void k_huff_dev_rune_plan(" in unit
    body = open(os.path.join(SRC, "huff_small_body.h")).read()
    assert body.count("uint32_t run_path(") == 1 and body.count("void emit_path(") == 1      # one decoder, not two
    assert body.count("plan_tree<IDB>(") == 1 and body.count("plan_codes<IDB>(") == 1          # ... and one tree in a wavefront: wave_tree calls them
