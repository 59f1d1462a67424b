"""The grouped rune encoder's planner (raisin_amd/csrc/huff_plan_rune.h: the code k_huff_batch_rune_enc runs per member, with
huff_plan_small.h's tree and codes at 9 bits of node id) against the host's Go-exact leaf order, tree, codes and header
(huff_host.cpp), compiled together with g++ and the address and undefined-behaviour sanitizers.  Runs on any machine."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")


@pytest.fixture(scope="module")
def planner_test(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the planner test")
    exe = str(tmp_path_factory.mktemp("rune_plan") / "huff_rune_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + SRC, os.path.join(ROOT, "tests", "huff_rune_plan_test.cpp"), os.path.join(SRC, "huff_host.cpp"), "-o", exe],
                   check=True, capture_output=True)
    return exe


def test_rune_planner_equals_host(planner_test):
    # 2 symbols, 256 equal counts, counts 1..256, Fibonacci counts, the header's special entries, every alphabet size, 2000 random alphabets
    r = subprocess.run([planner_test, "2000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    n = int(r.stdout.split()[-1])
    assert n >= 2000 + 2 * 255 + 14, r.stdout


def test_rune_planner_is_the_code_the_kernel_runs():
    # one header for the host test and the kernel, the tree and the codes shared with the byte planner, the UTF-8 rule shared with the flat path
    text = open(os.path.join(SRC, "huff_plan_rune.h")).read()
    assert '#include "huff_plan_small.h"' in text and "plan_rune_ranks" in text
    # both rune encoders reach them through their one body, and the body reaches the tree through the one wavefront helper: the planner's
    # code is named there and nowhere beside it
    body = open(os.path.join(SRC, "huff_rune_body.h")).read()
    assert '#include "huff_plan_rune.h"' in body and '#include "huff_utf8.h"' in body and '#include "huff_small_body.h"' in body
    assert body.count("wave_tree<PLAN_RUNE_IDB>(") == 1 and "plan_tree<" not in body
    shared = open(os.path.join(SRC, "huff_small_body.h")).read()
    assert '#include "huff_plan_small.h"' in shared and shared.count("plan_tree<IDB>(") == 1 and shared.count("plan_codes<IDB>(") == 1
    for unit in ("huff_rune.hip", "huff_rune_mid.hip"):
        kernel = open(os.path.join(SRC, unit)).read()
        assert '#include "huff_rune_body.h"' in kernel and "huff_rune_enc_body<" in kernel and "plan_tree" not in kernel, unit
    flat = open(os.path.join(SRC, "huff_encode.hip")).read()
    assert '#include "huff_utf8.h"' in flat and "int seq_len(" not in flat
