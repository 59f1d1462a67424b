"""The grouped Huffman encoder's planner (raisin_amd/csrc/huff_plan_small.h: the code k_huff_batch_enc runs in one wavefront per member)
against the host's Go-exact tree, codes and header (huff_host.cpp), compiled together with g++.  Runs on any machine."""
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
    exe = str(tmp_path_factory.mktemp("plan") / "huff_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + SRC, os.path.join(ROOT, "tests", "huff_plan_test.cpp"),
                    os.path.join(SRC, "huff_host.cpp"), "-o", exe], check=True, capture_output=True)
    return exe


def test_planner_equals_host_on_tie_heavy_and_random_tables(planner_test):
    r = subprocess.run([planner_test, "100000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    n = int(r.stdout.split()[-1])
    assert n >= 100000 + 127 * 7, r.stdout


def test_planner_header_compiles_for_the_device_too():
    # the kernel includes the same header (huff_small.hip); the host half of it must not need the device compiler
    # (the qualifier that says so is tile_layout.h's RSN_HD_FN, the one every plain-code header uses)
    text = open(os.path.join(SRC, "huff_plan_small.h")).read()
    shared = open(os.path.join(SRC, "tile_layout.h")).read()
    assert '#include "tile_layout.h"' in text and "RSN_HD_FN" in text and "__HIPCC__" not in text
    assert "#if defined(__HIPCC__)\n#define RSN_HD_FN __host__ __device__" in shared and "#else\n#define RSN_HD_FN inline\n#endif" in shared
    assert '#include "huff_plan_small.h"' in open(os.path.join(SRC, "huff_small.hip")).read()
