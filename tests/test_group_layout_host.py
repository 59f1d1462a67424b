"""The staging layout of the grouped batch kernels (raisin_amd/csrc/group_layout.h: the cut into groups and the members' offsets that
group_run.h's run_groups packs by), compiled alone with g++: what keeps a kernel inside its buffers, checked on any machine."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")


@pytest.fixture(scope="module")
def layout_test(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the layout test")
    exe = str(tmp_path_factory.mktemp("layout") / "group_layout_test")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", "-I" + SRC, os.path.join(ROOT, "tests", "group_layout_test.cpp"),
                    "-o", exe], check=True, capture_output=True)
    return exe


def test_groups_and_offsets_of_the_four_classes(layout_test):
    r = subprocess.run([layout_test, "3000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert int(r.stdout.split()[-2]) > 7 * 3000 * 8, r.stdout


def test_the_packer_lays_out_by_the_header_under_test():
    # group_layout.h includes nothing of HIP's (the program above compiled with g++ alone), and run_groups takes its offsets from it
    includes = [line for line in open(os.path.join(SRC, "group_layout.h")) if line.startswith("#include")]
    assert includes and all(line.split()[1] in ("<cstddef>", "<cstdint>") for line in includes), includes
    packer = open(os.path.join(SRC, "group_run.h")).read()
    assert '#include "group_layout.h"' in packer and "next_group(" in packer and "GroupLayout " in packer
