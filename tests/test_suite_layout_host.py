"""CPU test of the batch suite's plan (raisin_amd/csrc/suite_layout.h): the prefix tree of the layer lists, which node
outputs are kept, the run need that counts them and the decompress-only stats block are held against a brute-force statement by a
stand-alone g++ program -- plain host arithmetic, no device."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")


@pytest.fixture(scope="module")
def gxx():
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the layout test")
    return "g++"


def _layout_test(gxx, tmp_path, *flags):
    exe = str(tmp_path / "suite_layout_test")
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I" + SRC, os.path.join(ROOT, "tests", "suite_layout_test.cpp"),
                    "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe, "1500"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "suite layout:" in r.stdout and int(r.stdout.split()[-2]) > 100000, r.stdout


def test_the_plan_is_the_brute_force_statement(gxx, tmp_path):
    _layout_test(gxx, tmp_path)


def test_the_plan_under_the_sanitizers(gxx, tmp_path):
    # a stand-alone program of host code: AddressSanitizer and UBSan link into it directly
    _layout_test(gxx, tmp_path, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def test_the_library_includes_the_header_under_test():
    # suite_layout.h includes nothing of HIP's (the program above compiled with g++ alone), and both units that plan by it include it
    includes = [line.split()[1] for line in open(os.path.join(SRC, "suite_layout.h")) if line.startswith("#include")]
    assert includes and all(i.startswith("<") or i == '"roundtrip_batch_layout.h"' for i in includes), includes
    for unit in ("rsn_api.hip", "roundtrip_batch.hip"):
        assert '#include "suite_layout.h"' in open(os.path.join(SRC, unit)).read(), unit
    assert "suite_layout.h" in open(os.path.join(SRC, "Makefile")).read()
