"""The device-side plan of a Huffman stream (raisin_amd/csrc/huff_parse_small.h: the code k_huff_dev_plan runs, a workgroup per member of
rsn_huffman_decompress_batch_dev) against the host's parse_header + build_tree + assign_codes (huff_host.cpp), restated as
small_dec_plan's fields, compiled together with g++ alone.  Runs on any machine; once more under AddressSanitizer and UBSan, where the
plan works on a copy of the stream in an allocation of exactly n bytes."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")


def _run(tmp_path, rounds, *flags):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the parse test")
    exe = str(tmp_path / "huff_parse_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I" + SRC, os.path.join(ROOT, "tests", "huff_parse_test.cpp"),
                    os.path.join(SRC, "huff_host.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe, str(rounds)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[0] == "ok", r.stdout
    return {k: int(v) for k, v in zip(words[2::2], words[3::2])} | {"streams": int(words[1])}


def test_plan_equals_the_host_on_own_foreign_and_malformed_headers(tmp_path):
    got = _run(tmp_path, 40000)
    assert got["streams"] > 40000 and got["planned"] > 1500, got
    # the device refuses a count of 65536 that the host takes: exactly the two streams the program constructs
    assert got["stricter"] == 2, got
    # the Fibonacci tables reach codes far beyond the lookup table's DEC_K = 9 bits (K < the deepest code: the tree walk behind the table)
    assert got["deepest"] >= 21, got


def test_plan_under_the_sanitizers(tmp_path):
    # a stand-alone program of host code: AddressSanitizer and UBSan link into it directly
    got = _run(tmp_path, 5000, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")
    assert got["stricter"] == 2, got


def test_the_header_compiles_for_the_device_too():
    text = open(os.path.join(SRC, "huff_parse_small.h")).read()
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert includes == ['"huff_plan_small.h"'], includes                # no HIP include on the host side
    # the qualifier is tile_layout.h's, the one every plain-code header uses, which huff_plan_small.h includes and nothing else
    plan = open(os.path.join(SRC, "huff_plan_small.h")).read()
    assert [line.split()[1] for line in plan.splitlines() if line.startswith("#include")] == ["<cstdint>", '"tile_layout.h"']
    shared = open(os.path.join(SRC, "tile_layout.h")).read()
    assert "RSN_HD_FN" in text and "#define RSN_HD_FN __host__ __device__" in shared
    assert [line.split()[1] for line in shared.splitlines() if line.startswith("#include")] == ["<cstdint>"]
    kernel = open(os.path.join(SRC, "huff_dev.hip")).read()
    assert '#include "huff_parse_small.h"' in kernel and "parse_scan(" in kernel and "wave_tree<8>(" in kernel
    # ... the tree through the one wavefront helper, which is where plan_tree is called
    body = open(os.path.join(SRC, "huff_small_body.h")).read()
    assert '#include "huff_small_body.h"' in kernel and body.count("plan_tree<IDB>(") == 1 and body.count("plan_codes<IDB>(") == 1
