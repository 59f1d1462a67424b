"""The arithmetic under the grouped batch classes' shared host code, compiled alone with g++ and run on any machine: the layout of a run of
host members through a class's device form (raisin_amd/csrc/group_layout.h's RunLayout, group_run.h's run_members_staged -- production runs are 256 MiB,
so this is where the cut into runs is covered), and which members the rune classes behind the rows take (raisin_amd/csrc/huff_rune_select.h,
codecs.h's BehindClass)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")
PROGRAMS = {"run_layout_test": ("run layout:", 20000), "rune_select_test": ("rune select:", 50)}


def _build_and_run(tmp_path, name, *flags):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the host tests")
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-Werror", *flags, "-I" + SRC, os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe],
                   check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    words, least = PROGRAMS[name]
    assert r.stdout.startswith(words) and int(r.stdout.split()[-2]) >= least, r.stdout


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_program(tmp_path, name):
    _build_and_run(tmp_path, name)


@pytest.mark.parametrize("name", sorted(PROGRAMS))
def test_program_under_the_sanitizers(tmp_path, name):
    # a stand-alone program of host code: AddressSanitizer and UBSan link into it directly
    _build_and_run(tmp_path, name, "-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _own_includes(header):
    return [line.split()[1] for line in open(os.path.join(SRC, header)) if line.startswith("#include") and '"' in line]


def test_the_drivers_go_by_the_headers_under_test():
    # neither header includes anything of HIP's (the programs above compiled with g++ alone) ...
    assert _own_includes("group_layout.h") == []
    assert _own_includes("huff_rune_select.h") == ['"group_layout.h"', '"huff_parse_small.h"']
    # ... the one run takes its cut, its offsets and `down` from the first, and both tiled classes go through that run
    runner = open(os.path.join(SRC, "group_run.h")).read()
    assert '#include "group_layout.h"' in runner and "run_need(" in runner and "RunLayout " in runner and "run_down(" in runner
    # (the decoder, which packs a plan table, by its own call; the classes whose input goes up as it is through run_members_copied, its one user)
    assert runner.count("run_members_staged<") == 1 and runner.count("return run_members_staged<0>(") == 1 and runner.count("int run_members_copied(") == 1
    for unit, call in (("huff_big.hip", "run_members_copied("), ("huff_big_dec.hip", "run_members_staged<"), ("lzss_tile.hip", "run_members_copied("), ("lzss_tile_dec.hip", "run_members_copied(")):
        text = open(os.path.join(SRC, unit)).read()
        assert text.count(call) == 1 and text.count("run_members_staged<") + text.count("run_members_copied(") == 1 and "STAGE_IN" not in text and "next_group(" not in text, unit
    # ... and both forms of both offers choose through the second: the flows hold no selection of their own
    # (the decoders' two offers are one pair for both classes, huff_rune_dec_body.h, and each unit instantiates the pair once)
    enc, dec = (open(os.path.join(SRC, u)).read() for u in ("huff_rune.hip", "huff_rune_dec_body.h"))
    assert enc.count("rune_class_members(") == 2
    assert dec.count("rune_dec_candidates<L>(") == 2 and dec.count("rune_dec_leave<L>(") == 2 and dec.count("rune_dec_planned<L>(") == 3
    for u in ("huff_rune_dec.hip", "huff_rune_mid_dec.hip"):
        text = open(os.path.join(SRC, u)).read()
        assert text.count("rune_dec_offer<") == 1 and text.count("rune_dec_offer_dev<") == 1 and "rune_dec_candidates" not in text and "rune_dec_leave" not in text and "rune_dec_planned" not in text, u
    api = open(os.path.join(SRC, "rsn_api.hip")).read()
    assert "rune_class_members" not in api and "rune_dec_" not in api and "huff_rune_class(" not in api and "huff_rune_dec_class(" not in api
    assert api.count("->offer(") + api.count(".offer(") == 1 and api.count("offer_dev(") == 1
