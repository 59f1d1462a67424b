"""The host side of the mid-size grouped rune decoder (raisin_amd/csrc/huff_rune_mid_dec.hip), on any machine: the parse at the
mid limits against the host's parse_header, build_tree and assign_codes, the default limits against today's constants, and the select
rules against a brute-force statement (tests/huff_rune_mid_dec_plan_test.cpp: g++ alone, a stand-alone program, once more under the address
and undefined-behaviour sanitizers); the constants the Python package mirrors; how the class is wired through the shared pieces; and the
verdict of the CPU model of the lane maps (tests/lane_maps.py, unchanged, with this class's shape) on every member the GPU tests run
(tests/rune_mid_dec_cases.py)."""
import os
import re
import shutil
import subprocess

import pytest

import rune_mid_dec_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")
SANITIZERS = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all")


def _run(tmp_path, *flags):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the host tests")
    exe = str(tmp_path / "huff_rune_mid_dec_plan_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", *flags, "-I" + SRC, os.path.join(ROOT, "tests", "huff_rune_mid_dec_plan_test.cpp"),
                    os.path.join(SRC, "huff_host.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe, "400"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("rune mid dec: ok"), r.stdout
    w = r.stdout.split()
    return {w[k]: int(w[k + 1]) for k in (3, 5, 7, 9, 11)}, [int(x) for x in w[w.index("consts") + 1:]]


@pytest.mark.parametrize("flags", [(), SANITIZERS], ids=["plain", "sanitizers"])
def test_parse_and_rules_against_the_host(tmp_path, flags):
    # a stand-alone program of host code: AddressSanitizer and UBSan link into it directly
    figures, _ = _run(tmp_path, *flags)
    # (400 random streams and the 18 edges, each at both sets of limits)
    assert figures["ok"] >= 2 * (400 + 18) and figures["planned"] >= 200 and figures["trials"] >= 3000 and figures["took"] >= 500 and figures["below"] >= 20, figures


def test_mirrored_constants_are_the_headers(tmp_path):
    from raisin_amd import huffman
    _, consts = _run(tmp_path)
    out_max, pay_max, group_min, stream_max, pay_min = consts
    assert (huffman.RUNE_MID_OUT_MAX, huffman.RUNE_MID_PAY_MAX, huffman.RUNE_MID_DEC_GROUP_MIN) == (out_max, pay_max, group_min) == (65536, 69120, 16)
    assert pay_max == 960 * 576 // 8 and stream_max == 256 * 10 + 3 + 8 + pay_max and pay_min == 513
    assert (C.OUT_MAX, C.PAY_MAX, C.N, C.OUT_MIN) == (out_max, pay_max, group_min, huffman.RUNE_OUT_MAX)
    assert (C.SHAPE.lanes, C.SHAPE.blocks, C.SHAPE.s_max, C.SHAPE.pay_max, C.SHAPE.out_max, C.SHAPE.runes) == (960, 1, 576, pay_max, out_max, True)
    # the values the other rune tests pin stay
    assert (huffman.RUNE_GROUP_MIN, huffman.RUNE_SYMS_MAX, huffman.RUNE_OUT_MAX, huffman.RUNE_PAY_MAX, huffman.RUNE_DEC_GROUP_MIN) == (16, 256, 16384, 18432, 16)
    assert "RUNE_MID_OUT_MAX" in huffman.DecompressBatch.__doc__


def test_the_class_is_wired_through_the_shared_pieces():
    # plain host selection, one set of three steps for both decoders, at the class's rules; both forms of both classes choose through it;
    # listed behind the 16 KiB class; the API unit names no class
    sel = open(os.path.join(SRC, "huff_rune_select.h")).read()
    assert [ln.split()[1] for ln in sel.splitlines() if ln.startswith("#include") and '"' in ln] == ['"group_layout.h"', '"huff_parse_small.h"'] and "hip" not in sel.replace(".hip", "")
    for step in ("std::vector<size_t> rune_dec_candidates(", "void rune_dec_planned(", "bool rune_dec_leave(", "bool rune_dec_summary_ok("):
        assert sel.count(step) == 1, step
    assert "L::len_may(" in sel and "L::GROUP_MIN" in sel and "L::OUT_MIN" in sel and "L::OUT_MAX" in sel and "L::PAY_MAX" in sel
    assert "HUFF_RUNE_DEC_GROUP_MIN" not in sel and "HUFF_RUNE_OUT_MAX" not in sel and "class L =" not in sel and "group_min" not in sel      # (no class's figures, no default class, no default argument)
    assert not os.path.exists(os.path.join(SRC, "huff_rune_mid_dec_select.h"))
    body = open(os.path.join(SRC, "huff_rune_dec_body.h")).read()
    assert body.count("rune_dec_candidates<L>(") == 2 and body.count("rune_dec_leave<L>(") == 2 and body.count("rune_dec_planned<L>(") == 3
    assert body.count("int rune_dec_offer(") == 1 and body.count("int rune_dec_offer_dev(") == 1 and body.count("void rune_dec_body(") == 1
    assert '#include "huff_rune_dec_plan.h"' in body and body.count("rune_light_plan<T, L>(") == 1 and body.count("parse_rune_light<L>(") == 1
    assert body.count("wave_tree<PLAN_RUNE_IDB>(") == 1 and body.count("plan_rune_ranks(") == 1 and body.count("lane_dec_body<") == 1
    assert body.count("block_excl_scan<") == 2 and body.count("parse_rune_child(") == 2 and body.count("parse_rune_write(") == 1      # (compaction and expand; the two children)
    code = body.split("#pragma once")[1]
    assert "rune_mid" not in code and "ParseRuneMid" not in code and "ParseRuneSmall" not in code and "asm" not in code and '"huffman batch decompress"' in code       # (names no class)
    assert "the %s plan kernel left a summary that is none" in body
    unit = open(os.path.join(SRC, "huff_rune_mid_dec.hip")).read()
    small = open(os.path.join(SRC, "huff_rune_dec.hip")).read()
    assert '"huff_batch_rune_mid_dec"' in unit and '"huff_dev_rune_mid_plan"' in unit and unit.count("func_dyn_lds(") == 1 and "Slot::GD_RUNE_MID_PLANS" in unit and '"mid rune"' in unit
    assert '"huff_batch_rune_dec"' in small and '"huff_dev_rune_plan"' in small and "func_dyn_lds(" not in small and "Slot::GD_RUNE_PLANS" in small and '"rune"' in small
    assert "extern __shared__ uint4 md_lds[]" in unit and "extern __shared__" not in small and small.count("__shared__") == 2
    # no count loop, scan, table, tree or selection of its own in either unit: each is its LDS, one call of the one body at its class's
    # limits, the plan kernel's one-liner and the class struct the one pair of offers is instantiated with
    for text, L, C in ((unit, "ML", "RuneMidDecClass"), (small, "RS", "RuneDecClass")):
        assert '#include "huff_rune_dec_body.h"' in text and text.count("#include") == 1
        assert text.count("rune_dec_body<%s>(" % L) == 1 and text.count("rune_dec_body<") == 1 and text.count("rune_plan_body<%s>(" % L) == 1 and text.count("rune_plan_body<") == 1
        assert text.count("rune_dec_offer<%s>" % C) == 1 and text.count("rune_dec_offer_dev<%s>" % C) == 1 and text.count("rune_dec_offer<") == 1 and text.count("rune_dec_offer_dev<") == 1
        for own in ("parse_rune_scan", "parse_rune_put", "parse_rune_decode", "parse_sep_at", "plan_tree", "plan_codes", "atomicMin", "atomicAdd", "atomicCAS", "run_path(", "emit_path(",
                    "rune_light_plan", "wave_tree", "plan_rune_ranks", "lane_dec_body<", "block_excl_scan", "parse_rune_child", "parse_rune_write", "parse_rune_light",
                    "rune_dec_candidates", "rune_dec_planned", "rune_dec_leave", "run_member_groups", "run_groups_dev", "plan_where_they_lie", "asm", "for ("):
            assert own not in text, own
    assert "using ML = ParseRuneMid;" in unit and "using RS = ParseRuneSmall;" in small
    shared = open(os.path.join(SRC, "huff_rune_dec_plan.h")).read()
    assert shared.count("bool rune_light_plan(") == 1 and shared.count("void rune_plan_body(") == 1
    lanes = open(os.path.join(SRC, "huff_small_body.h")).read()
    assert lanes.count("uint32_t run_path(") == 1 and lanes.count("void emit_path(") == 1 and lanes.count("uint32_t lane_dec_body(") == 1
    parse = open(os.path.join(SRC, "huff_parse_rune.h")).read()
    assert parse.count("bool parse_rune_scan(") == 1 and parse.count("void parse_rune_plan_serial(") == 1 and "struct ParseRuneMid" in parse and "struct ParseRuneSmall" in parse
    # each limit's figure stated once a class, and only there
    csrc = {f: open(os.path.join(SRC, f)).read() for f in os.listdir(SRC) if f.endswith((".h", ".hip", ".cpp"))}
    for literal, where in ((" = 16384", 1), (" = 65536", 1), (" = 960", 1), (" = 576", 2)):
        assert parse.count(literal) == where, literal
    for f in ("huff_rune_dec.hip", "huff_rune_mid_dec.hip", "huff_rune_dec_body.h", "huff_rune_dec_plan.h", "huff_rune_select.h", "group_layout.h"):
        code = re.sub(r"//.*", "", csrc[f])                                # (comments may say the figures)
        assert not re.search(r"\b(16384|65536|960|576)\b", code.replace("HUFF_RUNE_IN_MAX = 16384", "")), f
    rows = open(os.path.join(SRC, "codecs.h")).read()
    assert "huff_dec_behind[] = {&huff_rune_dec_class(), &huff_rune_mid_dec_class()}" in rows and "huff_rune_mid_dec_takes_the_encoder()" in rows and "huff_rune_dec_takes_the_encoder()" in rows
    assert '#include "huff_parse_rune.h"' in rows and "huff_rune_mid_dec_select.h" not in "".join(csrc.values())
    api = open(os.path.join(SRC, "rsn_api.hip")).read()
    assert "rune_mid" not in api and "rune_dec" not in api
    common = open(os.path.join(SRC, "rsn_common.h")).read()
    assert "GD_RUNE_PLANS = 54," in common and "GD_RUNE_MID_PLANS = 60," in common and "HUFF_DEV_PLANS = slot_mask(S::GD_PLANS, S::GD_RUNE_PLANS, S::GD_RUNE_MID_PLANS)" in common
    make = open(os.path.join(SRC, "Makefile")).read()
    assert "huff_rune_mid_dec.hip" in make and "huff_rune_dec.hip" in make and "huff_rune_dec_body.h" in make and "huff_rune_dec_plan.h" in make and "huff_rune_select.h" in make and "huff_rune_mid_dec_select.h" not in make


# ---------------------------------------------------------------- the lane model's verdicts on the GPU tests' members
@pytest.mark.parametrize("n", C.MODEL_SIZES)
def test_model_takes_the_texts(n):
    took, why, S, T = C.verdict_of_member(C.text(n, 0))
    assert (took, why) == (True, None) and T <= 960
    assert S == {16385: 96, 16400: 96, 20000: 96, 32768: 160, 40001: 192, 49152: 256, 65535: 320, 65536: 320}[n]


def test_model_takes_the_hand_built_members():
    s, leaves = C.two_kinds(0)
    assert C.verdict(s, C.table_of(leaves)) == (True, None, 64, 256) and C.payload(s) == 2048
    assert C.verdict_of_member(C.counter(0)) [:3] == (True, None, 288)
    s, leaves = C.one_bit(0)
    assert C.verdict(s, C.table_of(leaves))[:2] == (True, None) and sum(c * len(r.encode()) for c, r in leaves) == 64373
    assert {len(code) for code in C._codes([(c, ord(r)) for c, r in leaves]).values()} == {1}


def test_model_verdicts_of_every_gpu_member():
    """every variant of every shape: what the GPU tests expect is what the model says, and it says taken -- a hand-back for phases or rounds
    would be expected back on the GPU, never "either" """
    for v in range(C.N):
        for name, s, (took, why) in C.shapes(v) + C.limits_taken(v):
            assert (took, why) == (True, None), (name, v, why)
            assert C.payload(s) >= 513 and C.payload(s) <= C.PAY_MAX, (name, v)
    rows = C.limits_taken(0)
    assert C.payload(rows[0][1]) == C.PAY_MAX and C.R.DEPTH_OF_Z[57] == 32 and C.R.DEPTH_OF_Z[58] == 33
    assert C.R.depth(C.R.deep_leaves(57, True, (20000, 20001))) == 32 and C.R.depth(C.R.deep_leaves(58, True, (20000, 20001))) == 33
    nt = dict(C.not_taken(0))
    assert C.payload(nt["a payload of 69121 bytes"]) == C.PAY_MAX + 1 and C.payload(nt["promises 16384 from more than 18432 bytes"]) == 18433
    assert b"65537|a" in nt["a count of 65537"]
