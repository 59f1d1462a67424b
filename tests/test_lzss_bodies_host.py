"""The stage helpers the LZSS batch kernels share (csrc/lzss_enc_body.h, lzss_dec_body.h, block_dev.h), as far as they show
without a device: the item arithmetic of lzss.go:143 against snprintf over every length and distance (tests/lzss_item_test.cpp, a plain
program under the address and undefined-behaviour sanitizers), and that each stage is written once -- the small, mid and tiled units call
the helpers and hold no copy of their own.  Runs on any machine."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")


def _read(name):
    """the file without its // comments: the tests speak of code"""
    return re.sub(r"//[^\n]*", "", open(os.path.join(SRC, name)).read())


def test_item_arithmetic_against_snprintf(tmp_path):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the host tests")
    exe = str(tmp_path / "lzss_item_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + SRC, os.path.join(ROOT, "tests", "lzss_item_test.cpp"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["ok", str((4096 + 64 + 1) * 65536)], r.stdout


ENCODERS = ("lzss_small.hip", "lzss_mid.hip", "lzss_tile.hip")
# the kernels that kept their copy of a stage: k_lzss_mid_enc's and k_lzss_tile_chain's greedy chain, which measured slower through the
# helper, and lzss_small_dec_body's unescape (LEDGER)
OWN_CHAIN = ("lzss_mid.hip", "lzss_tile.hip")
OWN_UNESCAPE = "lzss_small.hip"


def test_the_encoders_hold_no_copy_of_the_token_text_or_the_escape_rule():
    for name in ENCODERS:
        text = _read(name)
        assert not re.search(r"[^=!<>]=\s*'>'", text), name               # no '>' character store of its own
        assert "0x3C ? (uint8_t)0xFF" not in text, name
        assert '#include "lzss_enc_body.h"' in text, name
        assert not re.search(r"3 \+ \w*digits\(", text), name            # nor the token's length
    body = _read("lzss_enc_body.h")
    assert body.count("s_out[--p] = '>'") == 1 and body.count("0x3C ? (uint8_t)0xFF") == 1 and len(re.findall(r"3 \+ \w*digits\(", body)) == 1
    assert len(re.findall(r"\bchain_digits\(uint32_t v\) \{", body)) == 1 and not re.search(r"\b(sl|mid)_digits\b", "".join(_read(n) for n in ENCODERS))
    # who calls what: the escape pair and the item's write in all three, the chain where there is one
    calls = {name: _read(name) for name in ENCODERS}
    for name in ENCODERS:
        assert calls[name].count("lzss_esc_len(") >= 1 and calls[name].count("lzss_esc_put(") >= 1 and calls[name].count("lzss_item_put(") == 1, name
        own = name in OWN_CHAIN
        assert calls[name].count("lzss_greedy_chain<") == (0 if own else 1) and calls[name].count("reach <<= 1") == (1 if own else 0), name
    assert calls["lzss_small.hip"].count("lzss_item(") == 1 and calls["lzss_mid.hip"].count("lzss_item(") == 1 and calls["lzss_tile.hip"].count("lzss_item(") == 2
    assert calls["lzss_tile.hip"].count("~LZT_KEY_ON") == 1              # emit strips the mark; chain reads keys that do not carry it yet


def test_the_decoders_parse_and_unescape_through_one_body():
    body = _read("lzss_dec_body.h")
    assert len(re.findall(r"\bvoid lzd_items\(", body)) == 1 and len(re.findall(r"\bbool lzd_token\(", body)) == 1 and body.count("struct TileItems") == 1
    for name in ("lzss_small.hip", "lzss_mid.hip", "lzss_tile_dec.hip"):
        text = _read(name)
        assert '#include "lzss_dec_body.h"' in text and text.count("lzd_items(") == 1, name
        assert "struct TileItems" not in text and "v * 10" not in text, name                          # no parser of its own
        # nor an unescape, but for the one kernel body that kept its copy: lzss_small_dec_body, slower as a single call through the helpers (LEDGER)
        assert text.count("lzd_unesc_write(") == (0 if name == OWN_UNESCAPE else 1), name
    assert "lzss_match.h" not in _read("lzss_tile_dec.hip")


def test_every_shared_piece_has_one_home():
    match = _read("lzss_match.h")
    assert not re.search(r"\bchain_\w+\s*\(", match) and "CHAIN_NONE" not in match and "lds_load8" in match
    small = _read("lzss_small.hip")
    assert not re.search(r"\bint (flags_wait|group_wait)\(", small)
    assert small.count("return small_call(") == 2                       # both single calls go through the one staged call
    driver = _read("group_dev.hip")
    assert len(re.findall(r"\bint flags_wait\(", driver)) == 1 and len(re.findall(r"\bint group_wait\(", driver)) == 1
    units = [n for n in os.listdir(SRC) if n.endswith((".hip", ".h", ".cpp"))]
    for pattern, home in ((r"\bvoid block_done\(", "block_dev.h"), (r"\buint32_t block_scan\(", "block_dev.h"), (r"\buint32_t chain_best\(", "lzss_enc_body.h"),
                          (r"\buint32_t chain_hash\(", "lzss_enc_body.h")):
        assert [n for n in units if re.search(pattern, _read(n))] == [home], pattern
    everything = "".join(_read(n) for n in units)
    for gone in ("sl_done", "mid_done", "sl_scan", "mid_scan", "chain_scan", "mid_hash", "mid_digits", "sl_digits"):
        assert not re.search(r"\b%s\b" % gone, everything), gone
    assert '#include "block_dev.h"' in _read("huff_small_body.h")
    make = _read("Makefile")
    assert all(h in make.split("HDRS :=")[1].split("\n")[0].split() for h in ("lzss_enc_body.h", "lzss_dec_body.h", "block_dev.h", "lzss_match.h"))
