"""The tiled class of the LZSS decompress batch (csrc/lzss_tile_dec.hip) as far as it shows without a device: the tiles of
the stream and of the output, the entries of the output tiles, the scratch and which tile stores which byte against a serial restatement
(tests/lzss_tile_dec_layout_test.cpp, also under the address and undefined-behaviour sanitizers as a plain program); the constants of
csrc/lzss_tile_dec_layout.h, their one home, and the names csrc/codecs.h gives them against their mirrors in raisin_amd/lz.py; the closure over the tiled encoder's caps; where
the class sits in the routing.  Runs on any machine."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "raisin_amd", "csrc")


def _build(tmp_path_factory, name, extra):
    if shutil.which("g++") is None:
        pytest.fail("g++ is needed to build the layout test")
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + SRC] + extra + [os.path.join(ROOT, "tests", "lzss_tile_dec_layout_test.cpp"), "-o", exe],
                   check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def layout_test(tmp_path_factory):
    return _build(tmp_path_factory, "lzss_tile_dec_layout_test", ["-O2"])


def _ok(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    word, streams, outputs, stored = r.stdout.split()
    assert word == "ok"
    return int(streams), int(outputs), int(stored)


def _constant(path, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, open(os.path.join(SRC, path)).read())
    assert m, name
    return m.group(1).strip()


def _constants(exe):
    r = subprocess.run([exe, "constants"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return {k: int(v) for k, v in (ln.split() for ln in r.stdout.splitlines())}


def test_layout_against_the_serial_restatement(layout_test):
    from raisin_amd import lz
    streams, outputs, stored = _ok(layout_test)
    assert streams >= 3 * (lz.TILE_DEC_IN_MAX // lz.TILE_POS - 1)                  # three lengths an edge from 2049 on
    assert outputs >= 3 * (lz.TILE_DEC_OUT_MAX // lz.TILE_POS) and stored >= outputs * 1024 // 4


def test_the_same_under_the_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "lzss_tile_dec_layout_test_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert _ok(exe)[0] > 0


def test_mirrored_constants_are_the_headers(layout_test):
    from raisin_amd import lz
    assert _constant("codecs.h", "LZSS_TILE_DEC_IN_MAX") == "LZTD_IN_MAX" and _constant("codecs.h", "LZSS_TILE_DEC_OUT_MAX") == "LZTD_OUT_MAX"
    assert _constant("lzss_tile_dec_layout.h", "LZTD_IN_MAX") == "LZT_E_MAX" and _constant("lzss_tile_dec_layout.h", "LZTD_OUT_MAX") == "LZT_E_MAX"
    assert _constant("codecs.h", "LZSS_TILE_E_MAX") == "LZT_E_MAX"
    assert lz.TILE_DEC_IN_MAX == lz.TILE_DEC_OUT_MAX == lz.TILE_E_MAX
    m = re.search(r"#ifndef RSN_LZSS_TILE_DEC_GROUP_MIN\n#define RSN_LZSS_TILE_DEC_GROUP_MIN (\d+)\n#endif", open(os.path.join(SRC, "codecs.h")).read())
    assert m and lz.TILE_DEC_GROUP_MIN == int(m.group(1)) >= 2 and _constant("codecs.h", "LZSS_TILE_DEC_GROUP_MIN") == "RSN_LZSS_TILE_DEC_GROUP_MIN"
    lay = _constants(layout_test)
    assert (lay["LZTD_IN_MAX"], lay["LZTD_OUT_MAX"], lay["LZTD_TILE"]) == (lz.TILE_DEC_IN_MAX, lz.TILE_DEC_OUT_MAX, lz.TILE_POS)
    assert lay["LZTD_IN_MIN"] == 2048                                             # the small decoder's cutoff: candidates are longer
    assert lay["LZTD_TOKEN_TEXT"] == 23 and lay["LZTD_REACH"] == 22 <= lay["LZTD_HALO"]   # '<' ten digits ',' ten digits '>'
    assert lay["LZTD_IN_TILES_MAX"] * lz.TILE_POS >= lz.TILE_DEC_IN_MAX > (lay["LZTD_IN_TILES_MAX"] - 1) * lz.TILE_POS
    assert lay["LZTD_OUT_TILES_MAX"] * lz.TILE_POS >= lz.TILE_DEC_OUT_MAX > (lay["LZTD_OUT_TILES_MAX"] - 1) * lz.TILE_POS
    # the multiple of the staging that sizes the scratch slot, for the shortest candidate
    assert 4 * lay["LZTD_SCR_WORDS"] <= lay["LZTD_SCR_PER_STAGING"] * ((2049 + 15) // 16 * 16 + 32 + lz.TILE_DEC_OUT_MAX + 16)
    src = open(os.path.join(SRC, "Makefile")).read()
    assert "lzss_tile_dec.hip" in src and "lzss_tile_dec_layout.h" in src and "lzss_dec_body.h" in src


def test_the_decoder_takes_every_stream_the_tiled_encoder_writes(layout_test):
    """the encoder's stream is at most lzt_e_cap(n) bytes -- an item is never longer than what it stands for -- and its escaped length at most TILE_E_MAX"""
    from raisin_amd import lz
    lay = _constants(layout_test)
    assert lay["LZT_E_CAP_MAX"] == min(lz.TILE_IN_MAX + lz.TILE_IN_MAX // 2, lz.TILE_E_MAX) <= lz.TILE_DEC_IN_MAX
    assert lay["LZT_E_MAX"] == lz.TILE_E_MAX <= lz.TILE_DEC_OUT_MAX
    assert lz.MID_E_MAX < lz.TILE_DEC_IN_MAX                                      # and what the mid class hands back for its output is a candidate
    src = open(os.path.join(SRC, "codecs.h")).read()
    assert re.search(r"static_assert\(LZSS_TILE_DEC_IN_MAX >= lzt_e_cap\(LZSS_TILE_IN_MAX\) && LZSS_TILE_DEC_OUT_MAX >= LZSS_TILE_E_MAX", src)


def test_candidates(layout_test):
    from raisin_amd import lz

    def candidate(n):
        r = subprocess.run([layout_test, "candidate", str(n)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.strip() == "1"
    assert [candidate(n) for n in (0, 2048, 2049, lz.MID_E_MAX, lz.MID_E_MAX + 1, lz.TILE_DEC_IN_MAX, lz.TILE_DEC_IN_MAX + 1)] == [False, False, True, True, True, True, False]


def test_the_class_stands_behind_the_rows():
    """behind the rows of LZSS decompress, which are as they were; the launch names hold no "mid" (test_gpu_lzss_mid.py tells the classes apart by it)"""
    src = open(os.path.join(SRC, "codecs.h")).read()
    assert re.search(r"lzss_dec\[\] = \{&lzss_small_class\(false\), &lzss_mid_class\(false\)\}", src)
    assert re.search(r"lzss_dec_behind\[\] = \{&lzss_tile_dec_class\(\)\}", src) and "BatchRows(lzss_dec, lzss_dec_behind)" in src
    kernels = re.findall(r'RSN_LAUNCH\("(\w+)"', open(os.path.join(SRC, "lzss_tile_dec.hip")).read())
    assert kernels == ["lzss_batch_tile_dec_parse", "lzss_batch_tile_dec_plan", "lzss_batch_tile_dec_resolve", "lzss_batch_tile_dec_finish"]
    assert not [k for k in kernels if "mid" in k]
    common = open(os.path.join(SRC, "rsn_common.h")).read()
    assert re.search(r"GD_LZSS_TILE_DEC = 59,", common) and re.search(r"GROUP_DEV = slot_mask\([^)]*S::GD_LZSS_TILE_DEC\)", common)
