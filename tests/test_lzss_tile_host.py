"""The tiled class of the LZSS compress batch (csrc/lzss_tile.hip) as far as it shows without a device: the tiles, the
scratch, the slots, the window's first position and which tile stores which byte against a serial restatement
(tests/lzss_tile_layout_test.cpp, which sweeps csrc/tile_layout.h's tile_store first; also under the address and undefined-behaviour
sanitizers as a plain program); the constants of csrc/lzss_tile_layout.h, their one home, and the names csrc/codecs.h gives them against
their mirrors in raisin_amd/lz.py; what the class takes.  Runs on any machine."""
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
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + SRC] + extra + [os.path.join(ROOT, "tests", "lzss_tile_layout_test.cpp"), "-o", exe],
                   check=True, capture_output=True)
    return exe


@pytest.fixture(scope="module")
def layout_test(tmp_path_factory):
    return _build(tmp_path_factory, "lzss_tile_layout_test", ["-O2"])


def _ok(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    word, members, stored = r.stdout.split()
    assert word == "ok"
    return int(members), int(stored)


def test_layout_against_the_serial_restatement(layout_test):
    from raisin_amd import lz
    members, stored = _ok(layout_test)
    edges = (lz.TILE_IN_MAX - lz.MID_IN_MAX) // lz.TILE_POS
    assert members >= 3 * edges and stored >= members * lz.MID_IN_MAX // 4     # three lengths an edge at least, each with a stream stored byte by byte


def test_the_same_under_the_sanitizers(tmp_path_factory):
    exe = _build(tmp_path_factory, "lzss_tile_layout_test_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert _ok(exe)[0] > 0


def _defined(path, name):
    """the default of a constant a probe build may override (#ifndef NAME / #define NAME value)"""
    m = re.search(r"#ifndef %s\b[^\n]*\n#define %s (\d+)\n#endif" % (name, name), open(os.path.join(SRC, path)).read())
    assert m, (path, name)
    return int(m.group(1))


def _constant(path, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*([^;]+);" % name, open(os.path.join(SRC, path)).read())
    assert m, name
    return m.group(1).strip()


def test_mirrored_constants_are_the_headers(layout_test):
    from raisin_amd import lz
    # the class's limits are stated in the layout header alone; codecs.h names them
    assert lz.TILE_IN_MAX == _defined("lzss_tile_layout.h", "RSN_LZSS_TILE_IN_MAX")
    assert "#define RSN_LZSS_TILE_IN_MAX" not in open(os.path.join(SRC, "codecs.h")).read()
    assert lz.TILE_GROUP_MIN == _defined("codecs.h", "RSN_LZSS_TILE_GROUP_MIN") >= 2
    assert _constant("codecs.h", "LZSS_TILE_IN_MAX") == "LZT_IN_MAX" and _constant("lzss_tile_layout.h", "LZT_IN_MAX") == "RSN_LZSS_TILE_IN_MAX"
    assert _constant("codecs.h", "LZSS_TILE_GROUP_MIN") == "RSN_LZSS_TILE_GROUP_MIN"
    assert _constant("codecs.h", "LZSS_TILE_E_MAX") == "LZT_E_MAX" and _constant("lzss_tile_layout.h", "LZT_E_MAX") == "LZT_IN_MAX + LZT_IN_MAX / 16"
    assert lz.TILE_E_MAX == lz.TILE_IN_MAX + lz.TILE_IN_MAX // 16             # the mid class's proportion
    assert lz.MID_E_MAX == lz.MID_IN_MAX + lz.MID_IN_MAX // 16
    assert _constant("codecs.h", "LZSS_TILE_POS") == "LZT_TILE" and lz.TILE_POS == int(_constant("lzss_tile_layout.h", "LZT_TILE")) == 2048
    assert lz.TILE_GROUP_BYTES == int(_constant("codecs.h", "LZSS_TILE_GROUP_BYTES"))
    r = subprocess.run([layout_test, "constants"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    lay = {k: int(v) for k, v in (ln.split() for ln in r.stdout.splitlines())}
    assert (lay["LZT_IN_MIN"], lay["LZT_IN_MAX"], lay["LZT_E_MAX"], lay["LZT_TILE"]) == (lz.MID_IN_MAX, lz.TILE_IN_MAX, lz.TILE_E_MAX, lz.TILE_POS)
    assert lay["LZT_W_MAX"] == lz.DefaultWindowSize == 4096
    assert lay["LZT_TILES_MAX"] * lz.TILE_POS >= lz.TILE_E_MAX > (lay["LZT_TILES_MAX"] - 1) * lz.TILE_POS
    assert lz.TILE_E_MAX < 1 << 31 and lay["LZT_W_MAX"] < 1 << 15             # a key is L << 16 | distance, its top bit the chain's mark
    src = open(os.path.join(SRC, "Makefile")).read()
    assert "lzss_tile.hip" in src and "lzss_tile_layout.h" in src and "tile_layout.h tile_dev.h" in src


def test_what_the_class_takes(layout_test):
    from raisin_amd import lz

    def takes(n, w):
        r = subprocess.run([layout_test, "takes", str(n), str(w)], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout.strip() == "1"
    assert [takes(n, 4096) for n in (0, 65536, 65537, lz.TILE_IN_MAX, lz.TILE_IN_MAX + 1)] == [False, False, True, True, False]
    assert [takes(100000, w) for w in (-1, 0, 1, 4096, 4097, 8192)] == [False, False, True, True, False, False]
    assert lz.MID_IN_MAX == 65536 and (lz.MID_IN_MAX, lz.MID_E_MAX, lz.MID_GROUP_MIN) == (65536, 69632, 64)   # the other classes' cutoffs did not move


def test_the_other_rows_come_first():
    """the tiled class sits behind the small and the mid rows of LZSS compress, and the decompress rows are as they were"""
    src = open(os.path.join(SRC, "codecs.h")).read()
    assert re.search(r"lzss_enc\[\] = \{&lzss_small_class\(true\), &lzss_mid_class\(true\), &lzss_tile_class\(\)\}", src)
    assert re.search(r"lzss_dec\[\] = \{&lzss_small_class\(false\), &lzss_mid_class\(false\)\}", src)
