"""GPU: multi-file lists under several layers (the CLI's default lzss,huffman) go through the layers' batch calls in turn -- in
engine.CompressFiles / DecompressFiles and in the C++ host -- with the per-file loop's files, printed lines and failure semantics."""
import os
import random
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
README = [b"Hello world!\n", b"abcabcabcabcabcabcabcabc\n"]
WORDS = [b"the", b"quick", b"brown", b"fox", b"jumps", b"over", b"lazy", b"dog", b"compression", b"a", b"I", b"Sam", b"ham"]
LAYERS = ["lzss", "huffman"]


def _text(seed, n):
    rng = random.Random(seed)
    t = bytearray()
    while len(t) < n:
        t += rng.choice(WORDS) + rng.choice([b" ", b"\n", b", ", b". "])
    return bytes(t[:n])


def _files(tmp_path, stem, datas):
    paths = []
    for i, d in enumerate(datas):
        p = tmp_path / ("%s%d.txt" % (stem, i))
        p.write_bytes(d)
        paths.append(str(p))
    return paths


def _prof(fn):
    from raisin_amd import _lib
    _lib.prof_enable(True)
    _lib.prof_reset()
    try:
        fn()
        return {k: v[0] for k, v in _lib.prof_get().items() if v[0]}
    finally:
        _lib.prof_enable(False)


@pytest.fixture(scope="module")
def exe():
    e = os.path.join(ROOT, "raisin_amd", "host", "rsn")
    subprocess.check_call(["make", "-s", "-C", os.path.dirname(e)])
    return e


def _datas():
    return [README[k % 2] if k < 16 else _text(k, 13 + 15 * k) for k in range(64)]      # (LZSS groups inputs of up to 1 KiB)


def test_engine_runs_layered_lists_through_the_batch_calls(tmp_path, capsys):
    from raisin_amd import engine
    datas = _datas()
    paths = _files(tmp_path, "f", datas)
    for p in paths:                                                    # the per-file loop
        engine.CompressFile(LAYERS, p, p + ".one")
    loop_out = capsys.readouterr().out
    prof = _prof(lambda: engine.CompressFiles(LAYERS, paths, ".all"))
    batch_out = capsys.readouterr().out
    assert batch_out == loop_out and batch_out.count("Compressing...") == len(datas)
    assert prof == {"lzss_batch_enc": 1, "huff_batch_enc": 1}, prof
    for p in paths:
        assert open(p + ".all", "rb").read() == open(p + ".one", "rb").read()
    comp = [p + ".all" for p in paths]
    for c in comp:
        engine.DecompressFile(LAYERS, c, c + ".one")
    loop_out = capsys.readouterr().out
    prof = _prof(lambda: engine.DecompressFiles(LAYERS, comp, ".dec"))
    batch_out = capsys.readouterr().out
    assert batch_out == loop_out
    assert prof == {"huff_batch_dec": 1, "lzss_batch_dec": 1}, prof
    for c, d in zip(comp, datas):
        assert open(c + ".dec", "rb").read() == open(c + ".one", "rb").read() == d


def test_cli_default_algorithm_matches_the_loop(tmp_path, exe):
    from raisin_amd import engine
    datas = _datas() + [_text(99, 300000), b"z"]
    paths = _files(tmp_path, "g", datas)
    out = subprocess.check_output([exe, "-compress", ",".join(paths), "-outext=cl"]).decode()
    lines = []
    for p, d in zip(paths, datas):
        want = engine.compress(d, LAYERS)
        assert open(p + ".cl", "rb").read() == want
        ratio = np.float32(len(want)) / np.float32(len(d)) * np.float32(100)     # (the host's single-precision arithmetic)
        lines += ["Compressing...", "Original bytes: %d" % len(d), "Compressed bytes: %d" % len(want), "Compression ratio: %.2f%%" % float(ratio)]
    assert out.splitlines() == lines
    comp = [p + ".cl" for p in paths]
    out = subprocess.check_output([exe, "-decompress", ",".join(comp), "-outext=dd", "-delete=false"]).decode()
    assert out.splitlines() == ["Decompressing..."] * len(comp)
    for c, d in zip(comp, datas):
        assert open(c + ".dd", "rb").read() == engine.decompress(engine.compress(d, LAYERS), LAYERS)


def test_layered_lists_keep_the_loops_semantics_when_the_third_file_fails(tmp_path, exe):
    from raisin_amd import RsnError, engine
    datas = [_text(1, 500), _text(2, 900), b"x", _text(3, 700)]
    for bad_kind in ("missing", "empty"):
        paths = _files(tmp_path, "h" + bad_kind, datas)
        if bad_kind == "missing":
            paths[2] = str(tmp_path / "not_there.txt")
        else:
            open(paths[2], "wb").close()
        with pytest.raises((OSError, RsnError)):
            engine.CompressFiles(LAYERS, paths, ".pyl")
        r = subprocess.run([exe, "-compress", ",".join(paths), "-outext=cl"], capture_output=True, text=True)
        assert r.returncode != 0 and r.stdout.count("Compressing...") == (2 if bad_kind == "missing" else 3), r.stdout
        for ext in (".pyl", ".cl"):
            for k in (0, 1):
                assert open(paths[k] + ext, "rb").read() == engine.compress(datas[k], LAYERS)
            assert not os.path.exists(paths[3] + ext)
    # decompress: a third stream that is not one
    src = _files(tmp_path, "k", datas)
    comp = []
    for i, (p, d) in enumerate(zip(src, datas)):
        open(p + ".z", "wb").write(b"1|a1|b" if i == 2 else engine.compress(d, LAYERS))
        comp.append(p + ".z")
    with pytest.raises(RsnError):
        engine.DecompressFiles(LAYERS, comp, ".py")
    r = subprocess.run([exe, "-decompress", ",".join(comp), "-outext=cc"], capture_output=True, text=True)
    assert r.returncode != 0
    for ext in (".py", ".cc"):
        for k in (0, 1):
            assert open(comp[k] + ext, "rb").read() == datas[k]
        assert not os.path.exists(comp[3] + ext)
    assert all(os.path.exists(c) for c in comp)
