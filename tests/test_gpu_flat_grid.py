"""GPU parity of the flat Huffman kernels (k_emit_flat, k_dec_flat) at chunk counts around their persistent grid.  The grid is the
number of blocks the occupancy query says are resident -- on MI355X 1536 at L = 7, 1792 (encode) and 2048 (decode) at
L = 4, and 2048 was the constant before it: these inputs end one chunk short of each, on it and past it, so that some blocks walk one
chunk more than others, and the last block's chunk is ragged.  Also: sharded slices that start at
other bit phases and span more chunks than the grid, eight callers that meet the grid cache on its first use, and the sliced host-buffer
decode (a grid per slice)."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 8192                                       # symbols a block takes per chunk (FE_SYMS = FLAT_SYMS)
COUNTS = [1535, 1536, 1537, 1791, 1792, 1793, 2047, 2048, 2049, 3073, 4097]
RAGGED = [2047 * CHUNK + 1, 2047 * CHUNK + 4095, 2048 * CHUNK + 1, 2048 * CHUNK + 4095]


def _flat(n, symbols, seed):
    """n bytes drawn uniformly from `symbols` values: every code has the same length (7 bits for 128, 4 for 16)."""
    return np.random.default_rng(seed).integers(0, symbols, size=n, dtype=np.uint8).tobytes()


def _threads(oracle):
    return max(1, min(16, oracle.host_cores()))


@pytest.mark.parametrize("symbols,width", [(128, 7), (16, 4)])
def test_flat_chunk_counts_around_the_grid(oracle, symbols, width):
    from raisin_amd import huffman
    sizes = [c * CHUNK for c in COUNTS] + RAGGED
    for i, n in enumerate(sizes):
        data = _flat(n, symbols, 1000 + i)
        c = huffman.Compress(data)
        assert abs(len(c) - width * n / 8) < 4096, (n, width)                   # really the flat code of that width (+ the header)
        assert c == oracle.huffman_compress_mt(data, _threads(oracle)), (n, symbols)
        assert huffman.Decompress(c) == data, (n, symbols)


@pytest.mark.parametrize("G", [3, 7])
def test_flat_sharded_slices_at_other_bit_phases(G):
    """Slices of 17 MiB and more (over 2048 chunks each, more than any grid) whose first code bit sits at a phase other than the stream's: the block that
    starts each chunk recomputes the word in front of it from the input -- the same stream as the single call."""
    from raisin_amd import huffman
    data = _flat((120 << 20) + 4097, 128, 77)
    ref = huffman.Compress(data)
    assert huffman.CompressSharded(data, G) == ref
    assert huffman.Decompress(ref) == data


_THREADED = """
import hashlib, sys, threading
sys.path.insert(0, %r)
import numpy as np
from raisin_amd import huffman
sizes = [(16 << 20) + k * ((3 << 20) + 999) for k in range(8)]
datas = [np.random.default_rng(500 + k).integers(0, (128, 16)[k %% 2], size=n, dtype=np.uint8).tobytes() for k, n in enumerate(sizes)]
out = [None] * 8
go = threading.Barrier(8)
def work(k):
    go.wait()
    c = huffman.Compress(datas[k])
    d = huffman.Decompress(c)
    out[k] = hashlib.sha256(c).hexdigest() + ":" + str(d == datas[k])
ts = [threading.Thread(target=work, args=(k,)) for k in range(8)]
for t in ts: t.start()
for t in ts: t.join()
print(" ".join(out))
"""


def test_flat_concurrent_callers_on_a_cold_grid_cache():
    """Eight threads of a fresh process compress and decompress flat inputs of 16 to 40 MiB at once: the first launches of every caller
    ask the grid cache together.  Each stream is the single call's, and each decodes to its input."""
    from raisin_amd import huffman
    out = subprocess.run([sys.executable, "-c", _THREADED % ROOT], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    got = out.stdout.strip().splitlines()[-1].split()
    sizes = [(16 << 20) + k * ((3 << 20) + 999) for k in range(8)]
    assert sizes[-1] <= 40 << 20
    for k, n in enumerate(sizes):
        data = np.random.default_rng(500 + k).integers(0, (128, 16)[k % 2], size=n, dtype=np.uint8).tobytes()
        assert got[k] == hashlib.sha256(huffman.Compress(data)).hexdigest() + ":True", k


def test_flat_sliced_host_decode_is_the_serial_decode():
    """The host-buffer decode of a 150 MiB flat stream runs in slices of 64 MiB of payload: two full slices and a partial one, each
    launched with its own grid -- the serial call's bytes, which are the input."""
    from raisin_amd import huffman
    data = _flat((150 << 20) + 12345, 128, 91)
    c = huffman.Compress(data)
    got = huffman.Decompress(c)
    assert got == data
    code = ("import sys, hashlib; sys.path.insert(0, %r)\nfrom raisin_amd import huffman\n"
            "print(hashlib.sha256(huffman.Decompress(open(sys.argv[1], 'rb').read())).hexdigest())\n" % ROOT)
    import tempfile
    with tempfile.NamedTemporaryFile(suffix=".rsn") as f:
        f.write(c)
        f.flush()
        out = subprocess.run([sys.executable, "-c", code, f.name], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, RSN_HOST_SERIAL="1"))
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().splitlines()[-1] == hashlib.sha256(data).hexdigest()
