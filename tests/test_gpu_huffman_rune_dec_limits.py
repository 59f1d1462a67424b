"""GPU: the grouped rune decoder (k_huff_batch_rune_dec, raisin_amd/csrc/huff_rune_dec.hip) at its limits -- a header whose 256 entries lie in
one probe chain that wraps from slot 511 to slot 0, trees of 24, 25 and 32 bits built by one wavefront and walked behind the 9-bit table
(33 bits: refused), deep codes at the payload's first and last bits, twenty in a row and across the lanes' starts, and a payload of
exactly 256 lanes of 576 bits (one byte more: refused) -- and the byte decoder classes, which share parse_depths, at 32 and 33 bits.
The streams are built by hand in tests/rune_limits.py (with _build and _codes of test_gpu_huffman_rune_dec_batch.py), which
tests/test_rune_limits_host.py holds against the kernel's own plan on a CPU.  Every expected byte is the CPU oracle's
(oracle.huffman_decompress).  The instruments are tests/test_gpu_batch_dev.py's: streams back to back in ONE allocation with hostile
bytes between them, out_cap exactly the result size wherever the class takes the stream, the library's launch profile.  Every list of
streams expected to be taken also runs on its own, and no kernel of the single call may appear then: taken means taken.

The lane decoder hands a member back legitimately on more than four phases or on DEC_ROUNDS rounds (_counter in
test_gpu_huffman_rune_dec_batch.py).  A payload that trips that gets another seed (R.PAY_SEED, the filler's seed in R.deep_text), never
an exemption; no seed has been rejected so far."""
import pytest

import rune_limits as R
from test_gpu_batch_dev import _prof, _ru16
from test_gpu_huffman_batch_dev import DEC, _run_slots
from test_gpu_huffman_rune_dec_batch import RUNE, RUNE_PLAN, _general

pytestmark = pytest.mark.gpu

TAKEN_DEV = {"huff_dev_plan": 1, RUNE_PLAN: 1, "group_gather": 1, RUNE: 1, "group_scatter": 1}     # the device form's launches when the rune class takes every member


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman
    _lib.check(_lib.lib().rsn_device_set(0))
    assert huffman.RUNE_DEC_GROUP_MIN == R.COPIES and huffman.RUNE_OUT_MAX == 16384 and huffman.RUNE_PAY_MAX == R.PAY_MAX
    return _lib, huffman


def _rows(keep=lambda name: True):
    """the hand-built streams in R.COPIES variants: [(name, stream, text, taken)]"""
    return [(n + ", variant %d" % v, s, t, k) for v in range(R.COPIES) for n, s, t, k in R.dec_streams(v) if keep(n)]


def _both_forms(mods, oracle, rows, kernel=RUNE, taken_dev=TAKEN_DEV):
    """the list, then the streams expected to be taken on their own, each through the host form and the device form"""
    _lib, huffman = mods
    streams, taken, names = [r[1] for r in rows], [r[3] for r in rows], [r[0] for r in rows]
    want = [oracle.huffman_decompress(s) for s in streams]
    for w, r in zip(want, rows):
        assert w == r[2].encode() and len(w) <= 40001, r[0]
    mixed = not all(taken)
    assert sum(taken) >= R.COPIES
    got, prof = _prof(_lib, lambda: huffman.DecompressBatch(streams))[:2]
    for g, w, n in zip(got, want, names):
        assert g == w, n
    assert prof.get(kernel) == 1 and _general(prof) == mixed, prof
    caps = [len(w) if t else _ru16(len(w)) + 16 for w, t in zip(want, taken)]      # exact sizes where the class takes the member
    got, prof, _ = _run_slots(_lib, DEC, streams, caps, behind=lambda i: b"\xac\xbf\x80")
    for g, w, n in zip(got, want, names):
        assert g == w, n
    assert prof.get(kernel) == 1 and _general(prof) == mixed, prof
    # taken really means taken: alone, nothing of the single call runs
    idx = [i for i, t in enumerate(taken) if t]
    only, prof = _prof(_lib, lambda: huffman.DecompressBatch([streams[i] for i in idx]))[:2]
    assert only == [want[i] for i in idx]
    assert prof == {kernel: 1}, prof
    only, prof, _ = _run_slots(_lib, DEC, [streams[i] for i in idx], [len(want[i]) for i in idx], behind=lambda i: b"\xac\xbf\x80")
    assert only == [want[i] for i in idx]
    assert prof == taken_dev, prof


def test_collision_chains_in_the_header(mods, oracle):
    """256 colliders of slot 511 as entries in descending order; the same with an earlier entry for every fourth, which the later one
    replaces down the chain; 257 colliders, which the table refuses"""
    _both_forms(mods, oracle, _rows(lambda n: "colliders" in n))


def test_codes_of_24_25_32_and_33_bits(mods, oracle):
    """z zero-count runes make a comb of z - 1 ... bits: 24 and 25 (the encoders' limit lies between, the decoder's does not), 32 (taken)
    and 33 (refused: the single call decodes it)"""
    rows = _rows(lambda n: n.startswith("depth"))
    assert {r[0][:8]: r[3] for r in rows} == {"depth 24": True, "depth 25": True, "depth 32": True, "depth 33": False}
    _both_forms(mods, oracle, rows)


def test_the_payload_limit(mods, oracle):
    """24-bit codes among shallower ones in 18432 bytes of payload -- 256 lanes of 576 bits -- and in 18433 and 18436 bytes, which no
    lane plan holds"""
    rows = _rows(lambda n: n.startswith("a payload"))
    assert [len(r[1]) - r[1].index(b"\\\n") - 3 for r in rows[:3]] == [R.PAY_MAX, R.PAY_MAX + 1, R.PAY_MAX + 4]
    _both_forms(mods, oracle, rows)


@pytest.mark.parametrize("mid", (False, True), ids=("small", "mid"))
def test_the_byte_decoder_classes_at_32_and_33_bits(mods, oracle, mid):
    """parse_depths is the byte plans' too: the same pair of trees over ASCII, in the class of k_huff_batch_dec and -- with a header that
    promises 40001 bytes and a payload above 4 KiB -- in the mid class, which needs four members"""
    _, huffman = mods
    assert huffman.MID_GROUP_MIN <= 4
    rows = [(n + ", variant %d" % v, s, t, k) for v in range(4) for n, s, t, k in R.byte_streams(v, mid)]
    kernel = "huff_batch_mid_dec" if mid else "huff_batch_dec"
    _both_forms(mods, oracle, rows, kernel, {"huff_dev_plan": 1, "huff_dev_gather": 1, kernel: 1, "huff_dev_scatter": 1})
