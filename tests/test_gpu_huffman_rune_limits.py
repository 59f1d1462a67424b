"""GPU: the grouped rune encoder (k_huff_batch_rune_enc, raisin_amd/csrc/huff_rune.hip) at its limits -- probe chains of 256 runes that wrap
from slot 511 to slot 0, a table that fills while 256 threads insert, runes and invalid forms cut by a 16-byte unit and by the boundary
between two rounds of 256 units, the deepest tree 16 KiB allow and lanes that emit 16 deep codes.  The members come from
tests/rune_limits.py, which tests/test_rune_limits_host.py holds against the kernel's own hash on a CPU.  Every expected byte is the CPU
oracle's (oracle.huffman_compress); the instruments are tests/test_gpu_batch_dev.py's -- members back to back in ONE allocation with
hostile bytes between them, out_cap exactly the result size wherever the class takes the member, the library's launch profile.  Every
shape comes in RUNE_GROUP_MIN varied copies and every list runs through the host form and the device form."""
import pytest

import rune_limits as R
from test_gpu_huffman_batch_dev import ENC, _run_slots
from test_gpu_batch_dev import _prof
from test_gpu_huffman_rune_batch import GENERAL, RUNE

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mods():
    from raisin_amd import _lib, huffman
    _lib.check(_lib.lib().rsn_device_set(0))
    assert huffman.RUNE_GROUP_MIN == R.COPIES and huffman.RUNE_SYMS_MAX == 256
    return _lib, huffman


def _general(prof):
    return any(any(f in k for f in GENERAL) for k in prof)


def _members(shapes):
    """every shape in R.COPIES variants, shape-major: (datas, names)"""
    datas, names = [], []
    for name, variant in shapes:
        for v in range(R.COPIES):
            datas.append(variant(v))
            names.append("%s, variant %d" % (name, v))
    assert len(set(datas)) == len(datas) and max(map(len, datas)) <= 16384 and all(max(d) >= 0x80 for d in datas)
    return datas, names


def _both_forms(mods, oracle, shapes, taken):
    """the list through the host form and the device form: the oracle's bytes, one launch of the rune encoder, and the single call's
    kernels exactly where the class hands the members back"""
    _lib, huffman = mods
    datas, names = _members(shapes)
    want = [oracle.huffman_compress(d) for d in datas]
    got, prof = _prof(_lib, lambda: huffman.CompressBatch(datas))[:2]
    assert len(got) == len(datas)
    for g, w, n in zip(got, want, names):
        assert g == w, n
    assert prof.get(RUNE) == 1 and prof.get("huff_batch_enc") == 1 and not (taken and _general(prof)), prof     # (a rune member's single call shows no launch in the host form: the device form below tells the hand-back)
    caps = [len(w) if taken else _lib.lib().rsn_huffman_compress_bound(len(d)) for d, w in zip(datas, want)]
    got, prof, _ = _run_slots(_lib, ENC, datas, caps, behind=lambda i: b"\xac\xbf\x80", loose=() if taken else range(len(datas)))
    for g, w, n in zip(got, want, names):
        assert g == w, n
    assert prof.get(RUNE) == 1 and _general(prof) == (not taken), prof
    return datas, want


def test_collision_chains(mods, oracle):
    """256 runes in one chain from slot 511 through slots 0 to 254, from slot 0, from U+FFFD's slot with invalid bytes and a literal
    EF BF BD among them, and seven chains of 36 from slots 505 to 511 that run into each other across the wrap"""
    _both_forms(mods, oracle, [(n, (lambda n: lambda v: R.chain_member(n, v))(n)) for n in R.CHAINS], True)


def test_more_runes_than_the_table_takes(mods, oracle):
    """257 colliders, 300 runes, and 5461 distinct runes that fill all 512 slots while 256 threads insert: handed back, the single call's bytes"""
    _both_forms(mods, oracle, R.overflow_shapes(), False)


def test_runes_at_every_phase_of_the_units_and_the_rounds(mods, oracle):
    """3- and 4-byte runes behind 0 to 15 ASCII bytes, past byte 4096 and byte 8192"""
    _both_forms(mods, oracle, R.phase_shapes(), True)


def test_member_ends_and_split_invalid_forms(mods, oracle):
    """a last rune that ends on byte 16384, a last 4-byte rune cut after 1, 2 and 3 bytes, and every invalid form with a unit boundary
    (byte 64) and a round boundary (byte 4096) at every split"""
    _both_forms(mods, oracle, R.end_shapes() + R.split_shapes(), True)


def test_the_deepest_tree_and_the_densest_lanes(mods, oracle):
    """Fibonacci counts over 20 symbols in 16384 bytes: codes of 18 bits (the kernel's comment derives 20 as the ceiling; Go's heap
    breaks the ties of every other sequence tried towards a flatter tree).  Shuffled, sorted, and with 16 codes of 14 and 13 bits from
    one lane -- aligned to a unit, across one, in the member's last unit, across byte 4096"""
    datas, _ = _both_forms(mods, oracle, R.fib_shapes(), True)
    for d in datas[::R.COPIES]:
        assert max(t[3] for t in oracle.huffman_table(d)) == 18 == R.FIB_DEPTH
