"""CPU tests for the long-code suite (test_gpu_huffman_long_codes.py): the library's host tree builder gives the reference's codes on every
deep table that suite decodes, up to 64 bits, and refuses 65 and 66; the stream builder (long_codes.py) writes streams that both oracles
decode to the runes it meant -- so that a wrong stream can neither pass nor fail a GPU test."""
import numpy as np
import pytest

import long_codes as LC

LENGTHS = (31, 32, 33, 40, 48, 63, 64)


@pytest.fixture(scope="module")
def built():
    import __graft_entry__ as g
    g.build()
    from raisin_amd import _lib
    return _lib


def _plan_codes(counts):
    from raisin_amd import huffman
    table, header = huffman.plan(counts)
    return {r: format(c, "0%db" % l) for r, c, l in table}, [r for r, _, _ in table], header


def _literal_order(counts):
    from oracle import literal
    vals, bins = literal.print_codes(literal.build_tree(dict(counts)))
    return dict(zip(vals, bins)), vals


@pytest.mark.parametrize("alphabet", LC.ALPHABET_NAMES)
def test_plan_matches_literal_on_deep_tables(built, alphabet):
    for L in LENGTHS:
        counts = LC.tree(alphabet, L)
        want, order = _literal_order(counts)
        got, got_order, header = _plan_codes(counts)
        assert got_order == order and got == want, (alphabet, L)           # (rune, code, length) in printCodes order
        assert max(len(c) for c in got.values()) == L
        assert header == LC.header(counts)
        if L <= 40:                                                          # counts past 2**32 (the wide heap): the same tree
            s = 61 - max(counts.values()).bit_length()
            assert _plan_codes({r: c << s for r, c in counts.items()})[:2] == (got, got_order), (alphabet, L)
            assert max(counts.values()) << s < 1 << 62


def test_plan_matches_literal_on_fibonacci_tables(built):
    for k in (25, 26, 33, 34, 36, 40):
        for alphabet in LC.ALPHABETS:
            counts = LC.fib_counts(k, alphabet)
            want, order = _literal_order(counts)
            got, got_order, _ = _plan_codes(counts)
            assert got_order == order and got == want
            assert max(len(c) for c in got.values()) == k - 1
    # the halved header of the pipeline test
    counts = {r: c // 2 for r, c in LC.fib_counts(40).items()}
    assert _plan_codes(counts)[:2] == _literal_order(counts)
    assert max(len(c) for c in _literal_order(counts)[0].values()) >= 36


def test_plan_matches_literal_on_layered_tables(built):
    for L in (42, 48, 54):
        counts = LC.layered_tree(L)
        want, order = _literal_order(counts)
        assert _plan_codes(counts)[:2] == (want, order)
        assert max(len(c) for c in want.values()) == L and all(len(c) % 3 == 0 for c in want.values())


@pytest.mark.parametrize("alphabet", LC.ALPHABET_NAMES)
@pytest.mark.parametrize("L", [65, 66])
def test_plan_refuses_codes_past_64_bits(built, alphabet, L):
    from raisin_amd import RsnError, huffman
    counts = LC.tree(alphabet, L)
    assert max(len(c) for c in LC.codes(counts).values()) == L
    with pytest.raises(RsnError) as e:
        huffman.plan(counts)
    assert e.value.code == -6                                                # RSN_ERR_LIMIT
    with pytest.raises(RsnError) as e:                                       # the wide heap refuses it as well
        huffman.plan({r: c << 14 for r, c in counts.items()})
    assert e.value.code == -6


def _boundaries(s, cs):
    """Payload bit (pad included) at which each codeword begins, walking the code table -- for checking placements."""
    sep = s.index(LC.SEP)
    pad = s[sep + 2]
    bits = "".join(format(b, "08b") for b in s[sep + 3:])
    inv = {c: r for r, c in cs.items()}
    out, i, cur = {}, pad, ""
    start = pad
    while i < len(bits):
        cur += bits[i]
        i += 1
        if cur in inv:
            out[start] = inv[cur]
            cur, start = "", i
    assert cur == ""
    return out


@pytest.mark.parametrize("alphabet", LC.ALPHABET_NAMES)
def test_builder_streams_decode_to_their_runes(oracle, alphabet):
    from oracle import literal
    for L in LENGTHS + (65, 66):
        counts = LC.tree(alphabet, L)
        pick, cs = LC.picker(counts)
        rng = np.random.default_rng(L)
        syms = [int(x) for x in pick(rng, 300)]
        s = LC.stream(counts, syms, cs)
        want = b"".join(LC.utf8(r) for r in syms)
        assert oracle.huffman_decompress(s) == want == literal.huffman_decompress(s)
        assert s.startswith(LC.header(counts) + LC.SEP)
        for periodic in (False, True):
            s, want = LC.block_stream(counts, pick, 3000, seed=L, periodic=periodic, cs=cs)
            assert oracle.huffman_decompress(s) == want == literal.huffman_decompress(s)
            assert len(want) > 300
        if alphabet == "ascii" and L in (42, 48, 54):
            ec = LC.layered_tree(L)
            epick, ecs = LC.picker(ec)
            for periodic in (False, True):
                es, ewant = LC.block_stream(ec, epick, 3000, seed=L, periodic=periodic, cs=ecs)
                assert oracle.huffman_decompress(es) == ewant == literal.huffman_decompress(es)
        deep = max(cs, key=lambda r: (len(cs[r]), r))
        s, want = LC.block_stream(counts, pick, 6000, seed=L, place=[(9001, deep), (20000, deep)], cs=cs)
        assert oracle.huffman_decompress(s) == want
        b = _boundaries(s, cs)
        assert b[9001] == deep and b[20000] == deep
        long = sum(len(cs[r]) == L for r in b.values())
        assert 8 * long >= len(b), "long codewords are fewer than 1 in 8"


def test_builder_header_matches_the_oracle_encoder(oracle):
    """header() is the header the oracle's encoder writes for the same counts (the order rule: ascending, '\\' never last)."""
    for data in (b"a\nb\\\\\\", b"zz\\\\\n\n\n", "héllo \U0001F600 \\".encode() * 3):
        counts = {}
        for r in oracle.utf8_runes(data):
            counts[int(r)] = counts.get(int(r), 0) + 1
        ref = oracle.huffman_compress(data)
        assert LC.header(counts) == ref[:ref.index(LC.SEP)]
        assert LC.stream(counts, [int(r) for r in oracle.utf8_runes(data)]) == ref


def test_fibonacci_inputs(oracle):
    for k, alphabet, order in ((25, "ascii", "sorted"), (26, "rune2", "shuffled"), (27, "rune4", "shuffled")):
        data = LC.fib_data(k, alphabet, order, seed=k)
        t = oracle.huffman_table(data)
        assert sorted(f for _, f, _, _ in t) == LC.fib(k)
        assert max(l for _, _, _, l in t) == k - 1
        if order == "sorted":
            assert data == b"".join(LC.utf8(LC.ALPHABETS[alphabet](i)) * f for i, f in enumerate(LC.fib(k)))


def test_placing_the_rarest_symbols_at_chosen_bits(oracle):
    """move_to_bits (how the 268 MB input of the GPU suite puts its two 39-bit codewords across the sliced decode's cuts), at a size the
    oracle walks here: each rarest symbol begins within 6 bits before its target and the input keeps its counts."""
    k = 27
    counts = LC.fib_counts(k)
    cs = LC.codes(counts)
    lens = np.zeros(256, dtype=np.uint8)
    for i in range(k):
        lens[i] = len(cs[LC.ALPHABETS["ascii"](i)])
    idx = LC.fib_symbols(k, "shuffled", seed=3)
    targets = [1 << 17, (1 << 18) + 5, (1 << 18) + 3000]
    moved = LC.move_to_bits(idx, lens, [0, 1], targets[:2])
    assert np.array_equal(np.bincount(moved, minlength=k), np.bincount(idx, minlength=k))
    starts = np.concatenate(([0], np.cumsum(lens[moved].astype(np.int64))[:-1]))
    for w, t in zip((0, 1), targets):
        at = int(starts[np.nonzero(moved == w)[0][0]])
        assert t - 6 <= at <= t - 1 and at + int(lens[w]) > t
    data = LC.encode_symbols(moved, k)
    assert oracle.huffman_decompress(oracle.huffman_compress(data)) == data
