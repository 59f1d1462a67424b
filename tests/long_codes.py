"""Streams whose Huffman codes are 30 to 66 bits long, for the long-code tests (test_long_codes_host.py, test_gpu_huffman_long_codes.py).

Decoding builds the tree from the header's counts alone and takes the payload as it comes (huffman.go:196-227), so a header whose counts
grow like Fibonacci numbers gives codes of any length in a stream of a few KB.  This module writes such streams without the library:
  * header(counts)          the reference's header for {rune: count} (ascending rune, '\\n' escaped, a '\\' entry never last);
  * codes(counts)           {rune: '0'/'1' string}, from oracle/literal.py's build_tree + print_codes (independent of the library;
                            fast enough on these shapes, whose counts are distinct but for the bottom's);
  * stream(counts, syms)    header + separator + pad byte + payload for a list of runes (small streams);
  * block_stream(...)       the same for MBs of payload: a few hundred distinct random blocks, each a whole number of bytes, in random
                            order (or one block repeated: a periodic payload), with chosen runes' codewords placed at chosen bits;
  * fib_data(k, ...)        INPUT bytes with Fibonacci counts over k symbols: a longest code of k - 1 bits.
Families of counts: caterpillar(...) -- a chain on top of a balanced bottom of 2**b leaves, the longest code exactly L bits."""
import numpy as np

from oracle import literal

SEP = b"\\\n"


def fib(k):
    """F1..Fk."""
    out, a, b = [], 1, 1
    for _ in range(k):
        out.append(a)
        a, b = b, a + b
    return out


def caterpillar(L, bottom, chain):
    """Counts over `bottom` (2**b runes, count 1 each: a balanced subtree b deep) and the first L - b runes of `chain` (rarest first), each
    chain count just above what it has to stay above, so that every merge is forced (no ties): the bottom's leaves get codes of exactly L
    bits, chain rune j (from 0) gets L - b - j bits, the last one 1 bit."""
    b = len(bottom).bit_length() - 1
    assert len(bottom) == 1 << b and b >= 1
    m = L - b
    assert 0 < m <= len(chain), (L, b, len(chain))
    counts = {r: 1 for r in bottom}
    s_prev, c = 1 << b, (1 << (b - 1)) + 1                     # the bottom's two halves pair before the first chain rune joins
    for j in range(m):
        counts[chain[j]] = c
        s_prev, c = s_prev + c, max(s_prev, c) + 1               # the next chain rune stays above the subtree and the rune merged now
    assert len(counts) == len(bottom) + m
    return counts


def layered_tree(L, d=3, runes=range(1, 128)):
    """{rune: count} whose code lengths are all multiples of d, the longest L: a bottom of 2**d leaves, then levels of a complete subtree
    d deep whose 2**d slots hold the tree so far and 2**d - 1 leaves.  A parse that begins on the wrong residue mod d never meets a
    codeword boundary (the code does not self-synchronise; the pad in front keeps the residue of an even code, hence d = 3), and the
    counts grow 2**d-fold a level: for d = 3, L <= 54 in the 127 byte runes."""
    assert L % d == 0 and d <= L <= 60 - d
    runes = list(runes)
    counts = {r: 1 for r in runes[:1 << d]}
    S, k = 1 << d, 1 << d
    for _ in range(L // d - 1):
        for j in range(1, 1 << d):                              # S, S+1, ..., S+2**d-1: pairs, pairs of pairs, ... -- no ties
            counts[runes[k]] = S + j
            k += 1
        S = sum(range(S, S + (1 << d)))
    return counts


def header(counts):
    out = []
    for r in literal.header_order(counts):
        out.append(str(int(counts[r])).encode() + b"|" + (b"\\n" if r == 10 else literal.go_string_of_rune(r)))
    return b"".join(out)


def codes(counts):
    vals, bins = literal.print_codes(literal.build_tree(dict(counts)))
    return dict(zip(vals, bins))


def utf8(r):
    return literal.go_string_of_rune(r)


def _pack(bits):
    assert len(bits) % 8 == 0
    return np.packbits(np.frombuffer(bits.encode(), dtype=np.uint8) - 48).tobytes()


def _assemble(hdr, head, body=b""):
    """hdr + separator + pad byte + payload; `head` ('0'/'1') comes first, `body` (whole bytes) after it.  The pad goes in front of the
    payload (huffman.go:245-255, literal.as_byte_slice): the first payload byte holds `pad` zeros and the head's first bits."""
    pad = (8 - len(head) % 8) % 8
    return hdr + SEP + bytes([pad]) + _pack("0" * pad + head) + body


def stream(counts, symbols, cs=None):
    cs = cs or codes(counts)
    return _assemble(header(counts), "".join(cs[r] for r in symbols))


def payload_start(hdr_len):
    """(byte offset of the first payload byte, of the 16-byte boundary at or before it) -- the sliced decode counts its slices from the
    latter (huff_decode.hip: A0 = pay & ~15)."""
    pay = hdr_len + 3
    return pay, pay & ~15


def _fill(cs_by_len, nbits):
    """Runes whose codes add up to exactly nbits (greedy over the code lengths present: needs a 1-bit code)."""
    out = []
    lens = sorted(cs_by_len, reverse=True)
    assert lens[-1] == 1
    while nbits > 0:
        l = next(x for x in lens if x <= nbits)
        out.append(cs_by_len[l])
        nbits -= l
    return out


def block_stream(counts, pick, nbytes, seed, n_blocks=300, periodic=False, place=(), head_syms=3, cs=None):
    """A stream of about `nbytes` payload bytes for a header of `counts`.  `pick(rng, m)` draws m runes.  Returns (stream, the bytes it
    decodes to).  Blocks are drawn with bit lengths that are multiples of 8 (a block whose length is not is taken eight times over), so the
    payload is assembled from whole bytes; a head of `head_syms` runes in front makes the pad non-zero (usually).  `periodic`: one block
    repeated.  `place`: [(bit, rune)] -- that rune's codeword begins exactly at that bit of the payload (counted from the first payload
    byte's first bit: the pad's zeros included)."""
    rng = np.random.default_rng(seed)
    cs = cs or codes(counts)
    by_len = {}
    for r, c in sorted(cs.items()):
        by_len.setdefault(len(c), r)
    blocks_b, blocks_d = [], []
    for _ in range(1 if periodic else n_blocks):
        syms = [int(x) for x in pick(rng, int(rng.integers(4, 40)))]
        bits = "".join(cs[r] for r in syms)
        if len(bits) % 8:
            bits, syms = bits * 8, syms * 8
        blocks_b.append(_pack(bits))
        blocks_d.append(b"".join(utf8(r) for r in syms))
    head = [int(x) for x in pick(rng, head_syms)] if head_syms else []
    head_bits = "".join(cs[r] for r in head)
    pad = (8 - len(head_bits) % 8) % 8
    pos = pad + len(head_bits)                                 # payload bits so far; pad + head is whole bytes, so is all that follows
    body, dec = [], [b"".join(utf8(r) for r in head)]
    place = sorted(place)
    reach = 8 * max(len(x) for x in blocks_b)                  # (a block taken now must not pass the next placement)
    k = 0
    while pos < 8 * nbytes or k < len(place):
        if k < len(place) and place[k][0] < pos + reach:
            at, r = place[k]
            k += 1
            assert at >= pos, "placements too close together"
            run = _fill(by_len, at - pos) + [r]                # fillers to the bit, the codeword, fillers to the next byte boundary
            run += _fill(by_len, (8 - sum(len(cs[x]) for x in run) % 8) % 8)
            bits = "".join(cs[x] for x in run)
            body.append(_pack(bits))
            dec.append(b"".join(utf8(x) for x in run))
            pos += len(bits)
            continue
        i = 0 if periodic else int(rng.integers(0, len(blocks_b)))
        body.append(blocks_b[i])
        dec.append(blocks_d[i])
        pos += 8 * len(blocks_b[i])
    return _assemble(header(counts), head_bits, b"".join(body)), b"".join(dec)


# ---- input bytes with Fibonacci counts (encode tests)
ALPHABETS = {"ascii": lambda i: 33 + i, "rune2": lambda i: 0x100 + 7 * i, "rune4": lambda i: 0x1F300 + 13 * i}


def _mix(idx, rng, w=16):
    """Shuffles in place, well enough and ten times faster than a Fisher-Yates pass over 268 M bytes: rows of w shuffled, then each of
    the w columns rotated by a random amount (the w symbols of a row come from w unrelated rows)."""
    m = len(idx) // w * w
    a = idx[:m].reshape(-1, w)
    a[:] = a[rng.permutation(len(a))]
    for j in range(w):
        a[:, j] = np.roll(a[:, j], int(rng.integers(len(a))))
    rng.shuffle(idx[m:])


def fib_symbols(k, order="shuffled", seed=0):
    """Symbol indices 0..k-1 with counts F1..Fk (index 0 the rarest): a longest code of k - 1 bits.  `sorted`: the rarest first, in runs."""
    idx = np.repeat(np.arange(k, dtype=np.uint8), fib(k))
    if order == "shuffled":
        _mix(idx, np.random.default_rng(seed))
    else:
        assert order == "sorted"
    return idx


def encode_symbols(idx, k, alphabet="ascii"):
    table = [utf8(ALPHABETS[alphabet](i)) for i in range(k)]
    w = len(table[0])
    assert all(len(t) == w for t in table)
    tab = np.frombuffer(b"".join(table), dtype=np.uint8).reshape(k, w)
    return tab[idx].tobytes()


def fib_data(k, alphabet="ascii", order="shuffled", seed=0):
    return encode_symbols(fib_symbols(k, order, seed), k, alphabet)


def fib_counts(k, alphabet="ascii"):
    return {ALPHABETS[alphabet](i): f for i, f in enumerate(fib(k))}


def bit_positions_near(idx, lens, bit, chunk=1 << 22):
    """(i0, starts): starts[j] is the payload bit at which symbol idx[i0 + j] begins, over a stretch that covers `bit`."""
    pos = 0
    for i0 in range(0, len(idx), chunk):
        seg = lens[idx[i0:i0 + chunk]].astype(np.int64)
        tot = int(seg.sum())
        if pos + tot > bit:
            return i0, pos + np.concatenate(([0], np.cumsum(seg)[:-1]))
        pos += tot
    raise ValueError("bit %d is past the payload" % bit)


def move_to_bits(idx, lens, which, targets):
    """`idx` with the symbols `which` (each occurring once: the rarest) taken out and put back so that each begins within 6 bits before
    its target bit (ascending targets; a codeword that begins there and is longer than the distance crosses the target).  Where a long
    codeword covers those six bits, 1-bit symbols from just after it are moved in front of it.  The counts stay as they were."""
    rest = idx[~np.isin(idx, which)]
    out, start, shift = [], 0, 0
    for w, t in zip(which, targets):
        u = t - shift
        while True:
            i0, starts = bit_positions_near(rest, lens, u - 1)
            ok = np.nonzero((starts >= u - 6) & (starts <= u - 1))[0]
            if len(ok):
                break
            # a long codeword covers the six bits: move the next 1-bit symbol in front of it (its start moves on by one)
            j = i0 + int(np.nonzero(starts <= u - 1)[0][-1])
            q = j + 1 + int(np.nonzero(lens[rest[j + 1:j + 4096]] == 1)[0][0])
            rest[j:q + 1] = np.roll(rest[j:q + 1], 1)
        i = i0 + int(ok[-1])
        out += [rest[start:i], np.array([w], dtype=idx.dtype)]
        start = i
        shift += int(lens[w])                                  # the symbols put back before the next target push it on
    out.append(rest[start:])
    return np.concatenate(out)


# ---- the deep tables the tests decode: three alphabets, any longest code L
def _runes_of_widths(n, seed):
    """n runes of 2, 3 and 4 UTF-8 bytes in turn (never a surrogate)."""
    bases = (0x100, 0x1000, 0x10400)
    return [bases[i % 3] + 5 * i + seed for i in range(n)]


ALPHABET_NAMES = ("ascii", "runes", "big")


def tree(alphabet, L):
    """{rune: count} with a longest code of L bits.
    ascii: a chain on a bottom of 64 leaves, 127 byte runes at most -- many long codes in a byte alphabet, whose second-level tables
           must fit LDS;
    runes: 2-, 3- and 4-byte runes, a bottom of 16;
    big:   a bottom of 4096 CJK runes (codes of L bits, a second level that does not fit LDS) under a chain of 2- to 4-byte runes."""
    if alphabet == "ascii":
        r = list(range(1, 128))
        return caterpillar(L, r[:64], r[64:])
    if alphabet == "runes":
        r = _runes_of_widths(16 + 70, 1)
        return caterpillar(L, r[:16], r[16:])
    assert alphabet == "big"
    return caterpillar(L, [0x4E00 + i for i in range(4096)], _runes_of_widths(60, 2))


def picker(counts, deep=0.25):
    """pick(rng, m): a fraction `deep` of the runes from the deepest level (codes of L bits), the rest uniform over the others."""
    cs = codes(counts)
    L = max(len(c) for c in cs.values())
    bottom = np.array(sorted(r for r, c in cs.items() if len(c) == L))
    rest = np.array(sorted(r for r, c in cs.items() if len(c) < L))

    def pick(rng, m):
        return np.where(rng.random(m) < deep, rng.choice(bottom, m), rng.choice(rest, m))
    return pick, cs
