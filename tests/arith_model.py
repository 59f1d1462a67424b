"""A plain-Python statement of the adaptive arithmetic codec: the checker of tests/test_arith_host.py and
tests/test_gpu_arith.py.  Written from the codec's description, not from any other implementation; slow on purpose (one symbol at a
time, a 258-entry cumulative table) and exact.

encode(data) -> bytes                 the packed stream
decode(stream) -> bytes               raises FormatError where the library returns RSN_ERR_FORMAT
stats(data) -> dict                   max_pending / end_pending / nbits / runs of an encode
"""
import bisect

MAX_CODE = 0xFFFF
QUARTER = 0x4000
HALF = 0x8000
THREE_QUARTERS = 0xC000
MAX_FREQ = 16383
EOF = 256
TAIL_BITS = 4096            # RSN_ARITH_TAIL_BITS (include/rsn.h)
M32 = 0xFFFFFFFF


class FormatError(ValueError):
    """the stream is one the library refuses with RSN_ERR_FORMAT"""


class Model:
    def __init__(self):
        self.cf = list(range(258))
        self.frozen = False

    def code(self, s):
        """(cf[s], cf[s+1], cf[257]) as they stand, then the update"""
        cf = self.cf
        r = (cf[s], cf[s + 1], cf[257])
        if not self.frozen:
            cf[s + 1:] = [x + 1 for x in cf[s + 1:]]
            if cf[257] >= MAX_FREQ:
                self.frozen = True
        return r

    def find(self, sv):
        """the first i with sv < cf[i+1] (cf is strictly increasing), or None"""
        if sv >= self.cf[257]:
            return None
        return bisect.bisect_right(self.cf, sv) - 1


def encode_bits(data):
    """the coder's bits (a bytearray of 0/1) and {max_pending, end_pending, nbits, runs}; runs: for each pending run that was flushed,
    (its length, the position mod 32 of the deciding bit in front of it)"""
    low, high, pending, max_pending = 0, MAX_CODE, 0, 0
    m = Model()
    bits = bytearray()
    runs = []
    for s in list(bytes(data)) + [EOF]:
        d = high - low + 1
        lo, hi, tot = m.code(s)
        high = low + d * hi // tot - 1
        low = low + d * lo // tot
        while True:
            if high < HALF:
                if pending:
                    runs.append((pending, len(bits) % 32))
                bits.append(0)
                bits.extend(b"\x01" * pending)
                pending = 0
            elif low >= HALF:
                if pending:
                    runs.append((pending, len(bits) % 32))
                bits.append(1)
                bits.extend(b"\x00" * pending)
                pending = 0
            elif low >= QUARTER and high < THREE_QUARTERS:
                pending += 1
                max_pending = max(max_pending, pending)
                low -= QUARTER
                high -= QUARTER
            else:
                break
            high = (2 * high + 1) & MAX_CODE
            low = (2 * low) & MAX_CODE
    return bits, {"max_pending": max_pending, "end_pending": pending, "nbits": len(bits), "runs": runs}


def pack(bits):
    pad = 8 - len(bits) % 8
    allbits = bytearray(pad - 1) + b"\x01" + bits
    out = bytearray(len(allbits) // 8)
    for i in range(len(out)):
        v = 0
        for b in allbits[8 * i:8 * i + 8]:
            v = 2 * v + b
        out[i] = v
    return bytes(out)


def encode(data):
    return pack(encode_bits(data)[0])


def stats(data):
    return encode_bits(data)[1]


def decode(stream, tail_bits=TAIL_BITS):
    stream = bytes(stream)
    nbits = 8 * len(stream)
    big = int.from_bytes(stream, "big") if stream else 0
    if big == 0:
        raise FormatError("no 1 bit in the stream")
    start = nbits - big.bit_length() + 1            # the bit behind the first 1
    if nbits - start < 14:
        raise FormatError("fewer than 16 bits to start from")
    pos = start

    def nextbit():
        nonlocal pos
        if pos < nbits:
            b = (stream[pos >> 3] >> (7 - (pos & 7))) & 1
        else:
            b = 1 if pos == nbits else 0           # the appended 1, 0 -- then zeros for ever
        pos += 1
        return b

    value = 0
    for _ in range(16):
        value = 2 * value + nextbit()
    low, high = 0, MAX_CODE
    m = Model()
    out = bytearray()
    while True:
        if pos - nbits > tail_bits:                 # bits shifted in from behind the stream, the appended two included
            raise FormatError("no end symbol within %d bits behind the stream" % tail_bits)
        d = (high - low + 1) & M32
        sv = ((((value - low + 1) & M32) * m.cf[257] - 1) & M32) // d
        s = m.find(sv)
        if s is None:
            raise FormatError("a code value outside the table")
        lo, hi, tot = m.code(s)
        if s == EOF:
            return bytes(out)
        out.append(s)
        high = (low + d * hi // tot - 1) & M32
        low = (low + d * lo // tot) & M32
        while True:
            if high < HALF:
                pass
            elif low >= HALF:
                value = (value - HALF) & M32
                low -= HALF
                high -= HALF
            elif low >= QUARTER and high < THREE_QUARTERS:
                value = (value - QUARTER) & M32
                low -= QUARTER
                high -= QUARTER
            else:
                break
            low = (2 * low) & M32
            high = (2 * high + 1) & M32
            value = (2 * value + nextbit()) & M32


def greedy_input(steps=400, prefix=b""):
    """At each step the lowest byte whose sub-interval holds both 0x7FFF and 0x8000, else 0x41: the interval keeps straddling the
    middle, so pending bits pile up (runs of hundreds).  `prefix` is coded first (and returned in front): the picks start from the
    coder's state behind it."""
    low, high = 0, MAX_CODE
    m = Model()
    out = bytearray()
    prefix = bytes(prefix)
    for k in range(len(prefix) + steps):
        d = high - low + 1
        tot = m.cf[257]
        if k < len(prefix):
            pick = prefix[k]
        else:
            pick = 0x41
            for b in range(256):
                h = low + d * m.cf[b + 1] // tot - 1
                lw = low + d * m.cf[b] // tot
                if lw <= 0x7FFF and h >= 0x8000:
                    pick = b
                    break
        out.append(pick)
        lo, hi, tot = m.code(pick)
        high = low + d * hi // tot - 1
        low = low + d * lo // tot
        while True:
            if high < HALF or low >= HALF:
                pass
            elif low >= QUARTER and high < THREE_QUARTERS:
                low -= QUARTER
                high -= QUARTER
            else:
                break
            high = (2 * high + 1) & MAX_CODE
            low = (2 * low) & MAX_CODE
    return bytes(out)
