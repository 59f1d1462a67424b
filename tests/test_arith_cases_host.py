"""CPU: the claims of tests/arith_cases.py, asserted from the model's own statistics, and a demonstration that the corpus tells a subtly
wrong kernel from a right one -- a plain-Python restatement of the kernel's table layout (64 lanes of 4 registers: Table::at, find and
update of raisin_amd/csrc/arith.hip) and of its bit sink (BitSink::put / put_with_run) agrees with the model on every case, and each
of them with one fault switched in does not.  No GPU runs wrong code for this."""
import bisect

import pytest

import arith_cases as C
import arith_model as M


# ---------------------------------------------------------------- the corpus's claims
def test_every_symbol_and_every_position():
    for r in (1, 2, 3, 64):
        for name in ("all256x%d" % r, "rev256x%d" % r):
            d = C.CASES[name].data
            assert len(d) == 256 * r and all(d.count(s) == r for s in range(256))
    assert C.CASES["all256x2"].data[:3] == b"\x00\x01\x02" and C.CASES["rev256x2"].data[:3] == b"\xff\xfe\xfd"
    for k in range(4):
        for lane in C.LANES:
            d = C.CASES["reg%dlane%d" % (k, lane)].data
            s = 4 * lane + k
            other = 600 - d.count(s)                                      # a tenth of 600; at 0 and 255 half of those are clamped to s
            assert len(d) == 600 and (15 <= other <= 50 if s in (0, 255) else 35 <= other <= 90)
            assert set(d) == {max(s - 1, 0), s, min(s + 1, 255)}         # both neighbours occur (at 0 and 255, the one there is)
    assert set(C.LANES) == {0, 1, 31, 32, 62, 63}


def test_noise_lengths_freeze_and_slices():
    S = C.SLICE_SYMBOLS
    for n in C.NOISE_LENGTHS + (S - 1, S, S + 1):
        d = C.CASES["noise%d" % n].data
        assert len(d) == n
        if n >= 4097:
            assert len(set(d)) == 256
    assert C.NOISE_LENGTHS == (1, 2, 3, 17, 255, 256, 257, 1000, 4097, 16125, 16126, 16127, 40000)
    assert 257 + 16126 == M.MAX_FREQ                                      # the update that freezes the table is symbol 16126
    assert C.CASES["frozen-then-all"].data == b"a" * 16126 + bytes(range(256)) * 40


def test_at_least_five_cases_expand():
    assert sum(1 for c in C.CASES.values() if len(c.enc) > len(c.data)) >= 5
    big = C.CASES["noise%d" % C.SLICE_SYMBOLS]
    assert len(big.enc) > len(big.data)                                   # ... one of them across a slice's resume


def test_pending_runs_at_every_place_of_a_word():
    pend = {n: c for n, c in C.CASES.items() if n.startswith("pending")}
    assert 10 <= len(pend) <= 64
    places = {at for c in pend.values() for k, at in c.runs if k >= 32}
    assert places == set(range(32))
    assert {k for c in pend.values() for k, _ in c.runs} >= set(C.RUN_LENGTHS) == {31, 32, 33, 63, 64, 65}
    assert all(len(c.data) <= 11 + 60 + 1 and c.data[-1] == 0 for c in pend.values())
    # a run that goes on for whole words behind its head, from a word's first bit and from its last
    assert any(k >= 64 and at == 31 for c in pend.values() for k, at in c.runs)
    assert any(k >= 64 and at == 30 for c in pend.values() for k, at in c.runs)


def test_ends():
    cases = C.CASES.values()
    assert {c.nbits % 8 for c in cases} == set(range(8))
    assert sum(1 for c in cases if c.nbits % 32 == 0) >= 2
    assert {len(c.enc) % 16 for c in cases} >= {0, 1, 15}
    assert all(len(c.enc) == c.nbits // 8 + 1 for c in cases)


def test_sizes_stay_small():
    assert all(len(c.data) <= 70000 for c in C.CASES.values())
    assert sum(len(c.data) + 1 for c in C.CASES.values()) <= 1500000


def test_dev_subset_is_what_it_says():
    names = C.dev_subset()
    assert 10 <= len(names) <= 14 and set(names) <= set(C.CASES)
    assert any(n.startswith("noise") for n in names)
    assert {n[3] for n in names if n.startswith("reg")} == set("0123")
    for place in (30, 31):
        assert any(k >= 32 and at == place for n in names for k, at in C.CASES[n].runs)
    assert any(C.CASES[n].nbits % 32 == 0 for n in names)


@pytest.mark.parametrize("name", C.NAMES)
def test_model_round_trips(name):
    c = C.CASES[name]
    assert M.decode(c.enc) == c.data
    assert len(c.enc) <= 2 * len(c.data) + 4


# ---------------------------------------------------------------- the table in 64 lanes of 4 registers
AT, UPDATE, BALLOT_U2, NO_U2_TERM, HALF_BALLOT = "at reads u2 for k == 3", "update of u1 with >", "find ballots on u2", \
    "find drops sv >= u2", "the ballot sees lanes 0-31"
TABLE_FAULTS = (AT, UPDATE, BALLOT_U2, NO_U2_TERM, HALF_BALLOT)


class LaneTable:
    """u[k][l]: register k of lane l = cf[4l + k + 1]; tot = cf[257]"""

    def __init__(self, fault=None):
        self.u = [[4 * l + k + 1 for l in range(64)] for k in range(4)]
        self.tot = 257
        self.frozen = False
        self.fault = fault

    def at(self, i):
        j = i - 1
        k = j & 3
        if self.fault == AT and k == 3:
            k = 2
        return self.u[k][j >> 2]

    def update(self, s):
        for k in range(4):
            # lanes with 4l + k >= s
            if self.fault == UPDATE and k == 1:
                l0 = (s - k) // 4 + 1 if s >= k else 0                    # 4l + k > s
            else:
                l0 = max(0, (s - k + 3) // 4)
            uk = self.u[k]
            uk[l0:] = [x + 1 for x in uk[l0:]]
        self.tot += 1
        if self.tot >= M.MAX_FREQ:
            self.frozen = True

    def code(self, s):
        lo = 0 if s == 0 else self.at(s)
        hi = self.tot if s == 256 else self.at(s + 1)
        tot = self.tot
        if not self.frozen:
            self.update(s)
        return lo, hi, tot

    def find(self, sv):
        if sv >= self.tot:
            return None
        reg = self.u[2] if self.fault == BALLOT_U2 else self.u[3]
        lanes = 32 if self.fault == HALF_BALLOT else 64
        l = bisect.bisect_right(reg, sv, 0, lanes)                         # the first lane with sv < its register (they increase)
        if l == lanes:
            return 256
        k = (sv >= self.u[0][l]) + (sv >= self.u[1][l])
        if self.fault != NO_U2_TERM:
            k += sv >= self.u[2][l]
        return 4 * l + k


class Runaway(Exception):
    """a coder whose interval is no interval any more (a faulty table): more shifts for one symbol than a 16-bit coder can make"""


def _shift(low, high, value=None):
    """one step of the coder's loop -> (what happened, low, high, value); what: 0 / 1 the deciding bit, 2 a pending bit, None: done"""
    if high < M.HALF:
        what = 0
    elif low >= M.HALF:
        what, low, high = 1, low - M.HALF, high - M.HALF
        value = value - M.HALF if value is not None else None
    elif low >= M.QUARTER and high < M.THREE_QUARTERS:
        what, low, high = 2, low - M.QUARTER, high - M.QUARTER
        value = value - M.QUARTER if value is not None else None
    else:
        return None, low, high, value
    return what, (2 * low) & M.MAX_CODE, (2 * high + 1) & M.MAX_CODE, value


def _lane_encode(data, t):
    low, high, pending = 0, M.MAX_CODE, 0
    bits = bytearray()
    for s in list(data) + [M.EOF]:
        d = high - low + 1
        lo, hi, tot = t.code(s)
        high = low + d * hi // tot - 1
        low = low + d * lo // tot
        for n in range(40):
            what, low, high, _ = _shift(low, high)
            if what is None:
                break
            if what == 2:
                pending += 1
            else:
                bits.append(what)
                bits.extend(bytes([1 - what]) * pending)
                pending = 0
        else:
            raise Runaway()
    return M.pack(bits)


def _lane_decode(stream, t):
    nbits = 8 * len(stream)
    pos = nbits - int.from_bytes(stream, "big").bit_length() + 1

    def nextbit():
        nonlocal pos
        b = (stream[pos >> 3] >> (7 - (pos & 7))) & 1 if pos < nbits else int(pos == nbits)
        pos += 1
        return b
    value = 0
    for _ in range(16):
        value = 2 * value + nextbit()
    low, high = 0, M.MAX_CODE
    out = bytearray()
    while pos - nbits <= M.TAIL_BITS:
        d = high - low + 1
        sv = ((value - low + 1) * t.tot - 1) // d
        s = t.find(sv) if 0 <= sv else None
        if s is None:
            raise M.FormatError("a code value outside the table")
        lo, hi, tot = t.code(s)
        if s == M.EOF:
            return bytes(out)
        out.append(s)
        high = low + d * hi // tot - 1
        low = low + d * lo // tot
        for n in range(40):
            what, low, high, value = _shift(low, high, value)
            if what is None:
                break
            value = (2 * value + nextbit()) & M.MAX_CODE if 0 <= value <= M.MAX_CODE else value
        else:
            raise Runaway()
    raise M.FormatError("no end symbol")


def _lane_verdict(c, fault):
    """(stream, decode of the model's stream) with the table in lanes; a coder that fails or runs away gives None"""
    res = []
    for fn, arg in ((_lane_encode, c.data), (_lane_decode, c.enc)):
        try:
            res.append(fn(arg, LaneTable(fault)))
        except (M.FormatError, Runaway, ZeroDivisionError, IndexError):
            res.append(None)
    return tuple(res)


@pytest.mark.parametrize("name", C.NAMES)
def test_the_lane_layout_agrees_with_the_model(name):
    c = C.CASES[name]
    assert _lane_verdict(c, None) == (c.enc, c.data)


SMALL = [n for n in C.NAMES if n.startswith("reg") or n in ("all256x1", "rev256x1", "hello")]


@pytest.mark.parametrize("fault", TABLE_FAULTS)
def test_a_faulty_table_is_told_apart(fault):
    caught = [n for n in SMALL if _lane_verdict(C.CASES[n], fault) != (C.CASES[n].enc, C.CASES[n].data)]
    assert caught, fault
    # ... and by the cases made for it, not by luck: every symbol in order, and a symbol's own register
    assert "all256x1" in caught or "rev256x1" in caught
    if fault in (AT, BALLOT_U2):
        assert all("reg3lane%d" % l in caught for l in C.LANES)
    if fault == NO_U2_TERM:
        assert all("reg2lane%d" % l in caught or "reg3lane%d" % l in caught for l in C.LANES)
    if fault == UPDATE:
        assert all("reg1lane%d" % l in caught or "reg2lane%d" % l in caught for l in C.LANES)
    if fault == HALF_BALLOT:
        assert all("reg%dlane%d" % (k, l) in caught for k in range(4) for l in (32, 62, 63))


# ---------------------------------------------------------------- the bit sink
NO_HEAD, SHORT_LOOP = "the head omitted when acc_n == 0", "the whole-word loop once too few"


class Sink:
    """BitSink: an accumulator of fewer than 32 bits, whole words out"""

    def __init__(self, fault=None):
        self.acc, self.acc_n, self.words, self.fault = 0, 0, [], fault

    def put(self, v, k):
        assert 0 <= k <= 32 and v < (1 << k)
        self.acc = (self.acc << k) | v
        self.acc_n += k
        if self.acc_n >= 32:
            self.acc_n -= 32
            self.words.append(self.acc >> self.acc_n)
            self.acc &= (1 << self.acc_n) - 1

    def put_with_run(self, bit, run):
        if run < 32:
            self.put((1 << run) if bit else (1 << run) - 1, run + 1)
            return
        self.put(bit, 1)
        fill = 0 if bit else 0xFFFFFFFF
        head = min(run, 32 - self.acc_n)
        if not (self.fault == NO_HEAD and self.acc_n == 0):
            self.put(fill >> (32 - head), head)
        run -= head
        whole = run // 32
        run -= 32 * whole
        if self.fault == SHORT_LOOP:
            whole = max(whole - 1, 0)
        for _ in range(whole):
            assert self.acc_n == 0
            self.words.append(fill)
        if run:
            self.put(fill >> (32 - run), run)

    def stream(self):
        nbits = 32 * len(self.words) + self.acc_n
        words = self.words + ([self.acc << (32 - self.acc_n)] if self.acc_n else [])   # the last, partial word zero-filled
        raw = b"".join(w.to_bytes(4, "big") for w in words)
        bits = bytearray((raw[i >> 3] >> (7 - (i & 7))) & 1 for i in range(nbits))
        return M.pack(bits)


def _sink_stream(data, fault):
    """the model's coder, its bits through the sink"""
    low, high, pending = 0, M.MAX_CODE, 0
    m, o = M.Model(), Sink(fault)
    for s in list(data) + [M.EOF]:
        d = high - low + 1
        lo, hi, tot = m.code(s)
        high = low + d * hi // tot - 1
        low = low + d * lo // tot
        while True:
            if high < M.HALF:
                o.put_with_run(0, pending)
                pending = 0
            elif low >= M.HALF:
                o.put_with_run(1, pending)
                pending = 0
            elif low >= M.QUARTER and high < M.THREE_QUARTERS:
                pending += 1
                low -= M.QUARTER
                high -= M.QUARTER
            else:
                break
            high = (2 * high + 1) & M.MAX_CODE
            low = (2 * low) & M.MAX_CODE
    return o.stream()


@pytest.mark.parametrize("name", C.NAMES)
def test_the_sink_agrees_with_the_model(name):
    c = C.CASES[name]
    assert _sink_stream(c.data, None) == c.enc


@pytest.mark.parametrize("fault", (NO_HEAD, SHORT_LOOP))
def test_a_faulty_sink_is_told_apart(fault):
    pend = [n for n in C.NAMES if n.startswith("pending")]
    caught = [n for n in pend if _sink_stream(C.CASES[n].data, fault) != C.CASES[n].enc]
    assert caught, fault
    if fault == NO_HEAD:                                                  # exactly the cases with a long run behind a word's last bit
        assert set(caught) == {n for n in pend if any(k >= 32 and at == 31 for k, at in C.CASES[n].runs)}
    else:                                                                 # every case with a whole word behind the head
        assert set(caught) == {n for n in pend if any(k - min(k, 32 - (at + 1) % 32) >= 32 for k, at in C.CASES[n].runs if k >= 32)}
