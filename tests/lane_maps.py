"""The lane maps of the grouped Huffman decoders, restated on a CPU: lane_dec_body (raisin_amd/csrc/huff_small_body.h) as plain Python +
numpy over ONE array, nxt[p] = the end of the codeword that begins at code bit p.  Nothing of the library is imported: the shapes below are
the kernels' constants restated (tests/test_lane_maps_host.py holds them against the headers and the package's mirrored constants), the
codes are the CPU oracle's (oracle.huffman_table of the member the stream was written for), never assumed.

Coordinates: bits are counted from the stream's first code bit (behind the header's "\\\\\\n", the pad byte and the pad bits).  parse_lanes
(huff_parse_small.h) gives S bits a lane and T lanes; lane g is [g S, min(span, (g + 1) S)); a block (a tile) is DLN lanes.

The rule.  A lane does not know where its first codeword starts.  Lane 0 of a block is entered at bit 0 (block 0), at every one of its
first 32 bits (a later block), at flat0 alone (a flat code) or at the one given entry (the emit form of a tile); the exits that occur go
into a mask that lane 1 is offered in ascending order.  Every other lane first guesses its bit 0 (flat code: the first boundary in it).
In a round a lane is offered what the lane before it had published BEFORE the round, skips OFF_BAD and the starts it holds, and takes the
rest as new starts -- at most four in all, counting the ones that became fresh in the same round: a fifth sets `over`.  over: the block is
lost ("phases").  Nothing fresh in any lane: settled.  Otherwise, in a round numbered DEC_ROUNDS or more: lost ("rounds").  A settled
block's lanes compose into its 32-entry map, entry c -> (exit, symbols); a lost block's map is OFF_BAD throughout.  The blocks' maps compose
from bit 0 as bigd_chain (huff_big_dec_layout.h) and the multi-block single call compose them."""
import numpy as np

DEC_ROUNDS = 64          # huff_small_body.h: DEC_ROUNDS -- the one place this module states it
OFF_BAD = 0xFF           # huff_small_body.h: OFF_BAD
STARTS_MAX = 4           # starts a lane keeps (st[4], ex[4], cn[4])
ENTRIES = 32             # bits a later block's first lane is entered at

REASONS = ("phases", "rounds", "image", "promise", "end inside a codeword")


class Shape:
    """a decoding class: `lanes` lanes a block, `blocks` blocks at most, lanes of at most s_max bits; cap: the bytes of a block's output image
    (symbols + 16 must fit; None where one block holds the member); pay_max / out_max: payload bytes / decoded bytes of a member"""

    def __init__(self, name, lanes, blocks, s_max, cap, pay_max, out_max, runes=False):
        self.name, self.lanes, self.blocks, self.s_max, self.cap, self.pay_max, self.out_max, self.runes = name, lanes, blocks, s_max, cap, pay_max, out_max, runes


SHAPES = {
    "single": Shape("single", 256, 32, 96, 32768, 65536 + 2048, 65536),        # huff_small_body.h: DL, DEC_BLOCKS, DEC_S_MAX, DEC_OUT_CAP, DEC_STREAM_MAX, SMALL_MAX
    "small": Shape("small", 256, 1, 512, None, 16384, 32768),                  # HB_S_MAX, HB_PAY_MAX, HB_OUT_MAX
    "mid": Shape("mid", 960, 1, 480, None, 57344, 65536),                      # huff_mid.hip: HM_DL, HM_S_MAX; codecs.h: HUFF_MID_PAY_MAX, HUFF_MID_OUT_MAX
    "rune": Shape("rune", 256, 1, 576, None, 18432, 16384, runes=True),        # huff_rune_dec.hip; codecs.h: HUFF_RUNE_PAY_MAX, HUFF_RUNE_OUT_MAX (bytes)
    "tiled": Shape("tiled", 960, 30, 64, 32768, 229376, 262144),               # huff_big_dec_layout.h: BIGD_LANES, BIGD_TILES_MAX, BIGD_S, BIGD_OUT_CAP, BIGD_PAY_MAX, BIGD_OUT_MAX
}


def parse_lanes(span, lanes, s_max):
    """huff_parse_small.h: parse_lanes -> (S, T, does the class hold the span)"""
    s = max(64, ((span + lanes - 1) // lanes + 31) & ~31)
    return s, (span + s - 1) // s, s <= s_max


def split(stream):
    """(payload bytes, pad bits, span in code bits) of a stream: header, "\\\\\\n", the pad byte, the payload"""
    sep = stream.index(b"\\\n")
    pad, pay = stream[sep + 2], stream[sep + 3:]
    return pay, pad, 8 * len(pay) - pad


def code_ends(stream, table):
    """nxt[p] for p in [0, span): the end of the codeword that begins at bit p (past span: the codeword runs off the payload), and flat --
    the code's one length, 0 where lengths differ.  table: oracle.huffman_table's [(symbol, count, code, length)]."""
    pay, pad, span = split(stream)
    lens = sorted({l for _, _, _, l in table})
    mx = lens[-1]
    assert 1 <= lens[0] and mx <= 32 and span > 0
    bits = np.concatenate([np.unpackbits(np.frombuffer(pay, dtype=np.uint8))[pad:], np.zeros(mx, dtype=np.uint8)]).astype(np.uint64)
    win = np.zeros(span, dtype=np.uint64)                                     # the next mx bits at every position, zeros behind the end
    for i in range(mx):
        win |= bits[i:i + span] << np.uint64(mx - 1 - i)
    K = min(mx, 16)
    lut = np.zeros(1 << K, dtype=np.uint8)
    for _, _, code, l in table:
        if l <= K:
            lut[code << (K - l):(code + 1) << (K - l)] = l
    length = lut[(win >> np.uint64(mx - K)).astype(np.int64)].astype(np.int64)
    deep = np.nonzero(length == 0)[0]
    for l in lens:
        if l > K and len(deep):
            hit = np.isin(win[deep] >> np.uint64(mx - l), np.array([c for _, _, c, ll in table if ll == l], dtype=np.uint64))
            length[deep[hit]] = l
    assert (length > 0).all(), "the code is not complete"
    return np.arange(span, dtype=np.int64) + length, (lens[0] if len(lens) == 1 else 0)


class Cut:
    """the bit string cut every S bits: for every bit p, the codewords that start in [p, the end of p's piece) and where the last one ends
    -- run_path's answers for every `from` at once, by pointer doubling over nxt"""

    def __init__(self, nxt, S):
        span = len(nxt)
        p = np.arange(span, dtype=np.int64)
        hi = np.minimum(span, (p // S + 1) * S)
        last = nxt >= hi                                                      # the codeword at p is the last that starts in the piece
        to, cnt = np.where(last, p, nxt), (~last).astype(np.int64)
        while True:
            nto = to[to]
            if (nto == to).all():
                break
            cnt, to = cnt + cnt[to], nto
        end = nxt[to]
        self.span, self.S = span, S
        self.exit = np.where(end > span, OFF_BAD, end - hi)
        self.count = cnt + 1

    def run(self, frm, hi):
        """run_path: (exit offset from hi or OFF_BAD, codewords) from bit `frm` of the piece that ends at hi"""
        if frm >= hi:                                                         # (a short last piece entered behind its end: nothing starts)
            return (OFF_BAD if frm > self.span else frm - hi), 0
        return int(self.exit[frm]), int(self.count[frm])


class Block:
    """one block's lanes, settled or lost.  starts[t]: lane t's [start, exit, symbols, round it arrived in (-1: the first guess)] in the
    order the kernel holds them (lane 0: none); first[c]: lane 0 entered at bit c -> (exit, symbols), the entries that were answered."""
    pass


class Lanes:
    """a stream in a class's lanes: S, T, the blocks"""

    def __init__(self, nxt, flat, shape, rounds_cap=DEC_ROUNDS):
        self.nxt, self.flat, self.shape, self.span, self.rounds_cap = nxt, flat, shape, len(nxt), rounds_cap
        self.S, self.T, self.held = parse_lanes(self.span, shape.lanes * shape.blocks, shape.s_max)
        self.n_blocks = (self.T + shape.lanes - 1) // shape.lanes
        self.held = self.held and self.n_blocks <= shape.blocks
        self.cut = Cut(nxt, self.S)
        self._blocks = {}

    def _first_boundary(self, bit):
        return (self.flat - bit % self.flat) % self.flat if self.flat else 0

    def settle(self, b, entry=None):
        """block b's rounds.  entry: the emit form -- lane 0 is entered at that bit alone"""
        S, DLN, cut = self.S, self.shape.lanes, self.cut
        L = min(DLN, self.T - b * DLN)
        lo = b * DLN * S
        hi0 = min(self.span, lo + S)
        if entry is not None:
            entries = [entry]
        elif b == 0:
            entries = [0]
        elif self.flat:
            entries = [self._first_boundary(lo)]
        else:
            entries = range(ENTRIES)
        blk = Block()
        blk.b, blk.L, blk.lost, blk.why, blk.where = b, L, False, None, None
        blk.first = {c: cut.run(lo + c, hi0) for c in entries}
        mask = sorted({e for e, _ in blk.first.values() if e < ENTRIES})
        blk.mask = mask
        starts = [[] for _ in range(L)]
        for t in range(1, L):
            g = b * DLN + t
            off = self._first_boundary(g * S)
            starts[t].append([off, *cut.run(g * S + off, min(self.span, (g + 1) * S)), -1])
        work, rnd = range(1, L), 0
        while True:
            fresh, over = {}, None
            for t in work:
                offered = mask if t == 1 else [e[1] for e in starts[t - 1]]
                held = [e[0] for e in starts[t]]
                new = []
                for off in offered:
                    if off == OFF_BAD or off in held or off in new:
                        continue
                    if len(held) + len(new) >= STARTS_MAX:
                        over = over or (t, off)
                        break
                    new.append(off)
                if new:
                    fresh[t] = new
            if over:
                blk.lost, blk.why, blk.where = True, "phases", over
                break
            if not fresh:
                break
            for t, new in fresh.items():                                      # (the kernel adds them before it looks at the round's number: the same verdict)
                g = b * DLN + t
                for off in new:
                    starts[t].append([off, *cut.run(g * S + off, min(self.span, (g + 1) * S)), rnd])
            if rnd >= self.rounds_cap:
                blk.lost, blk.why, blk.where = True, "rounds", (max(fresh), fresh[max(fresh)][0])
                break
            work, rnd = [t + 1 for t in sorted(fresh) if t + 1 < L], rnd + 1
        blk.rounds = rnd                                                      # the rounds that learned something (a lost block: the round it was lost in)
        blk.starts = starts
        blk.fullest = max([len(s) for s in starts] + [0])
        return blk

    def block(self, b):
        if b not in self._blocks:
            self._blocks[b] = self.settle(b)
        return self._blocks[b]

    def follow(self, blk, e, c, per_lane=None):
        """from lane 0's answer (exit e, c symbols) through lanes 1 .. L - 1 -> (exit of the block's last lane, symbols of the block)"""
        for t in range(1, blk.L):
            if e == OFF_BAD:
                break
            hit = [x for x in blk.starts[t] if x[0] == e]
            if not hit:
                return OFF_BAD, c
            if per_lane is not None:
                per_lane.append((t, hit[0][0], hit[0][2]))
            e, c = hit[0][1], c + hit[0][2]
        return e, c

    def block_map(self, b):
        """the block's 32-entry map: [(exit, symbols)], (OFF_BAD, 0) where lost or not answered"""
        blk = self.block(b)
        out, memo = [(OFF_BAD, 0)] * ENTRIES, {}
        if blk.lost:
            return out
        for c, (e, n) in blk.first.items():
            if c >= ENTRIES:
                continue
            if e not in memo:
                memo[e] = self.follow(blk, e, 0)
            e2, n2 = memo[e]
            out[c] = (e2, n + n2) if e2 != OFF_BAD else (OFF_BAD, 0)
        return out

    def verdict(self, expect):
        """(taken, reason, records): the maps composed from bit 0.  records: per block (entry, first output symbol, symbols); reason: one
        of REASONS where handed back.  expect: the symbols the header promises."""
        c, base, recs = 0, 0, []
        for b in range(self.n_blocks):
            blk = self.block(b)
            if blk.lost:
                return False, blk.why, recs
            e, n = self.block_map(b)[c]
            if e >= ENTRIES:
                return False, "end inside a codeword", recs                  # the path runs off the payload
            if self.shape.cap is not None and n + 16 > self.shape.cap:
                return False, "image", recs
            if base + n > expect:
                return False, "promise", recs
            recs.append((c, base, n))
            base, c = base + n, e
        if c != 0:
            return False, "end inside a codeword", recs
        return True, None, recs

    def true_lanes(self, b, entry):
        """the true path through block b entered at `entry`: [(lane of the block, start, symbols)]"""
        blk = self.block(b)
        e, n = blk.first[entry]
        out = [(0, entry, n)]
        self.follow(blk, e, n, out)
        return out

    def emit(self, b, entry):
        """the emit form of tile b from its true entry -> (block, symbols it arrives at or None where it is lost or off the payload)"""
        blk = self.settle(b, entry)
        if blk.lost:
            return blk, None
        e, n = self.follow(blk, *blk.first[entry])
        return blk, (n if e != OFF_BAD else None)


def tile_model(nxt, tile_bits, flat=0):
    """The tile-level model of tests/huff_big_dec_plan_test.cpp restated over nxt: "the codewords that start in the tile from entry c" ->
    per tile the 32 answers (exit, symbols); OFF_BAD where the walk passes the end.  It has no lanes, so no phases and no rounds to lose."""
    cut = Cut(nxt, tile_bits)
    span = len(nxt)
    out = []
    for t in range((span + tile_bits - 1) // tile_bits):
        hi = min(span, (t + 1) * tile_bits)
        row = []
        for c in range(ENTRIES):
            e, n = cut.run(t * tile_bits + c, hi)
            row.append((e, n) if e != OFF_BAD else (OFF_BAD, 0))
        out.append(row)
    return out


def model(stream, table, cls, expect=None, rounds_cap=DEC_ROUNDS):
    """A stream in a class -> (Lanes, taken, reason).  The class must hold the span (Lanes.held); expect: the header's promise in symbols,
    by default what the oracle's table counts."""
    nxt, flat = code_ends(stream, table)
    ln = Lanes(nxt, flat, SHAPES[cls], rounds_cap)
    if expect is None:
        expect = sum(f for _, f, _, _ in table)
    taken, why, recs = ln.verdict(expect)
    ln.records = recs
    return ln, taken, why
