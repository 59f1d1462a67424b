"""The corpus the arithmetic kernels (raisin_amd/csrc/arith.hip) are held to: inputs chosen for what the kernels do with
them, each with the stream and the statistics tests/arith_model.py gives it -- never the library's.  Built once, at import.

every table position   all 256 symbols in both orders, and for register k of lane l an input that is mostly the symbol 4l + k with its
                       two neighbours mixed in: both bounds of the symbol move and are read across the lane boundary
noise                  uniform random bytes: a broad table at the freeze and at a slice's resume, streams longer than their inputs
pending runs           prefix + greedy picks + 00: runs of 32 bits and more whose deciding bit goes out at every place of a 32-bit word,
                       and runs of 31, 32, 33, 63, 64 and 65 bits
ends                   every front pad of the packed stream, bit counts that are whole words, stream lengths of 0, 1 and 15 mod 16

tests/test_arith_cases_host.py asserts each of these claims from the statistics kept here."""
import random
import re
import os
from collections import namedtuple

import arith_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SLICE_SYMBOLS = int(re.search(r"ARITH_SLICE_SYMBOLS\s*=\s*(\d+)", open(os.path.join(ROOT, "raisin_amd", "csrc", "codecs.h")).read()).group(1))

LANES = (0, 1, 31, 32, 62, 63)
NOISE_LENGTHS = (1, 2, 3, 17, 255, 256, 257, 1000, 4097, 16125, 16126, 16127, 40000)      # test_arith_host._inputs
RUN_LENGTHS = (31, 32, 33, 63, 64, 65)
PENDING_TRIES = 300

# data: the input; enc: the model's stream; nbits: the coder's bits (the stream is nbits // 8 + 1 bytes); runs: the flushed pending runs
# as (length, position mod 32 of the deciding bit)
Case = namedtuple("Case", "data enc nbits runs")


def noise(n, seed):
    rng = random.Random(seed)
    return bytes(rng.randrange(256) for _ in range(n))


def _case(data):
    bits, st = M.encode_bits(data)
    return Case(bytes(data), M.pack(bits), st["nbits"], tuple(st["runs"]))


def _position_input(lane, k):
    """600 bytes, 90 % the symbol of register k in `lane`, the rest its two neighbours"""
    s = 4 * lane + k
    rng = random.Random(0x7AB1E + s)
    near = (max(s - 1, 0), min(s + 1, 255))
    return bytes(s if rng.random() < 0.9 else near[rng.randrange(2)] for _ in range(600))


def _pending_cases():
    """of PENDING_TRIES seeded inputs, a few that cover: a run of 32 bits or more behind a deciding bit at each of the 32 places of a word,
    and a run of each of RUN_LENGTHS"""
    tries = []
    for t in range(PENDING_TRIES):
        rng = random.Random(0x9E2D0000 + t)
        prefix = bytes(rng.randrange(256) for _ in range(rng.randrange(12)))
        c = _case(M.greedy_input(rng.randrange(8, 61), prefix) + b"\x00")
        covers = {("at", at) for n, at in c.runs if n >= 32} | {("len", n) for n, _ in c.runs if n in RUN_LENGTHS}
        tries.append((t, c, covers))
    out = {}
    for _ in range(2):                                                   # each place and each length twice over, in different inputs
        want = set().union(*(cv for _, _, cv in tries))
        while want:                                                      # greedily, the try that covers most of what is still open
            t, c, cv = max((x for x in tries if "pending%03d" % x[0] not in out), key=lambda x: (len(x[2] & want), -x[0]))
            if not cv & want:
                break
            want -= cv
            out["pending%03d" % t] = c
    return out


def _end_conditions(cases):
    pads = {c.nbits % 8 for c in cases}
    whole = sum(1 for c in cases if c.nbits % 32 == 0)
    mod16 = {len(c.enc) % 16 for c in cases}
    return pads, whole, mod16


def _build():
    cases = {}
    every = bytes(range(256))
    for r in (1, 2, 3, 64):
        cases["all256x%d" % r] = _case(every * r)
        cases["rev256x%d" % r] = _case(every[::-1] * r)
    for k in range(4):
        for lane in LANES:
            cases["reg%dlane%d" % (k, lane)] = _case(_position_input(lane, k))
    for n in NOISE_LENGTHS + (SLICE_SYMBOLS - 1, SLICE_SYMBOLS, SLICE_SYMBOLS + 1):
        cases["noise%d" % n] = _case(noise(n, 0xA2170000 + n))
    cases["frozen-then-all"] = _case(b"a" * 16126 + every * 40)
    cases["hello"] = _case(b"Hello world!\n")
    cases.update(_pending_cases())
    # the ends: short noise until every front pad, two whole-word bit counts and the stream lengths 0, 1 and 15 mod 16 are there
    for n in range(1, 200):
        pads, whole, mod16 = _end_conditions(cases.values())
        if len(pads) == 8 and whole >= 2 and mod16 >= {0, 1, 15}:
            break
        c = _case(noise(n, 0xE2D50000 + n))
        if c.nbits % 8 not in pads or (whole < 2 and c.nbits % 32 == 0) or (len(c.enc) % 16 in {0, 1, 15} - mod16):
            cases["end%d" % n] = c
    return cases


CASES = _build()
NAMES = list(CASES)


def first(pred, what):
    """the first case name that meets pred(name, case)"""
    for name, c in CASES.items():
        if pred(name, c):
            return name
    raise AssertionError("no case in the corpus with " + what)


def dev_subset():
    """about a dozen names for the single device call: noise, one per register position, a pending run behind a deciding bit at place 31 of
    its word (the run starts a word) and at place 30 (one bit of it ends a word), and a bit count that is a whole number of words"""
    names = ["hello", "noise1000", "noise16127", "all256x3", "frozen-then-all", "reg0lane31", "reg1lane32", "reg2lane63", "reg3lane0",
             first(lambda n, c: any(k >= 32 and at == 31 for k, at in c.runs), "a run of 32 behind place 31"),
             first(lambda n, c: any(k >= 32 and at == 30 for k, at in c.runs), "a run of 32 behind place 30"),
             first(lambda n, c: c.nbits % 32 == 0, "a whole number of words")]
    return list(dict.fromkeys(names))
