// huff_rune_mid_dec_plan_test.cpp -- the host side of the mid-size grouped rune decoder (raisin_amd/csrc/huff_rune_mid_dec.hip), with g++ alone:
//   the parse   huff_parse_rune.h at ParseRuneMid's limits (what k_huff_mid_rune_dec runs per member, k_huff_dev_rune_mid_plan and the host's
//               classifier in front of the tree) against the host's parse_header + build_tree + assign_codes (huff_host.cpp), field by
//               field, at the class's edges -- counts of 16385, 65536 and 65537, promises of 16384, 16385, 65536 and 65537 bytes, payloads
//               of 69120 and 69121 bytes, codes of 32 and 33 bits -- and over random alphabets;
//   the default the same inputs through the default limits and through ParseRuneSmall: bit-identical plans, and the host's answer at the
//               16 KiB class's figures written out here as numbers;
//   the rules   huff_rune_select.h's one selection at both classes' rules (ParseRuneMid, ParseRuneSmall) against a brute-force statement: the
//               513-byte prefilter, the promise's lower bound, the minimum, `rest` untouched below it.
// Built and run by tests/test_huff_rune_mid_dec_host.py, plain and under the address and undefined-behaviour sanitizers.
// Prints "rune mid dec: ok <streams> planned <k> trials <t> took <t1> below <t2> consts <OUT_MAX> <PAY_MAX> <GROUP_MIN> <STREAM_MAX> <PAY_MIN>" and exits 0, or
// the first disagreement and 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "huff_host.h"
#include "huff_parse_rune.h"
#include "huff_rune_select.h"

using namespace rsn;

namespace {

struct Limits { uint32_t stream_max, out_max, count_max, lanes, s_max; };
constexpr Limits SMALL = {256 * 10 + 3 + 8 + 18432, 16384, 16384, 256, 576};         // the 16 KiB class's, as numbers
constexpr Limits MID = {256 * 10 + 3 + 8 + 69120, 65536, 65536, 960, 576};
static_assert(ParseRuneMid::STREAM_MAX == MID.stream_max && ParseRuneMid::OUT_MAX == MID.out_max && ParseRuneMid::COUNT_MAX == MID.count_max &&
              ParseRuneMid::LANES == MID.lanes && ParseRuneMid::S_MAX == MID.s_max && ParseRuneMid::PAY_MAX == 69120, "the mid limits");
static_assert(ParseRuneSmall::STREAM_MAX == SMALL.stream_max && ParseRuneSmall::OUT_MAX == SMALL.out_max && ParseRuneSmall::COUNT_MAX == SMALL.count_max &&
              ParseRuneSmall::LANES == SMALL.lanes && ParseRuneSmall::S_MAX == SMALL.s_max && ParseRuneSmall::PAY_MAX == 18432, "the default limits are the constants");
static_assert(HUFF_RUNE_MID_OUT_MAX == MID.out_max && HUFF_RUNE_MID_PAY_MAX == 69120 && HUFF_RUNE_MID_STREAM_MAX == MID.stream_max, "the class's limits are the parse's");

struct Ref {
    int verdict = 1;
    uint16_t child[512] = {0};
    uint32_t leaf_rune[256] = {0};
    uint32_t a = 0, root = 0, n_child = 0, K = 0, flat = 0, A0 = 0, p0 = 0, end = 0, pay_words = 0, max_len = 0;
    unsigned long long expect = 0;
};

// the plan as the host's own functions give it, at the limits L
void ref_plan(const uint8_t *in, size_t n, const Limits &L, Ref &r) {
    r = Ref();
    if (n < 8 || n > L.stream_max) return;
    size_t sep = (size_t)-1;
    for (size_t i = 0; i + 1 < std::min<size_t>(n, PARSE_RUNE_SCAN_MAX); i++) if (in[i] == 0x5C && in[i + 1] == 0x0A) { sep = i; break; }
    if (sep == (size_t)-1 || sep + 4 > n) return;
    std::vector<HuffSym> syms; std::string msg;
    if (!parse_header(in, sep, syms, msg) || syms.size() < 2 || syms.size() > 256) return;
    unsigned long long expect = 0;
    bool high = false;
    for (const HuffSym &sy : syms) { if (sy.freq > L.count_max) return; high = high || sy.rune >= 0x80; expect += sy.freq * (unsigned)utf8_len(sy.rune); }
    if (!high || expect == 0 || expect > L.out_max) return;
    const size_t pay = sep + 3, sn = n - sep - 2;
    const unsigned diff = in[sep + 2];
    const unsigned long long nbits = (unsigned long long)(sn - 1) * 8;
    if (diff >= nbits) return;
    const uint32_t span = (uint32_t)(nbits - diff);
    if (std::max<uint32_t>(64, ((span + L.lanes - 1) / L.lanes + 31) / 32 * 32) > L.s_max) return;
    HuffTree tree; HuffCodes codes;
    if (!build_tree(syms, tree, msg) || !assign_codes(tree, codes, msg, false)) return;
    r.max_len = codes.max_len;
    if (codes.max_len > 32 || codes.max_len == 0) return;
    const uint32_t A = tree.n_leaves;
    const size_t n_int = tree.freq.size() - A;
    for (size_t i = 0; i < n_int; i++) {
        const int32_t kids[2] = {tree.left[A + i], tree.right[A + i]};
        for (int b = 0; b < 2; b++) r.child[2 * i + b] = tree.is_leaf(kids[b]) ? (uint16_t)(0x8000u | (uint32_t)kids[b]) : (uint16_t)(kids[b] - (int32_t)A);
    }
    for (uint32_t l = 0; l < A; l++) r.leaf_rune[l] = tree.rune[l];
    r.a = A;
    r.root = (uint32_t)(tree.root - (int32_t)A);
    r.A0 = (uint32_t)(pay & ~(size_t)3);
    r.pay_words = (uint32_t)((n - r.A0 + 3) / 4) + 8;
    r.p0 = (uint32_t)(8 * (pay - r.A0) + diff);
    r.end = (uint32_t)(8 * (pay - r.A0) + nbits);
    r.K = std::min<unsigned>(codes.max_len, PARSE_K_MAX); r.n_child = (uint32_t)(2 * n_int);
    r.flat = codes.min_len == codes.max_len ? codes.max_len : 0u;
    r.expect = expect;
    r.verdict = 0;
}

long long g_streams = 0, g_planned = 0;

bool fail(const char *what, size_t n, const char *part, unsigned long long a, unsigned long long b) {
    printf("%s (n = %zu): %s differs: host %llu, plan %llu\n", what, n, part, a, b);
    return false;
}

// the subject gets a copy of n bytes in an allocation of exactly n bytes, so that the sanitizer sees a read at or behind n
template <class L>
bool check_at(const std::vector<uint8_t> &buf, const Limits &lim, const char *what, int want_verdict, uint32_t want_deepest, HuffRunePlan &plan) {
    const size_t n = buf.size();
    g_streams++;
    Ref r;
    ref_plan(buf.data(), n, lim, r);
    uint8_t *exact = (uint8_t *)malloc(n ? n : 1);
    memcpy(exact, buf.data(), n);
    ParseRuneInfo info;
    parse_rune_plan_serial<L>(exact, n, plan, &info);
    const HuffDevSummary light = parse_rune_light<L>(exact, n);
    free(exact);
    const HuffDevBounds &p = plan.b;
    if (want_verdict >= 0 && r.verdict != want_verdict) return fail(what, n, "the host's verdict from the expected one", (unsigned long long)r.verdict, (unsigned long long)want_verdict);
    if (want_deepest && (r.max_len != want_deepest || info.deepest != want_deepest)) return fail(what, n, "the deepest code from the expected one", r.max_len, info.deepest);
    if ((uint32_t)r.verdict != p.verdict) return fail(what, n, "verdict", (unsigned long long)r.verdict, p.verdict);
    if (r.verdict != 0) return true;                                    // (the light scan may still say planned: the depths need the tree)
    g_planned++;
    if (light.verdict != PARSE_PLANNED || light.A0 != r.A0 || light.span != r.end - r.p0 || light.expect != r.expect) return fail(what, n, "the light scan", r.expect, light.expect);
    if (r.a != plan.a) return fail(what, n, "leaves", r.a, plan.a);
    if (r.root != p.root) return fail(what, n, "root", r.root, p.root);
    if (r.n_child != p.n_child) return fail(what, n, "n_child", r.n_child, p.n_child);
    for (uint32_t i = 0; i < 512; i++) if (r.child[i] != plan.child[i]) return fail(what, n, "child", r.child[i], plan.child[i]);
    for (uint32_t i = 0; i < 256; i++) if (r.leaf_rune[i] != plan.leaf_rune[i]) return fail(what, n, "leaf rune", r.leaf_rune[i], plan.leaf_rune[i]);
    if (r.K != p.K) return fail(what, n, "K", r.K, p.K);
    if (r.flat != p.flat) return fail(what, n, "flat", r.flat, p.flat);
    if (r.A0 != p.A0) return fail(what, n, "A0", r.A0, p.A0);
    if (r.p0 != p.p0) return fail(what, n, "p0", r.p0, p.p0);
    if (r.end != p.end) return fail(what, n, "end", r.end, p.end);
    if (r.pay_words != p.pay_words) return fail(what, n, "pay_words", r.pay_words, p.pay_words);
    if (r.expect != p.expect) return fail(what, n, "expect", r.expect, p.expect);
    return true;
}

// the stream at the mid limits (want: the verdict expected there, -1: whatever the host says), and at the default limits three ways
bool check(const std::vector<uint8_t> &buf, const char *what, int want_mid = -1, uint32_t want_deepest = 0) {
    HuffRunePlan mid, small, dflt;
    if (!check_at<ParseRuneMid>(buf, MID, what, want_mid, want_deepest, mid)) return false;
    if (!check_at<ParseRuneSmall>(buf, SMALL, what, -1, 0, small)) return false;
    parse_rune_plan_serial(buf.data(), buf.size(), dflt);               // the default template argument: today's call
    const HuffDevSummary a = parse_rune_light(buf.data(), buf.size()), b = parse_rune_light<ParseRuneSmall>(buf.data(), buf.size());
    if (memcmp(&dflt, &small, sizeof(dflt)) != 0 || memcmp(&a, &b, sizeof(a)) != 0) return fail(what, buf.size(), "the default limits from ParseRuneSmall", 0, 1);
    return true;
}

void put_rune(std::string &s, uint32_t r) {
    uint8_t b[4];
    s.append((const char *)b, parse_rune_write(r, b));
}
std::string header(const std::vector<std::pair<uint32_t, uint32_t>> &ents /*(count, rune)*/) {
    std::string h;
    for (const auto &e : ents) { h += std::to_string(e.first); h += '|'; put_rune(h, e.second); }
    return h;
}
std::vector<uint8_t> stream_of(const std::string &hdr, size_t pay_bytes, std::mt19937_64 &rng, int diff = 0) {
    std::vector<uint8_t> out(hdr.begin(), hdr.end());
    out.push_back(0x5C); out.push_back(0x0A); out.push_back((uint8_t)diff);
    for (size_t i = 0; i < pay_bytes; i++) out.push_back((uint8_t)rng());
    return out;
}

bool edges(std::mt19937_64 &rng) {
    bool ok = true;
    // counts: 'a' as often as that, and a rune that does not occur
    ok = ok && check(stream_of(header({{16385, 'a'}, {1, 0xE9}}), 3000, rng), "a count of 16385", 0);
    ok = ok && check(stream_of(header({{65536, 'a'}, {0, 0xE9}}), 3000, rng), "a count of 65536", 0);
    ok = ok && check(stream_of(header({{65537, 'a'}, {0, 0xE9}}), 3000, rng), "a count of 65537", 1);
    ok = ok && check(stream_of(header({{100000, 'a'}, {0, 0xE9}}), 3000, rng), "a count of six digits", 1);
    // promises: p - 2 bytes of 'a' and one e-acute
    for (uint32_t p : {16384u, 16385u, 65536u}) ok = ok && check(stream_of(header({{p - 2, 'a'}, {1, 0xE9}}), 4000, rng), "a promise inside the parse's limits", 0);
    ok = ok && check(stream_of(header({{65535, 'a'}, {1, 0xE9}}), 4000, rng), "a promise of 65537", 1);
    ok = ok && check(stream_of(header({{16384, 0x1D11E}, {1, 'a'}}), 4000, rng), "a promise of 65537 in 4-byte runes", 1);
    // the payload: 960 lanes of 576 bits, and one byte more; a pad byte that brings it back inside
    const std::string h = header({{20000, 'a'}, {9000, 0xE9}, {700, 0x20AC}});
    ok = ok && check(stream_of(h, 69120, rng), "a payload of 69120 bytes", 0);
    ok = ok && check(stream_of(h, 69121, rng), "a payload of 69121 bytes", 1);
    ok = ok && check(stream_of(h, 69121, rng, 8), "69121 bytes of which the pad byte takes eight bits", 0);
    ok = ok && check(stream_of(h, 18432, rng), "a payload of 18432 bytes", 0);
    ok = ok && check(stream_of(h, 18433, rng), "a payload of 18433 bytes", 0);
    ok = ok && check(stream_of(h, 512, rng), "a payload of 512 bytes", 0);
    // the longest header in front of the largest payload: the stream's length limit
    {
        std::vector<std::pair<uint32_t, uint32_t>> e;
        for (uint32_t k = 0; k < 256; k++) e.push_back({k ? 10u : 10000u, 0x10000 + k});
        const std::string hh = header(e);
        ok = ok && check(stream_of(hh, 69120, rng), "256 four-byte runes, 69120 bytes", 0);
    }
    // depth: z runes that do not occur make a comb (Go's heap pops the zeros in that order) of z - 1 ... bits
    for (uint32_t z : {57u, 58u}) {
        std::vector<std::pair<uint32_t, uint32_t>> e;
        for (uint32_t k = 0; k < z; k++) e.push_back({0, 0x400 + k});
        e.push_back({20000, 'a'}); e.push_back({20001, 0xE9});
        ok = ok && check(stream_of(header(e), 4500, rng), z == 57 ? "depth 32" : "depth 33", z == 57 ? 0 : 1, z == 57 ? 32 : 33);
    }
    return ok;
}

bool random_streams(std::mt19937_64 &rng, int count) {
    for (int t = 0; t < count; t++) {
        const uint32_t a = 2 + (uint32_t)(rng() % 255), target = 1 + (uint32_t)(rng() % 70000);
        std::vector<std::pair<uint32_t, uint32_t>> e;
        uint32_t left = target;
        for (uint32_t k = 0; k < a; k++) {
            const uint32_t r = (k == 0) ? 0xE9 : (rng() % 4 == 0 ? 0x21 + k % 0x5E : rng() % 3 == 0 ? 0x10000 + k : 0x100 + 5 * k);
            if (r == '\\' || r == '|' || (r >= '0' && r <= '9')) { continue; }
            const uint32_t w = plan_rune_utf8_len(r), c = k + 1 == a ? left / w : (uint32_t)(rng() % (2 * (left / w) / (a - k) + 2));
            const uint32_t cc = std::min(c, left / w);
            e.push_back({cc, r});
            left -= cc * w;
        }
        std::shuffle(e.begin(), e.end(), rng);
        const size_t pay = rng() % 4 == 0 ? 69000 + rng() % 200 : 1 + rng() % 70000;
        if (!check(stream_of(header(e), pay, rng, (int)(rng() % 8)), "a random alphabet")) return false;
    }
    return true;
}

// ---- the select rules against a brute-force statement: the one selection (huff_rune_select.h) at each class's rules, the statement from
// the class's figures written out here as numbers
struct Rules { size_t len_min, stream_max; uint32_t out_min, out_max, pay_max; size_t group_min; };
constexpr Rules MID_RULES = {513 + 3, MID.stream_max, 16385, 65536, 69120, 16};     // the prefilter: 513 bytes of payload behind separator and pad byte
constexpr Rules SMALL_RULES = {0, SMALL.stream_max, 1, 16384, 18432, 16};
struct Member { size_t len; HuffDevSummary sum; bool may; };
long long g_trials = 0, g_took = 0, g_below = 0;       // trials; those in which members left `rest`; those with candidates and too few planned

template <class L>
bool select_trial(std::mt19937_64 &rng, const Rules &R) {
    g_trials++;
    const size_t n = 1 + rng() % 60;
    static const size_t LENS[] = {8, 515, 516, 517, 21003, 21004, HUFF_RUNE_MID_STREAM_MAX - 1, HUFF_RUNE_MID_STREAM_MAX, HUFF_RUNE_MID_STREAM_MAX + 1, 200000};
    static const uint32_t EXPECTS[] = {1, 16384, 16385, 40000, 65536, 65537, 0}, SPANS[] = {1, 8 * 18432 + 8, 8 * 69120 - 7, 8 * 69120, 8 * 69120 + 1, 8 * 18432, 8 * 18432 + 1};
    std::vector<Member> m(n);
    const bool mostly_good = rng() % 2;
    for (Member &x : m) {
        const bool good = mostly_good && rng() % 8 != 0;
        x.len = good ? R.len_min + rng() % (R.stream_max - R.len_min + 1) : LENS[rng() % 10];
        x.sum.verdict = good || rng() % 3 ? PARSE_PLANNED : PARSE_NOT_MINE;
        x.sum.A0 = good || rng() % 4 ? 4 * (uint32_t)(rng() % 128) : 1 + (uint32_t)(rng() % 300000);
        x.sum.expect = good ? R.out_min + (uint32_t)(rng() % (R.out_max - R.out_min + 1)) : EXPECTS[rng() % 7];
        x.sum.span = good ? 1 + (uint32_t)(rng() % (8 * R.pay_max)) : SPANS[rng() % 7];
        x.may = good || rng() % 4 != 0;
    }
    std::vector<size_t> rest;
    for (size_t i = 0; i < n; i++) if (mostly_good ? rng() % 10 != 0 : rng() % 2) rest.push_back(i);
    std::shuffle(rest.begin(), rest.end(), rng);
    // the statement
    std::vector<size_t> cand_want, idx_want, rest_want = rest;
    for (size_t i : rest) if (m[i].may && m[i].len >= R.len_min && m[i].len <= R.stream_max) cand_want.push_back(i);
    std::sort(cand_want.begin(), cand_want.end());
    if (cand_want.size() < R.group_min) cand_want.clear();
    for (size_t i : cand_want) {
        const HuffDevSummary &v = m[i].sum;
        if (v.verdict == PARSE_PLANNED && v.A0 % 4 == 0 && v.A0 <= m[i].len && v.expect >= R.out_min && v.expect <= R.out_max && (v.span + 7) / 8 <= R.pay_max) idx_want.push_back(i);
    }
    if (idx_want.size() < R.group_min) idx_want.clear();
    else {
        rest_want.clear();
        for (size_t i : rest) if (!std::binary_search(idx_want.begin(), idx_want.end(), i)) rest_want.push_back(i);
        std::sort(rest_want.begin(), rest_want.end());
    }
    // the rules, as both offers call them
    auto len = [&](size_t i) { return m[i].len; };
    const std::vector<size_t> cand = rune_dec_candidates<L>(rest, [&](size_t i) { return m[i].may; }, len);
    if (cand != cand_want) { printf("select trial %lld: the candidates differ\n", g_trials); return false; }
    std::vector<HuffDevSummary> sums;
    for (size_t i : cand) sums.push_back(m[i].sum);
    std::vector<size_t> idx;
    std::vector<uint32_t> expect;
    rune_dec_planned<L>(cand, cand.size(), sums.data(), len, idx, expect);
    const bool left = rune_dec_leave<L>(rest, idx);
    g_took += left; g_below += !left && !cand.empty();
    if (left != !idx_want.empty() || idx != idx_want || rest != rest_want) { printf("select trial %lld: who leaves `rest` differs\n", g_trials); return false; }
    for (size_t q = 0; q < idx.size(); q++) if (expect[q] != m[idx[q]].sum.expect) { printf("select trial %lld: a promise differs\n", g_trials); return false; }
    return true;
}

}  // namespace

int main(int argc, char **argv) {
    const int random_count = argc > 1 ? atoi(argv[1]) : 300;
    std::mt19937_64 rng(0x5EEDull);
    if (!edges(rng) || !random_streams(rng, random_count)) return 1;
    for (int t = 0; t < 3000; t++) if (!select_trial<ParseRuneMid>(rng, MID_RULES)) return 1;
    const long long mid_took = g_took, mid_below = g_below;
    for (int t = 0; t < 3000; t++) if (!select_trial<ParseRuneSmall>(rng, SMALL_RULES)) return 1;
    if (mid_took < 500 || mid_below < 20 || g_took - mid_took < 500 || g_below - mid_below < 20) { printf("too few trials took or fell below: %lld %lld %lld %lld\n", mid_took, mid_below, g_took, g_below); return 1; }
    // the prefilter's own statement: 512 bytes of payload at a bit a symbol and four bytes a rune promise 16384 bytes, no more
    if (!ParseRuneMid::len_may(516) || ParseRuneMid::len_may(515) || !ParseRuneMid::len_may(HUFF_RUNE_MID_STREAM_MAX) || ParseRuneMid::len_may(HUFF_RUNE_MID_STREAM_MAX + 1)) { printf("the length rule\n"); return 1; }
    if (!ParseRuneSmall::len_may(0) || !ParseRuneSmall::len_may(HUFF_RUNE_STREAM_MAX) || ParseRuneSmall::len_may(HUFF_RUNE_STREAM_MAX + 1)) { printf("the 16 KiB class's length rule\n"); return 1; }
    printf("rune mid dec: ok %lld planned %lld trials %lld took %lld below %lld consts %u %u %zu %u %u\n", g_streams, g_planned, g_trials, g_took, g_below, HUFF_RUNE_MID_OUT_MAX, HUFF_RUNE_MID_PAY_MAX,
           HUFF_RUNE_MID_DEC_GROUP_MIN, HUFF_RUNE_MID_STREAM_MAX, HUFF_RUNE_MID_DEC_PAY_MIN);
    return 0;
}
