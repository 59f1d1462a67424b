// The staging layout of the grouped batch kernels (raisin_amd/csrc/group_layout.h) as plain host code: the cut into groups, and what keeps a
// kernel inside its buffers -- 16-aligned offsets, disjoint slots, zero padding behind every input.  Prints the number of checks it made.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>
#include <vector>

#include "group_layout.h"

using namespace rsn;

static unsigned long long checks = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        checks++;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

// codecs.h, the kernel units and the closed formulas tests/test_gpu_lzss_mid.py and tests/test_gpu_huffman_mid.py restate
constexpr size_t GROUP_MAX = 4096, GROUP_BYTES = (size_t)16 << 20;
constexpr size_t MEMBER_ENTRY = 16, DEC_ENTRY = 608;                      // sizeof(SmallMember), sizeof(SmallDecArgs)
constexpr size_t SL_E_MAX = 2048, SL_DEC_E_MAX = 8192, MID_E_MAX = 69632, HDR_MAX = 1100;
static size_t up(size_t n) { return (n + 15) / 16 * 16; }

struct Member { size_t n, in_bytes, out_bytes, expect; };                  // n: the bytes copied into the input slot; expect: the output a decoder's header promises
struct Class {
    const char *name;
    size_t entry, pad, n_lo, n_hi;                                         // pad: zeros the kernel's loads rely on behind n bytes
    std::function<Member(size_t n, std::mt19937_64 &)> member;
    std::function<size_t(const Member &)> closed;                          // the need of a member, written out
};

static std::vector<Class> classes() {
    return {
        {"lzss small compress", MEMBER_ENTRY, 32, 1, 1024, [](size_t n, std::mt19937_64 &) { return Member{n, lzss_in_slot(n), lzss_enc_out_slot(n, SL_E_MAX), 0}; },
         [](const Member &m) { return 16 + up(m.n) + 32 + up(2 * m.n) + 16 + 16; }},
        {"lzss small decompress", MEMBER_ENTRY, 32, 1, 2048, [](size_t n, std::mt19937_64 &) { return Member{n, lzss_in_slot(n), lzss_dec_out_slot(SL_DEC_E_MAX), 0}; },
         [](const Member &m) { return 16 + up(m.n) + 32 + SL_DEC_E_MAX + 16 + 16; }},
        {"lzss mid compress", MEMBER_ENTRY, 32, 1, 65536, [](size_t n, std::mt19937_64 &) { return Member{n, lzss_in_slot(n), lzss_enc_out_slot(n, MID_E_MAX), 0}; },
         [](const Member &m) { return 16 + up(m.n) + 32 + up(std::min(2 * m.n, MID_E_MAX)) + 16 + 16; }},
        {"lzss mid decompress", MEMBER_ENTRY, 32, 1, MID_E_MAX, [](size_t n, std::mt19937_64 &) { return Member{n, lzss_in_slot(n), lzss_dec_out_slot(MID_E_MAX), 0}; },
         [](const Member &m) { return 16 + up(m.n) + 32 + MID_E_MAX + 16 + 16; }},
        {"huffman small compress", MEMBER_ENTRY, 16, 2, 16384, [](size_t n, std::mt19937_64 &) { return Member{n, huff_enc_in_slot(n), huff_small_enc_out_slot((uint32_t)n), 0}; },
         [](const Member &m) { return 16 + up(m.n) + 16 + up(HDR_MAX + m.n) + 16; }},
        {"huffman mid compress", MEMBER_ENTRY, 16, 16385, 65536, [](size_t n, std::mt19937_64 &) { return Member{n, huff_enc_in_slot(n), huff_mid_enc_out_slot((uint32_t)n), 0}; },
         [](const Member &m) { return 16 + up(m.n) + 16 + up(HDR_MAX + (7 * m.n + 7) / 8 + 3) + 16; }},
        // a decoder's member: n = the stream from the 4-byte boundary in front of its payload; the header promises up to 64 KiB of output
        {"huffman decompress", DEC_ENTRY, 64, 5, HDR_MAX + 8 + 57344, [](size_t n, std::mt19937_64 &rng) { const size_t e = 1 + rng() % 65536; return Member{n, huff_dec_in_slot(n), huff_dec_out_slot(e), e}; },
         [](const Member &m) { return DEC_ENTRY + up(m.n) + 64 + up(m.expect) + 16 + 16; }},
    };
}

static void test_next_group() {
    auto unit = [](size_t) { return (size_t)10; };
    // exactly max_members fill a group, one more starts the next
    GroupCut c = next_group(0, 8, 8, 1000, unit);
    CHECK(c.hi == 8 && c.bytes == 80);
    c = next_group(0, 9, 8, 1000, unit);
    CHECK(c.hi == 8 && c.bytes == 80);
    c = next_group(8, 9, 8, 1000, unit);
    CHECK(c.hi == 9 && c.bytes == 10);
    // the byte limit cuts where bytes + need first exceeds it, not a member earlier
    c = next_group(0, 100, 100, 50, unit);
    CHECK(c.hi == 5 && c.bytes == 50);
    c = next_group(0, 100, 100, 59, unit);
    CHECK(c.hi == 5 && c.bytes == 50);
    c = next_group(0, 100, 100, 60, unit);
    CHECK(c.hi == 6 && c.bytes == 60);
    // a member larger than max_bytes is a group of its own, wherever it stands
    const size_t sizes[] = {10, 500, 10, 10, 700, 10};
    auto sized = [&](size_t k) { return sizes[k]; };
    const size_t want_hi[] = {1, 2, 4, 5, 6};
    size_t lo = 0;
    for (size_t g = 0; g < 5; g++) { c = next_group(lo, 6, 100, 100, sized); CHECK(c.hi == want_hi[g]); lo = c.hi; }
    CHECK(lo == 6);
    c = next_group(3, 3, 8, 100, unit);                                    // nothing left
    CHECK(c.hi == 3 && c.bytes == 0);
    // the small LZSS decoder's members of at most 16 bytes: 8288 bytes each, 2024 to a group of 16 MiB
    auto readme = [](size_t) { return group_need(MEMBER_ENTRY, lzss_in_slot(13), lzss_dec_out_slot(SL_DEC_E_MAX)); };
    CHECK(readme(0) == 8288);
    c = next_group(0, 2025, GROUP_MAX, GROUP_BYTES, readme);
    CHECK(c.hi == 2024 && c.bytes == 2024 * 8288);
}

struct Span { size_t lo, hi; };

static void test_class(const Class &cl, unsigned long long seed, int lists) {
    std::mt19937_64 rng(seed);
    for (int it = 0; it < lists; it++) {
        // sizes: mostly random in the class's range, the ends and the 16-byte boundaries among them; now and then enough to cut a group
        const size_t count = it % 64 == 0 ? 4000 + rng() % 400 : 1 + rng() % 24;
        std::vector<Member> ms;
        for (size_t k = 0; k < count; k++) {
            size_t n;
            switch (rng() % 8) {
            case 0: n = cl.n_lo; break;
            case 1: n = cl.n_hi; break;
            case 2: n = std::min(cl.n_hi, std::max(cl.n_lo, (cl.n_lo + rng() % (cl.n_hi - cl.n_lo + 1)) / 16 * 16 + (rng() % 3) - 1)); break;
            default: n = cl.n_lo + rng() % (cl.n_hi - cl.n_lo + 1);
            }
            ms.push_back(cl.member(n, rng));
        }
        auto need = [&](size_t k) { return group_need(cl.entry, ms[k].in_bytes, ms[k].out_bytes); };
        size_t lo = 0, groups = 0;
        while (lo < count) {
            const GroupCut cut = next_group(lo, count, GROUP_MAX, GROUP_BYTES, need);
            const size_t g = cut.hi - lo;
            CHECK(cut.hi > lo && cut.hi <= count && g <= GROUP_MAX);                        // the groups partition [0, count) in order
            CHECK(g == 1 || cut.bytes <= GROUP_BYTES);
            CHECK(cut.hi == count || g == GROUP_MAX || cut.bytes + need(cut.hi) > GROUP_BYTES);   // (not cut a member early)
            GroupLayout lay(g, cl.entry);
            std::vector<Span> spans{{0, g * cl.entry}};
            size_t sum = 0, closed = 0;
            for (size_t k = lo; k < cut.hi; k++) {
                const Member &m = ms[k];
                const MemberSlots o = lay.member(m.in_bytes, m.out_bytes);
                CHECK(o.in % 16 == 0 && o.out % 16 == 0 && o.status % 16 == 0);
                CHECK(m.in_bytes >= m.n + cl.pad);                                          // zeros behind the member's bytes
                spans.push_back({o.in, o.in + m.in_bytes});
                spans.push_back({o.out, o.out + m.out_bytes});
                spans.push_back({o.status, o.status + GROUP_STATUS_BYTES});
                sum += need(k); closed += cl.closed(m);
            }
            // table, inputs, outputs and status words: handed out in rising order, so disjoint iff no span starts before its predecessor ends
            for (size_t q = 1; q < spans.size(); q++) CHECK(spans[q].lo >= spans[q - 1].hi && spans[q].hi > spans[q].lo);
            CHECK(spans.back().hi == lay.end());
            CHECK(lay.end() == sum && sum == cut.bytes && sum == closed);
            CHECK(lay.end() <= 0xFFFFFFFFull);
            lo = cut.hi; groups++;
        }
        CHECK(lo == count && groups >= 1);
    }
}

int main(int argc, char **argv) {
    const int lists = argc > 1 ? std::atoi(argv[1]) : 3000;
    test_next_group();
    unsigned long long seed = 20240;
    for (const Class &cl : classes()) test_class(cl, seed++, lists);
    std::printf("group layout: %llu checks\n", checks);
    return 0;
}
