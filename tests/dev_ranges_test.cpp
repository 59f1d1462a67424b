// The overlap check of the batch calls on device buffers (raisin_amd/csrc/dev_ranges.h) as plain host code, held against the quadratic
// comparison it replaces: random members on a small address line, where ranges touch, nest and coincide all the time.  Prints the number
// of checks it made.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "dev_ranges.h"

using namespace rsn;

static unsigned long long checks = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        checks++;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

struct Member { uintptr_t in, n, out, cap; };

static bool meet(uintptr_t a, uintptr_t na, uintptr_t b, uintptr_t nb) { return a && b && na && nb && a < b + nb && b < a + na; }

// 0 / 1 / 2 as dev_ranges_clash answers, every pair looked at
static int brute(const std::vector<Member> &ms) {
    for (size_t i = 0; i < ms.size(); i++)
        for (size_t j = i + 1; j < ms.size(); j++)
            if (meet(ms[i].out, ms[i].cap, ms[j].out, ms[j].cap)) return 1;
    for (size_t i = 0; i < ms.size(); i++)
        for (size_t j = 0; j < ms.size(); j++)
            if (meet(ms[i].out, ms[i].cap, ms[j].in, ms[j].n)) return 2;
    return 0;
}

static int fast(const std::vector<Member> &ms, size_t *a, size_t *b) {
    std::vector<DevRange> ins, outs;
    for (size_t i = 0; i < ms.size(); i++) {
        add_dev_range(ins, (const void *)ms[i].in, ms[i].n, i);
        add_dev_range(outs, (const void *)ms[i].out, ms[i].cap, i);
    }
    for (const DevRange &r : ins) CHECK(r.lo < r.hi);
    for (const DevRange &r : outs) CHECK(r.lo < r.hi);
    return dev_ranges_clash(ins, outs, a, b);
}

static void test_named_cases() {
    size_t a = 99, b = 99;
    // an output over ANOTHER member's input
    std::vector<Member> ms = {{0x1000, 64, 0x2000, 64}, {0x3000, 64, 0x1030, 64}};
    CHECK(fast(ms, &a, &b) == 2 && a == 1 && b == 0);
    // ... and over its own
    ms = {{0x1000, 64, 0x1010, 64}};
    CHECK(fast(ms, &a, &b) == 2 && a == 0 && b == 0);
    // two outputs
    ms = {{0x1000, 64, 0x2000, 64}, {0x3000, 64, 0x2030, 64}};
    CHECK(fast(ms, &a, &b) == 1 && a == 0 && b == 1);
    // ranges that touch end to start, one input handed in twice, an empty input inside an output, an empty output inside an input
    ms = {{0x1000, 64, 0x1040, 64}, {0x1000, 64, 0x1080, 64}, {0x1050, 0, 0x10C0, 16}, {0x1000, 16, 0x1008, 0}, {0, 0, 0, 0}};
    CHECK(fast(ms, &a, &b) == 0);
    // an input that spans several outputs meets the first of them
    ms = {{0x5000, 16, 0x1000, 16}, {0x5010, 16, 0x1010, 16}, {0x1008, 64, 0x6000, 16}};
    CHECK(fast(ms, &a, &b) == 2 && b == 2 && (a == 0 || a == 1));
    // one byte is enough
    ms = {{0x1000, 17, 0x1010, 16}};
    CHECK(fast(ms, &a, &b) == 2);
    ms = {{0x1000, 16, 0x1010, 16}};
    CHECK(fast(ms, &a, &b) == 0);
}

int main(int argc, char **argv) {
    const int lists = argc > 1 ? std::atoi(argv[1]) : 20000;
    test_named_cases();
    std::mt19937_64 rng(0xD0E5);
    int clean = 0, out_out = 0, out_in = 0;
    for (int it = 0; it < lists; it++) {
        const size_t count = 1 + rng() % (it % 16 == 0 ? 40 : 6);
        const uintptr_t line = 64 + rng() % (it % 3 == 0 ? 4096 : 512);   // (a crowded line and a roomy one)
        std::vector<Member> ms(count);
        for (Member &m : ms) {
            m.in = rng() % 8 == 0 ? 0 : 16 * (1 + rng() % line);
            m.n = rng() % 6 == 0 ? 0 : 1 + rng() % 48;
            m.out = rng() % 8 == 0 ? 0 : 16 * (1 + rng() % line);
            m.cap = rng() % 6 == 0 ? 0 : 1 + rng() % 48;
        }
        size_t a = 0, b = 0;
        const int want = brute(ms), got = fast(ms, &a, &b);
        CHECK(got == want);
        if (got == 1) { CHECK(a < b && b < count && meet(ms[a].out, ms[a].cap, ms[b].out, ms[b].cap)); out_out++; }
        else if (got == 2) { CHECK(a < count && b < count && meet(ms[a].out, ms[a].cap, ms[b].in, ms[b].n)); out_in++; }
        else clean++;
    }
    CHECK(clean > lists / 50 && out_out > lists / 50 && out_in > lists / 50);   // (the generator reaches all three answers)
    std::printf("dev ranges: %d clean, %d out/out, %d out/in; %llu checks\n", clean, out_out, out_in, checks);
    return 0;
}
