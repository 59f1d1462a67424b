// The item of a key (csrc/lzss_enc_body.h: lzss_item, lzss.go:143) against the text the reference formats: for every length L of 0 to
// 4096 + 64 and every distance d of 0 to 65535, el is the length of "<d,L>" as snprintf writes it (0 for a literal, L = 0) and sz is what
// the item puts out: one byte for a literal, else the shorter of the token and the L bytes it stands for.  273 million pairs: the lengths
// are dealt to eight threads.  Prints "ok" and the pairs.
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "lzss_enc_body.h"

using namespace rsn;

static_assert(lzss_item(0, 0).sz == 1 && lzss_item(0, 0).el == 0, "a literal");
static_assert(lzss_item(5, 5).el == 5 && lzss_item(5, 5).sz == 5 && lzss_item(6, 6).sz == 5, "\"<6,6>\" is the first token shorter than its match");
static_assert(lzss_item(4096, 4096).el == 11 && lzss_item(4096, 65535).el == 12, "the longest tokens");

int main() {
    const unsigned L_MAX = 4096 + 64, D_MAX = 65535, THREADS = 8;
    std::atomic<unsigned long long> pairs{0};
    std::atomic<int> wrong{0};
    std::vector<std::thread> pool;
    for (unsigned t = 0; t < THREADS; t++) pool.emplace_back([&, t] {
        char text[32];
        unsigned long long mine = 0;
        for (unsigned L = t; L <= L_MAX && !wrong; L += THREADS) {
            for (unsigned d = 0; d <= D_MAX; d++, mine++) {
                const int len = snprintf(text, sizeof text, "<%u,%u>", d, L);
                const LzssItem it = lzss_item(L, d);
                const unsigned el = L ? (unsigned)len : 0u, sz = L == 0 ? 1u : std::min(el, L);
                if (it.L == L && it.d == d && it.el == el && it.sz == sz) continue;
                if (!wrong.exchange(1)) printf("L = %u, d = %u: el %u (\"%s\": %u), sz %u (%u)\n", L, d, it.el, text, el, it.sz, sz);
                return;
            }
        }
        pairs += mine;
    });
    for (std::thread &th : pool) th.join();
    if (wrong) return 1;
    printf("ok %llu\n", pairs.load());
    return 0;
}
