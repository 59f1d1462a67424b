// The arithmetic of the batch round trip (raisin_amd/csrc/roundtrip_batch_layout.h) as plain host code, held against a brute-force
// statement of what it promises: the tiles of a member cover the longer of its two buffers exactly once in pieces of 64 KiB, the verify
// table and the stats block are disjoint regions at 16-byte offsets, an empty member has no tile but has a row, the 32-bit check fires at
// 2^32 and not below, and a member's run need grows with both lengths.  Prints the number of checks it made.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "roundtrip_batch_layout.h"

using namespace rsn;

static unsigned long long checks = 0;
#define CHECK(cond)                                                                                  \
    do {                                                                                             \
        checks++;                                                                                    \
        if (!(cond)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

static bool meet(size_t a, size_t na, size_t b, size_t nb) { return na && nb && a < b + nb && b < a + na; }

// the tiles of (n_o, n_d), piece by piece: consecutive, at most RB_TILE each, none empty, together max(n_o, n_d)
static void test_tiles(size_t n_o, size_t n_d) {
    const size_t top = n_o > n_d ? n_o : n_d, tiles = rb_tiles(n_o, n_d);
    CHECK(rb_tiles(n_d, n_o) == tiles);
    size_t at = 0;
    for (size_t t = 0; t < tiles; t++) {
        const size_t lo = rb_tile_lo(t), hi = rb_tile_hi(n_o, n_d, t);
        CHECK(lo == at && lo % 16 == 0 && hi > lo && hi - lo <= RB_TILE && hi <= top);
        if (t + 1 < tiles) CHECK(hi - lo == RB_TILE);
        at = hi;
    }
    CHECK(at == top);
    CHECK((tiles == 0) == (top == 0));
    if (top) CHECK(rb_tile_lo(tiles) >= top);                              // (no tile behind the last)
}

static void test_layout(size_t tiles, size_t m, bool hists) {
    const RbLayout l = rb_layout(tiles, m, hists);
    const size_t table = tiles * sizeof(RbEntry), words = m * RB_WORD, counts = hists ? m * RB_HIST_BYTES : 0;
    CHECK(l.table % 16 == 0 && l.words % 16 == 0 && l.hists % 16 == 0);
    CHECK(l.table + table <= l.words && l.words + words <= l.hists && l.hists + counts == l.bytes);
    CHECK(!meet(l.table, table, l.words, words) && !meet(l.table, table, l.hists, counts) && !meet(l.words, words, l.hists, counts));
    CHECK(l.words - (l.table + table) < 16 && l.hists - (l.words + words) < 16);   // (no more than the padding between them)
    CHECK(rb_stats_bytes(l) == l.bytes - l.words && rb_stats_bytes(l) >= words + counts);
    if (!hists) CHECK(l.hists == l.bytes);
    // every member has a row, whatever its tiles: member i's word and counters lie inside the stats block
    for (size_t i : {(size_t)0, m / 2, m ? m - 1 : 0}) {
        if (i >= m) continue;
        CHECK(l.words + (i + 1) * RB_WORD <= l.hists);
        if (hists) CHECK(l.hists + (i + 1) * RB_HIST_BYTES <= l.bytes);
    }
}

static void test_need(size_t staged, size_t enc_slot, size_t dec_slot, size_t n_o, size_t n_d, bool hists) {
    const size_t need = rb_member_need(staged, enc_slot, dec_slot, n_o, n_d, hists);
    const size_t slot = enc_slot > dec_slot ? enc_slot : dec_slot;
    CHECK(need == lb_round16(staged) + 2 * lb_slot_bytes(slot) + rb_tiles(n_o, n_d) * sizeof(RbEntry) + RB_WORD + (hists ? RB_HIST_BYTES : 0));
    // monotone in both lengths, and in everything else
    for (size_t more : {(size_t)1, (size_t)15, (size_t)16, RB_TILE, 3 * RB_TILE + 1}) {
        CHECK(rb_member_need(staged, enc_slot, dec_slot, n_o + more, n_d, hists) >= need);
        CHECK(rb_member_need(staged, enc_slot, dec_slot, n_o, n_d + more, hists) >= need);
        CHECK(rb_member_need(staged + more, enc_slot, dec_slot, n_o, n_d, hists) >= need);
        CHECK(rb_member_need(staged, enc_slot + more, dec_slot, n_o, n_d, hists) >= need);
        CHECK(rb_member_need(staged, enc_slot, dec_slot + more, n_o, n_d, hists) >= need);
    }
    CHECK(rb_member_need(staged, enc_slot, dec_slot, n_o, n_d, true) == rb_member_need(staged, enc_slot, dec_slot, n_o, n_d, false) + RB_HIST_BYTES);
}

int main(int argc, char **argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 4000;
    static_assert(sizeof(RbEntry) == 32 && RB_WORD == 8 && RB_HIST_BYTES == 2048 && RB_TILE == 65536, "the figures the documents state");
    // named cases: an empty member has no tile but has a row
    CHECK(rb_tiles(0, 0) == 0);
    { const RbLayout l = rb_layout(0, 1, true); CHECK(l.words == 0 && l.hists == 16 && l.bytes == 16 + RB_HIST_BYTES && rb_stats_bytes(l) == 16 + RB_HIST_BYTES); }
    { const RbLayout l = rb_layout(0, 3, false); CHECK(l.words == 0 && l.hists == 32 && l.bytes == 32); }
    CHECK(rb_tiles(1, 0) == 1 && rb_tiles(0, 1) == 1 && rb_tiles(RB_TILE, 4) == 1 && rb_tiles(4, RB_TILE + 1) == 2 && rb_tiles(200000, 200000) == 4);
    CHECK(rb_tile_hi(65537, 65539, 1) == 65539 && rb_tile_hi(65537, 65539, 0) == 65536);
    // the counters' limit: 2^32 - 1 bytes fit, 2^32 do not
    CHECK(rb_fits(0) && rb_fits((uint64_t)UINT32_MAX) && !rb_fits((uint64_t)UINT32_MAX + 1) && !rb_fits((uint64_t)1 << 32) && !rb_fits(~(uint64_t)0));
    CHECK(rb_tiles((size_t)UINT32_MAX, 0) == 65536);                       // (a tile index and a tile's first byte fit 32 bits)
    CHECK(rb_tile_lo(rb_tiles((size_t)UINT32_MAX, 0) - 1) < (size_t)UINT32_MAX);
    for (size_t a : {(size_t)0, (size_t)1, (size_t)15, (size_t)16, (size_t)17, RB_TILE - 1, RB_TILE, RB_TILE + 1, 4 * RB_TILE, 4 * RB_TILE + 4097})
        for (size_t b : {(size_t)0, (size_t)1, (size_t)16, RB_TILE - 1, RB_TILE, RB_TILE + 1, 5 * RB_TILE + 3}) test_tiles(a, b);
    for (size_t tiles : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)4097})
        for (size_t m : {(size_t)0, (size_t)1, (size_t)2, (size_t)3, (size_t)4096, (size_t)4097}) { test_layout(tiles, m, false); test_layout(tiles, m, true); }
    test_need(0, 0, 0, 0, 0, false); test_need(25, 66000, 70000, 25, 25, true);
    std::mt19937_64 rng(0x7B1D5);
    for (int it = 0; it < rounds; it++) {
        const size_t scale = it % 3 == 0 ? 40 : it % 3 == 1 ? 70000 : 9 * RB_TILE;
        const size_t a = rng() % 5 == 0 ? 0 : rng() % scale, b = rng() % 7 == 0 ? a : rng() % scale;
        test_tiles(a, b);
        test_layout(rng() % 5000, rng() % 5000, it % 2 == 0);
        test_need(it % 2 ? a : 0, rng() % (4 * scale), rng() % (4 * scale), a, b, it % 4 < 2);
    }
    std::printf("roundtrip batch layout: %llu checks\n", checks);
    return 0;
}
