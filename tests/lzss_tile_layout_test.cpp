// The arithmetic of the tiled class of the LZSS compress batch (csrc/lzss_tile_layout.h) against a serial restatement, as a plain program
// (tests/test_lzss_tile_host.py builds and runs it, also under the address and undefined-behaviour sanitizers):
//   lzss_tile_layout_test            tile_store (csrc/tile_layout.h) itself over every alignment of origin, first and last byte; then the
//                                    member lengths at the tile edges: tiles, scratch, slots, the window's first position, and a stream
//                                    stored tile by tile -- prints "ok <members> <bytes stored>"
//   lzss_tile_layout_test takes N W  prints 1 when the class takes a member of N bytes at window W, else 0
//   lzss_tile_layout_test constants  prints the header's constants, "NAME value" a line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lzss_tile_layout.h"

using namespace rsn;

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % below);
}

constexpr uint32_t IMAGE = LZT_TILE + 64;          // lzss_tile.hip: T_IMG, the bytes of a tile's image
constexpr uint32_t ITEM_MAX = 11;                  // a token of two four-digit numbers, or as many bytes

// a stream of `total` bytes whose tiles begin at off[t]: every byte stored once, by lzt_tile_store's units -> bytes stored
static size_t store_once(const std::vector<uint32_t> &off, uint32_t n) {
    const uint32_t T = (uint32_t)off.size() - 1, total = off[T], slot = lzt_out_slot(n);
    std::vector<uint8_t> hit(slot, 0);
    for (uint32_t t = 0; t < T; t++) {
        const uint32_t off0 = off[t], off1 = off[t + 1], u0 = lzt_image_first(off0);
        CHECK(u0 % 16 == 0 && u0 <= off0 && off0 - u0 < 16, "tile %u", t);
        for (uint32_t u = 0; u0 + 16 * u < off1; u++) {
            const LztStore s = lzt_tile_store(off0, off1, u);
            CHECK(s.lo <= s.hi && s.hi <= off1 && (s.lo >= off0 || s.lo == s.hi), "tile %u unit %u", t, u);
            CHECK(s.hi - u0 <= IMAGE, "tile %u unit %u: beyond the image", t, u);
            if (s.whole) CHECK(s.lo % 16 == 0 && s.hi == s.lo + 16 && s.lo == u0 + 16 * u, "tile %u unit %u: a whole unit", t, u);
            for (uint32_t x = s.lo; x < s.hi; x++) { CHECK(x < slot, "byte %u beyond the slot", x); hit[x]++; }
        }
    }
    for (uint32_t x = 0; x < slot; x++) CHECK(hit[x] == (x < total ? 1 : 0), "n %u: byte %u of %u stored %u times", n, x, total, hit[x]);
    return total;
}

// ---- tile_store itself.  One tile: the units a workgroup walks (tile_dev.h: tile_store_out's loop, origin + 16 u < hi) store exactly
// [lo, hi), every byte once; a unit inside the range goes out whole, and only the range's first and last unit go byte by byte.
static uint32_t one_tile(uint32_t origin, uint32_t lo, uint32_t hi, std::vector<uint8_t> &hit) {
    uint32_t partial = 0, u = 0;
    for (; origin + 16 * u < hi; u++) {
        const TileStore s = tile_store(origin, lo, hi, u);
        const uint32_t x0 = origin + 16 * u, x1 = x0 + 16;
        CHECK(s.lo <= s.hi, "origin %u [%u, %u) unit %u", origin, lo, hi, u);
        if (s.lo < s.hi) CHECK(s.lo >= lo && s.hi <= hi && s.lo >= x0 && s.hi <= x1, "origin %u [%u, %u) unit %u: [%u, %u)", origin, lo, hi, u, s.lo, s.hi);
        CHECK(s.whole == (x0 >= lo && x1 <= hi), "origin %u [%u, %u) unit %u: whole", origin, lo, hi, u);
        if (s.whole) CHECK(s.lo == x0 && s.hi == x1 && x0 % 16 == 0, "origin %u [%u, %u) unit %u: a whole unit", origin, lo, hi, u);
        else if (s.lo < s.hi) partial++;
        for (uint32_t x = s.lo; x < s.hi; x++) hit[x]++;
    }
    CHECK(partial <= 2, "origin %u [%u, %u): %u units byte by byte", origin, lo, hi, partial);
    for (uint32_t k = 0; k < 3; k++) {                                           // (the units behind the walk hold nothing of the range)
        const TileStore s = tile_store(origin, lo, hi, u + k);
        CHECK(s.lo == s.hi && !s.whole, "origin %u [%u, %u) unit %u behind the range", origin, lo, hi, u + k);
    }
    return hi - lo;
}
static size_t store_sweep() {
    size_t ranges = 0;
    std::vector<uint8_t> hit(256, 0);
    // origins of several units; lo from the origin to two units behind it -- lo in the NEXT unit is huff_big.hip's tile whose first bit
    // lies in a unit's last byte: unit 0 stores nothing -- and hi from lo (an empty range) over every alignment to three units on
    for (uint32_t origin = 0; origin <= 48; origin += 16)
        for (uint32_t lo = origin; lo <= origin + 32; lo++)
            for (uint32_t hi = lo; hi <= lo + 56; hi++) {
                std::fill(hit.begin(), hit.end(), 0);
                one_tile(origin, lo, hi, hit);
                for (uint32_t x = 0; x < hit.size(); x++) CHECK(hit[x] == (x >= lo && x < hi ? 1 : 0), "origin %u [%u, %u): byte %u stored %u times", origin, lo, hi, x, hit[x]);
                if (lo >= origin + 16) { const TileStore s = tile_store(origin, lo, hi, 0); CHECK(s.lo == s.hi && !s.whole, "origin %u [%u, %u): unit 0 stores nothing", origin, lo, hi); }
                ranges++;
            }
    // three tiles side by side, the cuts b and c at every alignment two units to either side (b == c: the middle tile is empty); a tile's
    // image begins at the unit of its first byte (back == 0: the LZSS classes) or of the byte in front of it (back == 1: huff_big.hip's
    // tile whose first bit lies inside the byte before its first own byte).  No byte twice, none left out, none outside.
    const uint32_t a = 5, d = 160;
    for (uint32_t b = 32 - 2; b <= 96 + 2; b++)
        for (uint32_t c = b; c <= 128 + 2; c++)
            for (uint32_t back = 0; back < 2; back++) {
                std::fill(hit.begin(), hit.end(), 0);
                const uint32_t cut[4] = {a, b, c, d};
                for (uint32_t t = 0; t < 3; t++) one_tile(tile_origin(cut[t] - (t ? back : 0)), cut[t], cut[t + 1], hit);
                for (uint32_t x = 0; x < hit.size(); x++) CHECK(hit[x] == (x >= a && x < d ? 1 : 0), "cuts %u %u back %u: byte %u stored %u times", b, c, back, x, hit[x]);
                ranges++;
            }
    CHECK(tile_origin(0) == 0 && tile_origin(15) == 0 && tile_origin(16) == 16 && tile_origin(0xFFFFFFFFu) == 0xFFFFFFF0u, "the unit an offset lies in");
    CHECK(tile_count(1, 16) == 1 && tile_count(16, 16) == 1 && tile_count(17, 16) == 2 && tile_len(17, 16, 0) == 16 && tile_len(17, 16, 1) == 1 && tile_len(32, 16, 1) == 16, "tiles of any size");
    return ranges;
}

static size_t member(uint32_t n, uint32_t e) {
    const uint32_t cap = lzt_e_cap(n);
    CHECK(e >= 1 && e <= cap && cap <= LZT_E_MAX && cap <= n + n / 2 && cap >= n, "n %u e %u cap %u", n, e, cap);
    // ---- tiles: a serial count
    uint32_t tiles = 0, sum = 0;
    for (uint32_t p = 0; p < e; p += LZT_TILE) tiles++;
    CHECK(lzt_tiles(e) == tiles && tiles <= LZT_TILES_MAX, "n %u e %u", n, e);
    for (uint32_t t = 0; t < tiles; t++) {
        const uint32_t len = lzt_tile_len(e, t);
        CHECK(len >= 1 && len <= LZT_TILE && (t + 1 == tiles || len == LZT_TILE), "tile %u of %u", t, tiles);
        sum += len;
    }
    CHECK(sum == e, "the tiles of %u cover %u", e, sum);
    // ---- scratch: the regions in order, disjoint, inside the member's words, whole 16-byte units, below 8 bytes a byte of input
    const uint64_t meta0 = 4ull * LZT_SCR_META, meta1 = meta0 + 32, off0 = 4ull * LZT_SCR_OFF, off1 = off0 + 4ull * (lzt_tiles(cap) + 1);
    const uint64_t key0 = 4ull * lzt_scr_keys(n), key1 = key0 + 4ull * cap, fc0 = 4ull * lzt_scr_fc(n), fc1 = fc0 + cap + LZT_FC_PAD, end = 4ull * lzt_scr_words(n);
    CHECK(meta1 <= off0 && off1 <= key0 && key1 <= fc0 && fc1 <= end, "n %u: the regions overlap", n);
    CHECK(LZT_META_GIVEUP < 8 && key0 % 16 == 0 && fc0 % 16 == 0 && end % 16 == 0, "n %u: alignment", n);
    CHECK(end <= 8ull * n, "n %u: %llu bytes of scratch", n, (unsigned long long)end);
    // ---- slots: the stream fits, whole units, and four times the two slots hold the scratch (lzss_tile.hip sizes the slot by it)
    const uint64_t in = lzt_in_slot(n), out = lzt_out_slot(n);
    CHECK(in % 16 == 0 && in >= n + 32 && out % 16 == 0 && out >= cap + 16 - 15 && out >= e, "n %u: slots", n);
    CHECK(end <= 4 * (in + out), "n %u: scratch against staging", n);
    // ---- the window's first position for every tile and the windows at the edges
    const uint32_t windows[] = {1, 2, 255, 1023, 1024, 1025, 4095, 4096};
    for (uint32_t t = 0; t < tiles; t++)
        for (uint32_t w : windows) {
            const uint32_t t0 = t * LZT_TILE, lo = lzt_window_lo(t0, w, 1024);
            uint32_t want = t0 > w ? t0 - w : 0;
            while (want % 1024) want--;
            CHECK(lo == want && lo <= t0 && t0 - lo <= LZT_W_MAX && lo % 4 == 0, "tile %u window %u", t, w);
        }
    // ---- a stream stored tile by tile: tile totals of every kind -- none (a match steps over the tile), a few bytes, the longest
    std::vector<uint32_t> off(tiles + 1, 0);
    for (uint32_t t = 0; t < tiles; t++) {                                       // (a stream is never longer than the e bytes it stands for)
        const uint32_t len = lzt_tile_len(e, t), room = e - off[t], most = len - 1 + ITEM_MAX < room ? len - 1 + ITEM_MAX : room;
        const uint32_t kind = rnd(8), total = kind == 0 ? 0 : kind == 1 ? most : kind == 2 ? rnd(17) % (most + 1) : rnd(most + 1);
        off[t + 1] = off[t] + total;
    }
    return store_once(off, n);
}

int main(int argc, char **argv) {
    if (argc > 1 && !std::strcmp(argv[1], "constants")) {
        std::printf("LZT_IN_MIN %u\nLZT_IN_MAX %u\nLZT_E_MAX %u\nLZT_TILE %u\nLZT_W_MAX %u\nLZT_TILES_MAX %u\n", LZT_IN_MIN, LZT_IN_MAX, LZT_E_MAX, LZT_TILE, LZT_W_MAX, LZT_TILES_MAX);
        return 0;
    }
    if (argc > 3 && !std::strcmp(argv[1], "takes")) {
        std::printf("%d\n", lzt_takes((size_t)std::strtoull(argv[2], nullptr, 10), std::strtoll(argv[3], nullptr, 10)) ? 1 : 0);
        return 0;
    }
    size_t members = 0, bytes = 0;
    CHECK(store_sweep() > 10000, "the sweep of tile_store");
    std::vector<uint32_t> lens = {LZT_IN_MIN + 1, LZT_IN_MAX - 1, LZT_IN_MAX};
    for (uint32_t k = LZT_IN_MIN / LZT_TILE; k * LZT_TILE <= LZT_IN_MAX; k++)
        for (int d = -1; d <= 1; d++) lens.push_back(k * LZT_TILE + d);
    for (uint32_t n : lens) {
        if (n <= LZT_IN_MIN || n > LZT_IN_MAX) continue;
        const uint32_t cap = lzt_e_cap(n);
        uint32_t es[] = {n, cap, cap - 1, n + 1, n / LZT_TILE * LZT_TILE + LZT_TILE - 1, n / LZT_TILE * LZT_TILE + LZT_TILE, n / LZT_TILE * LZT_TILE + LZT_TILE + 1};
        for (uint32_t e : es) {
            if (e < n || e > cap) continue;
            bytes += member(n, e);
            members++;
        }
    }
    CHECK(lzt_e_cap(LZT_IN_MAX) == LZT_E_MAX && lzt_e_cap(LZT_IN_MAX + 1) == LZT_E_MAX && lzt_e_cap(0xFFFFFFFFu) == LZT_E_MAX, "the cap of the largest member");
    CHECK(lzt_front_words(1) == 4 && lzt_front_words(4) == 4 && lzt_front_words(5) == 8 && lzt_front_words(4096) == 4096, "the table in front");
    std::printf("ok %zu %zu\n", members, bytes);
    return 0;
}
