// The arithmetic of the tiled class of the LZSS decompress batch (csrc/lzss_tile_dec_layout.h) against a serial restatement, as a plain
// program (tests/test_lzss_tile_dec_host.py builds and runs it, also under the address and undefined-behaviour sanitizers):
//   lzss_tile_dec_layout_test              stream lengths around every multiple of the tile from 2049 to LZTD_IN_MAX, escaped lengths around
//                                          every multiple of the tile up to LZTD_OUT_MAX and E = 1: the tiles cover the stream and the
//                                          output exactly once, every output tile finds its stream tiles, the scratch of neighbouring
//                                          members does not overlap and stays inside the stated multiple of the staging, offsets are whole
//                                          16-byte units, and every byte of a result is stored by exactly one tile.  Prints "ok <streams>
//                                          <outputs> <bytes stored>".
//   lzss_tile_dec_layout_test candidate N  prints 1 when a stream of N bytes is a candidate of the class, else 0
//   lzss_tile_dec_layout_test constants    prints the header's constants, "NAME value" a line
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lzss_tile_dec_layout.h"

using namespace rsn;

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd(uint32_t below) {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % below);
}

constexpr uint32_t IMAGE = LZTD_TILE + 64;         // lzss_tile_dec.hip: D_IMG, the bytes of a tile's image in the finish launch
constexpr uint32_t HELD = LZTD_HALO + LZTD_TILE + LZTD_HALO;   // lzss_tile_dec.hip: D_IN_BYTES, the stream a tile's workgroup holds

// ---- a stream of n bytes: its tiles, what a tile's workgroup holds, its slot
static void stream(uint32_t n) {
    CHECK(lztd_candidate(n), "n %u", n);
    uint32_t tiles = 0, sum = 0;
    for (uint32_t p = 0; p < n; p += LZTD_TILE) tiles++;
    CHECK(lztd_tiles(n) == tiles && tiles >= 1 && tiles <= LZTD_IN_TILES_MAX, "n %u", n);
    for (uint32_t t = 0; t < tiles; t++) {
        const uint32_t len = lztd_tile_len(n, t), c0 = t * LZTD_TILE;
        CHECK(len >= 1 && len <= LZTD_TILE && (t + 1 == tiles || len == LZTD_TILE), "tile %u of %u", t, tiles);
        sum += len;
        // a token whose '<' is the tile's last byte, and one whose '<' lies LZTD_REACH bytes in front of the tile, are held whole
        CHECK(c0 + len - 1 + LZTD_REACH < c0 + LZTD_TILE + LZTD_HALO && LZTD_REACH <= LZTD_HALO, "tile %u: a token's text", t);
        CHECK((uint64_t)LZTD_HALO + LZTD_TILE + LZTD_HALO == HELD && HELD % 16 == 0 && c0 % 16 == 0, "tile %u: whole units", t);
    }
    CHECK(sum == n, "the tiles of %u cover %u", n, sum);
    const uint64_t in = lztd_in_slot(n);
    CHECK(in % 16 == 0 && in >= (uint64_t)n + 32 && ((n + 15) & ~15u) <= in, "n %u: the input slot", n);
    // the scratch against the staging: the multiple that sizes the slot
    CHECK(4ull * LZTD_SCR_WORDS <= (uint64_t)LZTD_SCR_PER_STAGING * (in + lztd_out_slot()), "n %u: scratch against staging", n);
}

// ---- an output of e escaped bytes: its tiles, and a result whose tiles unescape to random lengths stored byte by byte
static size_t output(uint32_t e) {
    CHECK(e >= 1 && e <= LZTD_OUT_MAX, "e %u", e);
    uint32_t tiles = 0, sum = 0;
    for (uint32_t p = 0; p < e; p += LZTD_TILE) tiles++;
    CHECK(lztd_tiles(e) == tiles && tiles <= LZTD_OUT_TILES_MAX, "e %u", e);
    std::vector<uint32_t> off(tiles + 1, 0);
    for (uint32_t t = 0; t < tiles; t++) {
        const uint32_t len = lztd_tile_len(e, t);
        CHECK(len >= 1 && len <= LZTD_TILE && (t + 1 == tiles || len == LZTD_TILE), "tile %u of %u", t, tiles);
        sum += len;
        // unescaping a tile gives between half of its bytes (rounded down: a 5C pair split by the cut gives none here) and all of them
        const uint32_t kind = rnd(4), out = kind == 0 ? len : kind == 1 ? len / 2 : len / 2 + rnd(len - len / 2 + 1);
        off[t + 1] = off[t] + out;
    }
    CHECK(sum == e, "the tiles of %u cover %u", e, sum);
    const uint32_t total = off[tiles], slot = (uint32_t)lztd_out_slot();
    CHECK(total <= e && slot >= LZTD_OUT_MAX + 16 && slot % 16 == 0, "e %u: the output slot", e);
    std::vector<uint8_t> hit(slot, 0);
    for (uint32_t t = 0; t < tiles; t++) {
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
    for (uint32_t x = 0; x < slot; x++) CHECK(hit[x] == (x < total ? 1 : 0), "e %u: byte %u of %u stored %u times", e, x, total, hit[x]);
    return total;
}

// ---- the output tiles of a stream whose tiles put out cnt[t] bytes: the entry the plan launch gives an output tile against a serial scan,
// and the walk of the resolve launch from it -- every byte of the output tile comes from exactly one stream tile
static void entries(const std::vector<uint32_t> &cnt) {
    const uint32_t T = (uint32_t)cnt.size();
    std::vector<uint32_t> first(T + 1, 0);
    for (uint32_t t = 0; t < T; t++) first[t + 1] = first[t] + cnt[t];
    const uint32_t e = first[T];
    if (e == 0 || e > LZTD_OUT_MAX) return;                                       // (handed back: no output tile)
    for (uint32_t o = 0; o < lztd_tiles(e); o++) {
        const uint32_t s0 = o * LZTD_TILE, s1 = s0 + lztd_tile_len(e, o);
        uint32_t serial = 0;
        while (!(first[serial] <= s0 && s0 < first[serial + 1])) serial++;       // the stream tile that puts out byte s0
        const uint32_t got = lztd_entry_tile(first.data(), T, s0);
        CHECK(got == serial && got < T, "output tile %u: entry %u, serial %u", o, got, serial);
        uint32_t covered = 0, at = s0, steps = 0;
        for (uint32_t t = got; t < T && first[t] < s1; t++, steps++) {
            const uint32_t lo = first[t] > s0 ? first[t] : s0, hi = first[t + 1] < s1 ? first[t + 1] : s1;
            if (lo < hi) { CHECK(lo == at, "output tile %u: stream tile %u begins at %u, expected %u", o, t, lo, at); covered += hi - lo; at = hi; }
        }
        CHECK(covered == s1 - s0 && steps <= T, "output tile %u: %u of %u bytes", o, covered, s1 - s0);
    }
}

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "constants")) {
        std::printf("LZTD_IN_MIN %u\nLZTD_IN_MAX %u\nLZTD_OUT_MAX %u\nLZTD_TILE %u\nLZTD_TOKEN_TEXT %u\nLZTD_REACH %u\nLZTD_HALO %u\n", LZTD_IN_MIN, LZTD_IN_MAX, LZTD_OUT_MAX, LZTD_TILE,
                    LZTD_TOKEN_TEXT, LZTD_REACH, LZTD_HALO);
        std::printf("LZTD_IN_TILES_MAX %u\nLZTD_OUT_TILES_MAX %u\nLZTD_SCR_WORDS %u\nLZTD_SCR_PER_STAGING %u\nLZT_E_CAP_MAX %u\nLZT_E_MAX %u\n", LZTD_IN_TILES_MAX, LZTD_OUT_TILES_MAX,
                    LZTD_SCR_WORDS, LZTD_SCR_PER_STAGING, lzt_e_cap(LZT_IN_MAX), LZT_E_MAX);
        return 0;
    }
    if (argc == 3 && !std::strcmp(argv[1], "candidate")) {
        std::printf("%d\n", lztd_candidate((size_t)std::strtoull(argv[2], nullptr, 10)) ? 1 : 0);
        return 0;
    }
    // ---- a member's scratch: the regions in order, disjoint, whole 16-byte units; neighbours do not overlap
    const uint64_t reg[][2] = {
        {4ull * LZTD_SCR_META, 32}, {4ull * LZTD_SCR_CNT, 4ull * LZTD_IN_TILES_MAX}, {4ull * LZTD_SCR_FLAG, 4ull * LZTD_IN_TILES_MAX}, {4ull * LZTD_SCR_NEED, 4ull * LZTD_IN_TILES_MAX},
        {4ull * LZTD_SCR_FIRST, 4ull * (LZTD_IN_TILES_MAX + 1)}, {4ull * LZTD_SCR_OT_TILE, 4ull * LZTD_OUT_TILES_MAX}, {4ull * LZTD_SCR_OT_OFF, 4ull * LZTD_OUT_TILES_MAX},
        {4ull * LZTD_SCR_IMG, (uint64_t)LZTD_OUT_MAX + LZTD_IMG_PAD}, {4ull * LZTD_SCR_DESC, 4ull * LZTD_OUT_MAX}};
    uint64_t at = 0;
    for (const auto &r : reg) { CHECK(r[0] >= at && r[0] % 16 == 0, "a region at %llu, the one before ends at %llu", (unsigned long long)r[0], (unsigned long long)at); at = r[0] + r[1]; }
    CHECK(at <= 4ull * LZTD_SCR_WORDS && (4ull * LZTD_SCR_WORDS) % 16 == 0 && LZTD_META_E < 8, "the member's words");
    for (uint32_t q = 0; q < 4096; q++) CHECK(lztd_scr_at(q) + LZTD_SCR_WORDS == lztd_scr_at(q + 1) && (4 * lztd_scr_at(q)) % 16 == 0, "member %u", q);
    CHECK(lztd_tiles(LZTD_IN_MAX) == LZTD_IN_TILES_MAX && lztd_tiles(LZTD_OUT_MAX) == LZTD_OUT_TILES_MAX, "the largest member's tiles");
    CHECK((uint64_t)LZTD_IN_TILES_MAX * (LZTD_OUT_MAX + 1ull) < (1ull << 32), "the scan of the clamped outputs");
    CHECK(!lztd_candidate(0) && !lztd_candidate(LZTD_IN_MIN) && lztd_candidate(LZTD_IN_MIN + 1) && lztd_candidate(LZTD_IN_MAX) && !lztd_candidate(LZTD_IN_MAX + 1), "candidates");
    // ---- every stream the tiled encoder writes: at most lzt_e_cap(n) bytes that expand to at most LZT_E_MAX
    for (uint32_t n = LZT_IN_MIN + 1; n <= LZT_IN_MAX; n += 997) CHECK(lzt_e_cap(n) <= LZTD_IN_MAX && lzt_e_cap(n) <= LZTD_OUT_MAX, "n %u", n);
    CHECK(lzt_e_cap(LZT_IN_MAX) <= LZTD_IN_MAX && LZT_E_MAX <= LZTD_OUT_MAX, "the encoder's caps");
    size_t streams = 0, outputs = 0, stored = 0;
    for (uint32_t edge = LZTD_TILE; edge <= LZTD_IN_MAX + LZTD_TILE; edge += LZTD_TILE)
        for (int d = -1; d <= 1; d++) {
            const uint64_t n = (uint64_t)edge + d;
            if (n > LZTD_IN_MIN && n <= LZTD_IN_MAX) { stream((uint32_t)n); streams++; }
        }
    stream(LZTD_IN_MAX); streams++;
    stored += output(1); outputs++;
    for (uint32_t edge = LZTD_TILE; edge <= LZTD_OUT_MAX + LZTD_TILE; edge += LZTD_TILE)
        for (int d = -1; d <= 1; d++) {
            const uint64_t e = (uint64_t)edge + d;
            if (e >= 1 && e <= LZTD_OUT_MAX) { stored += output((uint32_t)e); outputs++; }
        }
    stored += output(LZTD_OUT_MAX); outputs++;
    // ---- entries: tiles that put out nothing, tiles that put out many output tiles, ordinary ones
    for (int round = 0; round < 400; round++) {
        const uint32_t T = 1 + rnd(LZTD_IN_TILES_MAX);
        std::vector<uint32_t> cnt(T);
        const uint32_t kind = rnd(4);
        for (uint32_t t = 0; t < T; t++) {
            const uint32_t k = rnd(8);
            cnt[t] = kind == 0 ? LZTD_TILE : k < 3 ? 0u : k == 3 ? rnd(40 * LZTD_TILE / T + 2) : k == 4 ? 1u : rnd(2 * LZTD_TILE + 1);
        }
        entries(cnt);
    }
    entries(std::vector<uint32_t>{0, 0, 0, 1});
    entries(std::vector<uint32_t>{LZTD_OUT_MAX});
    entries(std::vector<uint32_t>{1, 0, LZTD_TILE - 1, 0, 0, LZTD_TILE, 1});
    std::printf("ok %zu %zu %zu\n", streams, outputs, stored);
    return 0;
}
