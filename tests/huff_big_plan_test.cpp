// huff_big_plan_test.cpp -- the big class of the Huffman compress batch (raisin_amd/csrc/huff_big.hip) as far as it is plain code:
//   * the planner (huff_plan_small.h) at the class's counts -- up to HUFF_BIG_IN_MAX - 1, seven digits -- against the host's Go-exact
//     tree, codes and header (huff_host.cpp), field by field, and what the plan refuses (huff_big_layout.h: big_plan_refuses);
//   * the tiles, a member's scratch, the slot sizes and the tiles' bit offsets against naive loops;
//   * the rule "a byte belongs to the tile its first bit lies in": every tile coded on its own, the way k_huff_big_emit does it, into a
//     slot full of 0xAA and stored by tile_store's units (tile_layout.h) -- the stream must equal the serial one, every byte stored once,
//     nothing behind its end; some tile's first own byte must lie in the unit behind its image's first.
// Built and run by tests/test_huff_big_host.py.  Modes:
//   huff_big_plan_test [n_random]             all of the above; prints "ok <tables> <members>"
//   huff_big_plan_test table b:c [b:c ...]    one table of counts; prints "max_len <l> header <h> refused <0|1>"
// Exits 1 with the first disagreement.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "huff_host.h"
#include "huff_big_layout.h"

using namespace rsn;

namespace {
struct Arr {
    uint32_t v[256];
    Arr() { memset(v, 0, sizeof v); }
    uint32_t get(uint32_t i) const { return v[i]; }
    void set(uint32_t i, uint32_t x) { v[i] = x; }
};
constexpr uint32_t MID_IN_MAX = 65536;                                      // codecs.h: HUFF_MID_IN_MAX, where the class begins

long long g_tables = 0, g_members = 0, g_next_unit = 0;                     // (tiles whose first own byte lies in the unit behind the image's first)

struct Plan { uint32_t a, max_len, total_bits, H; uint32_t tab[128]; uint8_t hdr[2048]; };

// cnt[128]: at least two non-zero counts that sum to less than PLAN_COUNT_LIMIT_WIDE.  The plan, checked against the host's.
bool check(const uint32_t *cnt, const char *what, Plan &p) {
    g_tables++;
    std::vector<HuffSym> syms;
    unsigned long long sum = 0;
    for (uint32_t b = 0; b < 128; b++) if (cnt[b]) { syms.push_back({b, cnt[b]}); sum += cnt[b]; }
    if (sum >= PLAN_COUNT_LIMIT_WIDE) { printf("%s: the test's own table sums to %llu\n", what, sum); return false; }
    std::string hdr, msg;
    emit_header(syms, hdr);
    HuffTree tree; HuffCodes codes;
    std::vector<HuffSym> work = syms;
    if (!build_tree(work, tree, msg) || !assign_codes(tree, codes, msg, false)) { printf("%s: host failed: %s\n", what, msg.c_str()); return false; }
    const uint32_t a = (uint32_t)syms.size();
    uint32_t leaf[128], lf[128];
    for (uint32_t b = 0; b < 128; b++) if (cnt[b]) { const uint32_t r = plan_leaf_rank(cnt, b); leaf[r] = b; lf[r] = cnt[b]; }
    Arr heap, kids, code;
    for (uint32_t i = 0; i < a; i++) heap.set(i, plan_item(lf[i], i));
    const uint32_t root = plan_tree(a, heap, kids);
    plan_codes(a, root, kids, code);
    p.a = a; p.max_len = 0; p.total_bits = 0;
    memset(p.tab, 0, sizeof p.tab);
    for (uint32_t i = 0; i < a; i++) { const uint32_t l = code.get(i) >> 24; p.max_len = l > p.max_len ? l : p.max_len; p.total_bits += lf[i] * l; p.tab[leaf[i]] = code.get(i); }
    p.H = plan_header(cnt, p.total_bits, p.hdr);
    auto fail = [&](const char *part, uint32_t at) { printf("%s: %s differs (a = %u, at %u)\n", what, part, a, at); return false; };
    for (uint32_t i = 0; i < a; i++) if (tree.rune[i] != leaf[i] || tree.freq[i] != lf[i]) return fail("leaf order", i);
    if ((uint32_t)tree.root != root) return fail("root", root);
    for (uint32_t id = a; id <= root; id++) {
        const uint32_t k = kids.get(id - a);
        if ((uint32_t)tree.left[id] != (k & 0xFF) || (uint32_t)tree.right[id] != (k >> 8)) return fail("tree", id);
    }
    for (uint32_t i = 0; i < a; i++) {
        const uint32_t c = code.get(i);
        if ((c >> 24) != codes.len[i] || (c & 0xFFFFFFu) != (uint32_t)(codes.code[i] & 0xFFFFFFu)) return fail("code", i);
    }
    if (p.max_len != codes.max_len) return fail("max length", p.max_len);
    if (p.total_bits != codes.total_bits) return fail("total bits", p.total_bits);
    std::string want = hdr;
    want += "\\\n";
    want.push_back((char)((8 - codes.total_bits % 8) % 8));
    if (p.H != want.size()) return fail("header length", p.H);
    for (uint32_t i = 0; i < p.H; i++) if (p.hdr[i] != (uint8_t)want[i]) return fail("header byte", i);
    uint32_t entries = 0;
    for (uint32_t b = 0; b < 128; b++) if (cnt[b]) entries += plan_entry_len(cnt[b], b);
    if (entries + 3 != p.H) return fail("entry lengths", entries);
    return true;
}
bool refused(const Plan &p, uint32_t n) { return big_plan_refuses(p.max_len, p.H, p.H + (p.total_bits + 7) / 8, huff_big_enc_out_slot(n)); }

bool table_of(const std::vector<uint32_t> &bytes, const std::vector<uint32_t> &counts, const char *what, Plan *out = nullptr) {
    uint32_t cnt[128] = {0};
    for (size_t k = 0; k < bytes.size(); k++) cnt[bytes[k]] = counts[k];
    Plan p;
    const bool ok = check(cnt, what, p);
    if (out) *out = p;
    return ok;
}

// ---- the tiles and the scratch against naive loops
bool layout_of(uint32_t n) {
    uint32_t tiles = 0, covered = 0;
    for (uint32_t at = 0; at < n; at += BIGL_TILE) tiles++;
    if (big_tiles(n) != tiles || tiles > BIGL_TILES_MAX) { printf("n = %u: %u tiles, naive %u\n", n, big_tiles(n), tiles); return false; }
    for (uint32_t t = 0; t < tiles; t++) {
        uint32_t len = 0;
        for (uint32_t at = t * BIGL_TILE; at < n && at < (t + 1) * BIGL_TILE; at++) len++;
        if (big_tile_len(n, t) != len || len == 0) { printf("n = %u: tile %u has %u bytes, naive %u\n", n, t, big_tile_len(n, t), len); return false; }
        covered += len;
    }
    if (covered != n) { printf("n = %u: the tiles cover %u bytes\n", n, covered); return false; }
    const uint32_t slot = huff_big_enc_out_slot(n);
    unsigned long long pay = 0;
    for (uint32_t i = 0; i < n; i++) pay += 7;                               // at most 7 bits a byte
    if (slot % 16 || slot < HUFF_BIG_HDR_MAX + (pay + 7) / 8 || slot >= HUFF_BIG_HDR_MAX + (pay + 7) / 8 + 16) { printf("n = %u: an output slot of %u bytes\n", n, slot); return false; }
    return true;
}
bool scratch_layout() {
    struct Part { uint32_t at, words; } parts[] = {{BIG_SCR_HIST, BIGL_TILES_MAX * 128}, {BIG_SCR_FLAG, BIGL_TILES_MAX}, {BIG_SCR_TAB, 128},
                                                  {BIG_SCR_OFF, BIGL_TILES_MAX + 1}, {BIG_SCR_META, 3}};
    std::vector<int> used(BIG_SCR_WORDS, 0);
    for (const Part &p : parts) for (uint32_t w = p.at; w < p.at + p.words; w++) { if (w >= BIG_SCR_WORDS || used[w]++) { printf("scratch word %u is outside or used twice\n", w); return false; } }
    return true;
}
// the header's bound against a search of its own: the most digits of a counts that sum to at most n, by dynamic programming over the digits
uint32_t naive_hdr_bound(uint32_t n) {
    uint32_t best = 0;
    for (uint32_t a = 2; a <= 128; a++) {
        // cost[d]: the least sum of a counts with d digits in all
        std::vector<unsigned long long> cost(1, 0);
        for (uint32_t s = 0; s < a; s++) {
            std::vector<unsigned long long> next(cost.size() + 7, ~0ull);
            for (size_t d = 0; d < cost.size(); d++) {
                if (cost[d] == ~0ull) continue;
                unsigned long long least = 1;
                for (uint32_t k = 1; k <= 7; k++, least *= 10) next[d + k] = std::min(next[d + k], cost[d] + least);
            }
            cost.swap(next);
        }
        for (size_t d = 0; d < cost.size(); d++) if (cost[d] <= n) best = std::max<uint32_t>(best, (uint32_t)d + 2 * a + 1 + 3);
    }
    return best;
}

// ---- a member coded tile by tile, the way k_huff_big_emit does it
void put_bits(std::vector<uint8_t> &img, uint32_t at, uint32_t ent) {
    const uint32_t l = ent >> 24;
    for (uint32_t k = 0; k < l; k++) if ((ent >> (l - 1 - k)) & 1) img[(at + k) >> 3] |= (uint8_t)(0x80 >> ((at + k) & 7));
}
bool member_of(const std::vector<uint8_t> &in, const char *what) {
    g_members++;
    const uint32_t n = (uint32_t)in.size(), T = big_tiles(n);
    uint32_t cnt[128] = {0};
    std::vector<uint32_t> hist((size_t)T * 128, 0);
    for (uint32_t i = 0; i < n; i++) { cnt[in[i]]++; hist[(size_t)(i / BIGL_TILE) * 128 + in[i]]++; }
    Plan p;
    if (!check(cnt, what, p)) return false;
    if (refused(p, n)) { printf("%s: a member of %u bytes is refused\n", what, n); return false; }
    const uint32_t pad = (8 - p.total_bits % 8) % 8, total = p.H + (p.total_bits + pad) / 8;
    // the serial stream
    std::vector<uint8_t> want(total, 0);
    memcpy(want.data(), p.hdr, p.H);
    uint32_t at = 8 * p.H + pad;
    for (uint32_t i = 0; i < n; i++) { put_bits(want, at, p.tab[in[i]]); at += p.tab[in[i]] >> 24; }
    if (at != 8 * total) { printf("%s: the serial stream ends at bit %u of %u\n", what, at, 8 * total); return false; }
    // the tiles' offsets against a naive walk
    std::vector<uint32_t> tb(T), off(T + 1);
    for (uint32_t t = 0; t < T; t++) tb[t] = big_tile_bits(&hist[(size_t)t * 128], p.tab);
    big_tile_offsets(tb.data(), T, 8 * p.H + pad, off.data());
    at = 8 * p.H + pad;
    for (uint32_t i = 0; i < n; i++) {
        if (i % BIGL_TILE == 0 && off[i / BIGL_TILE] != at) { printf("%s: tile %u starts at bit %u, its offset says %u\n", what, i / BIGL_TILE, at, off[i / BIGL_TILE]); return false; }
        at += p.tab[in[i]] >> 24;
    }
    if (off[T] != 8 * total) { printf("%s: the last offset is %u, the stream has %u bits\n", what, off[T], 8 * total); return false; }
    // every tile on its own into a slot full of 0xAA
    const uint32_t slot = huff_big_enc_out_slot(n);
    std::vector<uint8_t> out(slot + 16, 0xAA);
    std::vector<int> stored(slot + 16, 0);
    memcpy(out.data(), p.hdr, p.H);
    for (uint32_t i = 0; i < p.H; i++) stored[i]++;
    for (uint32_t t = 0; t < T; t++) {
        const uint32_t b0 = off[t], b1 = off[t + 1], u0 = big_tile_origin(b0), i0 = b0 - 8 * u0, i1 = b1 - 8 * u0;
        std::vector<uint8_t> img((i1 + 7 + 24) / 8 + 8, 0);
        uint32_t q = i0;
        for (uint32_t i = t * BIGL_TILE; i < t * BIGL_TILE + big_tile_len(n, t); i++) { put_bits(img, q, p.tab[in[i]]); q += p.tab[in[i]] >> 24; }
        if (q != i1) { printf("%s: tile %u ends at image bit %u, not %u\n", what, t, q, i1); return false; }
        if ((i1 & 7) && t + 1 < T) {
            const uint32_t stop = (i1 + 7) & ~7u;
            for (uint32_t j = 0; j < 7 && q < stop; j++) {
                const uint32_t i = (t + 1) * BIGL_TILE + j;
                if (i >= n) break;
                put_bits(img, q, p.tab[in[i]]); q += p.tab[in[i]] >> 24;
            }
            if (q < stop) { printf("%s: tile %u cannot fill its last byte\n", what, t); return false; }
        }
        const uint32_t lo = big_tile_first_byte(t, b0), hi = big_tile_end_byte(b1);
        if (lo >= u0 + 16) g_next_unit++;
        for (uint32_t u = 0; u0 + 16 * u < hi; u++) {
            const TileStore st = tile_store(u0, lo, hi, u);
            for (uint32_t x = st.lo; x < st.hi; x++) { out[x] = img[x - u0]; stored[x]++; }
        }
    }
    for (uint32_t i = 0; i < total; i++) if (out[i] != want[i] || stored[i] != 1) { printf("%s: byte %u of %u: %02x for %02x, stored %d times\n", what, i, total, out[i], want[i], stored[i]); return false; }
    for (uint32_t i = total; i < slot + 16; i++) if (out[i] != 0xAA || stored[i]) { printf("%s: byte %u behind the stream's %u was written\n", what, i, total); return false; }
    return true;
}
std::vector<uint8_t> draw(std::mt19937_64 &rng, uint32_t n, const std::vector<uint8_t> &alphabet, const std::vector<uint32_t> &weight, bool sorted) {
    std::discrete_distribution<uint32_t> d(weight.begin(), weight.end());
    std::vector<uint8_t> v(n);
    for (auto &x : v) x = alphabet[d(rng)];
    if (sorted) std::sort(v.begin(), v.end());
    return v;
}
}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "table")) {
        uint32_t cnt[128] = {0};
        unsigned long long n = 0;
        for (int k = 2; k < argc; k++) { unsigned b = 0, c = 0; if (sscanf(argv[k], "%u:%u", &b, &c) != 2 || b >= 128) { printf("bad entry %s\n", argv[k]); return 1; } cnt[b] = c; n += c; }
        Plan p;
        if (!check(cnt, "table", p)) return 1;
        printf("max_len %u header %u refused %d\n", p.max_len, p.H, (int)refused(p, (uint32_t)std::min<unsigned long long>(n, BIGL_IN_MAX)));
        return 0;
    }
    const long long n_random = argc > 1 ? atoll(argv[1]) : 20000;
    std::mt19937_64 rng(20261019);
    auto pick_bytes = [&](uint32_t a, bool want_bs_last) {
        std::vector<uint32_t> all(128);
        for (uint32_t b = 0; b < 128; b++) all[b] = b;
        if (want_bs_last) all.resize(0x5C);
        std::shuffle(all.begin(), all.end(), rng);
        all.resize(want_bs_last ? a - 1 : a);
        if (want_bs_last) all.push_back(0x5C);
        return all;
    };
    // ---- tie-heavy tables at the class's counts, every alphabet size
    for (uint32_t a = 2; a <= 128; a++) {
        for (int bs = 0; bs < (a <= 0x5D ? 2 : 1); bs++) {
            const std::vector<uint32_t> bytes = pick_bytes(a, bs);
            std::vector<uint32_t> c(a);
            const uint32_t share = BIGL_IN_MAX / a;                          // equal counts that fill the class, and powers of ten around them
            const uint32_t equal_at[] = {share, share - 1, 65536, 65537, 99999, 100000};
            for (uint32_t v : equal_at) { if ((unsigned long long)v * a >= PLAN_COUNT_LIMIT_WIDE) continue; for (auto &x : c) x = v; if (!table_of(bytes, c, "equal counts")) return 1; }
            for (uint32_t k = 0; k < a; k++) c[k] = 1u << (k % 17);
            if (!table_of(bytes, c, "powers of two")) return 1;
            for (uint32_t k = 0; k < a; k++) c[k] = 1u << (16 - k % 17);
            if (!table_of(bytes, c, "powers of two, descending")) return 1;
            for (uint32_t k = 0; k < a; k++) c[k] = share - (uint32_t)(rng() % 4);
            if (!table_of(bytes, c, "counts near the class's end")) return 1;
            for (uint32_t k = 0; k < a; k++) c[k] = (k % 2) ? 70000 : 65536 + (k % 3);
            if (!table_of(bytes, c, "duplicate counts")) return 1;
        }
    }
    {   // the largest count, seven digits, newline and '\\'
        Plan p;
        if (!table_of({0, 127}, {1, BIGL_IN_MAX - 1}, "the largest count", &p) || refused(p, BIGL_IN_MAX)) return 1;
        if (!table_of({10, 0x5C}, {1000000, 48576}, "seven digits", &p) || refused(p, BIGL_IN_MAX)) return 1;
        if (!table_of({0, 10, 0x5C}, {999999, 9, 48568}, "edge bytes")) return 1;
        if (!table_of({65, 66, 67}, {1048574, 1, 1}, "two rare bytes")) return 1;
    }
    {   // Fibonacci counts: the deepest code of k symbols has k - 1 bits
        for (uint32_t k : {24u, 25u, 26u, 27u}) {
            std::vector<uint32_t> bytes(k), c(k);
            uint32_t f0 = 1, f1 = 1, n = 0;
            for (uint32_t i = 0; i < k; i++) { bytes[i] = 33 + i; c[i] = f0; n += f0; const uint32_t t = f0 + f1; f0 = f1; f1 = t; }
            Plan p;
            if (!table_of(bytes, c, "fibonacci", &p)) return 1;
            if (p.max_len != k - 1 || refused(p, n) != (k - 1 > 24)) { printf("fibonacci, %u symbols, %u bytes: a deepest code of %u bits, refused %d\n", k, n, p.max_len, (int)refused(p, n)); return 1; }
        }
    }
    {   // the header's bound: derived, reached, and exceeded by one
        if (naive_hdr_bound(BIGL_IN_MAX) != HUFF_BIG_HDR_MAX) { printf("the header's bound: %u derived, %u searched\n", HUFF_BIG_HDR_MAX, naive_hdr_bound(BIGL_IN_MAX)); return 1; }
        for (uint32_t n : {1000u, 65537u, 200000u, 999999u}) if (naive_hdr_bound(n) != big_hdr_bound(n)) { printf("the header's bound at %u: %u derived, %u searched\n", n, big_hdr_bound(n), naive_hdr_bound(n)); return 1; }
        // 128 counts of four digits cost 128 000 bytes, every fifth digit 9000 more: `five` counts of 10000 are what the class's largest member buys
        const uint32_t five = (BIGL_IN_MAX - 128 * 1000) / 9000;
        static_assert(BIGL_IN_MAX >= 128 * 1000 && (BIGL_IN_MAX - 128 * 1000) / 9000 < 128, "the longest header is counts of four and five digits");
        std::vector<uint32_t> bytes(128), c(128);
        for (uint32_t b = 0; b < 128; b++) { bytes[b] = b; c[b] = b < five ? 10000 : 1000; }
        Plan p;
        if (!table_of(bytes, c, "the longest header", &p)) return 1;
        if (p.H != HUFF_BIG_HDR_MAX || refused(p, five * 10000 + (128 - five) * 1000)) { printf("the longest header has %u bytes, the bound is %u\n", p.H, HUFF_BIG_HDR_MAX); return 1; }
        c[five] = 10000;                                                     // (more than the class's largest member: what the bound excludes)
        if (!table_of(bytes, c, "a header beyond the bound", &p)) return 1;
        if (p.H != HUFF_BIG_HDR_MAX + 1 || !refused(p, BIGL_IN_MAX)) { printf("a header of %u bytes is not refused\n", p.H); return 1; }
    }
    // ---- random tables that sum to at most the class's largest member
    for (long long t = 0; t < n_random; t++) {
        const uint32_t shape = (uint32_t)(rng() % 5);
        const uint32_t a = shape == 0 ? 2 + (uint32_t)(rng() % 4) : shape == 1 ? 128 : 2 + (uint32_t)(rng() % 127);
        const bool bs = a <= 0x5D && rng() % 8 == 0;
        const std::vector<uint32_t> bytes = pick_bytes(a, bs);
        std::vector<uint32_t> c(a);
        const uint32_t range = shape == 2 ? 4 : shape == 3 ? 1024 : BIGL_IN_MAX / a;
        for (auto &x : c) x = 1 + (uint32_t)(rng() % range);
        if (shape == 4) for (auto &x : c) x = 1u << (rng() % 13);
        if (!table_of(bytes, c, "random")) return 1;
    }
    // ---- the tiles and the slots
    if (!scratch_layout()) return 1;
    std::vector<uint32_t> sizes = {MID_IN_MAX + 1, BIGL_IN_MAX};
    for (uint32_t k = 1; k <= BIGL_TILES_MAX; k++) for (int d = -1; d <= 1; d++) { const long long n = (long long)k * BIGL_TILE + d; if (n > MID_IN_MAX && n <= BIGL_IN_MAX) sizes.push_back((uint32_t)n); }
    for (uint32_t n : sizes) if (!layout_of(n)) return 1;
    // ---- members coded tile by tile
    const std::vector<uint8_t> abc = {'a', 'b', 'c'}, ab = {'a', 'b'};
    std::vector<uint8_t> wide(96);
    std::vector<uint32_t> skew(96);
    for (uint32_t i = 0; i < 96; i++) { wide[i] = (uint8_t)(i == 0 ? 10 : 31 + i); skew[i] = 1 + (i * i * i) % 997 + (i < 4 ? 20000 : 0); }
    for (uint32_t n : {MID_IN_MAX + 1, 2 * BIGL_TILE * 2 + 1, 5 * BIGL_TILE - 1, 5 * BIGL_TILE, 5 * BIGL_TILE + 1, 7 * BIGL_TILE + 12345}) {
        for (int sorted = 0; sorted < 2; sorted++) {
            if (!member_of(draw(rng, n, abc, {2, 1, 1}, sorted), "three letters")) return 1;
            if (!member_of(draw(rng, n, ab, {1, 1}, sorted), "two letters")) return 1;
            if (!member_of(draw(rng, n, wide, skew, sorted), "96 letters")) return 1;
        }
    }
    if (!member_of(draw(rng, BIGL_IN_MAX, wide, skew, false), "the largest member")) return 1;
    if (g_next_unit == 0) { printf("no tile's first own byte lies in the unit behind its image's first\n"); return 1; }
    printf("ok %lld %lld\n", g_tables, g_members);
    return 0;
}
