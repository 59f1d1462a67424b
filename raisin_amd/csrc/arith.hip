// arith.hip -- the adaptive arithmetic codec (go-compression/raisin compressor/arithmetic): one wave64 per member, several
// members to a workgroup.  A single stream is one wave's serial work; a batch of members is where the device is used.
//
// The model: cf[0..257], cf[i] = i at the start; coding symbol s adds 1 to every cf[i] with i > s until cf[257] reaches 16383, then
// the table is frozen for good.  cf[0] never moves and cf[257] = 257 + the number of updates, so the wave keeps cf[1..256] in
// registers -- lane l holds cf[4l+1 .. 4l+4], the UPPER bounds of symbols 4l .. 4l+3 -- and cf[257] as a wave-uniform scalar.
//   update         a compare-and-add per lane and register
//   encoder lookup two lane reads at a wave-uniform index
//   decoder search one ballot over "sv < cf[4l+4]", then three compares in the lane found
// The coder state (low, high, value, pending), the division and the bit accumulators are wave-uniform: they live in scalar registers
// wherever the compiler proves it (the state is made uniform with readfirstlane when it is loaded).
//
// Both kernels work in SLICES: a launch codes at most `budget` (<= ARITH_SLICE_SYMBOLS) symbols per member, saves the table, the coder
// state and both cursors in the member's ArithState, and the next launch resumes from it -- no launch's length depends on a member's.
//
// The encoder writes the coder's bits as big-endian words to a raw area; the stream's front pad (8 - nbits % 8 bits, known only at the
// end) is put in front by k_arith_pack, which shifts the raw bits into place in parallel and compacts the members' results.
#include "codecs.h"
#include "rsn_common.h"

namespace rsn {

namespace {

constexpr int AR_WAVES = 4;                        // members of a workgroup
constexpr uint32_t AR_MAX_FREQ = 16383;
constexpr uint32_t AR_HALF = 0x8000, AR_QUARTER = 0x4000, AR_THREE_QUARTERS = 0xC000;
constexpr uint32_t AR_SCAN_CHUNKS = 4096;          // 256-byte chunks a launch looks through for the stream's first 1 bit

// ArithState::status
enum : int32_t { AR_RUN = 0, AR_DONE = 1, AR_SCAN = 2 };
// ArithSummary::detail of a failure
enum : uint32_t { AR_D_NONE = 0, AR_D_NO_ONE = 1, AR_D_SHORT = 2, AR_D_TAIL = 3, AR_D_TABLE = 4, AR_D_RAW_FULL = 5, AR_D_TOO_LONG = 6 };

struct ArithMember {
    const uint8_t *in;                 // the member's bytes (4-byte aligned; readable up to the next 4-byte boundary behind in + n)
    unsigned long long n;
    uint8_t *out;                      // encoder: the raw words (4-byte aligned); decoder: where byte `origin` of the result goes
    unsigned long long cap;            // bytes of `out`
    unsigned long long origin;         // decoder: the result offset that out[0] holds (a round of the host call starts a fresh window)
    uint32_t state, pad_;              // index of the member's ArithState / ArithSummary
};

struct ArithState {
    uint16_t cf[256];                  // cf[1..256]: lane l's four at [4l .. 4l+3]
    uint32_t tot, low, high, value, pending;
    int32_t status;
    uint32_t detail, acc, acc_n, overflow;
    unsigned long long in_pos;         // encoder: bytes coded; decoder: the next bit's position
    unsigned long long out_pos;        // encoder: raw words written; decoder: bytes produced
};

struct ArithSummary { int32_t status; uint32_t detail; unsigned long long total; };   // total: encoder: the stream's bytes; decoder: bytes produced so far

__device__ __forceinline__ uint32_t uni(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ unsigned long long uni64(unsigned long long v) {
    return ((unsigned long long)uni((uint32_t)(v >> 32)) << 32) | uni((uint32_t)v);
}

// the table in a wave's registers
struct Table {
    uint32_t u0, u1, u2, u3;           // cf[4l+1 .. 4l+4]
    uint32_t tot;                      // cf[257] (wave-uniform)
    __device__ __forceinline__ void init(int lane) { u0 = 4 * lane + 1; u1 = u0 + 1; u2 = u0 + 2; u3 = u0 + 3; tot = 257; }
    __device__ __forceinline__ void load(const ArithState &st, int lane) {
        const uint2 v = *reinterpret_cast<const uint2 *>(&st.cf[4 * lane]);
        u0 = v.x & 0xFFFF; u1 = v.x >> 16; u2 = v.y & 0xFFFF; u3 = v.y >> 16;
        tot = uni(st.tot);
    }
    __device__ __forceinline__ void save(ArithState &st, int lane) const {
        *reinterpret_cast<uint2 *>(&st.cf[4 * lane]) = make_uint2(u0 | (u1 << 16), u2 | (u3 << 16));
        if (lane == 0) st.tot = tot;
    }
    // cf[i] for a wave-uniform i in 1..256
    __device__ __forceinline__ uint32_t at(uint32_t i) const {
        const uint32_t j = i - 1, k = j & 3;
        const uint32_t v = k == 0 ? u0 : k == 1 ? u1 : k == 2 ? u2 : u3;
        return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)(j >> 2));
    }
    __device__ __forceinline__ void bounds(uint32_t s, uint32_t &lo, uint32_t &hi) const {
        lo = s == 0 ? 0u : at(s);
        hi = s == 256 ? tot : at(s + 1);
    }
    // cf[i] += 1 for all i > s; returns whether the table is frozen now
    __device__ __forceinline__ bool update(uint32_t s, int lane) {
        const uint32_t b = 4 * lane;
        u0 += b >= s; u1 += b + 1 >= s; u2 += b + 2 >= s; u3 += b + 3 >= s;
        return ++tot >= AR_MAX_FREQ;
    }
    // the first s with sv < cf[s+1] (sv < tot)
    __device__ __forceinline__ uint32_t find(uint32_t sv) const {
        const unsigned long long m = __ballot(sv < u3);
        if (m == 0) return 256;
        const int l = __builtin_ctzll(m);
        const uint32_t k = (sv >= u0) + (sv >= u1) + (sv >= u2);
        return 4 * l + (uint32_t)__builtin_amdgcn_readlane((int)k, l);
    }
};

// ---------------------------------------------------------------- encoder
// the coder's bits, MSB first: a wave-uniform accumulator of fewer than 32 bits, whole words in the lanes (word k of the pending 64 in
// lane k), stored 64 at a time
struct BitSink {
    uint32_t *raw; unsigned long long cap_words, wpos;
    unsigned long long acc; uint32_t acc_n, wcnt, wreg, overflow;
    int lane;
    __device__ __forceinline__ void flush() {
        if ((uint32_t)lane < wcnt) {
            if (wpos + lane < cap_words) raw[wpos + lane] = wreg;
        }
        if (wpos + wcnt > cap_words) overflow = 1;
        wpos += wcnt; wcnt = 0;
    }
    __device__ __forceinline__ void word(uint32_t w) {
        if ((uint32_t)lane == wcnt) wreg = __builtin_bswap32(w);
        if (++wcnt == 64) flush();
    }
    __device__ __forceinline__ void put(uint32_t v, uint32_t k) {   // k <= 32 bits, v < 2^k
        acc = (acc << k) | v; acc_n += k;
        if (acc_n >= 32) { acc_n -= 32; word((uint32_t)(acc >> acc_n)); acc &= (1ull << acc_n) - 1; }
    }
    // `bit`, then `run` times its opposite: a run goes out whole words at a time
    __device__ __forceinline__ void put_with_run(uint32_t bit, uint32_t run) {
        if (run < 32) { put(bit ? (1u << run) : ((1u << run) - 1), run + 1); return; }
        put(bit, 1);
        const uint32_t fill = bit ? 0u : 0xFFFFFFFFu;
        const uint32_t head = min(run, 32 - acc_n);                  // up to the word boundary
        put(fill >> (32 - head), head); run -= head;
        for (; run >= 32; run -= 32) word(fill);                     // (acc_n == 0 here whenever run >= 32 is left)
        if (run) put(fill >> (32 - run), run);
    }
};

template <bool FROZEN>
__device__ __forceinline__ void enc_symbol(Table &t, BitSink &o, uint32_t s, uint32_t &low, uint32_t &high, uint32_t &pending, bool &frozen, int lane) {
    const uint32_t d = high - low + 1;
    uint32_t lo, hi; t.bounds(s, lo, hi);
    const uint32_t tot = FROZEN ? AR_MAX_FREQ : t.tot;
    if (!FROZEN) frozen = t.update(s, lane);
    high = low + d * hi / tot - 1;
    low = low + d * lo / tot;
    for (;;) {
        if (high < AR_HALF) { o.put_with_run(0, pending); pending = 0; }
        else if (low >= AR_HALF) { o.put_with_run(1, pending); pending = 0; }
        else if (low >= AR_QUARTER && high < AR_THREE_QUARTERS) { pending++; low -= AR_QUARTER; high -= AR_QUARTER; }
        else break;
        high = (2 * high + 1) & 0xFFFF;
        low = (2 * low) & 0xFFFF;
    }
}

__global__ __launch_bounds__(64 * AR_WAVES) void k_arith_enc(const ArithMember *__restrict__ mem, ArithState *__restrict__ states,
                                                            ArithSummary *__restrict__ summ, unsigned long long *__restrict__ slot_bytes,
                                                            uint32_t n_members, uint32_t budget, int first) {
    const int lane = threadIdx.x & 63;
    const uint32_t m = uni(blockIdx.x * AR_WAVES + (threadIdx.x >> 6));
    if (m >= n_members) return;
    const ArithMember me = mem[m];
    ArithState &st = states[me.state];
    Table t; BitSink o;
    uint32_t low, high, pending;
    unsigned long long in_pos;
    o.raw = reinterpret_cast<uint32_t *>(me.out); o.cap_words = me.cap / 4; o.lane = lane; o.wcnt = 0; o.wreg = 0;
    if (first) {
        t.init(lane); low = 0; high = 0xFFFF; pending = 0; in_pos = 0;
        o.wpos = 0; o.acc = 0; o.acc_n = 0; o.overflow = 0;
    } else {
        if (uni((uint32_t)st.status) != (uint32_t)AR_RUN) return;
        t.load(st, lane); low = uni(st.low); high = uni(st.high); pending = uni(st.pending); in_pos = uni64(st.in_pos);
        o.wpos = uni64(st.out_pos); o.acc = uni(st.acc); o.acc_n = uni(st.acc_n); o.overflow = uni(st.overflow);
    }
    const unsigned long long n = me.n;
    bool frozen = t.tot >= AR_MAX_FREQ, done = false;
    uint32_t bytes = 0;                                               // lane l: byte (in_pos & ~63) + l
    auto fetch = [&]() { const unsigned long long p = (in_pos & ~63ull) + lane; bytes = p < n ? me.in[p] : 0; };
    if (in_pos < n) fetch();
    uint32_t left = budget;
    while (left && !done) {                                           // (two loops: the frozen table's has no update in it)
        if (!frozen) {
            for (; left && !done && !frozen; left--) {
                uint32_t s = 256;
                if (in_pos < n) { s = (uint32_t)__builtin_amdgcn_readlane((int)bytes, (int)(in_pos & 63)); if (((++in_pos) & 63) == 0 && in_pos < n) fetch(); }
                else done = true;
                enc_symbol<false>(t, o, s, low, high, pending, frozen, lane);
            }
        } else {
            for (; left && !done; left--) {
                uint32_t s = 256;
                if (in_pos < n) { s = (uint32_t)__builtin_amdgcn_readlane((int)bytes, (int)(in_pos & 63)); if (((++in_pos) & 63) == 0 && in_pos < n) fetch(); }
                else done = true;
                enc_symbol<true>(t, o, s, low, high, pending, frozen, lane);
            }
        }
    }
    o.flush();
    if (done) {
        // nothing is flushed at the end (pending bits are dropped); the last, partial word goes out zero-filled
        const unsigned long long nbits = o.wpos * 32 + o.acc_n;
        if (o.acc_n) {
            if (o.wpos < o.cap_words) { if (lane == 0) o.raw[o.wpos] = __builtin_bswap32((uint32_t)(o.acc << (32 - o.acc_n))); }
            else o.overflow = 1;
        }
        if (lane == 0) {
            const unsigned long long total = nbits / 8 + 1;
            summ[me.state].status = o.overflow ? RSN_ERR_DEVICE : AR_DONE;
            summ[me.state].detail = o.overflow ? AR_D_RAW_FULL : AR_D_NONE;
            summ[me.state].total = total;
            slot_bytes[me.state] = (total + 15) & ~15ull;
            st.status = AR_DONE;
            st.out_pos = nbits;                                       // (from here on: the bit count, for k_arith_pack)
        }
        return;
    }
    t.save(st, lane);
    if (lane == 0) {
        st.low = low; st.high = high; st.pending = pending; st.value = 0; st.status = AR_RUN; st.detail = 0;
        st.acc = (uint32_t)o.acc; st.acc_n = o.acc_n; st.overflow = o.overflow; st.in_pos = in_pos; st.out_pos = o.wpos;
        summ[me.state].status = AR_RUN; summ[me.state].detail = 0; summ[me.state].total = 0;
    }
}

// The raw bits into place behind the front pad -- p = 8 - nbits % 8 bits, all zero but the last -- and the members' streams side by side:
// member k's at out + offs[k] (offs: the exclusive scan of the 16-byte rounded sizes).  A thread makes 16 bytes of one member's stream:
// byte j is the last p bits of raw byte j - 1 and the first 8 - p of raw byte j.  Only the stream's own bytes are stored.
// OWN (the batch call on device buffers): member k's stream goes to its own buffer, dests[k].dst, instead of out + offs[k] -- the scan only
// deals the threads out -- and only when the whole of it fits dests[k].cap.
struct ArithDest { uint8_t *dst; unsigned long long cap; };
template <bool OWN>
__global__ __launch_bounds__(256) void k_arith_pack(const ArithMember *__restrict__ mem, const ArithState *__restrict__ states,
                                                    const unsigned long long *__restrict__ offs, const unsigned long long *__restrict__ total,
                                                    uint32_t n_members, uint8_t *__restrict__ out, const ArithDest *__restrict__ dests) {
    const unsigned long long units = *total / 16;
    for (unsigned long long u = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (unsigned long long)gridDim.x * blockDim.x) {
        const unsigned long long at = u * 16;
        uint32_t a = 0, b = n_members;                                // the last member with offs[k] <= at
        while (b - a > 1) { const uint32_t mid = (a + b) / 2; if (offs[mid] <= at) a = mid; else b = mid; }
        const ArithMember me = mem[a];
        const unsigned long long nbits = states[me.state].out_pos, len = nbits / 8 + 1, j0 = at - offs[a];
        if (j0 >= len) continue;
        uint8_t *dst = out + at;
        if constexpr (OWN) {
            const ArithDest d = dests[a];
            if (len > d.cap) continue;
            dst = d.dst + j0;
        }
        const uint32_t p = 8 - (uint32_t)(nbits & 7);
        const uint4 r4 = *reinterpret_cast<const uint4 *>(me.out + j0);
        const uint32_t r[4] = {r4.x, r4.y, r4.z, r4.w};
        uint32_t prev = j0 ? me.out[j0 - 1] : 0;
        uint32_t f[4];
#pragma unroll
        for (int w = 0; w < 4; w++) {
            f[w] = 0;
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t cur = (r[w] >> (8 * i)) & 0xFF;
                f[w] |= ((((prev << 8) | cur) >> p) & 0xFF) << (8 * i);
                prev = cur;
            }
        }
        if (j0 == 0) f[0] |= 1u << (8 - p);
        if (j0 + 16 <= len) *reinterpret_cast<uint4 *>(dst) = make_uint4(f[0], f[1], f[2], f[3]);
        else for (uint32_t i = 0; j0 + i < len; i++) dst[i] = (uint8_t)(f[i >> 2] >> (8 * (i & 3)));
    }
}

// ---------------------------------------------------------------- decoder
// the stream's bits behind its first 1, then the appended 1, 0, then zeros for ever: lane l holds big-endian word l of the 256-byte
// chunk in hand, the word in hand is wave-uniform
struct BitSource {
    const uint8_t *in; unsigned long long n, nbits, pos;
    uint32_t words, cur; bool fresh;
    int lane;
    __device__ __forceinline__ void chunk(unsigned long long c) {     // bytes at and behind n read as zero
        const unsigned long long off = c * 256 + 4ull * lane;
        uint32_t w = 0;
        if (off < n) {
            w = __builtin_bswap32(*reinterpret_cast<const uint32_t *>(in + off));
            if (off + 4 > n) w &= ~0u << (8 * (uint32_t)(off + 4 - n));
        }
        words = w;
    }
    __device__ __forceinline__ uint32_t next() {
        uint32_t b;
        if (pos < nbits) {
            if (fresh || (pos & 31) == 0) {
                if (fresh || (pos & 2047) == 0) chunk(pos >> 11);
                cur = (uint32_t)__builtin_amdgcn_readlane((int)words, (int)((pos >> 5) & 63));
                fresh = false;
            }
            b = (cur >> (31 - (uint32_t)(pos & 31))) & 1;
        } else b = pos == nbits;
        pos++;
        return b;
    }
};

struct ByteSink {
    uint8_t *out; unsigned long long cap, origin, pos;
    uint32_t cnt, reg; int lane;
    __device__ __forceinline__ void flush() {
        const unsigned long long at = pos - origin + lane;
        if ((uint32_t)lane < cnt && at < cap) out[at] = (uint8_t)reg;
        pos += cnt; cnt = 0;
    }
    __device__ __forceinline__ void put(uint32_t s) {
        if ((uint32_t)lane == cnt) reg = s;
        if (++cnt == 64) flush();
    }
};

// one symbol; returns 0, AR_DONE at the end symbol, or a negative code (detail set)
template <bool FROZEN>
__device__ __forceinline__ int dec_symbol(Table &t, BitSource &in, ByteSink &o, uint32_t &low, uint32_t &high, uint32_t &value, bool &frozen,
                                          uint32_t &detail, int lane) {
    if (in.pos > in.nbits + RSN_ARITH_TAIL_BITS) { detail = AR_D_TAIL; return RSN_ERR_FORMAT; }
    const uint32_t tot = FROZEN ? AR_MAX_FREQ : t.tot;
    const uint32_t d = high - low + 1;
    const uint32_t sv = ((value - low + 1) * tot - 1) / d;
    if (sv >= tot) { detail = AR_D_TABLE; return RSN_ERR_FORMAT; }
    const uint32_t s = uni(t.find(sv));
    uint32_t lo, hi; t.bounds(s, lo, hi);
    if (!FROZEN) frozen = t.update(s, lane);
    if (s == 256) return AR_DONE;
    o.put(s);
    high = low + d * hi / tot - 1;
    low = low + d * lo / tot;
    for (;;) {
        if (high < AR_HALF) {}
        else if (low >= AR_HALF) { value -= AR_HALF; low -= AR_HALF; high -= AR_HALF; }
        else if (low >= AR_QUARTER && high < AR_THREE_QUARTERS) { value -= AR_QUARTER; low -= AR_QUARTER; high -= AR_QUARTER; }
        else break;
        low <<= 1; high = 2 * high + 1;
        value = 2 * value + in.next();
    }
    return 0;
}

__global__ __launch_bounds__(64 * AR_WAVES) void k_arith_dec(const ArithMember *__restrict__ mem, ArithState *__restrict__ states,
                                                            ArithSummary *__restrict__ summ, uint32_t n_members, uint32_t budget, int first,
                                                            unsigned long long max_out) {
    const int lane = threadIdx.x & 63;
    const uint32_t m = uni(blockIdx.x * AR_WAVES + (threadIdx.x >> 6));
    if (m >= n_members) return;
    const ArithMember me = mem[m];
    ArithState &st = states[me.state];
    Table t; BitSource in; ByteSink o;
    uint32_t low, high, value, detail = 0;
    int32_t status;
    in.in = me.in; in.n = me.n; in.nbits = me.n * 8; in.lane = lane; in.fresh = true; in.words = 0; in.cur = 0;
    o.out = me.out; o.cap = me.cap; o.origin = me.origin; o.lane = lane; o.cnt = 0; o.reg = 0;
    if (first) { t.init(lane); low = 0; high = 0xFFFF; value = 0; in.pos = 0; o.pos = 0; status = AR_SCAN; }
    else {
        status = (int32_t)uni((uint32_t)st.status);
        if (status != AR_RUN && status != AR_SCAN) return;
        t.load(st, lane); low = uni(st.low); high = uni(st.high); value = uni(st.value); in.pos = uni64(st.in_pos); o.pos = uni64(st.out_pos);
    }
    if (status == AR_SCAN) {
        // everything up to and including the first 1 bit is dropped; a stream without one, or with fewer than 14 bits behind it (16 with
        // the appended two), is where the reference panics
        unsigned long long c = in.pos >> 11;
        const unsigned long long c_end = (in.n + 255) / 256;
        for (uint32_t k = 0; k < AR_SCAN_CHUNKS && c < c_end && status == AR_SCAN; k++, c++) {
            in.chunk(c);
            const unsigned long long mask = __ballot(in.words != 0);
            if (mask) {
                const int l = __builtin_ctzll(mask);
                const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)in.words, l);
                in.pos = c * 2048 + 32ull * l + __builtin_clz(w) + 1;
                status = AR_RUN;
            }
        }
        if (status == AR_SCAN) {
            in.pos = c * 2048;
            if (c >= c_end) { status = RSN_ERR_FORMAT; detail = AR_D_NO_ONE; }
        } else if (in.nbits - in.pos < 14) { status = RSN_ERR_FORMAT; detail = AR_D_SHORT; }
        else { in.fresh = true; for (int k = 0; k < 16; k++) value = 2 * value + in.next(); }
    }
    if (status == AR_RUN) {
        bool frozen = t.tot >= AR_MAX_FREQ;
        uint32_t left = budget;
        int r = 0;
        while (left && r == 0) {
            if (!frozen) { for (; left && r == 0 && !frozen; left--) r = dec_symbol<false>(t, in, o, low, high, value, frozen, detail, lane); }
            else { for (; left && r == 0; left--) r = dec_symbol<true>(t, in, o, low, high, value, frozen, detail, lane); }
        }
        o.flush();
        if (r) status = r;
        else if (o.pos > max_out) { status = RSN_ERR_LIMIT; detail = AR_D_TOO_LONG; }
    }
    if (status == AR_RUN || status == AR_SCAN) t.save(st, lane);
    if (lane == 0) {
        st.low = low; st.high = high; st.value = value; st.pending = 0; st.status = status; st.detail = detail;
        st.in_pos = in.pos; st.out_pos = o.pos;
        summ[me.state].status = status; summ[me.state].detail = detail; summ[me.state].total = o.pos;
    }
}

// ---------------------------------------------------------------- host side
constexpr size_t AR_GROUP_BYTES = (size_t)256 << 20;     // a group of a batch: its members' inputs (decoder) / raw areas (encoder) ...
constexpr size_t AR_GROUP_MAX = 32768;                   // ... and how many members
constexpr size_t AR_ARENA_BYTES = (size_t)8 << 20;       // host-buffer decode: the window a round's output lands in, shared by the running members

struct StateArea { ArithState *st; ArithSummary *summ; unsigned long long *slot_bytes, *offs, *total; };
int state_area(Ctx &c, size_t m, StateArea &a) {
    const size_t st_b = round_up(m * sizeof(ArithState), 16), su_b = round_up(m * sizeof(ArithSummary), 16), u_b = round_up(m * 8, 16);
    void *p; int rc = dev_buf(c, Slot::AR_STATE, st_b + su_b + 2 * u_b + 16, &p); if (rc) return rc;
    uint8_t *b = (uint8_t *)p;
    a.st = (ArithState *)b; a.summ = (ArithSummary *)(b + st_b); a.slot_bytes = (unsigned long long *)(b + st_b + su_b);
    a.offs = a.slot_bytes + u_b / 8; a.total = a.offs + u_b / 8;
    return RSN_OK;
}

const char *detail_text(uint32_t d) {
    switch (d) {
    case AR_D_NO_ONE: return "no 1 bit in the stream (the reference panics in Unpack)";
    case AR_D_SHORT: return "fewer than 16 bits to start from (the reference indexes out of range)";
    case AR_D_TAIL: return "no end symbol within RSN_ARITH_TAIL_BITS bits behind the stream (the reference would decode for ever)";
    case AR_D_TABLE: return "a code value outside the table (the reference divides by zero)";
    case AR_D_RAW_FULL: return "internal error: the encoder's bits outgrew rsn_arithmetic_compress_bound";
    case AR_D_TOO_LONG: return "the stream decodes to more than the size limit (DESIGN 7)";
    }
    return "unknown failure";
}
int member_fail(Ctx &c, const ArithSummary &s) { return c.fail(s.status, "arithmetic: %s", detail_text(s.detail)); }

dim3 member_grid(size_t m) { return dim3((uint32_t)ceil_div(m, AR_WAVES)); }

// The encoder over m members whose descriptors are at d_mem: the slices, the scan of the sizes, and the summaries (with the total behind
// them) down into `h` (m summaries + 1 word, pinned or not).  Synchronises.
int encode_run(Ctx &c, hipStream_t s, const ArithMember *d_mem, const StateArea &a, size_t m, size_t max_n, ArithSummary *h, unsigned long long *h_total) {
    const size_t launches = ceil_div(max_n + 1, (size_t)ARITH_SLICE_SYMBOLS);
    for (size_t k = 0; k < launches; k++)
        RSN_LAUNCH("k_arith_enc", k_arith_enc, member_grid(m), dim3(64 * AR_WAVES), 0, s, d_mem, a.st, a.summ, a.slot_bytes, (uint32_t)m, ARITH_SLICE_SYMBOLS, k == 0 ? 1 : 0);
    int rc = scan_u64(c, s, "arith_scan", a.slot_bytes, a.offs, (uint32_t)m, a.total); if (rc) return rc;
    RSN_HIP(copy_async(h, a.summ, m * sizeof(ArithSummary), hipMemcpyDeviceToHost, s));
    RSN_HIP(copy_async(h_total, a.total, 8, hipMemcpyDeviceToHost, s));
    RSN_HIP(hipStreamSynchronize(s));
    return RSN_OK;
}
int pack_run(Ctx &c, hipStream_t s, const ArithMember *d_mem, const StateArea &a, size_t m, unsigned long long total, uint8_t *d_out) {
    const uint32_t blocks = (uint32_t)std::min<size_t>(ceil_div((size_t)total / 16, 256), 4096);
    if (blocks) RSN_LAUNCH("k_arith_pack", k_arith_pack<false>, dim3(blocks), dim3(256), 0, s, d_mem, (const ArithState *)a.st, (const unsigned long long *)a.offs, (const unsigned long long *)a.total, (uint32_t)m, d_out, (const ArithDest *)nullptr);
    return RSN_OK;
}
int pack_own_run(Ctx &c, hipStream_t s, const ArithMember *d_mem, const StateArea &a, size_t m, unsigned long long total, const ArithDest *d_dests) {
    const uint32_t blocks = (uint32_t)std::min<size_t>(ceil_div((size_t)total / 16, 256), 4096);
    if (blocks) RSN_LAUNCH("k_arith_pack_own", k_arith_pack<true>, dim3(blocks), dim3(256), 0, s, d_mem, (const ArithState *)a.st, (const unsigned long long *)a.offs, (const unsigned long long *)a.total, (uint32_t)m, (uint8_t *)nullptr, d_dests);
    return RSN_OK;
}

size_t raw_bytes(size_t n) { return round_up(arith_compress_bound(n), 16) + 16; }

// members idx[lo, hi) in one go
int compress_group(Ctx &c, hipStream_t s, const std::vector<size_t> &idx, size_t lo, size_t hi, const uint8_t *const *ins, const size_t *lens,
                   const SmallTake &take, size_t *failed) {
    const size_t m = hi - lo;
    const size_t desc_b = round_up(m * sizeof(ArithMember), 16);
    size_t in_b = 0, raw_b = 0, max_n = 0;
    for (size_t k = lo; k < hi; k++) { const size_t n = lens[idx[k]]; in_b += round_up(n, 16) + 16; raw_b += raw_bytes(n); max_n = std::max(max_n, n); }
    Admission gate(c, slotset::ARITH_HOST); gate.admit(desc_b + in_b + 2 * raw_b, ADMIT_FROM);
    *failed = idx[lo];
    void *p_up, *d_up, *d_raw; StateArea a;
    const size_t summ_b = round_up(m * sizeof(ArithSummary), 16) + 16;
    int rc = pinned_buf(c, desc_b + in_b + summ_b, &p_up); if (rc) return rc;
    rc = dev_buf(c, Slot::STAGE_IN, desc_b + in_b, &d_up); if (rc) return rc;
    rc = dev_buf(c, Slot::AR_RAW, raw_b, &d_raw); if (rc) return rc;
    rc = state_area(c, m, a); if (rc) return rc;
    ArithMember *hm = (ArithMember *)p_up;
    size_t io = desc_b, ro = 0;
    for (size_t k = lo; k < hi; k++) {
        const size_t i = idx[k], n = lens[i];
        ArithMember &me = hm[k - lo];
        me.in = (const uint8_t *)d_up + io; me.n = n; me.out = (uint8_t *)d_raw + ro; me.cap = raw_bytes(n); me.origin = 0; me.state = (uint32_t)(k - lo); me.pad_ = 0;
        if (n) memcpy((uint8_t *)p_up + io, ins[i], n);
        memset((uint8_t *)p_up + io + n, 0, round_up(n, 16) + 16 - n);
        io += round_up(n, 16) + 16; ro += raw_bytes(n);
    }
    RSN_HIP(copy_async(d_up, p_up, desc_b + in_b, hipMemcpyHostToDevice, s));
    ArithSummary *hs = (ArithSummary *)((uint8_t *)p_up + desc_b + in_b);
    unsigned long long *h_total = (unsigned long long *)((uint8_t *)hs + summ_b - 16);
    rc = encode_run(c, s, (const ArithMember *)d_up, a, m, max_n, hs, h_total); if (rc) return rc;
    for (size_t k = 0; k < m; k++) if (hs[k].status != AR_DONE) { *failed = idx[lo + k]; return member_fail(c, hs[k]); }
    const unsigned long long total = *h_total;
    std::vector<unsigned long long> sizes(m);
    for (size_t k = 0; k < m; k++) sizes[k] = hs[k].total;
    void *d_out; rc = dev_buf(c, Slot::STAGE_OUT, (size_t)total, &d_out); if (rc) return rc;
    rc = pack_run(c, s, (const ArithMember *)d_up, a, m, total, (uint8_t *)d_out); if (rc) return rc;
    void *p_down; rc = pinned_buf(c, (size_t)total, &p_down); if (rc) return rc;      // (the upload is done: the staging may move)
    RSN_HIP(copy_async(p_down, d_out, (size_t)total, hipMemcpyDeviceToHost, s));
    RSN_HIP(hipStreamSynchronize(s));
    size_t off = 0;
    for (size_t k = 0; k < m; k++) {
        rc = take(idx[lo + k], (const uint8_t *)p_down + off, (size_t)sizes[k]);
        if (rc) { *failed = idx[lo + k]; return rc; }
        off += round_up((size_t)sizes[k], 16);
    }
    return RSN_OK;
}

int decompress_group(Ctx &c, hipStream_t s, const std::vector<size_t> &idx, size_t lo, size_t hi, const uint8_t *const *ins, const size_t *lens,
                     const SmallTake &take, size_t *failed) {
    const size_t m = hi - lo;
    const size_t desc_b = round_up(m * sizeof(ArithMember), 16), summ_b = round_up(m * sizeof(ArithSummary), 16);
    size_t in_b = 0;
    for (size_t k = lo; k < hi; k++) in_b += round_up(lens[idx[k]], 16) + 16;
    Admission gate(c, slotset::ARITH_HOST); gate.admit(in_b + AR_ARENA_BYTES, ADMIT_FROM);
    *failed = idx[lo];
    // the staging: the streams (once), then per round the running members' descriptors up and their summaries and windows down
    void *p_pin, *d_in, *d_desc, *d_arena; StateArea a;
    int rc = pinned_buf(c, std::max(in_b, desc_b + summ_b + AR_ARENA_BYTES), &p_pin); if (rc) return rc;
    rc = dev_buf(c, Slot::STAGE_IN, in_b, &d_in); if (rc) return rc;
    rc = dev_buf(c, Slot::AR_RAW, desc_b, &d_desc); if (rc) return rc;
    rc = dev_buf(c, Slot::STAGE_OUT, AR_ARENA_BYTES, &d_arena); if (rc) return rc;
    rc = state_area(c, m, a); if (rc) return rc;
    std::vector<size_t> in_off(m);
    size_t io = 0;
    for (size_t k = 0; k < m; k++) {
        const size_t i = idx[lo + k], n = lens[i];
        in_off[k] = io;
        if (n) memcpy((uint8_t *)p_pin + io, ins[i], n);
        memset((uint8_t *)p_pin + io + n, 0, round_up(n, 16) + 16 - n);
        io += round_up(n, 16) + 16;
    }
    RSN_HIP(copy_async(d_in, p_pin, in_b, hipMemcpyHostToDevice, s));
    RSN_HIP(hipStreamSynchronize(s));                                     // (the staging is reused below)
    std::vector<std::vector<uint8_t>> res(m);
    std::vector<uint32_t> running(m);
    for (size_t k = 0; k < m; k++) running[k] = (uint32_t)k;
    ArithMember *hm = (ArithMember *)p_pin;
    ArithSummary *hs = (ArithSummary *)((uint8_t *)p_pin + desc_b);
    uint8_t *h_arena = (uint8_t *)p_pin + desc_b + summ_b;
    size_t first_fail = m; ArithSummary fail_s{};
    for (uint32_t round = 0; !running.empty(); round++) {
        // a round's budget: small at first (most members of a batch are small), never more than a slice or the member's share of the window
        const size_t r = running.size();
        size_t budget = std::min<size_t>(ARITH_SLICE_SYMBOLS, (size_t)1024 << std::min<uint32_t>(2 * round, 16));
        budget = std::max<size_t>(64, std::min(budget, AR_ARENA_BYTES / r / 64 * 64));
        // ... and once the budget is a whole slice, as many launches as the window takes (a long stream: fewer waits for the host)
        const size_t launches = budget == ARITH_SLICE_SYMBOLS ? std::max<size_t>(1, std::min<size_t>(8, AR_ARENA_BYTES / (r * budget))) : 1;
        const size_t window = budget * launches;
        for (size_t q = 0; q < r; q++) {
            const uint32_t k = running[q];
            ArithMember &me = hm[q];
            me.in = (const uint8_t *)d_in + in_off[k]; me.n = lens[idx[lo + k]]; me.out = (uint8_t *)d_arena + q * window; me.cap = window;
            me.origin = res[k].size(); me.state = k; me.pad_ = 0;
        }
        RSN_HIP(copy_async(d_desc, hm, r * sizeof(ArithMember), hipMemcpyHostToDevice, s));
        for (size_t l = 0; l < launches; l++)
            RSN_LAUNCH("k_arith_dec", k_arith_dec, member_grid(r), dim3(64 * AR_WAVES), 0, s, (const ArithMember *)d_desc, a.st, a.summ, (uint32_t)r, (uint32_t)budget,
                       round == 0 && l == 0 ? 1 : 0, (unsigned long long)ARITH_MAX_BYTES);
        RSN_HIP(copy_async(hs, a.summ, m * sizeof(ArithSummary), hipMemcpyDeviceToHost, s));
        RSN_HIP(copy_async(h_arena, d_arena, r * window, hipMemcpyDeviceToHost, s));
        RSN_HIP(hipStreamSynchronize(s));
        std::vector<uint32_t> next;
        for (size_t q = 0; q < r; q++) {
            const uint32_t k = running[q];
            const ArithSummary &su = hs[k];
            if (su.status < 0) { if (k < first_fail) { first_fail = k; fail_s = su; } continue; }
            const size_t have = res[k].size(), got = (size_t)su.total - have;
            if (got > window) return c.fail(RSN_ERR_DEVICE, "arithmetic: internal error: a round produced %zu bytes in a window of %zu", got, window);
            res[k].insert(res[k].end(), h_arena + q * window, h_arena + q * window + got);
            if (su.status != AR_DONE && k < first_fail) next.push_back(k);      // (what lies behind a failure cannot change the answer)
        }
        running.swap(next);
        while (!running.empty() && running.back() > first_fail) running.pop_back();
    }
    if (first_fail != m) { *failed = idx[lo + first_fail]; return member_fail(c, fail_s); }
    for (size_t k = 0; k < m; k++) {
        rc = take(idx[lo + k], res[k].data(), res[k].size());
        if (rc) { *failed = idx[lo + k]; return rc; }
    }
    return RSN_OK;
}

// the members in groups, in index order; a member above the size limit fails when its turn comes (those in front of it have run)
template <class Group>
int members_in_groups(Ctx &c, const std::vector<size_t> &idx, const size_t *lens, bool enc, size_t *failed, Group group) {
    const size_t limit = enc ? (size_t)ARITH_MAX_BYTES : arith_compress_bound(ARITH_MAX_BYTES);
    for (size_t lo = 0; lo < idx.size();) {
        if (lens[idx[lo]] > limit) {
            *failed = idx[lo];
            return c.fail(RSN_ERR_LIMIT, "arithmetic: %zu bytes are more than the %zu of one member (one wave's serial work: DESIGN 7)", lens[idx[lo]], limit);
        }
        size_t hi = lo, bytes = 0;
        while (hi < idx.size() && hi - lo < AR_GROUP_MAX && lens[idx[hi]] <= limit && (hi == lo || bytes + raw_bytes(lens[idx[hi]]) <= AR_GROUP_BYTES))
            bytes += raw_bytes(lens[idx[hi++]]);
        const int rc = group(lo, hi, failed); if (rc) return rc;
        lo = hi;
    }
    return RSN_OK;
}

// ---- the batch calls on device buffers (rsn.h): the members where they lie.  Members [lo, hi) of `mem` in one go; sizes[i]:
// the exact size of member i's result.  A member's failure: its code, *failed = the lowest such member.
int compress_group_dev(Ctx &c, hipStream_t s, const rsn_dev_member *mem, size_t lo, size_t hi, size_t *sizes, size_t *failed) {
    const size_t m = hi - lo;
    const size_t desc_b = round_up(m * sizeof(ArithMember), 16), dest_b = round_up(m * sizeof(ArithDest), 16), summ_b = round_up(m * sizeof(ArithSummary), 16) + 16;
    size_t raw_b = 0, max_n = 0;
    for (size_t k = lo; k < hi; k++) { raw_b += raw_bytes(mem[k].n); max_n = std::max(max_n, mem[k].n); }
    Admission gate(c, slotset::ARITH); gate.admit(desc_b + dest_b + raw_b, ADMIT_FROM);
    *failed = lo;
    void *p_up, *d_raw; StateArea a;
    int rc = pinned_buf(c, desc_b + dest_b + summ_b, &p_up); if (rc) return rc;
    rc = dev_buf(c, Slot::AR_RAW, desc_b + dest_b + raw_b, &d_raw); if (rc) return rc;      // (the descriptors and destinations in front)
    rc = state_area(c, m, a); if (rc) return rc;
    ArithMember *hm = (ArithMember *)p_up;
    ArithDest *hd = (ArithDest *)((uint8_t *)p_up + desc_b);
    size_t ro = desc_b + dest_b;
    for (size_t k = 0; k < m; k++) {
        const rsn_dev_member &x = mem[lo + k];
        ArithMember &me = hm[k];
        me.in = (const uint8_t *)x.d_in; me.n = x.n; me.out = (uint8_t *)d_raw + ro; me.cap = raw_bytes(x.n); me.origin = 0; me.state = (uint32_t)k; me.pad_ = 0;
        hd[k] = ArithDest{(uint8_t *)x.d_out, x.d_out ? (unsigned long long)x.out_cap : 0ull};
        ro += raw_bytes(x.n);
    }
    RSN_HIP(copy_async(d_raw, p_up, desc_b + dest_b, hipMemcpyHostToDevice, s));
    ArithSummary *hs = (ArithSummary *)((uint8_t *)p_up + desc_b + dest_b);
    unsigned long long *h_total = (unsigned long long *)((uint8_t *)hs + summ_b - 16);
    rc = encode_run(c, s, (const ArithMember *)d_raw, a, m, max_n, hs, h_total); if (rc) return rc;
    for (size_t k = 0; k < m; k++) if (hs[k].status != AR_DONE) { *failed = lo + k; return member_fail(c, hs[k]); }
    for (size_t k = 0; k < m; k++) sizes[lo + k] = (size_t)hs[k].total;
    return pack_own_run(c, s, (const ArithMember *)d_raw, a, m, *h_total, (const ArithDest *)((const uint8_t *)d_raw + desc_b));
}

// the decoder writes while it fits and keeps counting beyond: a member whose buffer is too small reports its exact need all the same
int decompress_group_dev(Ctx &c, hipStream_t s, const rsn_dev_member *mem, size_t lo, size_t hi, size_t *sizes, size_t *failed) {
    const size_t m = hi - lo;
    const size_t desc_b = round_up(m * sizeof(ArithMember), 16), summ_b = round_up(m * sizeof(ArithSummary), 16);
    *failed = lo;
    void *p_pin, *d_desc; StateArea a;
    int rc = pinned_buf(c, desc_b + summ_b, &p_pin); if (rc) return rc;
    rc = dev_buf(c, Slot::AR_RAW, desc_b, &d_desc); if (rc) return rc;
    rc = state_area(c, m, a); if (rc) return rc;
    ArithMember *hm = (ArithMember *)p_pin;
    ArithSummary *hs = (ArithSummary *)((uint8_t *)p_pin + desc_b);
    for (size_t k = 0; k < m; k++) {
        const rsn_dev_member &x = mem[lo + k];
        ArithMember &me = hm[k];
        me.in = (const uint8_t *)x.d_in; me.n = x.n; me.out = (uint8_t *)x.d_out; me.cap = x.d_out ? x.out_cap : 0; me.origin = 0; me.state = (uint32_t)k; me.pad_ = 0;
    }
    RSN_HIP(copy_async(d_desc, hm, m * sizeof(ArithMember), hipMemcpyHostToDevice, s));
    // the summaries are looked at after one launch, then after every eight (arith_decode_dev), until no member is running
    for (uint32_t round = 0;; round++) {
        for (int k = 0; k < (round ? 8 : 1); k++)
            RSN_LAUNCH("k_arith_dec", k_arith_dec, member_grid(m), dim3(64 * AR_WAVES), 0, s, (const ArithMember *)d_desc, a.st, a.summ, (uint32_t)m, ARITH_SLICE_SYMBOLS,
                       round == 0 && k == 0 ? 1 : 0, (unsigned long long)ARITH_MAX_BYTES);
        RSN_HIP(copy_async(hs, a.summ, m * sizeof(ArithSummary), hipMemcpyDeviceToHost, s));
        RSN_HIP(hipStreamSynchronize(s));
        bool running = false;
        for (size_t k = 0; k < m && !running; k++) running = hs[k].status == AR_RUN || hs[k].status == AR_SCAN;
        if (!running) break;
    }
    for (size_t k = 0; k < m; k++) if (hs[k].status != AR_DONE) { *failed = lo + k; return member_fail(c, hs[k]); }
    for (size_t k = 0; k < m; k++) sizes[lo + k] = (size_t)hs[k].total;
    return RSN_OK;
}

}  // namespace

size_t arith_compress_bound(size_t n) { return 2 * n + 4; }

int arith_members_dev(Ctx &c, hipStream_t s, bool enc, size_t n, const rsn_dev_member *mem, size_t *out_lens, size_t *failed) {
    // the host form's groups (members_in_groups), the single calls' limits and words: a member above the limit fails when its turn comes
    const size_t limit = enc ? (size_t)ARITH_MAX_BYTES : arith_compress_bound(ARITH_MAX_BYTES);
    for (size_t lo = 0; lo < n;) {
        if (mem[lo].n > limit) {
            *failed = lo;
            return enc ? c.fail(RSN_ERR_LIMIT, "arithmetic: %zu bytes are more than the %zu of one stream (one wave's serial work: DESIGN 7)", mem[lo].n, limit)
                       : c.fail(RSN_ERR_LIMIT, "arithmetic: a stream of %zu bytes is more than the %zu of one stream (DESIGN 7)", mem[lo].n, limit);
        }
        size_t hi = lo, bytes = 0;
        while (hi < n && hi - lo < AR_GROUP_MAX && mem[hi].n <= limit && (hi == lo || bytes + raw_bytes(mem[hi].n) <= AR_GROUP_BYTES)) bytes += raw_bytes(mem[hi++].n);
        const int rc = enc ? compress_group_dev(c, s, mem, lo, hi, out_lens, failed) : decompress_group_dev(c, s, mem, lo, hi, out_lens, failed);
        if (rc) return rc;
        lo = hi;
    }
    RSN_HIP(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; i++) {
        const size_t cap = mem[i].d_out ? mem[i].out_cap : 0;
        if (out_lens[i] > cap) { *failed = i; return c.fail(RSN_ERR_CAPACITY, "arithmetic: output needs %zu bytes, buffer holds %zu", out_lens[i], cap); }
    }
    return RSN_OK;
}

int arith_compress_members(Ctx &c, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, const SmallTake &take, size_t *failed) {
    hipStream_t s = c.own_stream;
    return members_in_groups(c, idx, lens, true, failed, [&](size_t lo, size_t hi, size_t *f) { return compress_group(c, s, idx, lo, hi, ins, lens, take, f); });
}

int arith_decompress_members(Ctx &c, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, const SmallTake &take, size_t *failed) {
    hipStream_t s = c.own_stream;
    return members_in_groups(c, idx, lens, false, failed, [&](size_t lo, size_t hi, size_t *f) { return decompress_group(c, s, idx, lo, hi, ins, lens, take, f); });
}

int arith_encode_dev(Ctx &c, hipStream_t s, const uint8_t *d_in, size_t n, uint8_t *d_out, size_t out_cap, size_t *out_n) {
    int rc;
    if (n > ARITH_MAX_BYTES) return c.fail(RSN_ERR_LIMIT, "arithmetic: %zu bytes are more than the %zu of one stream (one wave's serial work: DESIGN 7)", n, (size_t)ARITH_MAX_BYTES);
    Admission gate(c, slotset::ARITH); gate.admit(raw_bytes(n), ADMIT_FROM);
    void *d_raw; StateArea a;
    rc = dev_buf(c, Slot::AR_RAW, raw_bytes(n) + 64, &d_raw); if (rc) return rc;
    rc = state_area(c, 1, a); if (rc) return rc;
    ArithMember me{};
    me.in = d_in; me.n = n; me.out = (uint8_t *)d_raw + 64; me.cap = raw_bytes(n); me.state = 0;
    RSN_HIP(copy_async(d_raw, &me, sizeof me, hipMemcpyHostToDevice, s));       // (pageable and small: the copy has read it when the call returns)
    ArithSummary hs; unsigned long long total = 0;
    rc = encode_run(c, s, (const ArithMember *)d_raw, a, 1, n, &hs, &total); if (rc) return rc;
    if (hs.status != AR_DONE) return member_fail(c, hs);
    *out_n = (size_t)hs.total;
    if (!d_out || hs.total > out_cap) return c.fail(RSN_ERR_CAPACITY, "arithmetic: output needs %llu bytes, buffer holds %zu", hs.total, d_out ? out_cap : (size_t)0);
    rc = pack_run(c, s, (const ArithMember *)d_raw, a, 1, total, d_out); if (rc) return rc;
    RSN_HIP(hipStreamSynchronize(s));
    return RSN_OK;
}

int arith_decode_dev(Ctx &c, hipStream_t s, const uint8_t *d_in, size_t n, uint8_t *d_out, size_t out_cap, size_t *out_n) {
    int rc;
    if (n > arith_compress_bound(ARITH_MAX_BYTES)) return c.fail(RSN_ERR_LIMIT, "arithmetic: a stream of %zu bytes is more than the %zu of one stream (DESIGN 7)", n, arith_compress_bound(ARITH_MAX_BYTES));
    if (!d_out) out_cap = 0;
    void *d_desc; StateArea a;
    rc = dev_buf(c, Slot::AR_RAW, 64, &d_desc); if (rc) return rc;
    rc = state_area(c, 1, a); if (rc) return rc;
    ArithMember me{};
    me.in = d_in; me.n = n; me.out = d_out; me.cap = out_cap; me.origin = 0; me.state = 0;
    RSN_HIP(copy_async(d_desc, &me, sizeof me, hipMemcpyHostToDevice, s));
    ArithSummary hs{};
    // the decoded size is not known in advance: slices until the end symbol, looked at after one launch, then after every eight
    for (uint32_t round = 0;; round++) {
        for (int k = 0; k < (round ? 8 : 1); k++)
            RSN_LAUNCH("k_arith_dec", k_arith_dec, dim3(1), dim3(64 * AR_WAVES), 0, s, (const ArithMember *)d_desc, a.st, a.summ, 1u, ARITH_SLICE_SYMBOLS,
                       round == 0 ? 1 : 0, (unsigned long long)ARITH_MAX_BYTES);
        RSN_HIP(copy_async(&hs, a.summ, sizeof hs, hipMemcpyDeviceToHost, s));
        RSN_HIP(hipStreamSynchronize(s));
        if (hs.status != AR_RUN && hs.status != AR_SCAN) break;
    }
    if (hs.status != AR_DONE) return member_fail(c, hs);
    *out_n = (size_t)hs.total;
    if (hs.total > out_cap) return c.fail(RSN_ERR_CAPACITY, "arithmetic: output needs %llu bytes, buffer holds %zu", hs.total, out_cap);
    return RSN_OK;
}

}  // namespace rsn
