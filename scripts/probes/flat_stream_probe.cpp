// Probe: what does this GPU give the TRAFFIC of the flat Huffman kernels at L = 7, with no lookups, in each block shape?
//   emit: read N bytes with 16-byte loads, write 7N/8 bytes from a dword-aligned (not 16-aligned) address
//   dec : read 7N/8 bytes from a dword-aligned address, write N bytes with 16-byte stores
// in three skeletons and one variant of the second:
//   (a) a plain 16-byte grid-stride copy
//   (b) a persistent block of 256 lanes, 8 KiB of symbols a chunk through one LDS image between block barriers (three for emit, two
//       for dec, as in k_emit_flat / k_dec_flat), 16-byte drain, the grid from the occupancy query
//   (c) the same without block barriers: every wavefront a 2 KiB unit of its own through a private LDS region, units dealt over
//       all resident wavefronts
//   (d) the kernel of (b) with one chunk a block, not persistent (grid = chunks): the hardware staggers the blocks.  This is the
//       shape the library launches
// (b) and (c) carry a 16 KiB table in LDS so that as many blocks fit a CU as in the library.  Rows added to (d), to see whether
// more reads in flight would help it (LEDGER, "reads in flight"):
//   res N   the LDS table padded or shrunk so that N = 2..8 blocks fit a CU (the occupancy query's count is printed beside the row)
//   -bot    without the barrier at the bottom of the chunk loop, which guards nothing when a block takes one chunk
//   (e)     emit with two barriers: the unshifted words go to LDS behind the word in front of the chunk (slot 0, from the 8 bytes in
//           front of the chunk, loaded by lane 0 with the chunk's own loads); the drain reads words i and i + 1 and funnel-shifts them
//           itself, with no exchange between wavefronts.  Once with its 16-byte stores dword-aligned as in (b), once 16-byte-aligned
//           with a narrow head and tail
//   (2c)    a block issues the loads of two chunks before its first barrier: 16 KiB in flight a block, half the blocks and tables
// Median of ten launches after three warm-ups.  build: hipcc --offload-arch=gfx950 -O3 -o flat_stream_probe flat_stream_probe.cpp ; run: ./flat_stream_probe [MiB]
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define CK(x) do { hipError_t e__ = (x); if (e__ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e__)); exit(2); } } while (0)

typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));
constexpr int B = 256, L = 7, SPL = 32;          // lanes a block, words per lane's 32 symbols, symbols a lane
constexpr int CHUNK = B * SPL, UNIT = 64 * SPL;  // symbols per block chunk (b), per wavefront unit (c)

__device__ __forceinline__ uint32_t swz(uint32_t j) { return j + (j >> 5); }

// ---- (a): unit i of 16 bytes on the wide side <-> unit i - i/8 on the narrow side (every eighth unit has no partner)
__global__ void emit_a(const uint4 *in, uint32_t *outw, size_t units) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < units; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 v = in[i];
        if ((i & 7) != 7) { u32x4_a4 x = {v.x, v.y, v.z, v.w}; *reinterpret_cast<u32x4_a4 *>(outw + (i - (i >> 3)) * 4) = x; }
    }
}
__global__ void dec_a(const uint32_t *inw, uint4 *out, size_t units) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < units; i += (size_t)gridDim.x * blockDim.x) {
        u32x4_a4 x = {0, 0, 0, 0};
        if ((i & 7) != 7) x = *reinterpret_cast<const u32x4_a4 *>(inw + (i - (i >> 3)) * 4);
        out[i] = make_uint4(x.x, x.y, x.z, x.w);
    }
}

// ---- (b): block chunks between block barriers
// (TABW: words of the table; at most 4096 of them are written.  BOTTOM = false only with one chunk a block)
template <int TABW = 4096, bool BOTTOM = true>
__global__ __launch_bounds__(B) void emit_b(const uint8_t *in, uint32_t *outw, uint32_t chunks, int never) {
    __shared__ uint32_t s_tab[TABW], s_o[B * L + B * L / 32 + 2], s_last[B / 64];
    const int tid = threadIdx.x;
    for (int i = tid; i < (TABW < 4096 ? TABW : 4096); i += B) s_tab[i] = i;
    __syncthreads();
    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint4 *src = reinterpret_cast<const uint4 *>(in + (size_t)c * CHUNK + (size_t)tid * SPL);
        const uint4 x = src[0], y = src[1];
        uint32_t v[L] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z ^ y.w};
        if ((tid & 63) == 63) s_last[tid >> 6] = v[L - 1];
        __syncthreads();
        if ((tid & 63) == 0 && tid) v[0] ^= s_last[(tid >> 6) - 1];
#pragma unroll
        for (int j = 0; j < L; j++) s_o[swz(tid * L + j)] = v[j];
        __syncthreads();
        uint32_t *dst = outw + (size_t)c * (B * L);
        for (int q = tid; q < B * L / 4; q += B) {
            const uint32_t *sp = s_o + swz(4 * q);
            u32x4_a4 o = {sp[0], sp[1], sp[2], sp[3]};
            *reinterpret_cast<u32x4_a4 *>(dst + 4 * q) = o;
        }
        if (BOTTOM) __syncthreads();
    }
    if (never) outw[tid] = s_tab[(uint32_t)(tid * never) % TABW];
}
template <int TABW = 4096, bool BOTTOM = true>
__global__ __launch_bounds__(B) void dec_b(const uint32_t *inw, uint8_t *out, uint32_t chunks, int never) {
    constexpr int WORDS = B * L + 2;
    __shared__ uint32_t s_tab[TABW], s_d[WORDS + WORDS / 32 + 2];
    const int tid = threadIdx.x;
    for (int i = tid; i < (TABW < 4096 ? TABW : 4096); i += B) s_tab[i] = i;
    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint32_t *src = inw + (size_t)c * (B * L);
        constexpr int PER = (WORDS + B - 1) / B;
        uint32_t v[PER];
#pragma unroll
        for (int k = 0; k < PER; k++) { const int i = tid + k * B; if (i < WORDS) v[k] = src[i]; }
#pragma unroll
        for (int k = 0; k < PER; k++) { const int i = tid + k * B; if (i < WORDS) s_d[swz(i)] = v[k]; }
        __syncthreads();
        uint32_t w[L + 1];
#pragma unroll
        for (int j = 0; j <= L; j++) w[j] = s_d[swz(tid * L + j)];
        uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)c * CHUNK + (size_t)tid * SPL);
        dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
        dst[1] = make_uint4(w[4], w[5], w[6], w[7] ^ w[0]);
        if (BOTTOM) __syncthreads();
    }
    if (never) out[tid] = (uint8_t)s_tab[(uint32_t)(tid * never) % TABW];
}

// ---- (e): emit in two barriers, the funnel shift by o0 on the drain side.  s_o[0] is the word in front of the chunk.
template <int TABW, bool A16>
__global__ __launch_bounds__(B) void emit_e(const uint8_t *in, uint32_t *outw, uint32_t chunks, uint32_t o0, int never) {
    constexpr int SO = B * L + 1;
    __shared__ uint32_t s_tab[TABW], s_o[SO + SO / 32 + 2];
    const int tid = threadIdx.x;
    for (int i = tid; i < (TABW < 4096 ? TABW : 4096); i += B) s_tab[i] = i;
    __syncthreads();
    for (uint32_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint4 *src = reinterpret_cast<const uint4 *>(in + (size_t)c * CHUNK + (size_t)tid * SPL);
        const uint4 x = src[0], y = src[1];
        uint32_t prev = 0;
        if (tid == 0 && c) { const uint2 p = *reinterpret_cast<const uint2 *>(in + (size_t)c * CHUNK - 8); prev = p.x ^ p.y; }
        uint32_t v[L] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z ^ y.w};
        if (tid == 0) s_o[0] = prev;
#pragma unroll
        for (int j = 0; j < L; j++) s_o[swz(1 + tid * L + j)] = v[j];
        __syncthreads();
        uint32_t *dst = outw + (size_t)c * (B * L);
        auto word = [&](int i) { return (uint32_t)((((unsigned long long)s_o[swz(i)] << 32) | s_o[swz(i + 1)]) >> o0); };
        auto four = [&](int i, uint32_t *o) {
            uint32_t w[5];
#pragma unroll
            for (int k = 0; k < 5; k++) w[k] = s_o[swz(i + k)];
#pragma unroll
            for (int k = 0; k < 4; k++) o[k] = (uint32_t)((((unsigned long long)w[k] << 32) | w[k + 1]) >> o0);
        };
        if (A16) {
            const int head = (int)((4 - ((reinterpret_cast<uintptr_t>(dst) >> 2) & 3)) & 3);   // words in front of the first 16-byte line
            const int nfull = (B * L - head) / 4, tail = B * L - head - 4 * nfull;
            for (int q = tid; q < nfull; q += B) {
                uint32_t o[4]; four(head + 4 * q, o);
                *reinterpret_cast<uint4 *>(dst + head + 4 * q) = make_uint4(o[0], o[1], o[2], o[3]);
            }
            if (tid < head) dst[tid] = word(tid);
            else if (tid < head + tail) dst[4 * nfull + tid] = word(4 * nfull + tid);
        } else {
            for (int q = tid; q < B * L / 4; q += B) {
                uint32_t o[4]; four(4 * q, o);
                u32x4_a4 ov = {o[0], o[1], o[2], o[3]};
                *reinterpret_cast<u32x4_a4 *>(dst + 4 * q) = ov;
            }
        }
        __syncthreads();
    }
    if (never) outw[tid] = s_tab[(uint32_t)(tid * never) % TABW];
}

// ---- (2c): the loads of two chunks before the first barrier, one LDS image each
template <int TABW>
__global__ __launch_bounds__(B) void emit_2c(const uint8_t *in, uint32_t *outw, uint32_t chunks, int never) {
    constexpr int SO = B * L + B * L / 32 + 2;
    __shared__ uint32_t s_tab[TABW], s_o[2][SO], s_last[2][B / 64];
    const int tid = threadIdx.x;
    for (int i = tid; i < (TABW < 4096 ? TABW : 4096); i += B) s_tab[i] = i;
    __syncthreads();
    for (uint32_t c = 2 * blockIdx.x; c < chunks; c += 2 * gridDim.x) {
        const int nc = c + 1 < chunks ? 2 : 1;                  // (block-uniform)
        uint4 x[2], y[2];
#pragma unroll
        for (int h = 0; h < 2; h++) if (h < nc) {
            const uint4 *src = reinterpret_cast<const uint4 *>(in + (size_t)(c + h) * CHUNK + (size_t)tid * SPL);
            x[h] = src[0]; y[h] = src[1];
        }
        uint32_t v[2][L];
#pragma unroll
        for (int h = 0; h < 2; h++) if (h < nc) {
            const uint32_t t[L] = {x[h].x, x[h].y, x[h].z, x[h].w, y[h].x, y[h].y, y[h].z ^ y[h].w};
#pragma unroll
            for (int j = 0; j < L; j++) v[h][j] = t[j];
            if ((tid & 63) == 63) s_last[h][tid >> 6] = v[h][L - 1];
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; h++) if (h < nc) {
            if ((tid & 63) == 0 && tid) v[h][0] ^= s_last[h][(tid >> 6) - 1];
#pragma unroll
            for (int j = 0; j < L; j++) s_o[h][swz(tid * L + j)] = v[h][j];
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; h++) if (h < nc) {
            uint32_t *dst = outw + (size_t)(c + h) * (B * L);
            for (int q = tid; q < B * L / 4; q += B) {
                const uint32_t *sp = s_o[h] + swz(4 * q);
                u32x4_a4 o = {sp[0], sp[1], sp[2], sp[3]};
                *reinterpret_cast<u32x4_a4 *>(dst + 4 * q) = o;
            }
        }
        __syncthreads();
    }
    if (never) outw[tid] = s_tab[(uint32_t)(tid * never) % TABW];
}
template <int TABW>
__global__ __launch_bounds__(B) void dec_2c(const uint32_t *inw, uint8_t *out, uint32_t chunks, int never) {
    constexpr int WORDS = B * L + 2, PER = (WORDS + B - 1) / B;
    __shared__ uint32_t s_tab[TABW], s_d[2][WORDS + WORDS / 32 + 2];
    const int tid = threadIdx.x;
    for (int i = tid; i < (TABW < 4096 ? TABW : 4096); i += B) s_tab[i] = i;
    for (uint32_t c = 2 * blockIdx.x; c < chunks; c += 2 * gridDim.x) {
        const int nc = c + 1 < chunks ? 2 : 1;
        uint32_t v[2][PER];
#pragma unroll
        for (int h = 0; h < 2; h++) if (h < nc) {
            const uint32_t *src = inw + (size_t)(c + h) * (B * L);
#pragma unroll
            for (int k = 0; k < PER; k++) { const int i = tid + k * B; if (i < WORDS) v[h][k] = src[i]; }
        }
#pragma unroll
        for (int h = 0; h < 2; h++) if (h < nc) {
#pragma unroll
            for (int k = 0; k < PER; k++) { const int i = tid + k * B; if (i < WORDS) s_d[h][swz(i)] = v[h][k]; }
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; h++) if (h < nc) {
            uint32_t w[L + 1];
#pragma unroll
            for (int j = 0; j <= L; j++) w[j] = s_d[h][swz(tid * L + j)];
            uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)(c + h) * CHUNK + (size_t)tid * SPL);
            dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
            dst[1] = make_uint4(w[4], w[5], w[6], w[7] ^ w[0]);
        }
        __syncthreads();
    }
    if (never) out[tid] = (uint8_t)s_tab[(uint32_t)(tid * never) % TABW];
}

// ---- (c): wavefront units, no block barrier in the loop
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__global__ __launch_bounds__(B) void emit_c(const uint8_t *in, uint32_t *outw, uint32_t units, int never) {
    constexpr int UW = 64 * L;
    __shared__ uint32_t s_tab[4096], s_o[B / 64][UW + UW / 32 + 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < 4096; i += B) s_tab[i] = i;
    __syncthreads();
    uint32_t *so = s_o[wv];
    uint32_t carry = 0;
    for (uint32_t u = blockIdx.x * (B / 64) + wv; u < units; u += gridDim.x * (B / 64)) {
        const uint4 *src = reinterpret_cast<const uint4 *>(in + (size_t)u * UNIT + (size_t)lane * SPL);
        const uint4 x = src[0], y = src[1];
        uint32_t v[L] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z ^ y.w};
        if (lane == 0) v[0] ^= carry;
        carry = (uint32_t)__builtin_amdgcn_readlane((int)v[L - 1], 63);
#pragma unroll
        for (int j = 0; j < L; j++) so[swz(lane * L + j)] = v[j];
        wave_sync();
        uint32_t *dst = outw + (size_t)u * UW;
#pragma unroll
        for (int k = 0; k < (UW / 4 + 63) / 64; k++) {
            const int i = 4 * (lane + 64 * k);
            if (i < UW) {
                const uint32_t *sp = so + swz(i);
                u32x4_a4 o = {sp[0], sp[1], sp[2], sp[3]};
                *reinterpret_cast<u32x4_a4 *>(dst + i) = o;
            }
        }
        wave_sync();
    }
    if (never) outw[tid] = s_tab[(tid * never) & 4095];
}
__global__ __launch_bounds__(B) void dec_c(const uint32_t *inw, uint8_t *out, uint32_t units, int never) {
    constexpr int WORDS = 64 * L + 1;
    __shared__ uint32_t s_tab[4096], s_d[B / 64][WORDS + WORDS / 32 + 1];
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    for (int i = tid; i < 4096; i += B) s_tab[i] = i;
    __syncthreads();
    uint32_t *sd = s_d[wv];
    for (uint32_t u = blockIdx.x * (B / 64) + wv; u < units; u += gridDim.x * (B / 64)) {
        const uint32_t *src = inw + (size_t)u * (64 * L);
        uint32_t v[L + 1];
#pragma unroll
        for (int k = 0; k < L; k++) v[k] = src[lane + 64 * k];
        if (lane == 0) v[L] = src[64 * L];
#pragma unroll
        for (int k = 0; k < L; k++) sd[swz(lane + 64 * k)] = v[k];
        if (lane == 0) sd[swz(64 * L)] = v[L];
        wave_sync();
        uint32_t w[L + 1];
#pragma unroll
        for (int j = 0; j <= L; j++) w[j] = sd[swz(lane * L + j)];
        uint4 *dst = reinterpret_cast<uint4 *>(out + (size_t)u * UNIT + (size_t)lane * SPL);
        dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
        dst[1] = make_uint4(w[4], w[5], w[6], w[7] ^ w[0]);
        wave_sync();
    }
    if (never) out[tid] = (uint8_t)s_tab[(tid * never) & 4095];
}

template <class F> static double median_ms(F launch) {
    hipEvent_t a, b; CK(hipEventCreate(&a)); CK(hipEventCreate(&b));
    for (int i = 0; i < 3; i++) launch();
    CK(hipDeviceSynchronize());
    std::vector<float> t(10);
    for (float &x : t) { CK(hipEventRecord(a)); launch(); CK(hipEventRecord(b)); CK(hipEventSynchronize(b)); CK(hipGetLastError()); CK(hipEventElapsedTime(&x, a, b)); }
    std::sort(t.begin(), t.end());
    return 0.5 * (t[4] + t[5]);
}

template <class K> static int per_cu(K k) {
    int n = 0;
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, k, B, 0));
    return n;
}
template <class K> static int resident(K k) {
    int per_cu = 0, cus = 0;
    CK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k, B, 0));
    CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    return per_cu * cus;
}

int main(int argc, char **argv) {
    const size_t mib = argc > 1 ? (size_t)atol(argv[1]) : 1024;
    const size_t N = mib << 20, NARROW = N / 8 * L;            // N is a multiple of CHUNK: whole chunks and units only
    const size_t SLACK = 4096;                                  // the look-ahead words of the last chunk / unit, and the dword offset
    uint8_t *wide, *narrow;
    CK(hipMalloc(&wide, N + SLACK)); CK(hipMalloc(&narrow, NARROW + SLACK));
    CK(hipMemset(wide, 0x55, N + SLACK)); CK(hipMemset(narrow, 0x33, NARROW + SLACK));
    uint32_t *nw = reinterpret_cast<uint32_t *>(narrow) + 1;    // dword-aligned, not 16-aligned: where a payload starts
    const uint32_t chunks = (uint32_t)(N / CHUNK), units = (uint32_t)(N / UNIT);
    const size_t u16 = N / 16;
    const double bytes = (double)N + (double)NARROW;
    int cus = 0; CK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0));
    const int ga = cus * 8, geb = resident(emit_b<>), gdb = resident(dec_b<>), gec = resident(emit_c), gdc = resident(dec_c);
    auto grid = [](int g, size_t work) { return dim3((uint32_t)std::min<size_t>((size_t)g, work)); };
    struct Row { const char *name; double ms; int blocks; } rows[] = {
        {"emit (a) 16-byte grid-stride copy", median_ms([&] { emit_a<<<ga, B>>>(reinterpret_cast<const uint4 *>(wide), nw, u16); }), ga},
        {"emit (b) block chunks, 3 barriers", median_ms([&] { emit_b<><<<grid(geb, chunks), B>>>(wide, nw, chunks, 0); }), geb},
        {"emit (c) wavefront units, none   ", median_ms([&] { emit_c<<<grid(gec, units / 4), B>>>(wide, nw, units, 0); }), gec},
        {"emit (d) (b), one chunk a block  ", median_ms([&] { emit_b<><<<chunks, B>>>(wide, nw, chunks, 0); }), (int)chunks},
        {"dec  (a) 16-byte grid-stride copy", median_ms([&] { dec_a<<<ga, B>>>(nw, reinterpret_cast<uint4 *>(wide), u16); }), ga},
        {"dec  (b) block chunks, 2 barriers", median_ms([&] { dec_b<><<<grid(gdb, chunks), B>>>(nw, wide, chunks, 0); }), gdb},
        {"dec  (c) wavefront units, none   ", median_ms([&] { dec_c<<<grid(gdc, units / 4), B>>>(nw, wide, units, 0); }), gdc},
        {"dec  (d) (b), one chunk a block  ", median_ms([&] { dec_b<><<<chunks, B>>>(nw, wide, chunks, 0); }), (int)chunks},
    };
    printf("# flat_stream_probe: N = %zu MiB wide, %zu MiB narrow at a dword-aligned address, %d CUs; median of 10 launches after 3 warm-ups\n", mib, NARROW >> 20, cus);
    for (const Row &r : rows) printf("%s  blocks %6d  %.4f ms  %.2f TB/s\n", r.name, r.blocks, r.ms, bytes / (r.ms * 1e-3) / 1e12);
    // ---- rows added to (d): one chunk a block (two for 2c), the resident blocks a CU from the occupancy query
    const uint32_t o0 = 8;                                      // the phase of a headline stream is a whole byte; any non-zero value shifts
    const uint32_t pairs = (chunks + 1) / 2;
    struct Row2 { const char *name; double ms; int per_cu; };
#define EMIT_D(T, BOT) {"emit (d) " #T " table words, bottom barrier " #BOT, median_ms([&] { emit_b<T, BOT><<<chunks, B>>>(wide, nw, chunks, 0); }), per_cu(emit_b<T, BOT>)}
#define DEC_D(T, BOT) {"dec  (d) " #T " table words, bottom barrier " #BOT, median_ms([&] { dec_b<T, BOT><<<chunks, B>>>(nw, wide, chunks, 0); }), per_cu(dec_b<T, BOT>)}
#define EMIT_E(T, A) {"emit (e) " #T " table words, 16-aligned " #A, median_ms([&] { emit_e<T, A><<<chunks, B>>>(wide, nw, chunks, o0, 0); }), per_cu(emit_e<T, A>)}
#define EMIT_2C(T) {"emit (2c) " #T " table words", median_ms([&] { emit_2c<T><<<pairs, B>>>(wide, nw, chunks, 0); }), per_cu(emit_2c<T>)}
#define DEC_2C(T) {"dec  (2c) " #T " table words", median_ms([&] { dec_2c<T><<<pairs, B>>>(nw, wide, chunks, 0); }), per_cu(dec_2c<T>)}
    const Row2 rows2[] = {
        EMIT_D(13312, true), EMIT_D(10240, true), EMIT_D(7168, true), EMIT_D(5632, true), EMIT_D(4096, true), EMIT_D(3584, true), EMIT_D(3072, true), EMIT_D(4096, false), EMIT_D(3072, false),
        EMIT_E(4096, false), EMIT_E(4096, true), EMIT_E(3072, false), EMIT_E(3072, true),
        EMIT_2C(8192), EMIT_2C(6144), EMIT_2C(4096), EMIT_2C(2048), EMIT_2C(1024),
        DEC_D(10240, true), DEC_D(7168, true), DEC_D(5632, true), DEC_D(4096, true), DEC_D(3584, true), DEC_D(3072, true), DEC_D(4096, false), DEC_D(3072, false),
        DEC_2C(4096), DEC_2C(2048), DEC_2C(1024),
    };
    printf("# rows added to (d): [table words, bottom barrier] / (e) two-barrier emit [table words, 16-byte-aligned stores] / (2c) two chunks' loads a block\n");
    for (const Row2 &r : rows2) printf("%-52s  resident a CU %d  %.4f ms  %.2f TB/s\n", r.name, r.per_cu, r.ms, bytes / (r.ms * 1e-3) / 1e12);
    CK(hipFree(wide)); CK(hipFree(narrow));
    return 0;
}
