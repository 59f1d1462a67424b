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
// (b) and (c) carry a 16 KiB table in LDS so that as many blocks fit a CU as in the library.  Median of ten launches after three
// warm-ups.  build: hipcc --offload-arch=gfx950 -O3 -o flat_stream_probe flat_stream_probe.cpp ; run: ./flat_stream_probe [MiB]
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
__global__ __launch_bounds__(B) void emit_b(const uint8_t *in, uint32_t *outw, uint32_t chunks, int never) {
    __shared__ uint32_t s_tab[4096], s_o[B * L + B * L / 32 + 2], s_last[B / 64];
    const int tid = threadIdx.x;
    for (int i = tid; i < 4096; i += B) s_tab[i] = i;
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
        __syncthreads();
    }
    if (never) outw[tid] = s_tab[(tid * never) & 4095];
}
__global__ __launch_bounds__(B) void dec_b(const uint32_t *inw, uint8_t *out, uint32_t chunks, int never) {
    constexpr int WORDS = B * L + 2;
    __shared__ uint32_t s_tab[4096], s_d[WORDS + WORDS / 32 + 2];
    const int tid = threadIdx.x;
    for (int i = tid; i < 4096; i += B) s_tab[i] = i;
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
        __syncthreads();
    }
    if (never) out[tid] = (uint8_t)s_tab[(tid * never) & 4095];
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
    const int ga = cus * 8, geb = resident(emit_b), gdb = resident(dec_b), gec = resident(emit_c), gdc = resident(dec_c);
    auto grid = [](int g, size_t work) { return dim3((uint32_t)std::min<size_t>((size_t)g, work)); };
    struct Row { const char *name; double ms; int blocks; } rows[] = {
        {"emit (a) 16-byte grid-stride copy", median_ms([&] { emit_a<<<ga, B>>>(reinterpret_cast<const uint4 *>(wide), nw, u16); }), ga},
        {"emit (b) block chunks, 3 barriers", median_ms([&] { emit_b<<<grid(geb, chunks), B>>>(wide, nw, chunks, 0); }), geb},
        {"emit (c) wavefront units, none   ", median_ms([&] { emit_c<<<grid(gec, units / 4), B>>>(wide, nw, units, 0); }), gec},
        {"emit (d) (b), one chunk a block  ", median_ms([&] { emit_b<<<chunks, B>>>(wide, nw, chunks, 0); }), (int)chunks},
        {"dec  (a) 16-byte grid-stride copy", median_ms([&] { dec_a<<<ga, B>>>(nw, reinterpret_cast<uint4 *>(wide), u16); }), ga},
        {"dec  (b) block chunks, 2 barriers", median_ms([&] { dec_b<<<grid(gdb, chunks), B>>>(nw, wide, chunks, 0); }), gdb},
        {"dec  (c) wavefront units, none   ", median_ms([&] { dec_c<<<grid(gdc, units / 4), B>>>(nw, wide, units, 0); }), gdc},
        {"dec  (d) (b), one chunk a block  ", median_ms([&] { dec_b<<<chunks, B>>>(nw, wide, chunks, 0); }), (int)chunks},
    };
    printf("# flat_stream_probe: N = %zu MiB wide, %zu MiB narrow at a dword-aligned address, %d CUs; median of 10 launches after 3 warm-ups\n", mib, NARROW >> 20, cus);
    for (const Row &r : rows) printf("%s  blocks %6d  %.4f ms  %.2f TB/s\n", r.name, r.blocks, r.ms, bytes / (r.ms * 1e-3) / 1e12);
    CK(hipFree(wide)); CK(hipFree(narrow));
    return 0;
}
