// layers_batch.hip -- k_members_move, the one kernel of the layered batch calls (rsn.h: rsn_layers_*_batch, rsn_layers_*_batch_dev;
// DESIGN 4.11).  The steps of such a call leave every member at the front of a slot sized for the worst case; this kernel moves the
// members' actual bytes -- into one packed region that goes down in one copy (the host form), or into the callers' buffers (the device
// form without layers).  The flow itself is rsn_api.hip's layers_batch.
#include "codecs.h"
#include "layers_batch_layout.h"

namespace rsn {

namespace {

constexpr int MV_THREADS = 256;
static_assert(sizeof(MoveEntry) == 24, "the move table: three 8-byte words an entry");

// A workgroup per table entry, an entry per tile of at most LB_TILE bytes (the host cuts a member into its tiles, so a large member is
// spread over the CUs): whole 16-byte units, four a thread in flight, then the tail byte by byte.  src and dst are 16-byte aligned.
// Never a byte at or behind dst + len; nothing is loaded at or behind src + len rounded up to 16 (the tail is read byte by byte as well).
__global__ __launch_bounds__(MV_THREADS) void k_members_move(const MoveEntry *__restrict__ tab) {
    const MoveEntry e = tab[blockIdx.x];
    const uint4 *__restrict__ src = reinterpret_cast<const uint4 *>(e.src);
    uint4 *__restrict__ dst = reinterpret_cast<uint4 *>(e.dst);
    const uint32_t len = (uint32_t)e.len, full = len / 16;
    uint32_t u = threadIdx.x;
    for (; u + 3 * MV_THREADS < full; u += 4 * MV_THREADS) {
        const uint4 a = src[u], b = src[u + MV_THREADS], c2 = src[u + 2 * MV_THREADS], d = src[u + 3 * MV_THREADS];
        dst[u] = a; dst[u + MV_THREADS] = b; dst[u + 2 * MV_THREADS] = c2; dst[u + 3 * MV_THREADS] = d;
    }
    for (; u < full; u += MV_THREADS) dst[u] = src[u];
    const uint32_t i = full * 16 + threadIdx.x;
    if (threadIdx.x < 16 && i < len) e.dst[i] = e.src[i];
}

}  // namespace

int members_move(Ctx &c, hipStream_t s, const MoveEntry *h_tab, MoveEntry *d_tab, size_t tiles) {
    if (tiles == 0) return RSN_OK;
    if (tiles > 0x7FFFFFFFull) return c.fail(RSN_ERR_LIMIT, "layers: %zu tiles to move in one launch", tiles);
    for (size_t t = 0; t < tiles; t++)
        if (h_tab[t].len == 0 || h_tab[t].len > LB_TILE || (((uintptr_t)h_tab[t].src | (uintptr_t)h_tab[t].dst) & 15))
            return c.fail(RSN_ERR_DEVICE, "layers: internal error: tile %zu of the move table (%zu bytes) is not one", t, (size_t)h_tab[t].len);
    RSN_HIP(copy_async(d_tab, h_tab, tiles * sizeof(MoveEntry), hipMemcpyHostToDevice, s));
    RSN_LAUNCH("members_move", k_members_move, dim3((uint32_t)tiles), dim3(MV_THREADS), 0, s, (const MoveEntry *)d_tab);
    return RSN_OK;
}

}  // namespace rsn
