// rsn_api.hip -- extern "C" surface of librsn (include/rsn.h) and the per-thread
// context.  Host-buffer entry points stage through device memory and call the
// device-resident codecs; there is no CPU compute path.
#include "codecs.h"
#include "dev_ranges.h"
#include "layers_batch_layout.h"
#include "roundtrip_batch_layout.h"
#include "suite_layout.h"
#include "group_layout.h"
#include "rsn_common.h"
#include "rsn_helpers.h"

#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

namespace rsn {

namespace {
int env_int(const char *name, int dflt) { const char *e = getenv(name); return e && *e ? atoi(e) : dflt; }
std::atomic<size_t> g_arena_bytes[64];                                   // device scratch held by all contexts of the process, per device
}  // namespace

Ctx &ctx() {
    static thread_local Ctx c;
    return c;
}

// A thread that exits leaves its stream, scratch buffers and pinned staging behind for the next
// thread that needs a context on the same device: nothing leaks when callers come and go (a Go
// runtime retires OS threads), and no HIP call runs inside a thread-exit or process-exit destructor.
namespace {
struct Parked {
    int device; hipStream_t stream; Ctx::Buf bufs[Ctx::N_BUFS]; void *pinned; size_t pinned_cap; std::vector<hipEvent_t> events;
};
std::mutex g_park_mu;
std::vector<Parked> *g_parked = nullptr;      // heap-allocated and never destroyed: still valid while other threads unwind at exit

void release_parked(Parked &pk) {              // (HIP calls: only from a live thread, never from a thread-exit destructor)
    if (hipSetDevice(pk.device) != hipSuccess) return;
    for (auto &b : pk.bufs) if (b.p) { (void)hipFree(b.p); g_arena_bytes[pk.device & 63] -= b.cap; }
    if (pk.pinned) (void)hipHostFree(pk.pinned);
    for (auto e : pk.events) (void)hipEventDestroy(e);
    if (pk.stream) (void)hipStreamDestroy(pk.stream);
}

// A storm of short-lived caller threads (a Go runtime under load retires and creates OS threads) must not leave an unbounded
// number of parked scratch arenas in HBM: beyond RSN_MAX_PARKED the OLDEST ones are released by the next thread that initialises
// a context.
// (default: 8 plus three per visible device -- a batch call over G devices retires an uploader, an encoder and a downloader thread per device,
//  and the next batch wants their rings back)
size_t max_parked() {
    static const size_t v = [] {
        if (getenv("RSN_MAX_PARKED")) return (size_t)std::max(0, atoi(getenv("RSN_MAX_PARKED")));
        int cnt = 0;
        if (hipGetDeviceCount(&cnt) != hipSuccess || cnt < 0) cnt = 0;
        return (size_t)(8 + 3 * cnt);
    }();
    return v;
}

void trim_parked_excess(int restore_device) {
    std::vector<Parked> victims;
    {
        std::lock_guard<std::mutex> lk(g_park_mu);
        if (!g_parked) return;
        while (g_parked->size() > max_parked()) { victims.push_back(std::move(g_parked->front())); g_parked->erase(g_parked->begin()); }
    }
    if (victims.empty()) return;
    for (auto &pk : victims) release_parked(pk);
    (void)hipSetDevice(restore_device);
}

// The device of a thread that never called rsn_device_set(): 0, or RSN_DEVICE=<n>; RSN_DEVICE=rr hands the visible devices
// out round-robin, one per new thread context -- how a Go host whose goroutines land on different OS threads
// (runtime.LockOSThread in the shim) spreads its concurrent calls over the GPUs of a node without any API of its own.
std::atomic<unsigned> g_rr{0};
int default_device(int cnt) {
    const char *e = getenv("RSN_DEVICE");
    if (!e || !*e) return 0;
    if (!strcmp(e, "rr") || !strcmp(e, "all")) return (int)(g_rr.fetch_add(1) % (unsigned)cnt);
    return atoi(e);
}
}  // namespace

Ctx::~Ctx() {
    if (!inited) return;
    std::lock_guard<std::mutex> lk(g_park_mu);
    if (!g_parked) g_parked = new std::vector<Parked>();
    Parked pk;
    pk.device = device; pk.stream = own_stream; pk.pinned = pinned; pk.pinned_cap = pinned_cap;
    for (int i = 0; i < N_BUFS; i++) pk.bufs[i] = bufs[i];
    pk.events = free_events;
    for (auto &sl : slots) for (auto &pr : sl.pending) { pk.events.push_back(pr.first); pk.events.push_back(pr.second); }
    g_parked->push_back(std::move(pk));
}

int ctx_init(Ctx &c) {
    if (c.inited) {
        hipError_t e = hipSetDevice(c.device);
        if (e != hipSuccess) return c.fail(RSN_ERR_DEVICE, "hipSetDevice(%d): %s", c.device, hipGetErrorString(e));
        return RSN_OK;
    }
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0)
        return c.fail(RSN_ERR_DEVICE, "no HIP device available (%s); librsn has no CPU fallback", e != hipSuccess ? hipGetErrorString(e) : "device count 0");
    if (!c.device_chosen) { c.device = default_device(cnt); c.device_chosen = true; }
    if (c.device < 0 || c.device >= cnt) return c.fail(RSN_ERR_DEVICE, "device %d out of range (%d visible)", c.device, cnt);
    RSN_HIP(hipSetDevice(c.device));
    trim_parked_excess(c.device);
    {
        std::lock_guard<std::mutex> lk(g_park_mu);
        if (g_parked)
            for (size_t i = g_parked->size(); i-- > 0;)
                if ((*g_parked)[i].device == c.device) {                  // adopt what an earlier thread left behind (most recent first: its buffers are the warm ones)
                    Parked &pk = (*g_parked)[i];
                    if (c.pinned) (void)hipHostFree(c.pinned);              // a context that switched devices kept its staging: do not leak it
                    c.own_stream = pk.stream; c.pinned = pk.pinned; c.pinned_cap = pk.pinned_cap;
                    for (int k = 0; k < Ctx::N_BUFS; k++) c.bufs[k] = pk.bufs[k];
                    c.free_events = std::move(pk.events);
                    g_parked->erase(g_parked->begin() + (long)i);
                    c.inited = true;
                    return RSN_OK;
                }
    }
    RSN_HIP(hipStreamCreateWithFlags(&c.own_stream, hipStreamNonBlocking));
    c.inited = true;
    return RSN_OK;
}

// ---- admission of calls that need gigabytes of scratch (LZSS encode: ~12 bytes per position).  Every calling thread has an arena of
// its own, so 64 goroutines compressing 1 GiB files at once would ask for 64 x 12 GiB: instead of hipErrorOutOfMemory for most of
// them, a call states its need up front and WAITS while the needs of the calls in flight on its device add up to more than the
// device holds (RSN_SCRATCH_GIB, default 85 % of the device's memory); a call that finishes while others wait, or while the arenas
// on the device have grown past half of that, gives its large buffers back instead of keeping them for its thread's next call.
namespace {
struct ScratchGate { std::mutex mu; std::condition_variable cv; size_t cap = 0, in_flight = 0; int calls = 0, waiting = 0; unsigned long long queued = 0; };
ScratchGate g_gate[64];
}  // namespace

size_t scratch_admit(Ctx &c, size_t need) {
    if (c.gate_held || need == 0) return 0;                               // inside a host-buffer call that stated staging + codec scratch up front (host_call)
    ScratchGate &g = g_gate[c.device & 63];
    std::unique_lock<std::mutex> lk(g.mu);
    if (g.cap == 0) {
        const char *e = getenv("RSN_SCRATCH_GIB");
        size_t fr = 0, tot = 0;
        if (e && atof(e) > 0) g.cap = (size_t)(atof(e) * (double)((size_t)1 << 30));
        else if (hipMemGetInfo(&fr, &tot) == hipSuccess && tot) g.cap = tot / 100 * 85;
        else g.cap = (size_t)64 << 30;
    }
    if (g.calls > 0 && g.in_flight + need > g.cap) {                     // (a lone call always runs: its own allocation failing is the answer then)
        static const bool dbg = getenv("RSN_SCRATCH_DEBUG") != nullptr;
        g.waiting++; g.queued++;
        if (dbg) fprintf(stderr, "librsn: a call that needs %.2f GiB of scratch waits: %d in flight need %.2f of %.2f GiB\n", need / 1073741824.0, g.calls, g.in_flight / 1073741824.0, g.cap / 1073741824.0);
        g.cv.wait(lk, [&] { return g.calls == 0 || g.in_flight + need <= g.cap; });
        g.waiting--;
    }
    g.calls++; g.in_flight += need;
    c.gate_held = need;
    return need;
}

void scratch_release(Ctx &c, size_t need, unsigned long long slots) {
    if (need == 0) return;
    c.gate_held = 0;
    ScratchGate &g = g_gate[c.device & 63];
    bool give_back;
    {
        std::lock_guard<std::mutex> lk(g.mu);
        g.calls--; g.in_flight -= need;
        give_back = g.waiting > 0 || g_arena_bytes[c.device & 63].load() > g.cap / 2;
    }
    if (give_back && hipSetDevice(c.device) == hipSuccess) {
        for (int k = 0; k < Ctx::N_BUFS; k++) {
            if (!((slots >> k) & 1ull)) continue;
            Ctx::Buf &b = c.bufs[k];
            if (b.p && b.cap >= ((size_t)64 << 20)) { (void)hipFree(b.p); g_arena_bytes[c.device & 63] -= b.cap; b.p = nullptr; b.cap = 0; }
        }
    }
    g.cv.notify_all();
}

void scratch_forget(Ctx &c, size_t bytes) { g_arena_bytes[c.device & 63] -= bytes; }
unsigned long long scratch_queued(int device) { ScratchGate &g = g_gate[device & 63]; std::lock_guard<std::mutex> lk(g.mu); return g.queued; }

// the calling thread's scratch and staging back to the device / the host (rsn_trim; an idle helper when memory runs out)
static void trim_own_context() {
    Ctx &c = ctx();
    if (c.inited && hipSetDevice(c.device) == hipSuccess) {
        (void)hipStreamSynchronize(c.own_stream);
        for (auto &b : c.bufs) { if (b.p) { (void)hipFree(b.p); g_arena_bytes[c.device & 63] -= b.cap; } b.p = nullptr; b.cap = 0; }
        if (c.pinned) (void)hipHostFree(c.pinned);
        c.pinned = nullptr; c.pinned_cap = 0;
    }
}

int dev_buf(Ctx &c, Slot slot, size_t bytes, void **out) {
    Ctx::Buf &b = c.buf(slot);
    if (bytes > b.cap) {
        if (b.p) { RSN_HIP(hipFree(b.p)); g_arena_bytes[c.device & 63] -= b.cap; b.p = nullptr; b.cap = 0; }
        const size_t want = round_up(bytes + bytes / 8, 4096);
        hipError_t e = hipMalloc(&b.p, want);
        if (e != hipSuccess) {                                            // what exited threads left parked on the device goes first, then once more
            (void)hipGetLastError();
            std::vector<Parked> victims;
            { std::lock_guard<std::mutex> lk(g_park_mu); if (g_parked) victims.swap(*g_parked); }
            for (auto &pk : victims) release_parked(pk);
            HelperPool::on_idle(trim_own_context);                        // (r06: idle helpers of the pipelined calls keep contexts of their own for half a minute)
            (void)hipSetDevice(c.device);
            e = hipMalloc(&b.p, want);
        }
        if (e != hipSuccess) { b.p = nullptr; return c.fail(RSN_ERR_NOMEM, "hipMalloc(%zu): %s", want, hipGetErrorString(e)); }
        b.cap = want;
        static std::atomic<unsigned long long> next_gen{0};
        b.gen = ++next_gen;
        g_arena_bytes[c.device & 63] += want;
    }
    *out = b.p;
    return RSN_OK;
}

int pinned_buf(Ctx &c, size_t bytes, void **out) {
    if (bytes > c.pinned_cap) {
        if (c.pinned) { RSN_HIP(hipHostFree(c.pinned)); c.pinned = nullptr; c.pinned_cap = 0; }
        hipError_t e = hipHostMalloc(&c.pinned, bytes, hipHostMallocDefault);
        if (e != hipSuccess) { c.pinned = nullptr; return c.fail(RSN_ERR_NOMEM, "hipHostMalloc(%zu): %s", bytes, hipGetErrorString(e)); }
        c.pinned_cap = bytes;
    }
    *out = c.pinned;
    return RSN_OK;
}

int func_dyn_lds(Ctx &c, const void *fn, size_t bytes) {
    static std::mutex mu;
    static std::vector<std::pair<std::pair<const void *, int>, size_t>> *seen = new std::vector<std::pair<std::pair<const void *, int>, size_t>>();
    std::lock_guard<std::mutex> lk(mu);
    for (auto &e : *seen)
        if (e.first.first == fn && e.first.second == c.device) {
            if (bytes <= e.second) return RSN_OK;
            RSN_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
            e.second = bytes;
            return RSN_OK;
        }
    RSN_HIP(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    seen->push_back({{fn, c.device}, bytes});
    return RSN_OK;
}

void prof_collect(Ctx &c) {
    for (auto &sl : c.slots) {
        for (auto &pr : sl.pending) {
            float ms = 0;
            if (hipEventSynchronize(pr.second) == hipSuccess && hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) {
                sl.total_ms += ms;
                sl.launches++;
            }
            c.free_events.push_back(pr.first);
            c.free_events.push_back(pr.second);
        }
        sl.pending.clear();
    }
}

namespace {

// Result buffers.  A fresh 1 GiB malloc costs ~150 ms of page faults when the D2H copy first
// touches it -- several times the PCIe transfer itself -- so blocks of 1 MiB and more go back
// to a small process-wide pool on rsn_free() and the next call of similar size reuses pages
// that are already mapped (the cgo shim's pattern: call, C.GoBytes, rsn_free).  A 64-byte header
// in front of the returned pointer carries the capacity.
constexpr size_t RES_HDR = 64, POOL_MIN = 1u << 20;
constexpr size_t POOL_BLOCKS = 12;      // a batch of 8 chunks holds 8 results at once
struct ResHdr { unsigned long long magic, cap; };
constexpr unsigned long long RES_MAGIC = 0x52534E5F52455330ull;
std::mutex g_pool_mu;
std::vector<std::pair<size_t, void *>> g_pool;                    // (capacity, base)

void *result_alloc(size_t n) {
    const size_t need = n ? n : 1;
    if (need >= POOL_MIN) {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        size_t best = g_pool.size();
        for (size_t i = 0; i < g_pool.size(); i++)
            if (g_pool[i].first >= need && g_pool[i].first <= 2 * need + (16u << 20) && (best == g_pool.size() || g_pool[i].first < g_pool[best].first)) best = i;
        if (best != g_pool.size()) {
            void *base = g_pool[best].second;
            g_pool.erase(g_pool.begin() + (long)best);
            return (uint8_t *)base + RES_HDR;
        }
    }
    const bool big = need >= POOL_MIN;
    const size_t cap = big ? round_up(need + need / 16, (size_t)2 << 20) : need;   // headroom: the next result is rarely the same size
    void *base = nullptr;
    if (posix_memalign(&base, big ? ((size_t)2 << 20) : 64, cap + RES_HDR)) return nullptr;
    if (big) (void)madvise(base, cap + RES_HDR, MADV_HUGEPAGE);
    ResHdr *h = (ResHdr *)base;
    h->magic = RES_MAGIC; h->cap = cap;
    return (uint8_t *)base + RES_HDR;
}

void result_free(void *p) {
    if (!p) return;
    void *base = (uint8_t *)p - RES_HDR;
    const ResHdr *h = (const ResHdr *)base;
    if (h->magic != RES_MAGIC) { fprintf(stderr, "librsn: rsn_free() of a pointer librsn did not return\n"); return; }
    if (h->cap >= POOL_MIN) {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        if (g_pool.size() < POOL_BLOCKS) { g_pool.emplace_back((size_t)h->cap, base); return; }
        size_t small = 0;                                              // keep the largest blocks
        for (size_t i = 1; i < g_pool.size(); i++) if (g_pool[i].first < g_pool[small].first) small = i;
        if (g_pool[small].first < h->cap) { void *victim = g_pool[small].second; g_pool[small] = {(size_t)h->cap, base}; base = victim; }
    }
    ((ResHdr *)base)->magic = 0;
    free(base);
}

// ---- how a result reaches the caller.  HostBlock owns a block across the ways out of a call that can still fail; result_from_host /
// result_from_dev are the two deliveries -- a fresh block, the bytes into it (from the device: copied down and the stream synchronised),
// then *out / *out_n; t_alloc: the RSN_HOST_TIMING stamp between the allocation and the copy.  drop_results undoes a batch's.
struct HostBlock { uint8_t *p = nullptr; ~HostBlock() { if (p) result_free(p); } uint8_t *release() { uint8_t *r = p; p = nullptr; return r; } };
double now_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
int result_block(Ctx &c, size_t len, HostBlock &b) {
    b.p = (uint8_t *)result_alloc(len);
    return b.p ? RSN_OK : c.fail(RSN_ERR_NOMEM, "allocating %zu result bytes failed", len);
}
int result_from_host(Ctx &c, const void *p, size_t len, uint8_t **out, size_t *out_n) {
    HostBlock b;
    int rc = result_block(c, len, b); if (rc) return rc;
    if (len) memcpy(b.p, p, len);
    *out = b.release(); *out_n = len;
    return RSN_OK;
}
int result_from_dev(Ctx &c, hipStream_t s, const void *d_src, size_t len, uint8_t **out, size_t *out_n, double *t_alloc = nullptr) {
    HostBlock b;
    int rc = result_block(c, len, b); if (rc) return rc;
    if (t_alloc) *t_alloc = now_ms();
    if (len) {
        RSN_HIP(copy_async(b.p, d_src, len, hipMemcpyDeviceToHost, s));
        RSN_HIP(hipStreamSynchronize(s));
    }
    *out = b.release(); *out_n = len;
    return RSN_OK;
}
SmallTake take_into(Ctx &c, uint8_t **outs, size_t *out_lens) {
    return [&c, outs, out_lens](size_t i, const uint8_t *p, size_t len) { return result_from_host(c, p, len, &outs[i], &out_lens[i]); };
}
void drop_results(size_t n, uint8_t **outs, size_t *out_lens) {
    for (size_t k = 0; k < n; k++) { if (outs[k]) result_free(outs[k]); outs[k] = nullptr; out_lens[k] = 0; }
}

// ---- the argument checks of the host-buffer forms, before a device is looked for.  host_args: one buffer, *out / *out_n zeroed once the
// pointers are known to be there.  batch_args: the arrays, outs[] / out_lens[] zeroed, then the members in index order -- member_word:
// the message names the member; empty_first: a batch of none is answered (RSN_OK, the caller returns too) before the arrays are looked
// at; empty_member: what a member of length 0 fails with (RSN_ERR_EMPTY), or nullptr where it is a member like any other.
int host_args(Ctx &c, const uint8_t *in, size_t n, uint8_t **out, size_t *out_n) {
    if (!out || !out_n || (!in && n)) return c.fail(RSN_ERR_ARG, "null argument");
    *out = nullptr; *out_n = 0;
    return RSN_OK;
}
int batch_args(Ctx &c, size_t n, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens, bool member_word, bool empty_first,
               const char *empty_member = nullptr) {
    if (empty_first && n == 0) return RSN_OK;
    if (!ins || !lens || !outs || !out_lens) return c.fail(RSN_ERR_ARG, "null argument");
    for (size_t i = 0; i < n; i++) { outs[i] = nullptr; out_lens[i] = 0; }
    for (size_t i = 0; i < n; i++) {
        if (!ins[i] && lens[i]) return member_word ? c.fail(RSN_ERR_ARG, "member %zu: null argument", i) : c.fail(RSN_ERR_ARG, "null argument");
        if (empty_member && lens[i] == 0) return c.fail(RSN_ERR_EMPTY, "%s", empty_member);
    }
    return RSN_OK;
}

// ---- what a helper thread leaves for the thread that waits for it: the FIRST failure's code and text.  The pipes and the barrier below
// hold their shared state under `mu` and wake their waiters through `cv`.  on_helper: what runs ON a helper -- an exception there (a
// vector that cannot grow) fails P at once, and the other stages, which wait on P, end.
struct FirstFailure {
    std::mutex mu; std::condition_variable cv;
    int rc = RSN_OK; std::string msg;
    void fail(int code, const char *m) noexcept { try { std::lock_guard<std::mutex> lk(mu); if (rc == RSN_OK) { rc = code; try { msg = m; } catch (...) {} } } catch (...) {} cv.notify_all(); }
};
template <class Body> auto on_helper(FirstFailure &P, Body body) {
    return [&P, body] { guarded_call<int>([&] { body(); return 0; }, [&](int code, const char *m) { P.fail(code, m); return 0; }); };
}

// ---- the caller's INPUT memory, registered in place for the pipelined calls, under a process-wide table (r06).  The input is borrowed and
// read-only (rsn.h), so two goroutines may hand the SAME bytes to two calls at once -- decompressing one blob twice is legal -- and r05's
// per-call hipHostRegister / hipHostUnregister then failed in a way found by tests/test_gpu_host_pipeline.py::test_four_pipelined_calls_at_once:
// the second call's registration is refused (already registered), its copies run from memory the FIRST call has pinned, and the first call
// unregisters it under them ("pointer does not correspond to a registered memory region"; once an abort inside the runtime).  Here a range
// is registered once and counted: an identical range is shared, a call whose bytes merely OVERLAP registered ranges (a serial call's
// upload, another slicing of the same buffer) holds them for as long as it copies, and the last one out unregisters.
namespace {
struct PinRange { uintptr_t lo, hi; int refs; };
std::mutex g_pin_mu;
std::vector<PinRange> *g_pins = nullptr;                                 // (never destroyed: helpers may release at exit)
struct PinHold { std::vector<std::pair<uintptr_t, uintptr_t>> held; bool registered = false; };   // what one acquire took: release() gives it back

// [p, p + len): registers it (true in h.registered) unless something overlapping is registered already -- an identical range is shared
// (registered stays true: it IS pinned), any other overlap is held as it is (registered false: the copy takes what it finds)
void pin_acquire(const void *p, size_t len, bool want_register, PinHold &h) {
    if (!len) return;
    const uintptr_t lo = (uintptr_t)p, hi = lo + len;
    std::lock_guard<std::mutex> lk(g_pin_mu);
    if (!g_pins) g_pins = new std::vector<PinRange>();
    bool overlap = false;
    for (PinRange &r : *g_pins)
        if (r.lo < hi && lo < r.hi) {
            overlap = true;
            r.refs++;
            h.held.emplace_back(r.lo, r.hi);
            if (r.lo == lo && r.hi == hi) h.registered = true;
        }
    if (overlap || !want_register) return;
    if (hipHostRegister((void *)p, len, hipHostRegisterDefault) != hipSuccess) { (void)hipGetLastError(); return; }   // (memory some other library has registered, a mapping that cannot be pinned: copied as it is)
    g_pins->push_back(PinRange{lo, hi, 1});
    h.held.emplace_back(lo, hi);
    h.registered = true;
}
void pin_release(PinHold &h) {
    std::vector<uintptr_t> gone;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        if (g_pins)
            for (auto &pr : h.held)
                for (size_t i = 0; i < g_pins->size(); i++)
                    if ((*g_pins)[i].lo == pr.first && (*g_pins)[i].hi == pr.second) {
                        if (--(*g_pins)[i].refs == 0) { gone.push_back(pr.first); g_pins->erase(g_pins->begin() + (long)i); }
                        break;
                    }
    }
    h.held.clear(); h.registered = false;
    for (uintptr_t a : gone) if (hipHostUnregister((void *)a) != hipSuccess) (void)hipGetLastError();
}
struct PinGuard { PinHold h; ~PinGuard() { pin_release(h); } };         // a serial upload: holds what overlaps for as long as it copies
// host -> device of [src, src + len) whose pages may be PARTLY inside ranges other calls have registered (h.held, h.registered false): one
// copy command per stretch that lies wholly inside one registered range or wholly outside all of them -- a single command over memory of
// two kinds is decided by how its first byte is mapped
hipError_t copy_up(void *dst, const void *src, size_t len, hipStream_t st, const PinHold &h) {
    if (h.registered || h.held.empty()) return len ? copy_async(dst, src, len, hipMemcpyHostToDevice, st) : hipSuccess;
    const uintptr_t a = (uintptr_t)src, b = a + len;
    std::vector<uintptr_t> cuts{a, b};
    for (const auto &pr : h.held) { if (pr.first > a && pr.first < b) cuts.push_back(pr.first); if (pr.second > a && pr.second < b) cuts.push_back(pr.second); }
    std::sort(cuts.begin(), cuts.end());
    for (size_t i = 0; i + 1 < cuts.size(); i++) {
        if (cuts[i + 1] == cuts[i]) continue;
        const hipError_t e = copy_async((uint8_t *)dst + (cuts[i] - a), (const void *)cuts[i], cuts[i + 1] - cuts[i], hipMemcpyHostToDevice, st);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// A host buffer onto the device, the way every kernel expects its input.  stage_buf: `slot` grown to round_up(n, 16) + 64 bytes, the 64
// bytes from the last 16-byte boundary at or before n zeroed (the kernels' vector loads see zeros behind the data, not an earlier call's
// bytes).  stage_input: that, then the copy -- bytes another call has registered stay registered under it (PinGuard), and the stream is
// synchronised before they can be released.  Both fail with the message in c.err.
int stage_buf(Ctx &c, hipStream_t s, Slot slot, size_t n, void **d_in) {
    int rc = dev_buf(c, slot, round_up(n, 16) + 64, d_in); if (rc) return rc;
    RSN_HIP(hipMemsetAsync((uint8_t *)*d_in + (n & ~(size_t)15), 0, 64, s));
    return RSN_OK;
}
int stage_input(Ctx &c, hipStream_t s, Slot slot, const uint8_t *in, size_t n, void **d_in) {
    int rc = stage_buf(c, s, slot, n, d_in); if (rc) return rc;
    PinGuard g;
    pin_acquire(in, n, false, g.h);
    RSN_HIP(copy_up(*d_in, in, n, s, g.h));
    if (!g.h.held.empty()) RSN_HIP(hipStreamSynchronize(s));
    return RSN_OK;
}
}  // namespace

// Host-buffer wrapper: H2D, run `fn` on device buffers, D2H into a library-owned result.
// codec_need: what the codec itself will ask the gate for (its scratch besides the two staging buffers): stated HERE, before the
// staging is allocated -- a call that waited behind the gate inside the codec already held n + 1.125 x bound bytes of staging, uncounted
// (64 goroutines with 1 GiB each: 218 GiB next to the admitted 85 %), and the codec's own admission is covered by this one.
template <class Fn>
int host_call(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n, size_t bound, size_t codec_need, Fn fn) {
    Ctx &c = ctx();
    int rc = host_args(c, in, n, out, out_n); if (rc) return rc;
    rc = ctx_init(c); if (rc) return rc;
    hipStream_t s = c.own_stream;
    Admission gate(c, slotset::HOST_CALL); gate.admit(round_up(n, 16) + 64 + bound + bound / 8 + codec_need, ADMIT_FROM);
    static const bool timing = getenv("RSN_HOST_TIMING") != nullptr;
    const double t_in = timing ? now_ms() : 0;
    void *d_in, *d_out;
    rc = stage_input(c, s, Slot::STAGE_IN, in, n, &d_in); if (rc) return rc;
    if (timing) RSN_HIP(hipStreamSynchronize(s));
    const double t_up = timing ? now_ms() : 0;
    size_t cap = bound, got = 0;
    for (int attempt = 0;; attempt++) {
        rc = dev_buf(c, Slot::STAGE_OUT, cap, &d_out); if (rc) return rc;
        rc = fn(c, s, (const uint8_t *)d_in, (uint8_t *)d_out, cap, &got);
        if (rc == RSN_ERR_CAPACITY && attempt == 0 && got > cap) { cap = got; continue; }
        break;
    }
    if (rc) return rc;
    if (timing) RSN_HIP(hipStreamSynchronize(s));
    const double t_codec = timing ? now_ms() : 0;
    double t_alloc = 0;
    rc = result_from_dev(c, s, d_out, got, out, out_n, timing ? &t_alloc : nullptr); if (rc) return rc;
    if (timing)
        fprintf(stderr, "host call %p: in at %.2f ms, %zu B up by +%.2f, codec +%.2f, result block +%.2f, %zu B down +%.2f\n", (void *)&c,
                fmod(t_in, 100000.0), n, t_up - t_in, t_codec - t_up, t_alloc - t_codec, got, now_ms() - t_alloc);
    return RSN_OK;
}

// ---- a host-buffer call as a PIPELINE: an uploader thread sends the input up in pieces, the calling thread runs the codec in slices as
// they land (`run` gets a SliceStream), a downloader thread brings every finished range of the output down while the next is produced.
// out_cap: what the output can take at most (the result block and the device buffer are that large); codec_need: the codec's scratch, for
// the admission.  `run` returns 1 when the stream turns out not to be for slicing: the caller then takes the serial call.
template <class Run>
static int piped_call(const uint8_t *in, size_t n, size_t out_cap, size_t codec_need, uint8_t **out, size_t *out_n, Run run) {
    // Pieces of 64 MiB, each REGISTERED (pinned in place, hipHostRegister: 0.65 ms for 64 MiB) before its copy is queued, the next
    // piece's registration under the copy of this one: copies of pageable memory in pieces ran at half the link's rate once the other
    // direction was busy too (measured: 27 ms up + the download behind it = the serial call's 36 ms; two 256 MiB copies at once: 94 GB/s).
    // The registrations are RELEASED when the codec has returned, not piece by piece: hipHostUnregister waits for every stream of the
    // process, the codec's kernels included (scripts/probes/copy_under_kernel.hip: 256 MiB up beside a 20 ms kernel in 4.8 ms when the
    // pieces stay registered, in 24-35 ms when each is released behind its copy -- the upload then only moves between kernels).
    constexpr size_t PIECE = (size_t)64 << 20;
    // [lo, hi) of a host range whose pages no neighbouring piece shares: piece k of a buffer at `base` is [cut(k), cut(k + 1))
    auto cut = [](const uint8_t *base, size_t total, size_t k) -> size_t {
        if (k == 0) return 0;
        const uintptr_t a = ((uintptr_t)base + k * PIECE + 4095) & ~(uintptr_t)4095;
        return std::min(total, (size_t)(a - (uintptr_t)base));
    };
    Ctx &c = ctx();
    int rc = ctx_init(c); if (rc) return rc;
    hipStream_t s = c.own_stream;
    Admission gate(c, slotset::HOST_CALL); gate.admit(round_up(n, 16) + 64 + out_cap + codec_need);
    void *d_in, *d_out;
    rc = stage_buf(c, s, Slot::STAGE_IN, n, &d_in); if (rc) return rc;               // (the uploader below sends the bytes)
    rc = dev_buf(c, Slot::STAGE_OUT, round_up(out_cap, 16) + 64, &d_out); if (rc) return rc;
    HostBlock block;                                                      // (allocated here, not by a result helper: it must exist before the codec runs)
    rc = result_block(c, out_cap, block); if (rc) return rc;
    uint8_t *const res = block.p;
    RSN_HIP(hipStreamSynchronize(s));                                     // (the zeroed tail, before the uploader's first piece lands on the same bytes)

    struct Pipe : FirstFailure {                                          // (rc: a failed transfer is RSN_ERR_DEVICE, a failed codec its own code)
        size_t uploaded = 0;                                              // bytes of the stream on the device
        std::vector<std::pair<size_t, size_t>> ready;                     // decoded ranges not yet asked for by the downloader
        size_t taken = 0; bool decoded_all = false;
        bool failed() const { return rc != RSN_OK; }                      // (under mu, or once the helpers have ended)
    } P;
    const int device = c.device;
    static const bool timing = getenv("RSN_HOST_TIMING") != nullptr;
    const auto t_start = std::chrono::steady_clock::now();
    auto since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(); };
    std::vector<PinHold> in_pinned((n + PIECE - 1) / PIECE + 2);         // the input's pieces: registered or shared through the table above (released below)
    // Both helpers come from the pool (rsn_helpers.h): no thread and no stream is created once a first call has run, and "no thread to be
    // had" is an answer, not an exception -- the caller then takes the serial call.
    HelperPool::Handle uploader = HelperPool::run(device, on_helper(P, [&] {
        if (rsn_device_set(device) != RSN_OK) { P.fail(RSN_ERR_DEVICE, rsn_last_error()); return; }
        hipStream_t su = ctx().own_stream;
        std::vector<PinHold> &pinned = in_pinned;
        auto pin = [&](size_t k) { const size_t lo = cut(in, n, k), hi = cut(in, n, k + 1); if (hi > lo) pin_acquire(in + lo, hi - lo, true, pinned[k]); };
        pin(0);
        for (size_t k = 0; cut(in, n, k) < n; k++) {
            const size_t lo = cut(in, n, k), hi = cut(in, n, k + 1);
            hipError_t e = copy_up((uint8_t *)d_in + lo, in + lo, hi - lo, su, pinned[k]);
            if (e == hipSuccess && hi < n) pin(k + 1);                        // (under this piece's copy)
            if (e == hipSuccess) e = hipStreamSynchronize(su);
            if (e != hipSuccess) { P.fail(RSN_ERR_DEVICE, hipGetErrorString(e)); return; }
            { std::lock_guard<std::mutex> lk(P.mu); if (P.failed()) return; P.uploaded = hi; }
            P.cv.notify_all();
        }
        if (timing) { size_t np_ = 0; for (const PinHold &x : pinned) np_ += x.registered; fprintf(stderr, "piped call: %zu B up by +%.2f ms (%zu pieces registered)\n", n, since(), np_); }
    }));
    if (!uploader) return 1;
    HelperPool::Handle downloader = HelperPool::run(device, on_helper(P, [&] {
        if (rsn_device_set(device) != RSN_OK) { P.fail(RSN_ERR_DEVICE, rsn_last_error()); return; }
        hipStream_t sd = ctx().own_stream;
        const size_t total_out = out_cap;
        std::vector<char> pinned((total_out + PIECE - 1) / PIECE + 1, 0);
        size_t next_pin = 0;                                              // pieces of the result block below this index have been tried
        for (;;) {
            std::pair<size_t, size_t> r;
            {
                std::unique_lock<std::mutex> lk(P.mu);
                P.cv.wait(lk, [&] { return P.failed() || P.taken < P.ready.size() || P.decoded_all; });
                if (P.failed() || P.taken >= P.ready.size()) break;
                r = P.ready[P.taken++];
            }
            if (!r.second) continue;
            auto pin_below = [&](size_t limit) {                              // the pieces of the result block that begin below `limit`
                while (cut(res, total_out, next_pin) < std::min(total_out, limit)) {
                    const size_t lo = cut(res, total_out, next_pin), hi = cut(res, total_out, next_pin + 1);
                    if (hi > lo) { pinned[next_pin] = hipHostRegister(res + lo, hi - lo, hipHostRegisterDefault) == hipSuccess; if (!pinned[next_pin]) (void)hipGetLastError(); }
                    next_pin++;
                }
            };
            pin_below(r.first + r.second);                                    // the pieces this range lands in (all but the first call's were pinned a range ahead)
            hipError_t e = hipSuccess;                                        // (a copy may not straddle two registrations: cut at the pieces' edges)
            for (size_t at = r.first, end = r.first + r.second; at < end && e == hipSuccess;) {
                size_t k = at / PIECE;                                        // the piece that holds `at`: cut(k) <= at < cut(k + 1)
                while (cut(res, total_out, k + 1) <= at) k++;
                while (k > 0 && cut(res, total_out, k) > at) k--;
                const size_t stop = std::min(end, cut(res, total_out, k + 1));
                e = copy_async(res + at, (const uint8_t *)d_out + at, stop - at, hipMemcpyDeviceToHost, sd);
                at = stop;
            }
            if (e == hipSuccess) pin_below(r.first + 2 * r.second);            // under these copies: where the next range will land
            if (e == hipSuccess) e = hipStreamSynchronize(sd);
            if (e != hipSuccess) { P.fail(RSN_ERR_DEVICE, hipGetErrorString(e)); break; }
            if (timing) fprintf(stderr, "piped call: [%zu, +%zu) down by +%.2f ms\n", r.first, r.second, since());
        }
        if (timing) { size_t np_ = 0; for (size_t k = 0; k < next_pin; k++) np_ += pinned[k] != 0; fprintf(stderr, "piped call: %zu of %zu pieces of the result registered\n", np_, next_pin); }
        for (size_t k = 0; k < next_pin; k++) if (pinned[k]) (void)hipHostUnregister(res + cut(res, total_out, k));
    }));
    if (!downloader) {                                                    // (the uploader is at work on P and d_in: it ends before they do)
        P.fail(RSN_ERR_NOMEM, "no helper thread for the downloads");
        HelperPool::wait(uploader);
        (void)hipSetDevice(c.device);
        for (PinHold &x : in_pinned) pin_release(x);
        return 1;
    }
    SliceStream st;
    st.slice_bytes = (size_t)64 << 20;
    st.need_in = [&](size_t bytes) { std::unique_lock<std::mutex> lk(P.mu); P.cv.wait(lk, [&] { return P.failed() || P.uploaded >= std::min(bytes, n); }); return !P.failed(); };
    st.in_so_far = [&] { std::lock_guard<std::mutex> lk(P.mu); return P.uploaded; };
    st.have_out = [&](size_t off, size_t len) {
        if (timing) fprintf(stderr, "piped call: [%zu, +%zu) decoded by +%.2f ms\n", off, len, since());
        { std::lock_guard<std::mutex> lk(P.mu); if (P.failed()) return false; P.ready.emplace_back(off, len); }
        P.cv.notify_all();
        return true;
    };
    size_t got = 0;
    // (an exception out of the codec -- a vector that cannot grow -- must not unwind this frame while the helpers work on it)
    rc = guarded_call<int>([&] { return run(c, s, (const uint8_t *)d_in, (uint8_t *)d_out, out_cap, &got, &st); },
                           [&](int code, const char *m) { try { c.err = m; } catch (...) {} return code; });
    if (rc != RSN_OK) P.fail(rc, c.err.c_str());                          // (stops both helpers)
    { std::lock_guard<std::mutex> lk(P.mu); P.decoded_all = true; }
    P.cv.notify_all();
    HelperPool::wait(uploader);
    HelperPool::wait(downloader);
    (void)hipSetDevice(c.device);
    for (PinHold &x : in_pinned) pin_release(x);
    if (timing) fprintf(stderr, "piped call: the codec returned %d (%s) at +%.2f ms\n", rc, rc > 0 || rc == RSN_OK ? "" : c.err.c_str(), since());
    if (rc == RSN_ERR_CAPACITY || rc == 1) return 1;                      // more output than the caller allowed for, or not a stream for slices: the serial call
    if (rc != RSN_OK && P.msg != c.err) return c.fail(rc, "%s (%s)", std::string(c.err).c_str(), P.msg.c_str());
    if (rc != RSN_OK) return rc;
    if (P.failed()) return c.fail(RSN_ERR_DEVICE, "a transfer of the pipelined call failed: %s", P.msg.c_str());
    *out = block.release(); *out_n = got;
    return RSN_OK;
}

// the codecs read d_in while they write d_out: the two ranges must not overlap
bool ranges_overlap(const void *a, size_t na, const void *b, size_t nb) {
    if (!a || !b || !na || !nb) return false;
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

int dev_prologue(Ctx &c, void *stream, hipStream_t *s) {
    int rc = ctx_init(c); if (rc) return rc;
    *s = stream ? (hipStream_t)stream : c.own_stream;
    return RSN_OK;
}

// The argument checks of the device-buffer form, then the context and the stream.  The calls differ in three rules, each as rsn.h states it:
// null_empty: a NULL d_in is an argument error only with a length (the Huffman calls refuse it with none, too); size_query: a NULL d_out
// makes out_cap count as 0 (the codec answers the size before it writes a byte); align: both buffers on 16-byte boundaries, the word in
// front of the message.
struct DevRules { bool null_empty, size_query; const char *align; };
int dev_args(Ctx &c, const DevRules &r, const void *d_in, size_t n, void *d_out, size_t *out_cap, size_t *out_n, void *stream, hipStream_t *s) {
    if ((!d_in && (n || !r.null_empty)) || !out_n) return c.fail(RSN_ERR_ARG, "null argument");
    if (r.size_query && !d_out) *out_cap = 0;
    if (ranges_overlap(d_in, n, d_out, *out_cap)) return c.fail(RSN_ERR_ARG, "input and output ranges overlap");
    if (r.align && (((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 15))) return c.fail(RSN_ERR_ARG, "%s: device buffers must be 16-byte aligned", r.align);
    return dev_prologue(c, stream, s);
}

// ---- the layers' codecs, one row per (RSN_LAYER_*, direction): what the serial host call gives the codec -- the output buffer's first
// size (typical outputs are smaller; the exact need comes back on RSN_ERR_CAPACITY) and the codec's own statement of scratch for the
// admission -- the codec on device buffers (window: the LZSS encoder's, ignored by the rest), the device-buffer call's argument rules, and
// the whole host-buffer call at the layers' window.  The single calls, the batch pipeline and the layered calls all read these rows, so a
// layered call admits and allocates what the chain of single calls does.  (The arithmetic codec is not a layer: arith.hip sizes itself.)
struct Codec {
    size_t (*cap)(size_t n);
    size_t (*scratch)(size_t n);
    int (*dev)(Ctx &c, hipStream_t s, const uint8_t *di, size_t n, int64_t window, uint8_t *dout, size_t cap, size_t *got);
    DevRules rules;
    int (*host)(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n);
};
const Codec &codec(int id, bool enc);

// the serial host-buffer call of a row: host_call around its codec
int host_codec(const Codec &k, const uint8_t *in, size_t n, int64_t window, uint8_t **out, size_t *out_n) {
    return host_call(in, n, out, out_n, k.cap(n), k.scratch(n),
                     [&k, n, window](Ctx &c, hipStream_t s, const uint8_t *di, uint8_t *dout, size_t cap, size_t *got) { return k.dev(c, s, di, n, window, dout, cap, got); });
}
// ... and its device-buffer call
int dev_codec(const Codec &k, const void *d_in, size_t n, int64_t window, void *d_out, size_t out_cap, size_t *out_n, void *stream) {
    Ctx &c = ctx(); hipStream_t s;
    int rc = dev_args(c, k.rules, d_in, n, d_out, &out_cap, out_n, stream, &s); if (rc) return rc;
    return k.dev(c, s, (const uint8_t *)d_in, n, window, (uint8_t *)d_out, out_cap, out_n);
}

}  // namespace
}  // namespace rsn

using namespace rsn;

// (implementations; the extern "C" wrappers that guard them are at the end of the file)

static int rsn_device_set_impl(int device) {
    Ctx &c = ctx();
    if (device < 0) return c.fail(RSN_ERR_ARG, "negative device");
    if (c.inited && c.device != device) {
        // drop per-device resources; they are re-created lazily on the new device
        (void)hipSetDevice(c.device);
        for (auto &b : c.bufs) { if (b.p) { (void)hipFree(b.p); g_arena_bytes[c.device & 63] -= b.cap; } b.p = nullptr; b.cap = 0; }
        if (c.own_stream) (void)hipStreamDestroy(c.own_stream);
        c.own_stream = nullptr;
        prof_collect(c);
        for (auto e : c.free_events) (void)hipEventDestroy(e);
        c.free_events.clear();
        c.inited = false;
    }
    c.device = device;
    c.device_chosen = true;
    return ctx_init(c);
}

static int rsn_device_count_impl(void) {
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess) return ctx().fail(RSN_ERR_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    return cnt;
}

const char *rsn_last_error(void) { return ctx().err.c_str(); }
const char *rsn_version(void) { return "librsn 0.1 (gfx950)"; }

static void rsn_trim_impl(void) {
    Ctx &c = ctx();
    trim_own_context();
    HelperPool::on_idle(trim_own_context);                                // the idle helpers of the pipelined calls keep contexts of their own
    std::vector<Parked> parked;
    {
        std::lock_guard<std::mutex> lk(g_park_mu);
        if (g_parked) parked.swap(*g_parked);
    }
    for (auto &pk : parked) release_parked(pk);
    if (c.inited) (void)hipSetDevice(c.device);
    std::vector<std::pair<size_t, void *>> pool;
    {
        std::lock_guard<std::mutex> lk(g_pool_mu);
        pool.swap(g_pool);
    }
    for (auto &pr : pool) { ((ResHdr *)pr.second)->magic = 0; free(pr.second); }
}
size_t rsn_huffman_compress_bound(size_t n) { return huff_compress_bound(n); }
size_t rsn_lzss_compress_bound(size_t n) { return lzss_compress_bound(n); }

static const char *const HUFF_EMPTY = "huffman: empty input (reference panics in heap.Pop, huffman.go:102)";
static int huffman_compress_single(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n) { return host_codec(codec(RSN_LAYER_HUFFMAN, true), in, n, 0, out, out_n); }

// the small-input codec's result (in pinned staging) into a block of the caller's; 1 stays 1
static int small_result(Ctx &c, int rc, const uint8_t *p, size_t got, uint8_t **out, size_t *out_n) {
    return rc != RSN_OK ? rc : result_from_host(c, p, got, out, out_n);
}

static int rsn_huffman_compress_impl(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n) {
    if (n == 0) return ctx().fail(RSN_ERR_EMPTY, "%s", HUFF_EMPTY);
    if (in && out && out_n && n <= 65536) {                              // (the general path for the same bytes: the device-pointer entry points, tests/test_gpu_huffman_small.py)
        Ctx &c = ctx(); const uint8_t *p = nullptr; size_t got = 0;
        const int rc = small_result(c, huff_small_compress(c, in, n, &p, &got), p, got, out, out_n);
        if (rc != 1) return rc;
    }
    // RSN_HUFF_SHARDS=<G> > 1: one stream out of G slices, a worker (and, with RSN_BATCH_DEVICES, a device) each -- same bytes
    static const int env_shards = env_int("RSN_HUFF_SHARDS", 0);
    if (env_shards > 1 && n >= ((size_t)1 << 16)) return rsn_huffman_compress_sharded(in, n, env_shards, out, out_n);
    return huffman_compress_single(in, n, out, out_n);
}

// A large host-buffer decode as a PIPELINE (what the cgo shim binds was upload, then codec, then download -- 16 + 0.5 + 19 ms
// for a GiB of 2a, the codec the smallest part).  The header is on the host already: its counts give the output's size (what a stream this
// library or the reference wrote decodes to), so the result block and both device buffers exist before a byte has moved; an uploader thread
// sends the stream up in pieces, this thread decodes slice after slice as the pieces land (huff_decode_dev with a SliceStream: a slice
// starts where its predecessor's last codeword ended), a downloader thread brings every finished slice down while the next decodes.  PCIe
// is full duplex: the call takes the longer of the two transfers, not their sum.  A stream whose payload decodes to more than its header
// says (a foreign header: the counts only shape the tree) is decoded again by the serial call.  ENCODE has nothing to overlap: the first
// output byte -- header counts, pad (huffman.go:245-255) -- depends on the last input byte.
// Returns 1 when the stream is not for this path (small, malformed, foreign): the caller takes the serial call, which also words the errors.
static int huffman_decompress_piped(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n) {
    constexpr size_t PIPE_MIN = (size_t)32 << 20;
    if (n < PIPE_MIN) return 1;
    // ---- the header: strings.SplitN(content, "\\\n", 2) (huffman.go:261), the counts (huffman.go:196-227)
    size_t sep = (size_t)-1;
    for (size_t i = 0; i + 1 < std::min(n, (size_t)64 << 20); i++) if (in[i] == 0x5C && in[i + 1] == 0x0A) { sep = i; break; }
    if (sep == (size_t)-1 || sep + 3 > n) return 1;
    std::vector<HuffSym> syms; std::string msg;
    if (!parse_header(in, sep, syms, msg) || syms.size() < 2) return 1;
    const size_t sn = n - sep - 2;
    const unsigned long long nbits = (unsigned long long)(sn - 1) * 8, diff = in[sep + 2];
    if (diff > nbits || nbits == diff) return 1;
    const unsigned long long max_bits = nbits - diff;
    unsigned long long total = 0, expect = 0;
    for (const HuffSym &sy : syms) {
        if (sy.freq > max_bits - total) return 1;                         // more symbols than the payload has bits: a foreign header
        total += sy.freq;
        expect += sy.freq * (unsigned long long)utf8_len(sy.rune);
    }
    if (expect == 0) return 1;
    return piped_call(in, n, (size_t)expect, codec(RSN_LAYER_HUFFMAN, false).scratch(n), out, out_n,
                      [n](Ctx &c, hipStream_t s, const uint8_t *di, uint8_t *dout, size_t cap, size_t *got, const SliceStream *st) {
                          return huff_decode_dev(c, s, di, n, dout, cap, got, st);
                      });
}

// (small = false: a member the batch's grouped kernel has handed back -- the single call's small-input kernel would hand it back too)
static int rsn_huffman_decompress_impl(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n, bool small = true) {
    Ctx &c = ctx();
    int rc0 = host_args(c, in, n, out, out_n); if (rc0) return rc0;
    static const bool serial = getenv("RSN_HOST_SERIAL") != nullptr;     // A/B switch (tests): upload, decode, download, one after the other
    if (small && n <= 65536 + 2048) {
        const uint8_t *p = nullptr; size_t got = 0;
        const int rc = small_result(c, huff_small_decompress(c, in, n, &p, &got), p, got, out, out_n);
        if (rc != 1) return rc;
    }
    if (!serial) {
        const int rc = huffman_decompress_piped(in, n, out, out_n);
        if (rc != 1) return rc;
    }
    return host_codec(codec(RSN_LAYER_HUFFMAN, false), in, n, 0, out, out_n);
}

static int rsn_lzss_compress_impl(const uint8_t *in, size_t n, int64_t window, uint8_t **out, size_t *out_n, bool small = true) {
    // From 128 MiB up, with the engine's kind of window: the pipeline (piped_call) -- sections of a quarter of the input (at most 256 MiB),
    // each encoded as soon as its bytes are up, its tokens on their way down while the next is encoded.  The upload (19 ms per GiB) and the
    // download (12) disappear under the encoder's 31; what does not: the first section's upload and the last one's download.  For inputs in
    // which nothing needs an escape (so the output is at most the input): the encoder checks the input as it lands and lets the first output
    // byte go only when it has seen the last input byte (the upload is done well before the encoder is); an input with a 5C or an FF in it,
    // and every call under RSN_HOST_SERIAL=1, takes the serial call.
    if (small && in && out && out_n && n <= 1024) {                       // (the reference's own table is files of 13-25 bytes, README.md:153-167: one launch, lzss_small.hip)
        Ctx &c = ctx(); const uint8_t *p = nullptr; size_t got = 0;
        *out = nullptr; *out_n = 0;
        const int rc = small_result(c, lzss_small_compress(c, in, n, window, &p, &got), p, got, out, out_n);
        if (rc != 1) return rc;
    }
    static const bool serial = getenv("RSN_HOST_SERIAL") != nullptr;
    if (!serial && in && out && out_n && n >= ((size_t)128 << 20) && window > 0 && window <= 4096) {
        const size_t sec = std::min((size_t)256 << 20, n / 4);            // (eight sections instead of four: the same 46 ms per GiB -- half a millisecond of fixed cost per section)
        const int rc = piped_call(in, n, n + 4096, 15 * (sec + ((size_t)1 << 20)), out, out_n,
                                  [n, window, sec](Ctx &c, hipStream_t s, const uint8_t *di, uint8_t *dout, size_t cap, size_t *got, const SliceStream *st) {
                                      SliceStream mine = *st;
                                      mine.slice_bytes = sec;
                                      return lzss_encode_sliced(c, s, di, n, window, dout, cap, got, mine);
                                  });
        if (rc != 1) return rc;
    }
    return host_codec(codec(RSN_LAYER_LZSS, true), in, n, window, out, out_n);
}

static int rsn_lzss_compress_legacy_impl(const uint8_t *in, size_t n, int64_t window, uint8_t **out, size_t *out_n) {
    Ctx &c = ctx();
    int rc = host_args(c, in, n, out, out_n); if (rc) return rc;
    {   // an O(n * W) serial loop that cannot be interrupted from Go: refuse what would run for hours (rsn.h)
        static const bool no_limit = getenv("RSN_LEGACY_NO_LIMIT") != nullptr;
        const size_t bound = (window <= 0 || window > 65536) ? ((size_t)1 << 20) : ((size_t)64 << 20);
        if (!no_limit && n > bound)
            return c.fail(RSN_ERR_LIMIT, "lz.Compress (legacy, host code): %zu bytes with window %lld is above the %zu-byte bound of this serial O(n*W) path; "
                          "use rsn_lzss_compress (CompressAsync), or set RSN_LEGACY_NO_LIMIT=1", n, (long long)window, bound);
    }
    std::string res;
    lzss_compress_legacy_host(in, n, window, res);
    return result_from_host(c, res.data(), res.size(), out, out_n);
}

static int rsn_lzss_decompress_impl(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n, bool small = true) {
    if (small && in && out && out_n && n <= 2048) {                       // (lzss_small.hip: one launch; what it does not take -- malformed, large output -- goes on below)
        Ctx &c = ctx(); const uint8_t *p = nullptr; size_t got = 0;
        *out = nullptr; *out_n = 0;
        const int rc = small_result(c, lzss_small_decompress(c, in, n, &p, &got), p, got, out, out_n);
        if (rc != 1) return rc;
    }
    // From 64 MiB up: the pipeline (piped_call + lzss_decode_sliced, r06) -- the stream is decoded slice by slice as its pieces land, every
    // slice's bytes on their way down while the next ones come up.  The result block must exist before the first byte is decoded and the
    // stream does not say how long it is (lzss.go:323-364 appends as it goes): the first 256 KiB are parsed HERE, on the host (4 MiB took 4 ms of a 27 ms call), and the
    // expansion they show + 15 % + 32 MiB is what is allocated; a stream that outgrows that, or holds a 5C, or whose sample has a token the
    // parser does not take, is decoded by the serial call below (which also words the errors).
    static const bool serial = getenv("RSN_HOST_SERIAL") != nullptr;
    if (!serial && in && out && out_n && n >= ((size_t)64 << 20)) {
        const size_t sample = std::min(n, (size_t)256 << 10);
        unsigned long long esc = 0; size_t i = 0; bool ok = true;
        while (i < sample && ok) {
            const uint8_t b = in[i];
            if (b == 0x5C) ok = false;
            else if (b != '<') { esc++; i++; }
            else {
                size_t q = i + 1; unsigned long long ptr = 0, len = 0; int nd = 0;
                while (q < n && nd < 10 && in[q] >= '0' && in[q] <= '9') { ptr = ptr * 10 + (in[q] - '0'); q++; nd++; }
                ok = nd && q < n && in[q] == ','; q++; nd = 0;
                while (ok && q < n && nd < 10 && in[q] >= '0' && in[q] <= '9') { len = len * 10 + (in[q] - '0'); q++; nd++; }
                ok = ok && nd && q < n && in[q] == '>' && len <= ptr;
                esc += len; i = q + 1;
            }
        }
        if (ok && i > 0) {
            const double ratio = (double)esc / (double)i;
            const size_t cap = (size_t)((double)n * ratio * 1.15) + ((size_t)32 << 20);
            if (cap < ((size_t)1 << 32) - ((size_t)1 << 20)) {
                const size_t slice = (size_t)64 << 20;
                const int rc = piped_call(in, n, cap, cap + 10 * (size_t)((double)slice * ratio) + ((size_t)64 << 20), out, out_n,
                                          [n](Ctx &c, hipStream_t s, const uint8_t *di, uint8_t *dout, size_t ocap, size_t *got, const SliceStream *st) {
                                              SliceStream mine = *st;
                                              mine.slice_bytes = slice;
                                              return lzss_decode_sliced(c, s, di, n, dout, ocap, got, mine);
                                          });
                if (rc != 1) return rc;
            }
        }
    }
    return host_codec(codec(RSN_LAYER_LZSS, false), in, n, 0, out, out_n);
}

// Independent chunks, one complete .rsn segment each (engine.CompressFiles: one file per input,
// engine.go:150-154).  A single host call is PCIe-bound -- ~4.7 ms per 256 MiB each way against 0.3 ms
// of kernels -- and PCIe is full duplex, so on ONE device the batch is a three-stage pipeline over a ring of
// device buffers: one thread uploads chunk k+1 while a second encodes chunk k and a third copies chunk k-1's
// segment down.  (Lanes that each run whole calls fall into step -- all uploading, then all downloading -- and
// overlap little: 58.6 ms against the serial loop's 73.5 on 8 x 256 MiB, r02k.)
// On a node with several GPUs the chunks are dealt out first: chunk k -> worker k mod G, worker w on device
// (caller's device + w) mod visible devices, every worker its own pipeline and its own PCIe link; results land in the
// caller's host arrays, so there is nothing to exchange between devices (no data-path collective).
//   RSN_BATCH_DEVICES=<d>|all  use up to d devices, starting at the caller's (default 1: the caller's device only)
//   RSN_BATCH_WORKERS=<w>  number of pipelines (default: one per device used); more workers than devices share
//                          devices round-robin -- how the split is exercised on a one-GPU box
//   RSN_BATCH_KEEP_MIB=<m> ring buffers above m MiB per worker (default 1024) are released when the batch ends instead of
//                          staying with the worker's (parked) context for the next batch
namespace {
struct BatchPipe : FirstFailure {
    size_t uploaded = 0, encoded = 0, downloaded = 0;      // chunks that have left each stage
    void *d_in[RING] = {}, *d_out[RING] = {}, *d_tmp[RING] = {};
    size_t got[RING] = {};
    // waits until `counter` has passed `want` chunks; false when another stage failed
    bool wait(const size_t &counter, size_t want) { std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return rc != RSN_OK || counter >= want; }); return rc == RSN_OK; }
    void done(size_t &counter) { { std::lock_guard<std::mutex> lk(mu); counter++; } cv.notify_all(); }
};

// The chunks `idx` through one device's pipeline, on the calling thread's context (already initialised on its device).
// On failure the chunks this worker has produced stay in outs[] for the caller to undo; the message is in c.err.
static int batch_on_device(Ctx &c, const std::vector<size_t> &idx, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens) {
    const size_t m = idx.size();
    if (m == 0) return RSN_OK;
    auto one_by_one = [&] {                                              // no pipeline: a single chunk, or no helper threads to be had
        for (size_t j = 0; j < m; j++) {
            const size_t i = idx[j];
            drop_results(1, &outs[i], &out_lens[i]);
            const int rc = rsn_huffman_compress(ins[i], lens[i], &outs[i], &out_lens[i]);
            if (rc != RSN_OK) return rc;
        }
        return (int)RSN_OK;
    };
    if (m < 2) return one_by_one();
    size_t max_len = 0;
    for (size_t i : idx) max_len = std::max(max_len, lens[i]);
    BatchPipe P;
    const size_t in_cap = round_up(max_len, 16) + 64, out_cap = codec(RSN_LAYER_HUFFMAN, true).cap(max_len);   // (a chunk that needs more gets its own block)
    for (int r = 0; r < RING; r++) {
        int rc = dev_buf(c, ring_in(r), in_cap, &P.d_in[r]); if (rc) return rc;
        rc = dev_buf(c, ring_out(r), out_cap, &P.d_out[r]); if (rc) return rc;
    }
    const int device = c.device;
    static const bool timing = getenv("RSN_HOST_TIMING") != nullptr;
    auto stamp = [] { return fmod(now_ms(), 100000.0); };

    HelperPool::Handle encoder = HelperPool::run(device, on_helper(P, [&] {
        if (rsn_device_set(device) != RSN_OK) { P.fail(RSN_ERR_DEVICE, rsn_last_error()); return; }
        Ctx &ce = ctx(); hipStream_t s = ce.own_stream;
        for (size_t j = 0; j < m; j++) {
            if (!P.wait(P.uploaded, j + 1)) return;
            const size_t i = idx[j];
            const int r = (int)(j % RING);
            size_t got = 0;
            int rc = huff_encode_dev(ce, s, (const uint8_t *)P.d_in[r], lens[i], (uint8_t *)P.d_out[r], out_cap, &got, nullptr, nullptr);
            if (rc == RSN_ERR_CAPACITY && got > out_cap) {
                if (hipMalloc(&P.d_tmp[r], got) != hipSuccess) { P.d_tmp[r] = nullptr; P.fail(RSN_ERR_NOMEM, "hipMalloc of an oversized segment failed"); return; }
                rc = huff_encode_dev(ce, s, (const uint8_t *)P.d_in[r], lens[i], (uint8_t *)P.d_tmp[r], got, &got, nullptr, nullptr);
            }
            if (rc == RSN_OK && hipStreamSynchronize(s) != hipSuccess) { rc = RSN_ERR_DEVICE; ce.fail(rc, "hipStreamSynchronize after encode failed"); }
            if (rc != RSN_OK) { P.fail(rc, rsn_last_error()); return; }
            P.got[r] = got;
            if (timing) fprintf(stderr, "batch dev %d chunk %zu encoded at %.2f ms\n", device, i, stamp());
            P.done(P.encoded);
        }
    }));
    if (!encoder) return one_by_one();
    HelperPool::Handle downloader = HelperPool::run(device, on_helper(P, [&] {
        if (rsn_device_set(device) != RSN_OK) { P.fail(RSN_ERR_DEVICE, rsn_last_error()); return; }
        Ctx &cd = ctx(); hipStream_t s = cd.own_stream;
        for (size_t j = 0; j < m; j++) {
            if (!P.wait(P.encoded, j + 1)) return;
            const size_t i = idx[j];
            const int r = (int)(j % RING);
            const int rc = result_from_dev(cd, s, P.d_tmp[r] ? P.d_tmp[r] : P.d_out[r], P.got[r], &outs[i], &out_lens[i]);
            if (P.d_tmp[r]) { (void)hipFree(P.d_tmp[r]); P.d_tmp[r] = nullptr; }
            if (rc != RSN_OK) { P.fail(rc, rc == RSN_ERR_NOMEM ? "allocating a result block failed" : cd.err.c_str()); return; }
            if (timing) fprintf(stderr, "batch dev %d chunk %zu down at %.2f ms\n", device, i, stamp());
            P.done(P.downloaded);
        }
    }));
    if (!downloader) {                                                    // (the encoder waits for the first upload: told to stop, it ends)
        P.fail(RSN_ERR_NOMEM, "no helper thread");
        HelperPool::wait(encoder);
        return one_by_one();
    }
    // this thread uploads
    for (size_t j = 0; j < m; j++) {
        if (j >= RING && !P.wait(P.downloaded, j + 1 - RING)) break;   // the ring slot is free once its segment is down
        const size_t i = idx[j];
        const int r = (int)(j % RING);
        hipStream_t s = c.own_stream;
        int rc = stage_input(c, s, ring_in(r), ins[i], lens[i], &P.d_in[r]);   // (in_cap holds every chunk: the slot does not move)
        if (rc == RSN_OK && hipStreamSynchronize(s) != hipSuccess) rc = c.fail(RSN_ERR_DEVICE, "hipStreamSynchronize after an upload failed");
        if (rc != RSN_OK) { P.fail(rc, c.err.c_str()); break; }
        if (timing) fprintf(stderr, "batch dev %d chunk %zu up at %.2f ms\n", device, i, stamp());
        P.done(P.uploaded);
    }
    HelperPool::wait(encoder);
    HelperPool::wait(downloader);
    for (int r = 0; r < RING; r++) if (P.d_tmp[r]) (void)hipFree(P.d_tmp[r]);
    if ((in_cap + out_cap) * RING > ((size_t)std::max(0, env_int("RSN_BATCH_KEEP_MIB", 1024)) << 20))
        for (int r = 0; r < RING; r++)
            for (Slot k : {ring_in(r), ring_out(r)}) { Ctx::Buf &b = c.buf(k); if (b.p) { (void)hipFree(b.p); scratch_forget(c, b.cap); } b.p = nullptr; b.cap = 0; }
    if (P.rc != RSN_OK) return c.fail(P.rc, "%s", P.msg.c_str());
    return RSN_OK;
}
}  // namespace

// Items 0 .. n_items - 1 dealt over the batch workers: item k -> worker k mod G, worker w on device (caller's + w mod D) mod visible, where
// D = RSN_BATCH_DEVICES (default 1) and G = RSN_BATCH_WORKERS (default D), never more workers than items.  Other devices are an opt-in
// (ADVICE r3): in the one-process-per-GPU model every rank sees every GPU, and a batch that spread by default would put contexts and ~GiB
// rings on the other ranks' devices.  work(w, idx) runs worker w's items, in order, on the context of the thread it is called on (ctx());
// one worker, or no helper thread to be had: on the calling thread and the caller's device.  rcs[w] / msgs[w]: worker w's answer.
struct DealPlan { int visible, n_dev; size_t n_workers; };
static DealPlan deal_plan(size_t n_items) {
    DealPlan d;
    d.visible = 1;
    if (hipGetDeviceCount(&d.visible) != hipSuccess || d.visible < 1) d.visible = 1;
    const char *bd = getenv("RSN_BATCH_DEVICES");
    const int want_dev = !bd || !*bd ? 1 : (!strcmp(bd, "all") ? d.visible : atoi(bd));
    d.n_dev = std::max(1, std::min(d.visible, want_dev));
    d.n_workers = std::min<size_t>((size_t)std::max(1, env_int("RSN_BATCH_WORKERS", d.n_dev)), std::max<size_t>(n_items, 1));
    return d;
}
static int worker_device(const DealPlan &d, int base, size_t w) { return (base + (int)(w % (size_t)d.n_dev)) % d.visible; }
template <class Work>
static void deal_items(Ctx &c, size_t n_items, Work work, std::vector<int> &rcs, std::vector<std::string> &msgs) {
    const DealPlan d = deal_plan(n_items);
    const size_t n_workers = d.n_workers;
    rcs.assign(n_workers, RSN_OK);
    msgs.assign(n_workers, std::string());
    if (n_workers <= 1) {                                        // one device, one worker, on the caller's own context
        std::vector<size_t> idx(n_items);
        for (size_t i = 0; i < n_items; i++) idx[i] = i;
        rcs[0] = work((size_t)0, idx);
        if (rcs[0] != RSN_OK) msgs[0] = c.err;
        return;
    }
    std::vector<HelperPool::Handle> workers(n_workers);
    const int base = c.device;
    auto share = [&](size_t w, bool own_thread) {                         // worker w's items; on the caller's thread they stay on the caller's device
        guarded_call<int>([&] {
            int rc = own_thread ? rsn_device_set(worker_device(d, base, w)) : RSN_OK;
            if (rc == RSN_OK) {
                std::vector<size_t> idx;
                for (size_t k = w; k < n_items; k += n_workers) idx.push_back(k);
                rc = work(w, idx);
            }
            rcs[w] = rc;
            if (rc != RSN_OK) msgs[w] = rsn_last_error();
            return 0;
        }, [&](int code, const char *m) { rcs[w] = code; try { msgs[w] = m; } catch (...) {} return 0; });
    };
    for (size_t w = 0; w < n_workers; w++) workers[w] = HelperPool::run(worker_device(d, base, w), [&share, w] { share(w, true); });
    for (size_t w = 0; w < n_workers; w++) if (!workers[w]) share(w, false);   // no thread to be had for that worker: its items on this one
    for (auto &t : workers) HelperPool::wait(t);
    (void)hipSetDevice(c.device);
}

// The members of a batch by class: per[r] = the members rows' r-th class takes and no earlier one does, in index order; a class with fewer
// members than its group_min is not grouped.  Those, and what no class takes, go to `rest` (not sorted).
// takes(row, i): whether the class takes member i -- the host form asks the bytes, the device form the plan's summary
template <class Takes>
static void classify_by(BatchRows rows, size_t n, Takes takes, std::vector<std::vector<size_t>> &per, std::vector<size_t> &rest) {
    per.assign(rows.n, {});
    for (size_t i = 0; i < n; i++) {
        size_t r = 0;
        while (r < rows.n && !takes(*rows.first[r], i)) r++;
        (r < rows.n ? per[r] : rest).push_back(i);
    }
    for (size_t r = 0; r < rows.n; r++)
        if (per[r].size() < rows.first[r]->group_min) { rest.insert(rest.end(), per[r].begin(), per[r].end()); per[r].clear(); }
}

// The front of both host flows (the Huffman compress batch, small_batch): the members by class, the rows in their order, then the classes behind
// them (codecs.h: BehindClass).  `back`, what the rows handed back, has joined `rest`, which is sorted.  A device failure stops it: its code.
static int batch_front(Ctx &c, BatchRows rows, int64_t window, size_t n, const uint8_t *const *ins, const size_t *lens, const SmallTake &take,
                       std::vector<size_t> &rest, std::vector<size_t> &back, size_t *failed) {
    std::vector<std::vector<size_t>> per;
    std::vector<size_t> runes;
    classify_by(rows, n, [&](const BatchClass &k, size_t i) { return k.takes(ins[i], lens[i], window); }, per, rest);
    int rc = RSN_OK;
    for (size_t r = 0; r < rows.n && rc == RSN_OK; r++)
        if (!per[r].empty()) rc = rows.first[r]->run(c, per[r], ins, lens, window, take, back, failed, &runes);
    rest.insert(rest.end(), back.begin(), back.end());
    for (size_t q = 0; q < rows.n_behind && rc == RSN_OK; q++)
        rc = rows.behind[q]->offer(c, rows.behind[q]->pool == BehindClass::RUNES ? runes : rest, rest, ins, lens, take, failed);
    rest.insert(rest.end(), runes.begin(), runes.end());                  // (no class behind the rows drew from them, or a failure came first)
    std::sort(rest.begin(), rest.end());
    return rc;
}

static int rsn_huffman_compress_batch_impl(size_t n_chunks, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens) {
    Ctx &c = ctx();
    int rc0 = batch_args(c, n_chunks, ins, lens, outs, out_lens, false, false, HUFF_EMPTY); if (rc0) return rc0;
    rc0 = ctx_init(c); if (rc0) return rc0;
    auto undo = [&](int rc, const char *msg) {
        drop_results(n_chunks, outs, out_lens);
        return c.fail(rc, "%s", msg);
    };
    // The members a class takes run grouped on this thread (codecs.h: the rows up to HUFF_BIG_IN_MAX, the rune class behind them, their
    // minimums).  The rest -- larger members, and those a kernel hands back -- take the pipeline below, dealt over the batch workers.
    std::vector<size_t> rest, back;
    size_t failed = 0;
    const int rc = batch_front(c, batch_classes(BatchLayer::HUFFMAN, true), 0, n_chunks, ins, lens, take_into(c, outs, out_lens), rest, back, &failed);
    if (rc != RSN_OK) { const std::string msg = c.err; return undo(rc, msg.c_str()); }
    if (rest.empty()) return RSN_OK;
    std::vector<int> rcs;
    std::vector<std::string> msgs;
    deal_items(c, rest.size(), [&](size_t, const std::vector<size_t> &ks) {
        std::vector<size_t> idx;
        idx.reserve(ks.size());
        for (size_t k : ks) idx.push_back(rest[k]);
        return batch_on_device(ctx(), idx, ins, lens, outs, out_lens);
    }, rcs, msgs);
    for (size_t w = 0; w < rcs.size(); w++) if (rcs[w] != RSN_OK) return undo(rcs[w], msgs[w].c_str());
    return RSN_OK;
}

// ---- one Huffman stream from G slices of ONE input ("intra-file sharding"): the slices' symbol counts are summed on the
// host, ONE tree and ONE header are built (so the result is byte for byte what rsn_huffman_compress returns), every slice's bit total
// is its counts times the code lengths, and slice w writes its code bits at bit offset base + sum of the totals before it: the single
// front pad of the format (huffman.go:245-255) makes the slices meet at BIT positions, so each worker encodes into a buffer of its own
// at the right bit phase and the bytes two neighbours share are ORed together on the way down.  Worker w runs on device
// (caller's + w mod D) mod visible, D from RSN_BATCH_DEVICES (default 1: the workers share the caller's device, which is how the
// split is exercised on a one-GPU box); on a node with several GPUs each slice has its own PCIe link, histogram and emit.
// Cuts fall on rune starts (a UTF-8 sequence is never split: huffman.go:309 decodes the whole string).
namespace {
struct ShardSync : FirstFailure {
    size_t arrived = 0, generation = 0, parties;
    explicit ShardSync(size_t p) : parties(p) {}
    // all parties meet; `last` runs on the last one to arrive, before the others go on.  false: somebody failed
    bool meet(const std::function<void()> &last) {
        std::unique_lock<std::mutex> lk(mu);
        if (rc != RSN_OK) return false;
        const size_t gen = generation;
        if (++arrived == parties) { lk.unlock(); last(); lk.lock(); arrived = 0; generation++; cv.notify_all(); }
        else cv.wait(lk, [&] { return generation != gen || rc != RSN_OK; });
        return rc == RSN_OK;
    }
};
}  // namespace


// ---- the batch forms of the other three host-buffer calls (rsn.h).  Members that a grouped kernel takes run on the calling
// thread, ONE launch per group of many (lzss_small.hip / huff_small.hip: a workgroup per member), so rsn_prof_* sees those launches; the
// rest -- a member a kernel handed back, larger ones, another alphabet -- goes through the single call's implementation, in index order,
// dealt over the batch workers like the compress batch's chunks (deal_items).  Every outs[i] is what the single call returns for ins[i]; on
// any failure every outs[i] is NULL and the answer is the lowest-index failing member's code, its message prefixed "member <i>: ".
// `rows`: the layer's and direction's classes (codecs.h), run in their order; `single(i, small)`: the single call for member i (small =
// false: the member was handed back by a grouped kernel whose body the single call's small path shares).
template <class Single>
static int small_batch(BatchRows rows, int64_t window, size_t n, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens,
                       bool back_skips_small, Single single) {
    Ctx &c = ctx();
    int rc = batch_args(c, n, ins, lens, outs, out_lens, true, true); if (rc || n == 0) return rc;
    rc = ctx_init(c); if (rc) return rc;                                  // (no device: RSN_ERR_DEVICE -- there is no CPU path)
    constexpr size_t NONE = (size_t)-1;
    struct Fail { size_t at = NONE; int rc = RSN_OK; std::string msg; };
    Fail f;
    auto note = [](Fail &x, size_t i, int code, const std::string &m) { if (i < x.at) { x.at = i; x.rc = code; x.msg = m; } };
    std::vector<size_t> rest, back;
    size_t failed = NONE;
    rc = batch_front(c, rows, window, n, ins, lens, take_into(c, outs, out_lens), rest, back, &failed);
    if (rc != RSN_OK) note(f, failed, rc, c.err);
    std::vector<char> handed(back_skips_small ? n : 0, 0);
    for (size_t i : back) if (back_skips_small) handed[i] = 1;
    while (!rest.empty() && rest.back() > f.at) rest.pop_back();          // (what lies behind a known failure cannot change the answer)
    if (!rest.empty()) {
        std::atomic<size_t> stop{f.at};                                   // the lowest failing member found so far: workers do not go past it
        std::vector<int> rcs;
        std::vector<std::string> msgs;
        std::vector<Fail> wf;
        std::vector<size_t> cur;
        wf.resize(deal_plan(rest.size()).n_workers);                      // (deal_items deals over exactly as many)
        cur.assign(wf.size(), NONE);
        deal_items(c, rest.size(), [&](size_t w, const std::vector<size_t> &idx) -> int {
            for (size_t k : idx) {
                const size_t i = rest[k];
                if (i > stop.load()) break;
                cur[w] = i;
                const int r = single(i, !(back_skips_small && handed[i]));
                if (r != RSN_OK) {
                    note(wf[w], i, r, ctx().err);
                    for (size_t s0 = stop.load(); i < s0 && !stop.compare_exchange_weak(s0, i);) {}
                    break;
                }
            }
            return RSN_OK;
        }, rcs, msgs);
        for (size_t w = 0; w < rcs.size() && w < wf.size(); w++) {
            if (wf[w].at != NONE) note(f, wf[w].at, wf[w].rc, wf[w].msg);
            else if (rcs[w] != RSN_OK) note(f, cur[w] == NONE ? 0 : cur[w], rcs[w], msgs[w]);   // (thrown: the member the worker was on)
        }
    }
    if (f.at == NONE) return RSN_OK;
    drop_results(n, outs, out_lens);
    return c.fail(f.rc, "member %zu: %s", f.at, f.msg.c_str());
}

static int rsn_huffman_decompress_batch_impl(size_t n, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens) {
    return small_batch(batch_classes(BatchLayer::HUFFMAN, false), 0, n, ins, lens, outs, out_lens, false,
                       [&](size_t i, bool small) { return rsn_huffman_decompress_impl(ins[i], lens[i], &outs[i], &out_lens[i], small); });
}

static int rsn_lzss_compress_batch_impl(size_t n, const uint8_t *const *ins, const size_t *lens, int64_t window, uint8_t **outs, size_t *out_lens) {
    return small_batch(batch_classes(BatchLayer::LZSS, true), window, n, ins, lens, outs, out_lens, true,
                       [&](size_t i, bool small) { return rsn_lzss_compress_impl(ins[i], lens[i], window, &outs[i], &out_lens[i], small);  });
}

static int rsn_lzss_decompress_batch_impl(size_t n, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens) {
    return small_batch(batch_classes(BatchLayer::LZSS, false), 0, n, ins, lens, outs, out_lens, true,
                       [&](size_t i, bool small) { return rsn_lzss_decompress_impl(ins[i], lens[i], &outs[i], &out_lens[i], small);  });
}

// ---- the arithmetic codec (arith.hip): the single call is a batch of one -- every member goes through the same two kernels
static int arithmetic_batch(bool enc, size_t n, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens) {
    Ctx &c = ctx();
    int rc = batch_args(c, n, ins, lens, outs, out_lens, true, true); if (rc || n == 0) return rc;
    rc = ctx_init(c); if (rc) return rc;                                  // (no device: RSN_ERR_DEVICE -- there is no CPU path)
    std::vector<size_t> idx(n);
    for (size_t i = 0; i < n; i++) idx[i] = i;
    const SmallTake take = take_into(c, outs, out_lens);
    size_t failed = 0;
    rc = enc ? arith_compress_members(c, idx, ins, lens, take, &failed) : arith_decompress_members(c, idx, ins, lens, take, &failed);
    if (rc == RSN_OK) return RSN_OK;
    drop_results(n, outs, out_lens);
    const std::string m = c.err;
    return c.fail(rc, "member %zu: %s", failed, m.c_str());
}
static int arithmetic_single(bool enc, const uint8_t *in, size_t n, uint8_t **out, size_t *out_n) {
    Ctx &c = ctx();
    int rc = host_args(c, in, n, out, out_n); if (rc) return rc;
    static const uint8_t none = 0;
    const uint8_t *ins[1] = {in ? in : &none};
    rc = arithmetic_batch(enc, 1, ins, &n, out, out_n);
    if (rc != RSN_OK && !c.err.compare(0, 10, "member 0: ")) c.err.erase(0, 10);
    return rc;
}
static int arithmetic_dev(bool enc, const void *d_in, size_t n, void *d_out, size_t out_cap, size_t *out_n, void *stream) {
    Ctx &c = ctx(); hipStream_t s;
    int rc = dev_args(c, DevRules{true, true, "arithmetic"}, d_in, n, d_out, &out_cap, out_n, stream, &s); if (rc) return rc;
    return enc ? arith_encode_dev(c, s, (const uint8_t *)d_in, n, (uint8_t *)d_out, out_cap, out_n)
               : arith_decode_dev(c, s, (const uint8_t *)d_in, n, (uint8_t *)d_out, out_cap, out_n);
}
size_t rsn_arithmetic_compress_bound(size_t n) { return arith_compress_bound(n); }

// ---- the batch calls on device buffers (rsn.h)
// The argument checks, before a device is looked for: the arrays, then the members in index order, then the ranges (dev_ranges.h).
// word: the codec's name in front of the alignment message, as the single calls word it.  RSN_OK with n == 0: the caller returns, too.
static int batch_dev_args(Ctx &c, size_t n, const rsn_dev_member *mem, size_t *out_lens, const char *word) {
    if (n == 0) return RSN_OK;
    if (!mem || !out_lens) return c.fail(RSN_ERR_ARG, "null argument");
    for (size_t i = 0; i < n; i++) out_lens[i] = 0;
    std::vector<DevRange> ins, outs;
    for (size_t i = 0; i < n; i++) {
        const rsn_dev_member &m = mem[i];
        if (!m.d_in && m.n) return c.fail(RSN_ERR_ARG, "member %zu: null argument", i);
        if (!m.d_out && m.out_cap) return c.fail(RSN_ERR_ARG, "member %zu: a null d_out with an out_cap of %zu (the size query is out_cap 0)", i, m.out_cap);
        if (((uintptr_t)m.d_in & 15) || ((uintptr_t)m.d_out & 15)) return c.fail(RSN_ERR_ARG, "member %zu: %s: device buffers must be 16-byte aligned", i, word);
        add_dev_range(ins, m.d_in, m.n, i);
        add_dev_range(outs, m.d_out, m.out_cap, i);
    }
    size_t a = 0, b = 0;
    const int clash = dev_ranges_clash(ins, outs, &a, &b);
    if (clash == 1) return c.fail(RSN_ERR_ARG, "member %zu: its output range and member %zu's output range overlap", a, b);
    if (clash == 2) return c.fail(RSN_ERR_ARG, "member %zu: its output range and member %zu's input range overlap", a, b);
    return RSN_OK;
}
// what the call answers once every member has run: a failure other than RSN_ERR_CAPACITY clears out_lens
static int batch_dev_answer(Ctx &c, int rc, size_t failed, size_t n, size_t *out_lens) {
    if (rc == RSN_OK) return RSN_OK;
    if (rc != RSN_ERR_CAPACITY) for (size_t i = 0; i < n; i++) out_lens[i] = 0;
    const std::string m = c.err;
    return c.fail(rc, "member %zu: %s", failed, m.c_str());
}

// LZSS and Huffman: the members by class as in the host form (classify_by: the same rows, the same cutoffs, the same minimums), each class
// through its device-form runner; what no class takes, what a class below its minimum holds and what a kernel hands back run the single
// call's codec (the layer's row of codec()) on the same stream, in index order, straight into the member's buffer.  No worker threads: one
// stream, device buffers.  A class that states takes_plan is asked through it with the member's planned summary -- the Huffman decoders,
// whose members' headers k_huff_dev_plan has read where they lie (huff_dev.hip); a member without one is not theirs.  slack: what the single
// call adds to a size rounded up to 16 when it reports a capacity (rsn.h), which a grouped member that did not fit reports too.
struct BatchDevLayer { BatchLayer rows; int codec_id; const char *word; size_t slack; const char *empty_member; };
static const BatchDevLayer &batch_dev_layer(int id, bool enc) {
    static const BatchDevLayer rows[2][2] = {
        {{BatchLayer::LZSS, RSN_LAYER_LZSS, "lzss", 16, nullptr}, {BatchLayer::LZSS, RSN_LAYER_LZSS, "lzss", 16, nullptr}},
        {{BatchLayer::HUFFMAN, RSN_LAYER_HUFFMAN, "huffman", 16, HUFF_EMPTY}, {BatchLayer::HUFFMAN, RSN_LAYER_HUFFMAN, "huffman", 32, HUFF_EMPTY}},
    };
    return rows[id == RSN_LAYER_HUFFMAN][enc];
}
// a member the layer does not take empty (Huffman compress, as the single call): RSN_ERR_EMPTY, the single call's message, *failed the lowest
static int layer_empty_member(Ctx &c, const BatchDevLayer &layer, bool enc, size_t n, const rsn_dev_member *mem, size_t *failed) {
    if (enc && layer.empty_member)
        for (size_t i = 0; i < n; i++) if (mem[i].n == 0) { *failed = i; return c.fail(RSN_ERR_EMPTY, "%s", layer.empty_member); }
    return RSN_OK;
}
// The flow on a table whose arguments are known to be good -- the caller's after batch_dev_args, or one the layered batch calls built over
// their arenas -- on a stream that is there.  Returns the code with the single call's message in c.err and the member it is
// about in *failed -- (size_t)-1 where it is about none: the stream's own failure; a failure other than RSN_ERR_CAPACITY clears out_lens.
static int layer_batch_run(Ctx &c, hipStream_t s, const BatchDevLayer &layer, bool enc, size_t n, const rsn_dev_member *mem, int64_t window, size_t *out_lens, size_t *failed) {
    constexpr size_t NONE = (size_t)-1;
    auto fails = [&](int rc, size_t i) { *failed = i; if (rc != RSN_ERR_CAPACITY) for (size_t k = 0; k < n; k++) out_lens[k] = 0; return rc; };
    int rc;
    *failed = NONE;
    const BatchRows rows = batch_classes(layer.rows, enc);
    const Codec &single = codec(layer.codec_id, enc);
    bool planned = false;
    for (size_t r = 0; r < rows.n; r++) planned = planned || rows.first[r]->takes_plan;
    DevPlans plans;
    Admission plan_gate(c, slotset::HUFF_DEV_PLANS);                      // (the plan table is the call's: no class's gate gives it back)
    if (planned) {
        plan_gate.admit(n * sizeof(HuffDevPlan), ADMIT_FROM);
        rc = huff_dev_plan(c, s, n, mem, plans);
        if (rc) return fails(rc, 0);
    }
    std::vector<std::vector<size_t>> per;
    std::vector<size_t> rest;
    classify_by(rows, n, [&](const BatchClass &k, size_t i) {
        if (!k.takes_plan) return k.takes((const uint8_t *)mem[i].d_in, mem[i].n, window);   // (such a takes() looks at no byte of the member)
        const HuffDevSummary *v = plans.of(i);
        return v && v->verdict == PARSE_PLANNED && k.takes_plan(mem[i].n, *v);
    }, per, rest);
    size_t tight = NONE; std::string tight_msg;                           // the lowest member that did not fit, and what the single call says of it
    auto cap_of = [&](size_t i) { return mem[i].d_out ? mem[i].out_cap : (size_t)0; };
    std::vector<uint32_t> answers;
    std::vector<size_t> runes;                                            // handed back as GROUP_BACK_RUNES (the Huffman byte encoders alone answer that)
    auto settle = [&](const std::vector<size_t> &idx) {                   // a class's answers for its members idx
        for (size_t q = 0; q < idx.size(); q++) {
            const size_t i = idx[q], got = answers[q];
            if (group_is_back(answers[q])) { (answers[q] == GROUP_BACK_RUNES ? runes : rest).push_back(i); continue; }
            if (got <= cap_of(i)) { out_lens[i] = got; continue; }
            out_lens[i] = round_up(got, 16) + layer.slack;                // (as the single call reports it)
            if (i < tight) { tight = i; c.fail(RSN_ERR_CAPACITY, "%s: output needs %zu bytes, buffer holds %zu", layer.word, got, cap_of(i)); tight_msg = c.err; }
        }
    };
    for (size_t r = 0; r < rows.n; r++) {
        if (per[r].empty()) continue;
        rc = rows.first[r]->run_dev(c, s, per[r], mem, window, planned ? &plans : nullptr, answers);
        if (rc) return fails(rc, per[r][0]);                              // (a device failure: nothing more is launched)
        settle(per[r]);
    }
    for (size_t q = 0; q < rows.n_behind; q++) {                          // (codecs.h: the classes behind the rows, each over its pool)
        const BehindClass &k = *rows.behind[q];
        std::vector<size_t> idx, &pool = k.pool == BehindClass::RUNES ? runes : rest;
        rc = k.offer_dev(c, s, pool, rest, mem, planned ? &plans : nullptr, idx, answers);
        if (rc) return fails(rc, behind_failed(idx, pool));
        settle(idx);
    }
    rest.insert(rest.end(), runes.begin(), runes.end());                  // (what no class behind the rows drew, and what one answered with the same word)
    std::sort(rest.begin(), rest.end());
    for (size_t i : rest) {
        size_t got = 0;
        rc = single.dev(c, s, (const uint8_t *)mem[i].d_in, mem[i].n, window, (uint8_t *)mem[i].d_out, cap_of(i), &got);
        if (rc != RSN_OK && rc != RSN_ERR_CAPACITY) return fails(rc, i);
        out_lens[i] = got;
        if (rc == RSN_ERR_CAPACITY && i < tight) { tight = i; tight_msg = c.err; }
    }
    RSN_HIP(hipStreamSynchronize(s));
    if (tight == NONE) return RSN_OK;
    c.err = tight_msg;
    return fails(RSN_ERR_CAPACITY, tight);
}
// the call on the caller's table: the argument checks and an empty member's answer before a device is looked for, then the flow
static int layer_batch_dev(const BatchDevLayer &layer, bool enc, size_t n, const rsn_dev_member *mem, int64_t window, size_t *out_lens, void *stream) {
    Ctx &c = ctx(); hipStream_t s;
    size_t failed = 0;
    int rc = batch_dev_args(c, n, mem, out_lens, layer.word); if (rc || n == 0) return rc;
    rc = layer_empty_member(c, layer, enc, n, mem, &failed); if (rc) return batch_dev_answer(c, rc, failed, n, out_lens);
    rc = dev_prologue(c, stream, &s); if (rc) return rc;
    rc = layer_batch_run(c, s, layer, enc, n, mem, window, out_lens, &failed);
    return failed == (size_t)-1 ? rc : batch_dev_answer(c, rc, failed, n, out_lens);
}
static int lzss_batch_dev(bool enc, size_t n, const rsn_dev_member *mem, int64_t window, size_t *out_lens, void *stream) {
    return layer_batch_dev(batch_dev_layer(RSN_LAYER_LZSS, enc), enc, n, mem, window, out_lens, stream);
}
static int huffman_batch_dev(bool enc, size_t n, const rsn_dev_member *mem, size_t *out_lens, void *stream) {
    return layer_batch_dev(batch_dev_layer(RSN_LAYER_HUFFMAN, enc), enc, n, mem, 0, out_lens, stream);
}

static int arithmetic_batch_dev(bool enc, size_t n, const rsn_dev_member *mem, size_t *out_lens, void *stream) {
    Ctx &c = ctx(); hipStream_t s;
    int rc = batch_dev_args(c, n, mem, out_lens, "arithmetic"); if (rc || n == 0) return rc;
    rc = dev_prologue(c, stream, &s); if (rc) return rc;
    size_t failed = 0;
    rc = arith_members_dev(c, s, enc, n, mem, out_lens, &failed);
    return batch_dev_answer(c, rc, failed, n, out_lens);
}

static int rsn_huffman_compress_sharded_impl(const uint8_t *in, size_t n, int shards, uint8_t **out, size_t *out_n) {
    Ctx &c = ctx();
    int rc0 = host_args(c, in, n, out, out_n); if (rc0) return rc0;
    if (n == 0) return c.fail(RSN_ERR_EMPTY, "%s", HUFF_EMPTY);
    rc0 = ctx_init(c); if (rc0) return rc0;
    int G = shards > 0 ? shards : env_int("RSN_HUFF_SHARDS", 0);
    const DealPlan dp = deal_plan(1);                                     // (the devices of the batch workers: RSN_BATCH_DEVICES)
    const int n_dev = dp.n_dev;
    if (G <= 0) G = n_dev;
    // (every slice is a thread with a stream and an arena of its own that meets the others at a barrier -- a few per device
    //  is all that can overlap anything; 64 or 255 of them only left that many parked contexts behind)
    G = std::min(G, std::max(16, 4 * n_dev));
    std::vector<size_t> cut;
    huff_slice_cuts(in, n, G, cut);                                       // on rune starts (huff_host.cpp: host logic, tested without a device)
    const size_t S = cut.size() - 1;                                      // slices
    if (S == 1) return huffman_compress_single(in, n, out, out_n);

    struct Slice { HuffSlice hs; unsigned long long bits = 0, start = 0; uint8_t edge[2] = {0, 0}; size_t first = 0, last = 0; bool has = false; };
    std::vector<Slice> sl(S);
    HuffTree tree; HuffCodes codes; std::string hdr;
    bool flat = false;
    HostBlock block; uint8_t *res = nullptr; size_t total = 0;
    ShardSync sync(S);
    const int base_dev = c.device;

    auto plan = [&] {                                                     // runs once, on the last worker to finish its histogram
        std::vector<HuffSym> all;
        bool ascii = true;
        for (auto &x : sl) { all.insert(all.end(), x.hs.syms.begin(), x.hs.syms.end()); ascii = ascii && x.hs.ascii; }
        std::sort(all.begin(), all.end(), [](const HuffSym &a, const HuffSym &b) { return a.rune < b.rune; });
        std::vector<HuffSym> syms;
        for (const HuffSym &y : all) { if (!syms.empty() && syms.back().rune == y.rune) syms.back().freq += y.freq; else syms.push_back(y); }
        emit_header(syms, hdr);
        std::vector<HuffSym> by_rune = syms;
        std::string msg;
        if (!build_tree(syms, tree, msg)) { sync.fail(RSN_ERR_EMPTY, msg.c_str()); return; }
        if (!assign_codes(tree, codes, msg, false)) { sync.fail(RSN_ERR_LIMIT, msg.c_str()); return; }
        std::vector<std::pair<uint32_t, uint8_t>> len_of(tree.n_leaves);  // rune -> code length, ascending rune
        for (uint32_t i = 0; i < tree.n_leaves; i++) len_of[i] = {tree.rune[i], codes.len[i]};
        std::sort(len_of.begin(), len_of.end());
        unsigned long long sum = 0;
        for (auto &x : sl) {
            x.bits = 0;
            for (const HuffSym &y : x.hs.syms) {
                const auto it = std::lower_bound(len_of.begin(), len_of.end(), std::make_pair(y.rune, (uint8_t)0));
                x.bits += y.freq * it->second;
            }
            sum += x.bits;
        }
        if (sum != codes.total_bits) { sync.fail(RSN_ERR_DEVICE, "huffman: the slices' bit totals do not add up (internal error)"); return; }
        const unsigned pad = (unsigned)((8 - codes.total_bits % 8) % 8);      // huffman.go:245-249
        hdr.append("\\\n");
        hdr.push_back((char)pad);
        unsigned long long at = 8ull * hdr.size() + pad;
        for (auto &x : sl) { x.start = at; at += x.bits; }
        total = hdr.size() + (size_t)((codes.total_bits + pad) / 8);
        flat = ascii && huff_flat_code(tree, codes);
        block.p = res = (uint8_t *)result_alloc(total);
        if (!res) sync.fail(RSN_ERR_NOMEM, "allocating the result block failed");
    };

    auto worker = [&](size_t w) {
        if (rsn_device_set(worker_device(dp, base_dev, w)) != RSN_OK) { sync.fail(RSN_ERR_DEVICE, rsn_last_error()); return; }
        Ctx &cw = ctx(); hipStream_t s = cw.own_stream;
        auto bail = [&](int rc) { sync.fail(rc, cw.err.c_str()); };
        const size_t n_w = cut[w + 1] - cut[w];
        void *d_in = nullptr, *d_out = nullptr;
        int rc = stage_input(cw, s, Slot::STAGE_IN, in + cut[w], n_w, &d_in); if (rc) return bail(rc);
        rc = huff_slice_hist(cw, s, (const uint8_t *)d_in, n_w, sl[w].hs); if (rc) return bail(rc);
        if (!sync.meet(plan)) return;
        Slice &x = sl[w];
        // the slice's buffer begins at a 16-byte boundary of the stream at or before its first bit (the kernels want that alignment)
        const size_t origin = w == 0 ? 0 : (size_t)(x.start / 8) & ~(size_t)15;
        const unsigned long long base = x.start - 8ull * origin;
        const size_t local = (size_t)((base + x.bits + 7) / 8);
        rc = dev_buf(cw, Slot::STAGE_OUT, round_up(local, 16) + 64, &d_out); if (rc) return bail(rc);
        rc = huff_slice_emit(cw, s, (const uint8_t *)d_in, n_w, x.hs, tree, codes, flat, w == 0 ? hdr : std::string(), base, x.bits, (uint8_t *)d_out);
        if (rc) return bail(rc);
        // down: the bytes that are this slice's alone straight into the result, its first and last payload byte (which a neighbour
        // may share) into `edge`, to be ORed in when everybody is done
        size_t lo = w == 0 ? 0 : (size_t)(x.start / 8), hi = x.bits ? (size_t)((x.start + x.bits - 1) / 8) : (w == 0 ? hdr.size() - 1 : lo);   // inclusive
        if (x.bits == 0 && w != 0) return;                                  // (writes nothing)
        x.has = x.bits != 0;
        x.first = (size_t)(x.start / 8); x.last = hi;
        const uint8_t *dl = (const uint8_t *)d_out - origin;                // dl[k] = byte k of the stream
        hipError_t e = hipSuccess;
        if (x.has) {
            e = copy_async(&x.edge[0], dl + x.first, 1, hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = copy_async(&x.edge[1], dl + x.last, 1, hipMemcpyDeviceToHost, s);
            if (w == 0 && x.first > 0 && e == hipSuccess) e = copy_async(res, dl, x.first, hipMemcpyDeviceToHost, s);   // the header
            if (x.last > x.first + 1 && e == hipSuccess) e = copy_async(res + x.first + 1, dl + x.first + 1, x.last - x.first - 1, hipMemcpyDeviceToHost, s);
        } else e = copy_async(res, dl, hi + 1 - lo, hipMemcpyDeviceToHost, s);   // one distinct symbol: the header is the stream
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) sync.fail(RSN_ERR_DEVICE, hipGetErrorString(e));
    };

    // a slice whose thread cannot be had, or whose worker throws, fails the call: the workers that did start stop at the barrier
    auto safely = [&](size_t w) { on_helper(sync, [&] { worker(w); })(); };
    std::vector<HelperPool::Handle> threads;
    threads.reserve(S);
    for (size_t w = 1; w < S; w++) {
        threads.push_back(HelperPool::run(worker_device(dp, base_dev, w), [&safely, w] { safely(w); }));
        if (!threads.back()) { sync.fail(RSN_ERR_NOMEM, "huffman: no helper thread for a slice of the sharded stream"); break; }
    }
    safely(0);                                                            // the caller is worker 0, on its own context
    for (auto &t : threads) HelperPool::wait(t);
    (void)hipSetDevice(c.device);
    if (sync.rc != RSN_OK) return c.fail(sync.rc, "%s", sync.msg.c_str());
    for (auto &x : sl) if (x.has) { res[x.first] = 0; res[x.last] = 0; }
    for (auto &x : sl) if (x.has) { res[x.first] |= x.edge[0]; if (x.last != x.first) res[x.last] |= x.edge[1]; }
    *out = block.release(); *out_n = total;
    return RSN_OK;
}

// ---- the codec rows (declared above host_codec)
namespace rsn {
namespace {
const Codec &codec(int id, bool enc) {
    using u8 = uint8_t;
    constexpr int64_t W = RSN_LZSS_DEFAULT_WINDOW;
    constexpr size_t BIG = (size_t)32 << 20;                              // from here up the LZSS codecs state scratch (below it: not worth the gate)
    static const Codec rows[2][2] = {
        {   // RSN_LAYER_LZSS: decompress, compress
            // (the decoder asks for 4 bytes per escaped byte from 64 MiB of them up, lzss_decode.hip: stated for an expansion of two -- text is
            //  1.5; a stream that expands further decodes inside this admission all the same)
            {[](size_t n) { return 8 * n + (1 << 16); }, [](size_t n) { return n < BIG ? 0 : 8 * n; },
             [](Ctx &c, hipStream_t s, const u8 *di, size_t n, int64_t, u8 *dout, size_t cap, size_t *got) { return lzss_decode_dev(c, s, di, n, dout, cap, got); },
             {true, false, nullptr}, [](const u8 *in, size_t n, u8 **out, size_t *out_n) { return rsn_lzss_decompress_impl(in, n, out, out_n); }},
            // (the encoder's own statement of need, lzss_encode_dev: ~13 bytes of scratch per position of a pass + the escaped stream)
            {[](size_t n) { return lzss_compress_bound(n); }, [](size_t n) { return n < BIG ? 0 : 13 * std::min(n, (size_t)3 << 29) + 2 * n; },
             [](Ctx &c, hipStream_t s, const u8 *di, size_t n, int64_t w, u8 *dout, size_t cap, size_t *got) { return lzss_encode_dev(c, s, di, n, w, dout, cap, got); },
             {true, true, nullptr}, [](const u8 *in, size_t n, u8 **out, size_t *out_n) { return rsn_lzss_compress_impl(in, n, W, out, out_n); }},
        },
        {   // RSN_LAYER_HUFFMAN
            {[](size_t n) { return 4 * n + (1 << 16); }, [](size_t n) { return n / 8; },
             [](Ctx &c, hipStream_t s, const u8 *di, size_t n, int64_t, u8 *dout, size_t cap, size_t *got) { return huff_decode_dev(c, s, di, n, dout, cap, got); },
             {false, false, nullptr}, [](const u8 *in, size_t n, u8 **out, size_t *out_n) { return rsn_huffman_decompress_impl(in, n, out, out_n); }},
            {[](size_t n) { return n + n / 8 + (1 << 16); }, [](size_t n) { return n / 32; },
             [](Ctx &c, hipStream_t s, const u8 *di, size_t n, int64_t, u8 *dout, size_t cap, size_t *got) { return huff_encode_dev(c, s, di, n, dout, cap, got, nullptr, nullptr); },
             {false, true, nullptr}, [](const u8 *in, size_t n, u8 **out, size_t *out_n) { return rsn_huffman_compress_impl(in, n, out, out_n); }},
        },
    };
    return rows[id == RSN_LAYER_HUFFMAN][enc];
}
}  // namespace
}  // namespace rsn

// ---- layered calls (rsn.h): a list of layers over one buffer, the stream kept on the device between the layers.
// host_call's shape -- an input slot, an output slot, fn(c, s, d_in, d_out, cap, &got) with one retry on RSN_ERR_CAPACITY -- with the
// two slots swapped per layer.  Slots of their own (Slot::L_IN, L_A, L_B, L_STAT); the gate releases host_call's and these.
namespace {
// host buffers up to this size run the chain of single host calls (RSN_LAYERS_CHAIN_MAX: the A/B of scripts/layers_bench.py)
size_t layers_chain_max() {
    static const size_t v = getenv("RSN_LAYERS_CHAIN_MAX") ? (size_t)atoll(getenv("RSN_LAYERS_CHAIN_MAX")) : (size_t)65536;
    return v;
}
const char *layer_name(int id) { return id == RSN_LAYER_LZSS ? "lzss" : "huffman"; }
int layers_check(Ctx &c, const int *layers, size_t n_layers) {
    if (n_layers > RSN_LAYERS_MAX) return c.fail(RSN_ERR_ARG, "%zu layers: at most %d in one call", n_layers, RSN_LAYERS_MAX);
    if (n_layers && !layers) return c.fail(RSN_ERR_ARG, "null layer list");
    for (size_t k = 0; k < n_layers; k++)
        if (layers[k] != RSN_LAYER_LZSS && layers[k] != RSN_LAYER_HUFFMAN) return c.fail(RSN_ERR_ARG, "layer %zu: unknown layer id %d", k, layers[k]);
    return RSN_OK;
}
int layer_fail(Ctx &c, int rc, size_t k, int id) { const std::string m = c.err; return c.fail(rc, "layer %zu (%s): %s", k, layer_name(id), m.c_str()); }
// the SUM of what is live at once, over the chain's steps: a step's input, its output buffer (dev_buf rounds up by an eighth) and its
// codec's scratch.  A step's input is not known before the step before it has run: compress takes its bound, decompress twice its input.
size_t layers_need(bool enc, const int *layers, size_t n_layers, size_t n) {
    size_t live = 0, cur = n;
    for (size_t k = 0; k < n_layers; k++) {
        const int id = layers[enc ? k : n_layers - 1 - k];
        const size_t cap = codec(id, enc).cap(cur);
        live = std::max(live, round_up(cur, 16) + 64 + cap + cap / 8 + codec(id, enc).scratch(cur));
        cur = enc ? cap : std::min(cap, 2 * cur);
    }
    return live;
}
}  // namespace

// the chain of single host calls: one layer (the call IS the single call), and host buffers below the cutoff
static int layers_host_chain(Ctx &c, bool enc, const uint8_t *in, size_t n, const int *layers, size_t n_layers, uint8_t **out, size_t *out_n) {
    HostBlock held;
    const uint8_t *cur = in; size_t cur_n = n;
    for (size_t k = 0; k < n_layers; k++) {
        const size_t li = enc ? k : n_layers - 1 - k;
        HostBlock next; size_t next_n = 0;
        const int rc = codec(layers[li], enc).host(cur, cur_n, &next.p, &next_n);
        if (rc) return layer_fail(c, rc, li, layers[li]);
        if (held.p) result_free(held.p);
        held.p = next.release(); cur = held.p; cur_n = next_n;
    }
    *out = held.release(); *out_n = cur_n;
    return RSN_OK;
}

// The layers over a stream that is on the device: step k reads what step k - 1 wrote, the slots L_A / L_B taking turns from `slot` on.
// The last step writes to `last_out` (the caller's buffer, no retry: RSN_ERR_CAPACITY and the need in *res_n) when there is one, else
// into a slot too.  Every codec synchronises `s` before it returns.  *res / *res_n: where the result is, and its size.
static int run_chain(Ctx &c, hipStream_t s, bool enc, const int *layers, size_t n_layers, const uint8_t *d_src, size_t n, Slot slot,
                     uint8_t *last_out, size_t last_cap, const uint8_t **res, size_t *res_n) {
    const uint8_t *cur = d_src; size_t cur_n = n;
    *res_n = 0;
    for (size_t k = 0; k < n_layers; k++) {
        const size_t li = enc ? k : n_layers - 1 - k;
        const int id = layers[li];
        const bool to_caller = last_out && k + 1 == n_layers;
        size_t cap = to_caller ? last_cap : codec(id, enc).cap(cur_n), got = 0;
        uint8_t *dst = last_out;
        int rc;
        for (int attempt = 0;; attempt++) {
            if (!to_caller) { void *p; rc = dev_buf(c, slot, cap + 80, &p); if (rc) return rc; dst = (uint8_t *)p; }
            rc = codec(id, enc).dev(c, s, cur, cur_n, RSN_LZSS_DEFAULT_WINDOW, dst, cap, &got);
            if (rc == RSN_ERR_CAPACITY && !to_caller && attempt == 0 && got > cap) { cap = got; continue; }   // (both decoders: the size is known after a pass)
            break;
        }
        if (rc) { if (rc == RSN_ERR_CAPACITY) *res_n = got; return layer_fail(c, rc, li, id); }
        if (!to_caller) RSN_HIP(hipMemsetAsync(dst + got, 0, round_up(got, 16) + 64 - got, s));   // zero behind the stream, as behind an uploaded input
        cur = dst; cur_n = got;
        slot = slot == Slot::L_A ? Slot::L_B : Slot::L_A;
    }
    *res = cur; *res_n = cur_n;
    return RSN_OK;
}

static int layers_host(bool enc, const uint8_t *in, size_t n, const int *layers, size_t n_layers, uint8_t **out, size_t *out_n) {
    Ctx &c = ctx();
    int rc = host_args(c, in, n, out, out_n); if (rc) return rc;
    rc = layers_check(c, layers, n_layers); if (rc) return rc;
    rc = ctx_init(c); if (rc) return rc;
    if (n_layers == 0) return result_from_host(c, in, n, out, out_n);     // the reference's loops do nothing: the input
    if (n_layers == 1 || n <= layers_chain_max()) return layers_host_chain(c, enc, in, n, layers, n_layers, out, out_n);
    hipStream_t s = c.own_stream;
    const size_t need = round_up(n, 16) + 64 + layers_need(enc, layers, n_layers, n);
    Admission gate(c, slotset::LAYERED_CALL); gate.admit(need, ADMIT_FROM);
    void *d_in;
    rc = stage_input(c, s, Slot::L_IN, in, n, &d_in); if (rc) return rc;
    const uint8_t *d_res; size_t got = 0;
    rc = run_chain(c, s, enc, layers, n_layers, (const uint8_t *)d_in, n, Slot::L_A, nullptr, 0, &d_res, &got); if (rc) return rc;
    return result_from_dev(c, s, d_res, got, out, out_n);
}

static int layers_dev(bool enc, const void *d_in, size_t n, const int *layers, size_t n_layers, void *d_out, size_t out_cap, size_t *out_n, void *stream) {
    Ctx &c = ctx(); hipStream_t s;
    if ((!d_in && n) || !out_n) return c.fail(RSN_ERR_ARG, "null argument");
    *out_n = 0;
    int rc = layers_check(c, layers, n_layers); if (rc) return rc;
    if (((uintptr_t)d_in & 15) || ((uintptr_t)d_out & 15)) return c.fail(RSN_ERR_ARG, "layers: device buffers must be 16-byte aligned");   // (before the overlap: its own line)
    rc = dev_args(c, DevRules{true, true, nullptr}, d_in, n, d_out, &out_cap, out_n, stream, &s); if (rc) return rc;
    if (n_layers == 0) {
        if (out_cap < n) { *out_n = round_up(n, 16) + 16; return c.fail(RSN_ERR_CAPACITY, "layers: output needs %zu bytes, buffer holds %zu", n, out_cap); }
        if (n) RSN_HIP(copy_async(d_out, d_in, n, hipMemcpyDeviceToDevice, s));
        RSN_HIP(hipStreamSynchronize(s));
        *out_n = n;
        return RSN_OK;
    }
    if (n_layers == 1 && (out_cap || !enc)) {                            // the single call, its own size query included (the decoders answer it)
        const int id = layers[0];
        rc = dev_codec(codec(id, enc), d_in, n, RSN_LZSS_DEFAULT_WINDOW, d_out, out_cap, out_n, stream);
        return rc ? layer_fail(c, rc, 0, id) : RSN_OK;
    }
    const size_t need = layers_need(enc, layers, n_layers, n);
    Admission gate(c, slotset::LAYERED_CALL); gate.admit(need, ADMIT_FROM);
    const uint8_t *d_res; size_t got = 0;
    rc = run_chain(c, s, enc, layers, n_layers, (const uint8_t *)d_in, n, Slot::L_A, out_cap ? (uint8_t *)d_out : nullptr, out_cap, &d_res, &got);
    if (rc) { if (rc == RSN_ERR_CAPACITY) *out_n = got; return rc; }
    if (!out_cap && got) {                                                // the size query: the chain has run, its last layer into scratch (an empty result has nothing to size: RSN_OK, as from the single calls)
        *out_n = round_up(got, 16) + 32;                                  // (what every last layer takes: the Huffman encoder asks for its size rounded up to 16, plus 32)
        return c.fail(RSN_ERR_CAPACITY, "layers: output needs %zu bytes", got);
    }
    *out_n = got;
    return RSN_OK;
}

// ---- layered batch calls (rsn.h): many members through a list of layers, layer-major, every member on the device from the
// first step to the last.  The members are cut into runs (layers_batch_layout.h); a run's step k is layer_batch_run over a member table
// built here: d_in where step k - 1 left the member, d_out a slot of the arena whose turn it is (LB_A / LB_B) -- or, behind the last step
// of the device form, the caller's buffer.  A slot holds the codec's bound (compress) or the single chain's first guess (decompress); the
// members that report more are run again alone, with the reported figures, into LB_XA / LB_XB, the others being complete.
namespace {
constexpr size_t LB_NONE = (size_t)-1;
size_t layers_batch_budget() {                                            // (read at every call: a test cuts runs at small sizes)
    const char *e = getenv("RSN_LAYERS_BATCH_BUDGET");
    return e && atoll(e) > 0 ? (size_t)atoll(e) : LB_BUDGET;
}
size_t layer_slot_cap(int id, bool enc, size_t n) {
    if (!enc) return codec(id, false).cap(n);
    return id == RSN_LAYER_HUFFMAN ? huff_compress_bound(n) : lzss_compress_bound(n);
}
// the largest slot a member of n bytes is expected to take over the chain, for the run cuts: compress bounds applied in turn are exact
// upper bounds; a decompress step's result is taken as layers_need takes it
size_t layers_batch_slot(bool enc, const int *layers, size_t n_layers, size_t n) {
    size_t most = 0, cur = n;
    for (size_t k = 0; k < n_layers; k++) {
        const size_t cap = layer_slot_cap(layers[enc ? k : n_layers - 1 - k], enc, cur);
        most = std::max(most, cap);
        cur = enc ? cap : std::min(cap, 2 * cur);
    }
    return most;
}
// what ended a call: the step (in run order) and the member (the call's numbering) of a failure other than RSN_ERR_CAPACITY
struct LbFailure { size_t step = LB_NONE, member = 0; int rc = RSN_OK; std::string msg; };
// where a run's members are and how long, step by step; tight: the lowest member that did not fit the caller's buffer behind the last step
struct LbRunState { std::vector<const uint8_t *> at; std::vector<size_t> len; size_t tight = LB_NONE; std::string tight_msg; };
// a call's members in its form: ins / lens (the host form: a run's inputs are staged in LB_STAGE and stay there to the end of the run),
// or mem (the device form: read where they lie)
struct LbMembers {
    const uint8_t *const *ins; const size_t *lens; const rsn_dev_member *mem;
    bool staged() const { return mem == nullptr; }
    size_t len(size_t i) const { return mem ? (size_t)mem[i].n : lens[i]; }
};
// the wait every flow of this family ends a run with
int stream_synced(Ctx &c, hipStream_t s) {
    const hipError_t e = hipStreamSynchronize(s);
    return e == hipSuccess ? RSN_OK : c.fail(RSN_ERR_DEVICE, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
}
}  // namespace

// The steps [0, steps) of the run [lo, lo + m) of a call's members; st.at / st.len: where they lie going in, and coming out.  `last`: the
// m members' d_out / out_cap behind the last step (the device form), or null: an arena slot, as behind every other step.  A step's failure
// is noted in `f` (and returned); a failure of the flow itself is returned with f.step untouched.  start: the arena of step 0 (0: LB_A and
// LB_XA, 1: LB_B and LB_XB) -- the batch round trip's second pass begins in the arena its first did not end in.
static int layers_batch_steps(Ctx &c, hipStream_t s, bool enc, const int *layers, size_t n_layers, size_t steps, size_t start, size_t lo, size_t m, const rsn_dev_member *last,
                              LbRunState &st, size_t *got, LbFailure &f) {
    std::vector<rsn_dev_member> tab(m);
    std::vector<size_t> caps(m), offs;
    for (size_t k = 0; k < steps; k++) {
        const size_t li = enc ? k : n_layers - 1 - k;
        const int id = layers[li];
        const BatchDevLayer &layer = batch_dev_layer(id, enc);
        const bool to_caller = last && k + 1 == n_layers;
        auto fails = [&](int rc, size_t member) { f.step = k; f.member = member; f.rc = rc; f.msg = c.err; return rc; };
        if (to_caller) {
            for (size_t i = 0; i < m; i++) tab[i] = rsn_dev_member{st.at[i], st.len[i], last[i].d_out, last[i].d_out ? last[i].out_cap : 0};
        } else {
            for (size_t i = 0; i < m; i++) caps[i] = layer_slot_cap(id, enc, st.len[i]);
            void *p;
            int rc = dev_buf(c, (k + start) & 1 ? Slot::LB_B : Slot::LB_A, lb_arena(caps.data(), m, offs), &p); if (rc) return rc;
            for (size_t i = 0; i < m; i++) tab[i] = rsn_dev_member{st.at[i], st.len[i], (uint8_t *)p + offs[i], caps[i]};
        }
        size_t failed = 0;
        int rc = layer_empty_member(c, layer, enc, m, tab.data(), &failed); if (rc) return fails(rc, lo + failed);
        rc = layer_batch_run(c, s, layer, enc, m, tab.data(), RSN_LZSS_DEFAULT_WINDOW, got, &failed);
        if (failed == LB_NONE && rc) return rc;
        if (rc && rc != RSN_ERR_CAPACITY) return fails(rc, lo + failed);
        if (rc == RSN_ERR_CAPACITY && to_caller) { st.tight = lo + failed; st.tight_msg = c.err; }
        if (rc == RSN_ERR_CAPACITY && !to_caller) {                       // the members that outgrew their slots, alone, with the reported figures
            std::vector<size_t> again, caps2, got2;
            for (size_t i = 0; i < m; i++) if (got[i] > caps[i]) { again.push_back(i); caps2.push_back(got[i]); }
            std::vector<rsn_dev_member> tab2(again.size());
            got2.assign(again.size(), 0);
            void *p;
            rc = dev_buf(c, (k + start) & 1 ? Slot::LB_XB : Slot::LB_XA, lb_arena(caps2.data(), again.size(), offs), &p); if (rc) return rc;
            for (size_t q = 0; q < again.size(); q++) tab2[q] = rsn_dev_member{st.at[again[q]], st.len[again[q]], (uint8_t *)p + offs[q], caps2[q]};
            rc = layer_batch_run(c, s, layer, enc, again.size(), tab2.data(), RSN_LZSS_DEFAULT_WINDOW, got2.data(), &failed);
            if (failed == LB_NONE && rc) return rc;
            if (rc) return fails(rc, lo + again[failed]);                 // (a figure that did not suffice after all: the codec's own error, worded as it words it)
            for (size_t q = 0; q < again.size(); q++) { tab[again[q]].d_out = tab2[q].d_out; got[again[q]] = got2[q]; }
        }
        for (size_t i = 0; i < m; i++) { st.at[i] = (const uint8_t *)tab[i].d_out; st.len[i] = got[i]; }
    }
    return RSN_OK;
}

// what the call answers once its runs are through: a step's failure in the words of rsn.h, k counting in compress order
static int layers_batch_failure(Ctx &c, bool enc, const int *layers, size_t n_layers, const LbFailure &f) {
    const size_t li = enc ? f.step : n_layers - 1 - f.step;
    return c.fail(f.rc, "member %zu: layer %zu (%s): %s", f.member, li, layer_name(layers[li]), f.msg.c_str());
}
// the runs of a call: the form's staged bytes of member i (0: it lies in the caller's device memory) and its largest slot, twice
template <class Len>
static std::vector<LbRun> layers_batch_runs(bool enc, const int *layers, size_t n_layers, size_t n, bool staged, Len len) {
    return lb_runs(n, layers_batch_budget(), [&](size_t i) { return lb_member_need(staged ? len(i) : 0, layers_batch_slot(enc, layers, n_layers, len(i))); });
}
// A host-form run on the way up: the m inputs packed at 16-byte offsets (lb_packed) in pinned staging, ONE copy into LB_STAGE, and the
// stream synchronised (the steps stage their tables through the same pinned block).  st: where the members lie and how long.
static int layers_batch_stage(Ctx &c, hipStream_t s, const uint8_t *const *ins, const size_t *lens, size_t m, std::vector<size_t> &offs, LbRunState &st) {
    const size_t up = lb_packed(lens, m, offs);
    void *hp, *dp;
    int rc = pinned_buf(c, up + 16, &hp); if (rc) return rc;
    rc = dev_buf(c, Slot::LB_STAGE, up + LB_SLACK, &dp); if (rc) return rc;
    st.at.resize(m); st.len.resize(m);
    for (size_t i = 0; i < m; i++) {
        if (lens[i]) memcpy((uint8_t *)hp + offs[i], ins[i], lens[i]);
        memset((uint8_t *)hp + offs[i] + lens[i], 0, lb_round16(lens[i]) - lens[i]);
        st.at[i] = (const uint8_t *)dp + offs[i]; st.len[i] = lens[i];
    }
    if (up) {
        const hipError_t e = copy_async(dp, hp, up, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) return c.fail(RSN_ERR_DEVICE, "the upload of %zu bytes failed: %s", up, hipGetErrorString(e));
    }
    return stream_synced(c, s);
}
// Where the run [lo, lo + m) of a call's members lies going in: the host form's staged (layers_batch_stage), the device form's where the
// caller has them.
static int layers_batch_enter(Ctx &c, hipStream_t s, const LbMembers &in, size_t lo, size_t m, LbRunState &st) {
    std::vector<size_t> offs;
    if (in.staged()) return layers_batch_stage(c, s, in.ins + lo, in.lens + lo, m, offs, st);
    st.at.resize(m); st.len.resize(m);
    for (size_t i = 0; i < m; i++) { st.at[i] = (const uint8_t *)in.mem[lo + i].d_in; st.len[i] = in.mem[lo + i].n; }
    return RSN_OK;
}
// the members' bytes as tiles of the move table; returns the entries written
static size_t move_tiles(MoveEntry *tab, const uint8_t *src, uint8_t *dst, size_t len) {
    size_t t = 0;
    for (size_t at = 0; at < len; at += LB_TILE) tab[t++] = MoveEntry{src + at, dst + at, (unsigned long long)std::min(LB_TILE, len - at)};
    return t;
}

static int layers_batch_dev(bool enc, size_t n, const rsn_dev_member *mem, const int *layers, size_t n_layers, size_t *out_lens, void *stream) {
    Ctx &c = ctx(); hipStream_t s;
    int rc = batch_dev_args(c, n, mem, out_lens, "layers"); if (rc || n == 0) return rc;
    rc = layers_check(c, layers, n_layers); if (rc) return rc;
    rc = dev_prologue(c, stream, &s); if (rc) return rc;
    auto cleared = [&](int code) { for (size_t i = 0; i < n; i++) out_lens[i] = 0; return code; };
    if (n_layers == 0) {                                                  // a copy of every member: one table up, one launch
        size_t tiles = 0, tight = LB_NONE;
        for (size_t i = 0; i < n; i++) tiles += lb_tiles(mem[i].n);
        Admission gate(c, slotset::LAYERS_BATCH_CALL); gate.admit(tiles * sizeof(MoveEntry), ADMIT_FROM);
        void *hp, *dp;
        rc = pinned_buf(c, tiles * sizeof(MoveEntry) + 16, &hp); if (rc) return cleared(rc);
        rc = dev_buf(c, Slot::LB_STAGE, tiles * sizeof(MoveEntry) + 16, &dp); if (rc) return cleared(rc);
        MoveEntry *tab = (MoveEntry *)hp;
        tiles = 0;
        for (size_t i = 0; i < n; i++) {
            const size_t cap = mem[i].d_out ? mem[i].out_cap : 0;
            if (mem[i].n <= cap) { out_lens[i] = mem[i].n; tiles += move_tiles(tab + tiles, (const uint8_t *)mem[i].d_in, (uint8_t *)mem[i].d_out, mem[i].n); continue; }
            out_lens[i] = round_up(mem[i].n, 16) + 16;                    // (layers_dev's figure)
            if (tight == LB_NONE) tight = i;
        }
        rc = members_move(c, s, tab, (MoveEntry *)dp, tiles); if (rc) return cleared(rc);
        rc = stream_synced(c, s); if (rc) return cleared(rc);
        if (tight == LB_NONE) return RSN_OK;
        return c.fail(RSN_ERR_CAPACITY, "member %zu: layers: output needs %zu bytes, buffer holds %zu", tight, (size_t)mem[tight].n, mem[tight].d_out ? (size_t)mem[tight].out_cap : (size_t)0);
    }
    const std::vector<LbRun> runs = layers_batch_runs(enc, layers, n_layers, n, false, [&](size_t i) { return (size_t)mem[i].n; });
    size_t most = 0;
    for (const LbRun &r : runs) most = std::max(most, r.bytes);
    Admission gate(c, slotset::LAYERS_BATCH_CALL); gate.admit(most, ADMIT_FROM);
    LbFailure f;
    size_t tight = LB_NONE; std::string tight_msg;
    size_t steps = n_layers;                                              // (behind a failure the later runs go as far as the steps in front of it: an earlier layer's failure there is the call's)
    for (const LbRun &r : runs) {
        if (steps == 0) break;
        const size_t m = r.hi - r.lo;
        LbRunState st;
        rc = layers_batch_enter(c, s, LbMembers{nullptr, nullptr, mem}, r.lo, m, st); if (rc) return cleared(rc);
        const size_t before = f.step;
        rc = layers_batch_steps(c, s, enc, layers, n_layers, steps, 0, r.lo, m, mem + r.lo, st, out_lens + r.lo, f);
        if (rc && f.step == before) return cleared(rc);
        if (rc) { steps = f.step; continue; }
        if (st.tight != LB_NONE && tight == LB_NONE) { tight = st.tight; tight_msg = st.tight_msg; }
    }
    if (f.step != LB_NONE) return cleared(layers_batch_failure(c, enc, layers, n_layers, f));
    if (tight == LB_NONE) return RSN_OK;
    const size_t li = enc ? n_layers - 1 : 0;
    return c.fail(RSN_ERR_CAPACITY, "member %zu: layer %zu (%s): %s", tight, li, layer_name(layers[li]), tight_msg.c_str());
}

static int layers_batch_host(bool enc, size_t n, const uint8_t *const *ins, const size_t *lens, const int *layers, size_t n_layers, uint8_t **outs, size_t *out_lens) {
    Ctx &c = ctx();
    int rc = batch_args(c, n, ins, lens, outs, out_lens, true, true); if (rc || n == 0) return rc;
    rc = layers_check(c, layers, n_layers); if (rc) return rc;
    rc = ctx_init(c); if (rc) return rc;                                  // (no device: RSN_ERR_DEVICE -- there is no CPU path)
    auto dropped = [&](int code) { drop_results(n, outs, out_lens); return code; };
    if (n_layers == 0) {                                                  // the reference's loops do nothing: the inputs
        for (size_t i = 0; i < n; i++) { rc = result_from_host(c, ins[i], lens[i], &outs[i], &out_lens[i]); if (rc) return dropped(rc); }
        return RSN_OK;
    }
    hipStream_t s = c.own_stream;
    const std::vector<LbRun> runs = layers_batch_runs(enc, layers, n_layers, n, true, [&](size_t i) { return lens[i]; });
    size_t most = 0;
    for (const LbRun &r : runs) most = std::max(most, r.bytes);
    Admission gate(c, slotset::LAYERS_BATCH_CALL); gate.admit(most, ADMIT_FROM);
    LbFailure f;
    size_t steps = n_layers;
    std::vector<size_t> offs, got;
    for (const LbRun &r : runs) {
        if (steps == 0) break;
        const size_t m = r.hi - r.lo;
        // up: the run's inputs packed at 16-byte offsets in pinned staging, ONE copy
        void *hp, *dp;
        LbRunState st;
        rc = layers_batch_stage(c, s, ins + r.lo, lens + r.lo, m, offs, st); if (rc) return dropped(rc);
        got.assign(m, 0);
        const size_t before = f.step;
        rc = layers_batch_steps(c, s, enc, layers, n_layers, steps, 0, r.lo, m, nullptr, st, got.data(), f);
        if (rc && f.step == before) return dropped(rc);
        if (rc) { steps = f.step; continue; }
        if (steps < n_layers) continue;                                   // (the call has failed: this run only looked for an earlier layer's failure)
        // down: the move table up, the members packed at 16-byte offsets by ONE launch, ONE copy, carved into the results
        size_t tiles = 0;
        for (size_t i = 0; i < m; i++) tiles += lb_tiles(st.len[i]);
        const size_t tb = round_up(tiles * sizeof(MoveEntry), 16), down = lb_packed(st.len.data(), m, offs);
        rc = pinned_buf(c, tb + down + 16, &hp); if (rc) return dropped(rc);
        rc = dev_buf(c, Slot::LB_STAGE, tb + down + LB_SLACK, &dp); if (rc) return dropped(rc);
        MoveEntry *tab = (MoveEntry *)hp;
        tiles = 0;
        for (size_t i = 0; i < m; i++) tiles += move_tiles(tab + tiles, st.at[i], (uint8_t *)dp + tb + offs[i], st.len[i]);
        rc = members_move(c, s, tab, (MoveEntry *)dp, tiles); if (rc) return dropped(rc);
        if (down) {
            const hipError_t e = copy_async((uint8_t *)hp + tb, (const uint8_t *)dp + tb, down, hipMemcpyDeviceToHost, s);
            if (e != hipSuccess) return dropped(c.fail(RSN_ERR_DEVICE, "the download of %zu bytes failed: %s", down, hipGetErrorString(e)));
        }
        rc = stream_synced(c, s); if (rc) return dropped(rc);
        for (size_t i = 0; i < m; i++) { rc = result_from_host(c, (const uint8_t *)hp + tb + offs[i], st.len[i], &outs[r.lo + i], &out_lens[r.lo + i]); if (rc) return dropped(rc); }
    }
    if (f.step != LB_NONE) return dropped(layers_batch_failure(c, enc, layers, n_layers, f));
    return RSN_OK;
}

// ---- batch round trip and batch suite (rsn.h): ONE flow, suite_batch_flow.  The suite is engine.BenchmarkFile's body
// over many members under MANY layer lists -- the reference's benchmark loop, files x algorithm lists -- with everything the lists have in
// common done once; the batch round trip is the suite of its one list, whose tree is a chain with nothing kept, and differs in what it
// hands the flow: its own slot set, answers without the "list <l>: " in front, and its histograms as the first verify launch's rows whole.
// The lists form a prefix tree (suite_layout.h).  A run stages its members once, walks the tree depth first and compresses every node
// once -- ONE step of layers_batch_steps, from where the parent's step left the members, in the arena a call of that list alone would
// use at that step -- or, a node with more users (a kept node), into its own slots of LB_KEEP, which the run carves before its first
// step and no step reuses.  From the node a list ends at: its decompress pass, beginning in the arena the compress pass did not end in,
// and ONE launch of k_members_verify (roundtrip_batch.hip) over a table of the run's tiles; the stats block is all that comes down.  The
// run's first verify launch counts both sides; every further list's is the instance that counts the decompressed side alone.
// A list's round trip is 2 L steps and every list keeps its own bookkeeping -- the two passes' failures, `limit`: how far its runs still
// go (behind a failure the later runs go as far as the steps in front of it), the 32-bit limit -- so its answer does not depend on the
// lists beside it; a node runs while any list through it still goes that far.
namespace {
// the largest slot of the decompress pass of a member of n bytes, for the run cuts: the stream behind compress layer k is at most its bound
// and taken as at most twice the member and a header -- an estimate, as layers_batch_slot's is for a decompress call
size_t roundtrip_dec_slot(const int *layers, size_t n_layers, size_t n) {
    size_t most = 0, cur = n;
    for (size_t k = 0; k < n_layers; k++) {
        cur = layer_slot_cap(layers[k], true, cur);
        most = std::max(most, layer_slot_cap(layers[k], false, std::min(cur, 2 * n + 4096)));
    }
    return most;
}
size_t suite_bound(int id, size_t len) { return layer_slot_cap(id, true, len); }
struct SuiteListState { LbFailure fc, fd; size_t limit = 0, big = LB_NONE; };   // big: the lowest member the 32-bit counters do not hold
int roundtrip_big_failure(Ctx &c, size_t big) {
    return c.fail(RSN_ERR_LIMIT, "member %zu: a round trip of %zu bytes or more in a batch: the counters are 32 bits (rsn_layers_roundtrip takes one large buffer)", big, (size_t)1 << 32);
}
// where a call's answers go: n_lists * n rows, and what the caller asked for beside them (null: not asked for).  rows: the one-list form's
// histograms, 512 words a member -- the first verify launch's stats rows, copied whole; h_orig / h_dec: the suite's, those rows split
struct SuiteOut {
    rsn_roundtrip_member *res; int *list_rc; uint32_t *h_orig, *h_dec, *rows, *best;
    bool counting() const { return h_orig || h_dec || rows; }
};
// The plan of a call: the lists, their tree, under[v]: the lists that are run -- the first of every set of equal lists -- whose path
// leads through node v (under[SUITE_ROOT]: all that are run), the run cuts and the largest run's bytes, for the admission.
struct SuitePlan {
    const int *lp[RSN_SUITE_LISTS_MAX]; size_t ln[RSN_SUITE_LISTS_MAX];
    SuiteTree tree;
    std::vector<size_t> kept;                                             // the kept nodes, ascending (one list: none)
    std::vector<std::vector<size_t>> under;
    std::vector<LbRun> runs; size_t most = 0;
    const std::vector<size_t> &ran() const { return under[SUITE_ROOT]; }
};
SuitePlan suite_plan(const LbMembers &mem, size_t n, size_t n_lists, const rsn_layer_list *lists, bool counting) {
    SuitePlan p;
    for (size_t l = 0; l < n_lists; l++) { p.lp[l] = lists[l].layers; p.ln[l] = lists[l].n_layers; }
    p.tree = suite_tree(p.lp, p.ln, n_lists);
    const std::vector<SuiteNode> &nodes = p.tree.nodes;
    p.under.resize(nodes.size());
    for (size_t v = 0; v < nodes.size(); v++) {
        if (nodes[v].kept) p.kept.push_back(v);
        if (nodes[v].ends.empty()) continue;
        for (size_t u = v;; u = nodes[u].parent) { p.under[u].push_back(nodes[v].ends[0]); if (u == SUITE_ROOT) break; }
    }
    std::vector<size_t> caps;
    p.runs = lb_runs(n, layers_batch_budget(), [&](size_t i) {
        const size_t len = mem.len(i);
        size_t enc = 0, dec = 0;                                          // the largest over the lists of the two passes' largest slots
        for (size_t l : p.ran()) { enc = std::max(enc, layers_batch_slot(true, p.lp[l], p.ln[l], len)); dec = std::max(dec, roundtrip_dec_slot(p.lp[l], p.ln[l], len)); }
        // (what comes back is taken as long as what went in: a member that comes back longer -- the Huffman codec's treatment of bytes that are
        //  not UTF-8 -- may take a table entry of 32 bytes more than the run was cut for)
        const size_t keep = p.kept.empty() ? 0 : suite_keep_bytes(p.tree, len, suite_bound, &caps);
        return suite_member_need(mem.staged() ? len : 0, enc, dec, keep, len, len, counting);
    });
    for (const LbRun &r : p.runs) p.most = std::max(p.most, r.bytes);
    return p;
}

// The run [lo, lo + m) of a call on its way through the tree.  orig: where its members lie going in; keep[v]: the m slots of kept node v
// as the d_out / out_cap of its step; verified: a list of this run has been through the verify launch, so the originals are counted.
struct SuiteRun {
    Ctx &c; hipStream_t s; const LbMembers &mem; size_t n; const SuitePlan &p; const SuiteOut &out; std::vector<SuiteListState> &ls;
    size_t lo, m;
    std::vector<const uint8_t *> orig;
    std::vector<size_t> got;
    std::vector<std::vector<rsn_dev_member>> keep;
    bool verified = false;

    int carve(const LbRunState &st0);
    int verify(size_t l, const LbRunState &in, const LbRunState &st);
    int list_finish(size_t l, const LbRunState &in);
    int node_walk(size_t v, const LbRunState &in);
};

// the kept nodes' slots: node-major in LB_KEEP, a slot a member of the compress bounds applied in turn from the root
int SuiteRun::carve(const LbRunState &st0) {
    const size_t V = p.tree.nodes.size();
    const std::vector<size_t> &kept = p.kept;
    keep.assign(V, {});
    if (kept.empty()) return RSN_OK;
    std::vector<size_t> caps, base(V, 0);
    std::vector<std::vector<size_t>> ncap(V), koffs(V);
    for (size_t v : kept) ncap[v].resize(m);
    for (size_t i = 0; i < m; i++) {
        suite_keep_bytes(p.tree, st0.len[i], suite_bound, &caps);
        for (size_t v : kept) ncap[v][i] = caps[v];
    }
    size_t total = 0;
    for (size_t v : kept) { base[v] = total; total += lb_arena(ncap[v].data(), m, koffs[v]); }
    void *kp = nullptr;
    if (total) { const int rc = dev_buf(c, Slot::LB_KEEP, total, &kp); if (rc) return rc; }
    for (size_t v : kept) {
        keep[v].resize(m);
        for (size_t i = 0; i < m; i++) keep[v][i] = rsn_dev_member{nullptr, 0, (uint8_t *)kp + base[v] + koffs[v][i], ncap[v][i]};
    }
    return RSN_OK;
}

// The verify pass of list l.  in: where its compress pass left the members (their compressed sizes); st: where its decompress pass did.
// The table up, ONE launch, the stats block down; then the rows, and the histograms where the caller wants them.
int SuiteRun::verify(size_t l, const LbRunState &in, const LbRunState &st) {
    size_t tiles = 0;
    for (size_t i = 0; i < m; i++) {
        if (!rb_fits(mem.len(lo + i)) || !rb_fits(st.len[i])) { ls[l].big = lo + i; return RSN_OK; }
        tiles += rb_tiles(mem.len(lo + i), st.len[i]);
    }
    const bool first = !verified, cnt = first ? out.counting() : out.h_dec != nullptr;
    const RbLayout lay = verify_layout(first, tiles, m, cnt);
    void *hp, *dp;
    int rc = pinned_buf(c, lay.bytes + 16, &hp); if (rc) return rc;
    rc = dev_buf(c, Slot::LB_VERIFY, lay.bytes + 16, &dp); if (rc) return rc;
    RbEntry *tab = (RbEntry *)((uint8_t *)hp + lay.table);
    tiles = 0;
    for (size_t i = 0; i < m; i++)
        for (size_t t = 0, k = rb_tiles(mem.len(lo + i), st.len[i]); t < k; t++)
            tab[tiles++] = RbEntry{orig[i], st.at[i], (uint32_t)mem.len(lo + i), (uint32_t)st.len[i], (uint32_t)i, (uint32_t)t};
    rc = members_verify(c, s, first, tab, tiles, m, cnt, dp); if (rc) return rc;
    {
        const size_t down = rb_stats_bytes(lay);
        const hipError_t e = copy_async((uint8_t *)hp + lay.words, (const uint8_t *)dp + lay.words, down, hipMemcpyDeviceToHost, s);
        if (e != hipSuccess) return c.fail(RSN_ERR_DEVICE, "the download of %zu bytes failed: %s", down, hipGetErrorString(e));
    }
    rc = stream_synced(c, s); if (rc) return rc;
    verified = true;
    const unsigned long long *words = (const unsigned long long *)((const uint8_t *)hp + lay.words);
    for (size_t i = 0; i < m; i++) {
        rsn_roundtrip_member &o = out.res[l * n + lo + i];
        o.original_n = mem.len(lo + i); o.compressed_n = in.len[i]; o.decompressed_n = st.len[i];
        o.first_difference = words[i] ? ~words[i] : (o.original_n == o.decompressed_n ? UINT64_MAX : std::min(o.original_n, o.decompressed_n));
        o.lossless = o.first_difference == UINT64_MAX;
    }
    if (!cnt) return RSN_OK;
    const uint32_t *rows = (const uint32_t *)((const uint8_t *)hp + lay.hists);
    uint32_t *dec_rows = out.h_dec ? out.h_dec + (l * n + lo) * SUITE_HIST_WORDS : nullptr;
    if (!first) { memcpy(dec_rows, rows, m * SUITE_HIST_BYTES); return RSN_OK; }
    if (out.rows) memcpy(out.rows + lo * RB_HIST_WORDS, rows, m * RB_HIST_BYTES);
    if (!out.h_orig && !dec_rows) return RSN_OK;
    for (size_t i = 0; i < m; i++) {                                      // the rows split: the original's half, then the decompressed half
        if (out.h_orig) memcpy(out.h_orig + (lo + i) * SUITE_HIST_WORDS, rows + i * RB_HIST_WORDS, SUITE_HIST_BYTES);
        if (dec_rows) memcpy(dec_rows + i * SUITE_HIST_WORDS, rows + i * RB_HIST_WORDS + SUITE_HIST_WORDS, SUITE_HIST_BYTES);
    }
    return RSN_OK;
}

// list l from the node it ends at (`in`: where that node left the members): the decompress pass -- steps L .. 2 L - 1 of its round trip,
// from the arena the compress pass did not end in -- and the verify pass
int SuiteRun::list_finish(size_t l, const LbRunState &in) {
    SuiteListState &q = ls[l];
    const size_t L = p.ln[l];
    if (L && q.limit <= L) return RSN_OK;                                 // (the list has failed in or right behind its compress pass: the run only looked for an earlier failure)
    LbRunState st;
    st.at = in.at; st.len = in.len;
    const size_t before = q.fd.step;
    const int rc = layers_batch_steps(c, s, false, p.lp[l], L, q.limit - L, L & 1, lo, m, nullptr, st, got.data(), q.fd);
    if (rc && q.fd.step == before) return rc;
    if (rc) { q.limit = L + q.fd.step; return RSN_OK; }
    if (q.limit < 2 * L || q.big != LB_NONE) return RSN_OK;
    return verify(l, in, st);
}

// node v and everything below it; `in`: where v's step left the members
int SuiteRun::node_walk(size_t v, const LbRunState &in) {
    const SuiteNode &node = p.tree.nodes[v];
    if (!node.ends.empty()) { const int rc = list_finish(node.ends[0], in); if (rc) return rc; }
    const size_t step = node.depth;                                       // a child's compress step, counted as a call of one of its lists alone counts it
    for (size_t kid : node.kids) {
        bool wanted = false;
        for (size_t l : p.under[kid]) wanted = wanted || ls[l].limit > step;
        if (!wanted) continue;
        const SuiteNode &k = p.tree.nodes[kid];
        LbRunState st;
        st.at = in.at; st.len = in.len;
        LbFailure f;
        int rc = layers_batch_steps(c, s, true, &k.layer, 1, 1, step & 1, lo, m, k.kept ? keep[kid].data() : nullptr, st, got.data(), f);
        if (rc && f.step == LB_NONE) return rc;
        if (rc) {                                                         // the step's failure is every list's that still went this far
            f.step = step;
            for (size_t l : p.under[kid]) if (ls[l].limit > step) { ls[l].fc = f; ls[l].limit = step; }
            continue;
        }
        if (st.tight != LB_NONE) return c.fail(RSN_ERR_DEVICE, "layers: internal error: member %zu outgrew the kept slot of its compress bound", st.tight);
        rc = node_walk(kid, st); if (rc) return rc;
    }
    return RSN_OK;
}

// every list's answer once the runs are through: its code, its rows zeroed when it failed, the equal lists' copies, list_rc and best;
// the call's answer is the lowest failing list's, prefixed: with "list <l>: " in front (the suite)
int suite_answers(Ctx &c, const SuitePlan &p, const std::vector<SuiteListState> &ls, size_t n, const SuiteOut &out, bool prefixed) {
    const size_t n_lists = ls.size();
    rsn_roundtrip_member *res = out.res;
    std::vector<int> code(n_lists, RSN_OK);
    std::vector<std::string> msg(n_lists);
    for (size_t l : p.ran()) {
        const SuiteListState &q = ls[l];
        if (q.fc.step != LB_NONE) code[l] = layers_batch_failure(c, true, p.lp[l], p.ln[l], q.fc);
        else if (q.fd.step != LB_NONE) code[l] = layers_batch_failure(c, false, p.lp[l], p.ln[l], q.fd);
        else if (q.big != LB_NONE) code[l] = roundtrip_big_failure(c, q.big);
        if (code[l]) { msg[l] = c.err; memset(res + l * n, 0, n * sizeof *res); }
    }
    for (const SuiteNode &node : p.tree.nodes)                            // equal lists: the rows of the one that ran
        for (size_t k = 1; k < node.ends.size(); k++) {
            const size_t from = node.ends[0], to = node.ends[k];
            code[to] = code[from]; msg[to] = msg[from];
            memcpy(res + to * n, res + from * n, n * sizeof *res);
            if (out.h_dec && !code[from]) memcpy(out.h_dec + to * n * SUITE_HIST_WORDS, out.h_dec + from * n * SUITE_HIST_WORDS, n * SUITE_HIST_BYTES);
        }
    if (out.list_rc) for (size_t l = 0; l < n_lists; l++) out.list_rc[l] = code[l];
    if (out.best)
        for (size_t i = 0; i < n; i++)
            out.best[i] = suite_best(n_lists, [&](size_t l) { return code[l] == RSN_OK; }, [&](size_t l) { return res[l * n + i].compressed_n; });
    for (size_t l = 0; l < n_lists; l++)
        if (code[l]) return prefixed ? c.fail(code[l], "list %zu: %s", l, msg[l].c_str()) : c.fail(code[l], "%s", msg[l].c_str());
    return RSN_OK;
}
}  // namespace

// The arguments have been checked and out.res zeroed.  slots: what the call's gate gives back.  A failure of the call as a whole zeroes
// every row and leaves list_rc and best alone.
static int suite_batch_flow(Ctx &c, hipStream_t s, size_t n, const LbMembers &mem, size_t n_lists, const rsn_layer_list *lists, unsigned long long slots, bool prefixed,
                            const SuiteOut &out) {
    auto zeroed = [&](int code) { memset(out.res, 0, n_lists * n * sizeof *out.res); return code; };
    const SuitePlan p = suite_plan(mem, n, n_lists, lists, out.counting());
    Admission gate(c, slots); gate.admit(p.most, ADMIT_FROM);
    std::vector<SuiteListState> ls(n_lists);
    for (size_t l : p.ran()) ls[l].limit = 2 * p.ln[l];
    for (const LbRun &r : p.runs) {
        bool any = false;
        for (size_t l : p.ran()) any = any || p.ln[l] == 0 || ls[l].limit > 0;
        if (!any) break;                                                  // (every list has failed at its first step: no earlier failure is left to find)
        SuiteRun run{c, s, mem, n, p, out, ls, r.lo, r.hi - r.lo};
        LbRunState st0;                                                   // up, ONCE for all lists; the host form's inputs stay in LB_STAGE to the end of the run
        int rc = layers_batch_enter(c, s, mem, r.lo, run.m, st0); if (rc) return zeroed(rc);
        run.orig = st0.at; run.got.assign(run.m, 0);
        rc = run.carve(st0); if (rc) return zeroed(rc);
        rc = run.node_walk(SUITE_ROOT, st0); if (rc) return zeroed(rc);
    }
    return suite_answers(c, p, ls, n, out, prefixed);
}

// the members of the round trip's and the suite's host forms, behind the arrays' own null checks
static int roundtrip_members_host(Ctx &c, size_t n, const uint8_t *const *ins, const size_t *lens) {
    for (size_t i = 0; i < n; i++) if (!ins[i] && lens[i]) return c.fail(RSN_ERR_ARG, "member %zu: null argument", i);
    return RSN_OK;
}
// ... and of their device forms: batch_dev_args' rules on d_in; these calls write no caller memory on the device
static int roundtrip_members_dev(Ctx &c, size_t n, const rsn_dev_member *mem) {
    for (size_t i = 0; i < n; i++) {
        if (!mem[i].d_in && mem[i].n) return c.fail(RSN_ERR_ARG, "member %zu: null argument", i);
        if (mem[i].d_out || mem[i].out_cap) return c.fail(RSN_ERR_ARG, "member %zu: d_out and out_cap are reserved in a round trip: NULL and 0", i);
        if ((uintptr_t)mem[i].d_in & 15) return c.fail(RSN_ERR_ARG, "member %zu: layers: device buffers must be 16-byte aligned", i);
    }
    return RSN_OK;
}

static int layers_roundtrip_batch_host(size_t n, const uint8_t *const *ins, const size_t *lens, const int *layers, size_t n_layers, rsn_roundtrip_member *res, uint32_t *hists) {
    Ctx &c = ctx();
    if (n == 0) return RSN_OK;
    if (!ins || !lens || !res) return c.fail(RSN_ERR_ARG, "null argument");
    memset(res, 0, n * sizeof *res);
    int rc = roundtrip_members_host(c, n, ins, lens); if (rc) return rc;
    rc = layers_check(c, layers, n_layers); if (rc) return rc;
    rc = ctx_init(c); if (rc) return rc;                                  // (no device: RSN_ERR_DEVICE -- there is no CPU path)
    const rsn_layer_list one{layers, n_layers};
    return suite_batch_flow(c, c.own_stream, n, LbMembers{ins, lens, nullptr}, 1, &one, slotset::ROUNDTRIP_BATCH_CALL, false, SuiteOut{res, nullptr, nullptr, nullptr, hists, nullptr});
}

static int layers_roundtrip_batch_dev(size_t n, const rsn_dev_member *mem, const int *layers, size_t n_layers, rsn_roundtrip_member *res, uint32_t *hists, void *stream) {
    Ctx &c = ctx(); hipStream_t s;
    if (n == 0) return RSN_OK;
    if (!mem || !res) return c.fail(RSN_ERR_ARG, "null argument");
    memset(res, 0, n * sizeof *res);
    int rc = roundtrip_members_dev(c, n, mem); if (rc) return rc;
    rc = layers_check(c, layers, n_layers); if (rc) return rc;
    rc = dev_prologue(c, stream, &s); if (rc) return rc;
    const rsn_layer_list one{layers, n_layers};
    return suite_batch_flow(c, s, n, LbMembers{nullptr, nullptr, mem}, 1, &one, slotset::ROUNDTRIP_BATCH_CALL, false, SuiteOut{res, nullptr, nullptr, nullptr, hists, nullptr});
}

// the layer lists of a suite call, behind the arrays and members: a null array, too many lists, then every list as layers_check takes it
static int suite_lists_check(Ctx &c, size_t n_lists, const rsn_layer_list *lists, const rsn_roundtrip_member *res) {
    if (!lists || !res) return c.fail(RSN_ERR_ARG, "null argument");
    if (n_lists > RSN_SUITE_LISTS_MAX) return c.fail(RSN_ERR_ARG, "%zu layer lists: at most %d in one call", n_lists, RSN_SUITE_LISTS_MAX);
    for (size_t l = 0; l < n_lists; l++) {
        const int rc = layers_check(c, lists[l].layers, lists[l].n_layers);
        if (rc) { const std::string m = c.err; return c.fail(rc, "list %zu: %s", l, m.c_str()); }
    }
    return RSN_OK;
}

static int layers_suite_batch_host(size_t n, const uint8_t *const *ins, const size_t *lens, size_t n_lists, const rsn_layer_list *lists, rsn_roundtrip_member *res, int *list_rc,
                                   uint32_t *h_orig, uint32_t *h_dec, uint32_t *best) {
    Ctx &c = ctx();
    if (n == 0) return RSN_OK;
    if (res && n_lists) memset(res, 0, n_lists * n * sizeof *res);
    if (!ins || !lens) return c.fail(RSN_ERR_ARG, "null argument");
    int rc = roundtrip_members_host(c, n, ins, lens); if (rc) return rc;
    if (n_lists == 0) return RSN_OK;
    rc = suite_lists_check(c, n_lists, lists, res); if (rc) return rc;
    rc = ctx_init(c); if (rc) return rc;                                  // (no device: RSN_ERR_DEVICE -- there is no CPU path)
    return suite_batch_flow(c, c.own_stream, n, LbMembers{ins, lens, nullptr}, n_lists, lists, slotset::SUITE_BATCH_CALL, true, SuiteOut{res, list_rc, h_orig, h_dec, nullptr, best});
}

static int layers_suite_batch_dev(size_t n, const rsn_dev_member *mem, size_t n_lists, const rsn_layer_list *lists, rsn_roundtrip_member *res, int *list_rc,
                                  uint32_t *h_orig, uint32_t *h_dec, uint32_t *best, void *stream) {
    Ctx &c = ctx(); hipStream_t s;
    if (n == 0) return RSN_OK;
    if (res && n_lists) memset(res, 0, n_lists * n * sizeof *res);
    if (!mem) return c.fail(RSN_ERR_ARG, "null argument");
    int rc = roundtrip_members_dev(c, n, mem); if (rc) return rc;
    if (n_lists == 0) return RSN_OK;
    rc = suite_lists_check(c, n_lists, lists, res); if (rc) return rc;
    rc = dev_prologue(c, stream, &s); if (rc) return rc;
    return suite_batch_flow(c, s, n, LbMembers{nullptr, nullptr, mem}, n_lists, lists, slotset::SUITE_BATCH_CALL, true, SuiteOut{res, list_rc, h_orig, h_dec, nullptr, best});
}

static int layers_roundtrip(const uint8_t *in, size_t n, const int *layers, size_t n_layers, rsn_roundtrip_result *res, uint8_t **compressed, size_t *compressed_n) {
    Ctx &c = ctx();
    if (!res || (!in && n) || (compressed && !compressed_n)) return c.fail(RSN_ERR_ARG, "null argument");
    memset(res, 0, sizeof *res);
    if (compressed) { *compressed = nullptr; *compressed_n = 0; }
    int rc = layers_check(c, layers, n_layers); if (rc) return rc;
    rc = ctx_init(c); if (rc) return rc;
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    rsn_roundtrip_result r;
    memset(&r, 0, sizeof r);
    r.original_n = n;
    HostBlock comp;
    const auto t0 = now();
    if (n <= layers_chain_max()) {                                        // a call of this size is its launches: the single host calls, and the host counts
        size_t cn = 0, dn = 0;
        HostBlock dec;
        rc = layers_host(true, in, n, layers, n_layers, &comp.p, &cn); if (rc) return rc;
        const auto t1 = now();
        rc = layers_host(false, comp.p, cn, layers, n_layers, &dec.p, &dn); if (rc) return rc;
        for (size_t i = 0; i < n; i++) r.hist_original[in[i]]++;
        for (size_t i = 0; i < dn; i++) r.hist_decompressed[dec.p[i]]++;
        const size_t m = std::min(n, dn);
        size_t at = 0;
        while (at < m && in[at] == dec.p[at]) at++;
        r.first_difference = at == m && n == dn ? UINT64_MAX : at;
        r.compressed_n = cn; r.decompressed_n = dn;
        r.compress_ms = ms(t0, t1); r.decompress_ms = ms(t1, now());
    } else {
        hipStream_t s = c.own_stream;
        const size_t need = round_up(n, 16) + 64 + layers_need(true, layers, n_layers, n) + 2 * n;
        Admission gate(c, slotset::LAYERED_CALL); gate.admit(need, ADMIT_FROM);
        void *d_up; rc = stage_input(c, s, Slot::L_IN, in, n, &d_up); if (rc) return rc;
        const uint8_t *d_in = (const uint8_t *)d_up;
        const uint8_t *d_c; size_t cn = 0;
        rc = run_chain(c, s, true, layers, n_layers, d_in, n, Slot::L_A, nullptr, 0, &d_c, &cn); if (rc) return rc;
        if (compressed) { size_t down = 0; rc = result_from_dev(c, s, d_c, cn, &comp.p, &down); if (rc) return rc; }
        const auto t1 = now();
        const uint8_t *d_d; size_t dn = 0;
        rc = run_chain(c, s, false, layers, n_layers, d_c, cn, d_c == (const uint8_t *)c.buf(Slot::L_A).p ? Slot::L_B : Slot::L_A, nullptr, 0, &d_d, &dn); if (rc) return rc;
        void *p, *hp;
        rc = dev_buf(c, Slot::L_STAT, 513 * 8 + 64, &p); if (rc) return rc;
        unsigned long long *d_stat = (unsigned long long *)p;
        rc = byte_hist256_dev(c, s, d_in, n, d_stat); if (rc) return rc;
        rc = byte_hist256_dev(c, s, d_d, dn, d_stat + 256); if (rc) return rc;
        rc = bytes_differ_dev(c, s, d_in, d_d, std::min(n, dn), d_stat + 512); if (rc) return rc;
        rc = pinned_buf(c, 513 * 8, &hp); if (rc) return rc;
        RSN_HIP(copy_async(hp, d_stat, 513 * 8, hipMemcpyDeviceToHost, s));
        RSN_HIP(hipStreamSynchronize(s));
        const unsigned long long *h = (const unsigned long long *)hp;
        for (int b = 0; b < 256; b++) { r.hist_original[b] = h[b]; r.hist_decompressed[b] = h[256 + b]; }
        r.first_difference = h[512] != ~0ull ? h[512] : (n == dn ? UINT64_MAX : (uint64_t)std::min(n, dn));
        r.compressed_n = cn; r.decompressed_n = dn;
        r.compress_ms = ms(t0, t1); r.decompress_ms = ms(t1, now());
    }
    r.lossless = r.first_difference == UINT64_MAX;
    *res = r;
    if (compressed) { *compressed = comp.release(); *compressed_n = (size_t)r.compressed_n; }
    return RSN_OK;
}

static void rsn_prof_reset_impl(void) {
    Ctx &c = ctx();
    g_copy_count.h2d.store(0); g_copy_count.d2h.store(0);
    prof_collect(c);
    for (auto &s : c.slots) { s.launches = 0; s.total_ms = 0; }
}
static int rsn_prof_get_impl(rsn_prof_entry *entries, int cap) {
    Ctx &c = ctx();
    prof_collect(c);
    int k = 0;
    for (auto &s : c.slots) {
        if (!s.launches) continue;
        if (k < cap && entries) {
            snprintf(entries[k].name, sizeof entries[k].name, "%s", s.name.c_str());
            entries[k].launches = s.launches;
            entries[k].total_ms = s.total_ms;
        }
        k++;
    }
    return k;
}

static int64_t rsn_huffman_table_impl(const uint8_t *in, size_t n, uint32_t *runes, uint64_t *freqs, uint64_t *codes, uint8_t *lens, size_t cap) {
    Ctx &c = ctx();
    if (n == 0) return c.fail(RSN_ERR_EMPTY, "huffman: empty input");
    int rc = ctx_init(c); if (rc) return rc;
    hipStream_t s = c.own_stream;
    void *d_in;
    rc = stage_input(c, s, Slot::STAGE_IN, in, n, &d_in); if (rc) return rc;
    HuffTree t; HuffCodes hc; size_t dummy = 0;
    rc = huff_encode_dev(c, s, (const uint8_t *)d_in, n, nullptr, 0, &dummy, &t, &hc);
    if (rc) return rc;
    for (size_t k = 0; k < hc.dfs.size() && k < cap; k++) {
        const uint32_t id = hc.dfs[k];
        runes[k] = t.rune[id]; freqs[k] = t.freq[id]; codes[k] = hc.code[id]; lens[k] = hc.len[id];
    }
    return (int64_t)hc.dfs.size();
}

static int64_t rsn_huffman_plan_impl(const uint32_t *runes, const uint64_t *counts, size_t n_syms, uint32_t *out_runes, uint64_t *out_codes,
                         uint8_t *out_lens, uint8_t *header, size_t header_cap, size_t *header_len) {
    Ctx &c = ctx();
    std::vector<HuffSym> syms(n_syms);
    for (size_t i = 0; i < n_syms; i++) syms[i] = {runes[i], counts[i]};
    std::sort(syms.begin(), syms.end(), [](const HuffSym &a, const HuffSym &b) { return a.rune < b.rune; });
    std::string hdr;
    emit_header(syms, hdr);
    if (header_len) *header_len = hdr.size();
    if (header) { if (hdr.size() > header_cap) return c.fail(RSN_ERR_CAPACITY, "header needs %zu bytes", hdr.size()); memcpy(header, hdr.data(), hdr.size()); }
    HuffTree t; HuffCodes hc; std::string msg;
    if (!build_tree(syms, t, msg)) return c.fail(RSN_ERR_EMPTY, "%s", msg.c_str());
    if (!assign_codes(t, hc, msg)) return c.fail(RSN_ERR_LIMIT, "%s", msg.c_str());
    for (size_t k = 0; k < hc.dfs.size(); k++) {
        const uint32_t id = hc.dfs[k];
        out_runes[k] = t.rune[id]; out_codes[k] = hc.code[id]; out_lens[k] = hc.len[id];
    }
    return (int64_t)hc.dfs.size();
}

static int64_t rsn_huffman_slice_cuts_impl(const uint8_t *in, size_t n, int shards, size_t *cuts, size_t cap) {
    Ctx &c = ctx();
    if ((!in && n) || !cuts) return c.fail(RSN_ERR_ARG, "null argument");
    if (n == 0) return c.fail(RSN_ERR_EMPTY, "huffman: empty input");
    std::vector<size_t> cut;
    huff_slice_cuts(in, n, shards, cut);
    if (cut.size() > cap) return c.fail(RSN_ERR_CAPACITY, "%zu cuts, room for %zu", cut.size(), cap);
    for (size_t i = 0; i < cut.size(); i++) cuts[i] = cut[i];
    return (int64_t)cut.size() - 1;
}

static int64_t rsn_huffman_parse_header_impl(const uint8_t *header, size_t n, uint32_t *runes, uint64_t *counts, size_t cap) {
    Ctx &c = ctx();
    std::vector<HuffSym> syms; std::string msg;
    if (!parse_header(header, n, syms, msg)) return c.fail(RSN_ERR_FORMAT, "%s", msg.c_str());
    for (size_t i = 0; i < syms.size() && i < cap; i++) { runes[i] = syms[i].rune; counts[i] = syms[i].freq; }
    return (int64_t)syms.size();
}


// ---- the entry points of rsn.h: each runs its implementation inside guarded_call (rsn_helpers.h) -- a std::bad_alloc, a
// std::system_error or anything else thrown on this side becomes a negative code and a message, never std::terminate in the host
// (engine.go:315-328 can recover a panic the shim raises from a code; nothing recovers a dead process).  A host-buffer call that
// ends that way hands out nothing: *out stays NULL.
namespace {
int boundary_error(int code, const char *m) noexcept { try { ctx().err = m; } catch (...) {} return code; }
// the three forms: a call that hands out nothing; one with (out, out_n); one with (n, outs, out_lens) -- what was handed out before the throw goes back
template <class F> auto guarded(F f) noexcept { return guarded_call<decltype(f())>(f, boundary_error); }
template <class F> int guarded_out(uint8_t **out, size_t *out_n, F f) noexcept {
    return guarded_call<int>(f, [&](int code, const char *m) { if (out && *out) { result_free(*out); *out = nullptr; } if (out_n) *out_n = 0; return boundary_error(code, m); });
}
template <class F> int guarded_outs(size_t n, uint8_t **outs, size_t *out_lens, F f) noexcept {
    return guarded_call<int>(f, [&](int code, const char *m) { if (outs && out_lens) drop_results(n, outs, out_lens); return boundary_error(code, m); });
}
// ... and the batch calls on device buffers: something thrown leaves every out_lens[i] 0, as every failure but RSN_ERR_CAPACITY does
template <class F> int guarded_lens(size_t n, const rsn_dev_member *members, size_t *out_lens, F f) noexcept {
    return guarded_call<int>(f, [&](int code, const char *m) { if (members && out_lens) for (size_t i = 0; i < n; i++) out_lens[i] = 0; return boundary_error(code, m); });
}
const Codec &HUFF_ENC = codec(RSN_LAYER_HUFFMAN, true), &HUFF_DEC = codec(RSN_LAYER_HUFFMAN, false), &LZSS_ENC = codec(RSN_LAYER_LZSS, true), &LZSS_DEC = codec(RSN_LAYER_LZSS, false);
}  // namespace

extern "C" {
int rsn_device_set(int device) { return guarded([&] { return rsn_device_set_impl(device); }); }
int rsn_device_count(void) { return guarded([&] { return rsn_device_count_impl(); }); }
void rsn_trim(void) { guarded([&] { rsn_trim_impl(); return 0; }); }
void rsn_free(void *p) { guarded([&] { result_free(p); return 0; }); }
int rsn_huffman_compress_dev(const void *d_in, size_t n, void *d_out, size_t out_cap, size_t *out_n, void *stream) { return guarded([&] { return dev_codec(HUFF_ENC, d_in, n, 0, d_out, out_cap, out_n, stream); }); }
int rsn_huffman_decompress_dev(const void *d_in, size_t n, void *d_out, size_t out_cap, size_t *out_n, void *stream) { return guarded([&] { return dev_codec(HUFF_DEC, d_in, n, 0, d_out, out_cap, out_n, stream); }); }
int rsn_lzss_compress_dev(const void *d_in, size_t n, int64_t window, void *d_out, size_t out_cap, size_t *out_n, void *stream) { return guarded([&] { return dev_codec(LZSS_ENC, d_in, n, window, d_out, out_cap, out_n, stream); }); }
int rsn_lzss_decompress_dev(const void *d_in, size_t n, void *d_out, size_t out_cap, size_t *out_n, void *stream) { return guarded([&] { return dev_codec(LZSS_DEC, d_in, n, 0, d_out, out_cap, out_n, stream); }); }
int rsn_huffman_compress(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n) { return guarded_out(out, out_n, [&] { return rsn_huffman_compress_impl(in, n, out, out_n); }); }
int rsn_huffman_decompress(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n) { return guarded_out(out, out_n, [&] { return rsn_huffman_decompress_impl(in, n, out, out_n); }); }
int rsn_lzss_compress(const uint8_t *in, size_t n, int64_t window, uint8_t **out, size_t *out_n) { return guarded_out(out, out_n, [&] { return rsn_lzss_compress_impl(in, n, window, out, out_n); }); }
int rsn_lzss_compress_legacy(const uint8_t *in, size_t n, int64_t window, uint8_t **out, size_t *out_n) { return guarded_out(out, out_n, [&] { return rsn_lzss_compress_legacy_impl(in, n, window, out, out_n); }); }
int rsn_lzss_decompress(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n) { return guarded_out(out, out_n, [&] { return rsn_lzss_decompress_impl(in, n, out, out_n); }); }
int rsn_huffman_compress_batch(size_t n_chunks, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens) { return guarded_outs(n_chunks, outs, out_lens, [&] { return rsn_huffman_compress_batch_impl(n_chunks, ins, lens, outs, out_lens); }); }
int rsn_huffman_decompress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens) { return guarded_outs(n, outs, out_lens, [&] { return rsn_huffman_decompress_batch_impl(n, ins, lens, outs, out_lens); }); }
int rsn_lzss_compress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, int64_t window, uint8_t **outs, size_t *out_lens) { return guarded_outs(n, outs, out_lens, [&] { return rsn_lzss_compress_batch_impl(n, ins, lens, window, outs, out_lens); }); }
int rsn_lzss_decompress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens) { return guarded_outs(n, outs, out_lens, [&] { return rsn_lzss_decompress_batch_impl(n, ins, lens, outs, out_lens); }); }
int rsn_arithmetic_compress(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n) { return guarded_out(out, out_n, [&] { return arithmetic_single(true, in, n, out, out_n); }); }
int rsn_arithmetic_decompress(const uint8_t *in, size_t n, uint8_t **out, size_t *out_n) { return guarded_out(out, out_n, [&] { return arithmetic_single(false, in, n, out, out_n); }); }
int rsn_arithmetic_compress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens) { return guarded_outs(n, outs, out_lens, [&] { return arithmetic_batch(true, n, ins, lens, outs, out_lens); }); }
int rsn_arithmetic_decompress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, uint8_t **outs, size_t *out_lens) { return guarded_outs(n, outs, out_lens, [&] { return arithmetic_batch(false, n, ins, lens, outs, out_lens); }); }
int rsn_arithmetic_compress_dev(const void *d_in, size_t n, void *d_out, size_t out_cap, size_t *out_n, void *stream) { return guarded([&] { return arithmetic_dev(true, d_in, n, d_out, out_cap, out_n, stream); }); }
int rsn_arithmetic_decompress_dev(const void *d_in, size_t n, void *d_out, size_t out_cap, size_t *out_n, void *stream) { return guarded([&] { return arithmetic_dev(false, d_in, n, d_out, out_cap, out_n, stream); }); }
int rsn_lzss_compress_batch_dev(size_t n, const rsn_dev_member *members, int64_t window, size_t *out_lens, void *stream) { return guarded_lens(n, members, out_lens, [&] { return lzss_batch_dev(true, n, members, window, out_lens, stream); }); }
int rsn_lzss_decompress_batch_dev(size_t n, const rsn_dev_member *members, size_t *out_lens, void *stream) { return guarded_lens(n, members, out_lens, [&] { return lzss_batch_dev(false, n, members, 0, out_lens, stream); }); }
int rsn_huffman_compress_batch_dev(size_t n, const rsn_dev_member *members, size_t *out_lens, void *stream) { return guarded_lens(n, members, out_lens, [&] { return huffman_batch_dev(true, n, members, out_lens, stream); }); }
int rsn_huffman_decompress_batch_dev(size_t n, const rsn_dev_member *members, size_t *out_lens, void *stream) { return guarded_lens(n, members, out_lens, [&] { return huffman_batch_dev(false, n, members, out_lens, stream); }); }
int rsn_arithmetic_compress_batch_dev(size_t n, const rsn_dev_member *members, size_t *out_lens, void *stream) { return guarded_lens(n, members, out_lens, [&] { return arithmetic_batch_dev(true, n, members, out_lens, stream); }); }
int rsn_arithmetic_decompress_batch_dev(size_t n, const rsn_dev_member *members, size_t *out_lens, void *stream) { return guarded_lens(n, members, out_lens, [&] { return arithmetic_batch_dev(false, n, members, out_lens, stream); }); }
int rsn_huffman_compress_sharded(const uint8_t *in, size_t n, int shards, uint8_t **out, size_t *out_n) { return guarded_out(out, out_n, [&] { return rsn_huffman_compress_sharded_impl(in, n, shards, out, out_n); }); }
int rsn_layers_compress(const uint8_t *in, size_t n, const int *layers, size_t n_layers, uint8_t **out, size_t *out_n) { return guarded_out(out, out_n, [&] { return layers_host(true, in, n, layers, n_layers, out, out_n); }); }
int rsn_layers_decompress(const uint8_t *in, size_t n, const int *layers, size_t n_layers, uint8_t **out, size_t *out_n) { return guarded_out(out, out_n, [&] { return layers_host(false, in, n, layers, n_layers, out, out_n); }); }
int rsn_layers_compress_dev(const void *d_in, size_t n, const int *layers, size_t n_layers, void *d_out, size_t out_cap, size_t *out_n, void *stream) { return guarded([&] { return layers_dev(true, d_in, n, layers, n_layers, d_out, out_cap, out_n, stream); }); }
int rsn_layers_decompress_dev(const void *d_in, size_t n, const int *layers, size_t n_layers, void *d_out, size_t out_cap, size_t *out_n, void *stream) { return guarded([&] { return layers_dev(false, d_in, n, layers, n_layers, d_out, out_cap, out_n, stream); }); }
int rsn_layers_compress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, const int *layers, size_t n_layers, uint8_t **outs, size_t *out_lens) { return guarded_outs(n, outs, out_lens, [&] { return layers_batch_host(true, n, ins, lens, layers, n_layers, outs, out_lens); }); }
int rsn_layers_decompress_batch(size_t n, const uint8_t *const *ins, const size_t *lens, const int *layers, size_t n_layers, uint8_t **outs, size_t *out_lens) { return guarded_outs(n, outs, out_lens, [&] { return layers_batch_host(false, n, ins, lens, layers, n_layers, outs, out_lens); }); }
int rsn_layers_compress_batch_dev(size_t n, const rsn_dev_member *members, const int *layers, size_t n_layers, size_t *out_lens, void *stream) { return guarded_lens(n, members, out_lens, [&] { return layers_batch_dev(true, n, members, layers, n_layers, out_lens, stream); }); }
int rsn_layers_decompress_batch_dev(size_t n, const rsn_dev_member *members, const int *layers, size_t n_layers, size_t *out_lens, void *stream) { return guarded_lens(n, members, out_lens, [&] { return layers_batch_dev(false, n, members, layers, n_layers, out_lens, stream); }); }
int rsn_layers_roundtrip(const uint8_t *in, size_t n, const int *layers, size_t n_layers, rsn_roundtrip_result *res, uint8_t **compressed, size_t *compressed_n) {
    return guarded_call<int>([&] { return layers_roundtrip(in, n, layers, n_layers, res, compressed, compressed_n); }, [&](int code, const char *m) {
        if (res) memset(res, 0, sizeof *res);
        if (compressed && *compressed) { result_free(*compressed); *compressed = nullptr; }
        if (compressed_n) *compressed_n = 0;
        return boundary_error(code, m);
    });
}
int rsn_layers_roundtrip_batch(size_t n, const uint8_t *const *ins, const size_t *lens, const int *layers, size_t n_layers, rsn_roundtrip_member *res, uint32_t *hists) {
    return guarded_call<int>([&] { return layers_roundtrip_batch_host(n, ins, lens, layers, n_layers, res, hists); },
                             [&](int code, const char *m) { if (res) memset(res, 0, n * sizeof *res); return boundary_error(code, m); });
}
int rsn_layers_roundtrip_batch_dev(size_t n, const rsn_dev_member *members, const int *layers, size_t n_layers, rsn_roundtrip_member *res, uint32_t *hists, void *stream) {
    return guarded_call<int>([&] { return layers_roundtrip_batch_dev(n, members, layers, n_layers, res, hists, stream); },
                             [&](int code, const char *m) { if (res) memset(res, 0, n * sizeof *res); return boundary_error(code, m); });
}
int rsn_layers_suite_batch(size_t n, const uint8_t *const *ins, const size_t *lens, size_t n_lists, const rsn_layer_list *lists, rsn_roundtrip_member *res, int *list_rc,
                           uint32_t *hists_original, uint32_t *hists_decompressed, uint32_t *best) {
    return guarded_call<int>([&] { return layers_suite_batch_host(n, ins, lens, n_lists, lists, res, list_rc, hists_original, hists_decompressed, best); },
                             [&](int code, const char *m) { if (res) memset(res, 0, n_lists * n * sizeof *res); return boundary_error(code, m); });
}
int rsn_layers_suite_batch_dev(size_t n, const rsn_dev_member *members, size_t n_lists, const rsn_layer_list *lists, rsn_roundtrip_member *res, int *list_rc,
                               uint32_t *hists_original, uint32_t *hists_decompressed, uint32_t *best, void *stream) {
    return guarded_call<int>([&] { return layers_suite_batch_dev(n, members, n_lists, lists, res, list_rc, hists_original, hists_decompressed, best, stream); },
                             [&](int code, const char *m) { if (res) memset(res, 0, n_lists * n * sizeof *res); return boundary_error(code, m); });
}
void rsn_prof_copied(uint64_t *h2d_bytes, uint64_t *d2h_bytes) { guarded([&] { if (h2d_bytes) *h2d_bytes = g_copy_count.h2d.load(); if (d2h_bytes) *d2h_bytes = g_copy_count.d2h.load(); return 0; }); }
void rsn_prof_enable(int on) { guarded([&] { ctx().prof = on != 0; g_copy_count.on.store(on != 0); return 0; }); }
void rsn_prof_reset(void) { guarded([&] { rsn_prof_reset_impl(); return 0; }); }
int rsn_prof_get(rsn_prof_entry *entries, int cap) { return guarded([&] { return rsn_prof_get_impl(entries, cap); }); }
int64_t rsn_huffman_table(const uint8_t *in, size_t n, uint32_t *runes, uint64_t *freqs, uint64_t *codes, uint8_t *lens, size_t cap) { return guarded([&] { return rsn_huffman_table_impl(in, n, runes, freqs, codes, lens, cap); }); }
int64_t rsn_huffman_plan(const uint32_t *runes, const uint64_t *counts, size_t n_syms, uint32_t *out_runes, uint64_t *out_codes, uint8_t *out_lens, uint8_t *header, size_t header_cap, size_t *header_len) { return guarded([&] { return rsn_huffman_plan_impl(runes, counts, n_syms, out_runes, out_codes, out_lens, header, header_cap, header_len); }); }
int64_t rsn_huffman_slice_cuts(const uint8_t *in, size_t n, int shards, size_t *cuts, size_t cap) { return guarded([&] { return rsn_huffman_slice_cuts_impl(in, n, shards, cuts, cap); }); }
int64_t rsn_huffman_parse_header(const uint8_t *header, size_t n, uint32_t *runes, uint64_t *counts, size_t cap) { return guarded([&] { return rsn_huffman_parse_header_impl(header, n, runes, counts, cap); }); }

}  // extern "C"
