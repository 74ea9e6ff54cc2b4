// The library's mutable state, all of it: the dispatch overrides, the clock ring with the pass marker that brackets it, and the
// per-device memory pool behind StreamScratch.  Every other host file is stateless apart from once-per-device caches.
#include "wkv6_host.h"

#include <atomic>
#include <mutex>

namespace wkv6 {
namespace {
std::atomic<int> g_dispatch[4] = {-1, -1, -1, -1};    // by WKV6_DISPATCH_*; -1: the library's own choice

__global__ void pass_marker_kernel() {}
// the clock ring: [2 kinds][n_launches][n_slots][4] uint64 of caller-owned device memory; the launchers of one process may run on
// several threads (the autograd engine's), so the ring's description and the launch counts are read and advanced under a lock
struct ClockRing {
    std::mutex mu;
    unsigned long long* buf = nullptr;
    int slots = 0, launches = 0;
    long count[2] = {0, 0};
} g_clock;

constexpr unsigned long long SCRATCH_KEEP = 1ull << 30;
hipMemPool_t scratch_pool_of(int dev)
{
    static std::mutex mu;
    static hipMemPool_t pools[64] = {};
    if (dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lk(mu);
    if (!pools[dev]) {
        hipMemPoolProps props = {};
        props.allocType = hipMemAllocationTypePinned;
        props.location.type = hipMemLocationTypeDevice;
        props.location.id = dev;
        hipMemPool_t pool = nullptr;
        if (hipMemPoolCreate(&pool, &props) != hipSuccess) return nullptr;
        unsigned long long keep = SCRATCH_KEEP;
        (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &keep);
        pools[dev] = pool;
    }
    return pools[dev];
}
}  // namespace

int dispatch_override(int what) { return g_dispatch[what].load(std::memory_order_relaxed); }

unsigned long long* clock_claim(int kind, int* slots)
{
    std::lock_guard<std::mutex> lk(g_clock.mu);
    *slots = g_clock.slots;
    if (!g_clock.buf) return nullptr;
    const long n = g_clock.count[kind]++;
    return g_clock.buf + ((size_t)kind * g_clock.launches + (size_t)(n % g_clock.launches)) * g_clock.slots * 4;
}

void* StreamScratch::get(size_t bytes, hipStream_t stream)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    st = stream;
    hipMemPool_t pool = scratch_pool_of(dev);
    const hipError_t e = pool ? hipMallocFromPoolAsync(&ptr, bytes, pool, st) : hipMallocAsync(&ptr, bytes, st);
    if (e != hipSuccess) ptr = nullptr;
    return ptr;
}

#if defined(WKV6_STAMP) || defined(WKV6_CLOCK) || defined(WKV6_DEBUG)
unsigned long long* g_stamp_buffer = nullptr;
#endif
}  // namespace wkv6

using namespace wkv6;

extern "C" {

#if defined(WKV6_STAMP) || defined(WKV6_CLOCK) || defined(WKV6_DEBUG)
void wkv6_set_debug_buffer(void* p) { g_stamp_buffer = reinterpret_cast<unsigned long long*>(p); }
#endif

void wkv6_set_clock_ring(void* buf, int n_slots, int n_launches)
{
    std::lock_guard<std::mutex> lk(g_clock.mu);
    const bool on = buf && n_slots > 0 && n_launches > 0;
    g_clock.buf = on ? reinterpret_cast<unsigned long long*>(buf) : nullptr;
    g_clock.slots = on ? n_slots : 0;
    g_clock.launches = on ? n_launches : 0;
    g_clock.count[0] = g_clock.count[1] = 0;
}
void wkv6_clock_ring_counts(long* fwd, long* bwd)
{
    std::lock_guard<std::mutex> lk(g_clock.mu);
    if (fwd) *fwd = g_clock.count[0];
    if (bwd) *bwd = g_clock.count[1];
}
int wkv6_pass_marker(void* stream) { return to_rc(launch<pass_marker_kernel>(dim3(1), dim3(64), 0, (hipStream_t)stream)); }
int wkv6_set_dispatch(int what, int value)
{
    if (what < WKV6_DISPATCH_SPLIT || what > WKV6_DISPATCH_BI_SLOTS) return WKV6_EINVAL;
    return g_dispatch[what].exchange(value);
}

}  // extern "C"
