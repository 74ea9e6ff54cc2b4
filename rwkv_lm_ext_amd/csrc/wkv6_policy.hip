// Launch-shape policy (host side): how many workgroups the chunked kernels run on.  The library's rules decide from the shape and the
// device's CU count; wkv6_set_dispatch() (include/wkv6_amd.h) overrides them, so that tests can reach every mode at small shapes.
// (tsplit_segments, the rule of the two-level scan over T, stands beside that scan in wkv6_tsplit.hip.)
#include "wkv6_host.h"

namespace wkv6 {

int cu_count()              // compute units of the current device (0: unknown)
{
    static int cus[16] = {};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) return 0;
    if (!cus[dev]) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
        cus[dev] = prop.multiProcessorCount;
    }
    return cus[dev];
}
// two workgroups per (batch, head) when one each would leave at least half of the CUs without work
int want_split(int BH)
{
    if (const int o = dispatch_override(WKV6_DISPATCH_SPLIT); o != -1) return o != 0;
    return 2 * BH <= cu_count();
}
// workgroup slots of the persistent wkv6_bi launches: one per CU at most (0: the halves run as two launches).  An override n >= 1 pins
// min(n, BH) slots, more than the CUs included: the slots never wait for one another (workgroup-private scratch, LDS-only tags), and the
// compact side buffers' slot carve (slot * T * 64) stays inside the [B,T,C] buffers as long as slots <= BH.
int bi_slots(int BH)
{
    if (want_split(BH)) return 0;
    if (dispatch_override(WKV6_DISPATCH_BI_FUSED) == 0) return 0;
    if (const int want = dispatch_override(WKV6_DISPATCH_BI_SLOTS); want >= 1) return BH < want ? BH : want;
    const int cus = cu_count();
    return cus > 0 ? (BH < cus ? BH : cus) : 0;
}

}  // namespace wkv6
