// Host-side helpers shared by the translation units of libdcv_hip.so (declared in dcv_common.hpp); no kernels.  A unit of its own so
// that det_reduce.hip stays the reduction alone and a unit that only sizes a grid (patch_dgrad.hip, attn_bwd3.hip) names what it uses.
#include <atomic>
#include "dcv_common.hpp"

// CU count of the current device, queried once per device (an immutable device property, cached; no allocation, no sync)
int dcv_cu_count() {
    static std::atomic<int> cached[16];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 16) dev = 0;
    int n = cached[dev].load(std::memory_order_relaxed);
    if (n <= 0) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cached[dev].store(n, std::memory_order_relaxed);
    }
    return n;
}
