// launch.h -- host-side launch plumbing shared by every launcher of csrc/: pointer alignment, the per-device dynamic-LDS limit and
// occupancy of a kernel, and the library's environment switches (INTEGRATION.md lists them).  Host only; no kernel is launched here.
#pragma once
#include "common.h"
#include "split16.h"
#include <atomic>
#include <mutex>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

// every pointer 16-byte aligned (NULL counts as aligned: an absent optional tensor does not veto the vector path)
template <class... P>
static inline bool aligned16(const P*... p) { return (((reinterpret_cast<uintptr_t>(p) & 15) == 0) && ...); }
// the conv kernels' float4 paths need 16-B aligned rows: W % 4 == 0 and 16-B aligned tensors
static inline int conv_vec_ok(const bnerv_conv_desc& d) { return (d.W % 4 == 0 && aligned16(d.x, d.out, d.out2, d.aux0, d.aux1, d.aux2)) ? 1 : 0; }

// ---- per-device kernel attributes.  The limit and the occupancy belong to (device, kernel): one fixed table per kernel instantiation,
// indexed by the current device.  A device index beyond the table is served without the cache.
constexpr int LAUNCH_MAX_DEVICES = 16;
static inline int launch_device_slot() {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev >= LAUNCH_MAX_DEVICES) dev = -1;
    return dev;
}

// Raises KERNEL's dynamic-LDS limit on the current device to `bytes` where that exceeds what the device was last given (grow-only).
// Forward and autograd threads both launch: the raise itself is serialised, so that a smaller request cannot land after a larger one.
template <auto KERNEL>
int dyn_lds(size_t bytes, const char* name) {
    static std::atomic<size_t> given[LAUNCH_MAX_DEVICES];
    static std::mutex raise;
    const int dev = launch_device_slot();
    if (dev >= 0 && bytes <= given[dev].load(std::memory_order_acquire)) return BNERV_OK;
    std::lock_guard<std::mutex> lock(raise);
    if (dev >= 0 && bytes <= given[dev].load(std::memory_order_relaxed)) return BNERV_OK;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return bnerv_set_error(BNERV_E_LAUNCH, "%s: dynamic LDS limit of %zu bytes: %s", name, bytes, hipGetErrorString(e));
    if (dev >= 0) given[dev].store(bytes, std::memory_order_release);
    return BNERV_OK;
}

// Resident blocks per CU of KERNEL at (threads, bytes of dynamic LDS), at most `cap`; a failed lookup or 0 counts as 1.  Remembers the
// last (bytes, answer) per device: the launchers ask with one or two distinct sizes.
template <auto KERNEL>
int blocks_per_cu(int threads, size_t bytes, int cap) {
    static std::atomic<uint64_t> last[LAUNCH_MAX_DEVICES];                   // bytes << 8 | blocks; 0: nothing yet
    const int dev = launch_device_slot();
    const uint64_t seen = dev >= 0 ? last[dev].load(std::memory_order_relaxed) : 0;
    int nb = (int)(seen & 255);
    if (nb == 0 || (seen >> 8) != bytes) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(KERNEL), threads, bytes) != hipSuccess || nb < 1) nb = 1;
        if (nb > 255) nb = 255;
        if (dev >= 0) last[dev].store(((uint64_t)bytes << 8) | (uint64_t)nb, std::memory_order_relaxed);
    }
    return nb > cap ? cap : nb;
}

// ---- environment switches.  Read where they are used: some per call (tests flip them inside one process), some once per process.
static inline const char* switch_str(const char* name) { return getenv(name); }
static inline bool switch_off(const char* name) { const char* e = switch_str(name); return e && e[0] == '0'; }
static inline int switch_int(const char* name, int dflt) { const char* e = switch_str(name); return e ? atoi(e) : dflt; }

// BNERV_SPLIT_WIDE = bf16x6 (default) | bf16x3 | off: arithmetic of the wide split kernels (convbf.hip, wgrad_bfw_body.h, conv5.hip);
// -1 for off.  Read once per process.
inline int split_wide_mode() {
    static const int v = [] {
        const char* e = switch_str("BNERV_SPLIT_WIDE");
        if (!e) return (int)SP_BF16X6;
        if (!strcmp(e, "off") || !strcmp(e, "0")) return -1;
        if (!strcmp(e, "bf16x3")) return (int)SP_BF16X3;
        return (int)SP_BF16X6;
    }();
    return v;
}
// BNERV_SPLIT_WIDE_MIN_TILES: the fewest 8x32 tiles (x batch) for which the wide split kernels take a layer (measured on C1 / C3 / C4:
// 16 >= 32 >= 64 >= 256; below it the f32 kernels' split policies win).  Read per call: tests lower it to reach the kernels with small shapes.
static inline int split_wide_min_tiles() { return switch_int("BNERV_SPLIT_WIDE_MIN_TILES", 16); }
