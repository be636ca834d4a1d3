// lds_pad.h -- a launch that carries an LDS footprint its kernel never touches (a "pad": the dispatcher then cannot place the workgroup
// on a compute unit whose LDS another latency chain holds; knobs.h: validate_lds_pad, verify_pad_kb), written once.
//   clamp:    the pad passed is min(wanted, limit - static): the device's LDS per workgroup less the kernel's own, asked once per
//             (kernel, device); the same key says when MaxDynamicSharedMemorySize has to be raised, and that call is checked;
//   fallback: an error already pending -> the plain launch, the error left for the caller. Otherwise the padded launch's result is
//             read; a runtime that refuses the footprint gets the plain launch, now and from then on for that (kernel, device).
// At most two reads of the error state per padded launch, no synchronisation. The decision takes its runtime as a template parameter
// and needs no HIP header (tests/lds_pad_check.cpp compiles it for the host); the HIP side follows it.
#pragma once
#include <stdint.h>
#include <atomic>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

namespace lwk {

constexpr int kPadMaxDevices = 64;                 // ordinals beyond launch without a pad
constexpr uint32_t kPadFreeBytes = 48u * 1024u;    // dynamic LDS a kernel may ask for without the attribute
constexpr uint32_t kPadRoomUnknown = 0xffffffffu;

struct PadCache {   // one per kernel (a static beside its launch), one entry per device ordinal
    struct Dev {
        std::atomic<uint32_t> room{kPadRoomUnknown};   // limit - static
        std::atomic<uint32_t> raised{0};               // what MaxDynamicSharedMemorySize was last set to
        std::atomic<bool> refused{false};              // a pad was refused here: plain launches from then on
    } dev[kPadMaxDevices];
};

// Rt: lds_static(), lds_limit() -> bytes; raise(bytes), peek(), take() -> an error code, 0 = none (peek leaves the pending error in
// place, take clears it); launch(dynamic_lds_bytes)
template <class Rt>
void launch_padded(PadCache &cache, int device, uint32_t wanted, Rt &&rt) {
    if (!wanted || device < 0 || device >= kPadMaxDevices) return rt.launch(0u);
    PadCache::Dev &d = cache.dev[device];
    if (d.refused.load(std::memory_order_relaxed) || rt.peek() != 0) return rt.launch(0u);
    uint32_t room = d.room.load(std::memory_order_relaxed);
    if (room == kPadRoomUnknown) {
        const uint32_t stat = rt.lds_static(), limit = rt.lds_limit();
        d.room.store(room = stat < limit ? limit - stat : 0u, std::memory_order_relaxed);
    }
    const uint32_t pad = wanted < room ? wanted : room;
    if (!pad) return rt.launch(0u);
    if (pad > kPadFreeBytes && pad > d.raised.load(std::memory_order_relaxed)) {
        if (rt.raise(pad) == 0) d.raised.store(pad, std::memory_order_relaxed);
        else wanted = 0;   // refused before the launch
    }
    if (wanted) rt.launch(pad);
    if (rt.take() == 0 && wanted) return;
    d.refused.store(true, std::memory_order_relaxed);
    rt.launch(0u);   // its error state stays, like any other launch's
}

#if defined(__HIPCC__)
template <class Launch>
struct HipPadRt {
    const void *kernel;
    int device;
    Launch &launch;
    uint32_t lds_static() const {   // a failed query (either one): no room, cached -- no pad for this (kernel, device) for good; its error stays pending for the caller
        hipFuncAttributes a;
        return hipFuncGetAttributes(&a, kernel) == hipSuccess ? (uint32_t)a.sharedSizeBytes : kPadRoomUnknown;
    }
    uint32_t lds_limit() const {
        int v = 0;
        return hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, device) == hipSuccess && v > 0 ? (uint32_t)v : 0u;
    }
    int raise(uint32_t bytes) const { return (int)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes); }
    int peek() const { return (int)hipPeekAtLastError(); }
    int take() const { return (int)hipGetLastError(); }
};

// launch(lds): enqueues `kernel` with lds bytes of dynamic LDS (hipLaunchKernelGGL); called once, or twice where the pad is refused
template <class Launch>
void launch_padded(PadCache &cache, const void *kernel, uint32_t wanted, Launch &&launch) {
    int device = -1;
    if (wanted && hipGetDevice(&device) != hipSuccess) device = -1;
    launch_padded(cache, device, wanted, HipPadRt<Launch>{kernel, device, launch});
}
#endif

}  // namespace lwk
