// carve.h -- one allocation cut into typed pieces, each rounded up to 256 bytes. With a null base it is the size probe: the same take()
// calls that place the pointers say how many bytes the block needs. No HIP header: tests/carve_check.cpp compiles it for the host.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace lwk {

struct Carver {
    uint8_t *base;
    size_t off = 0;
    explicit Carver(uint8_t *base_) : base(base_) {}
    template <class T>
    void take(T *&p, size_t bytes) {
        p = (T *)((uintptr_t)base + off);   // (an integer sum: the probe's null base takes no pointer arithmetic)
        off += (bytes + 255) & ~(size_t)255;
    }
    size_t bytes() const { return off; }
};

}  // namespace lwk
