// abi_guard.h -- nothing may unwind across the C ABI: every entry point that sizes host vectors by its arguments runs its body through this.
#pragma once
#include <new>
#include "engine.h"

namespace lwk {

template <class F>
C_KZG_RET guarded(const char *what, F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        set_error("%s: out of host memory", what);
        return C_KZG_MALLOC;
    } catch (...) {
        set_error("%s: unexpected exception", what);
        return C_KZG_ERROR;
    }
}

}  // namespace lwk
