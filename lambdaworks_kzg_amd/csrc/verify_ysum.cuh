// verify_ysum.cuh -- the arithmetic of k_verify_ysum (verify_async.hip): sum_{i < n} r^(first + i) y_i over Fr, cut into the share of
// one lane, the addition of two shares and the canonical bytes of the total. Host and device: the kernel runs these on 256 lanes and an
// LDS tree, tests/verify_ysum_check.hip runs the same functions lane after lane on a CPU against the plain field.
//
// fr28.cuh's arithmetic (Montgomery radix 2^280, lazy sums): a power in Montgomery form times the canonical integer y_i is the plain
// product r^i y_i below 2r, so a share is a limb-wise sum with one carry ripple per term -- value below 2 n r, far inside the 2^25 r a
// product's operand may have (n < 2^23) -- and the total comes back under r by one product with 2^280 mod r.
#pragma once
#include "fr28.cuh"

namespace lwk {

constexpr int kYsumLanes = 256, kYsumStepLog = 8;
static_assert(1 << kYsumStepLog == kYsumLanes, "the step r^T is the table's entry log2(T)");

LWK_HD Fr28 ysum_zero() {
    Fr28 z;
#pragma unroll
    for (int k = 0; k < 10; k++) z.l[k] = 0;
    return z;
}

LWK_HD Fr28 ysum_add(const Fr28 &a, const Fr28 &b) { return fr28_norm(fr28_add(a, b)); }

// lane t's terms i = t, t + T, t + 2T, ... < n. tab: r^(2^k) for k < 32, then r^first, in fr28's Montgomery form; y32: the y bytes in
// the mode's byte order. The lane's first power is r^first times the entries of the set bits of t, its step r^T is entry log2(T).
LWK_HD Fr28 ysum_lane(const Fr28 *tab, const uint8_t *y32, int le, uint32_t t, uint32_t n) {
    Fr28 acc = ysum_zero();
    if (t >= n) return acc;
    Fr28 p = tab[32];
#pragma unroll 1
    for (int k = 0; k < kYsumStepLog; k++)
        if ((t >> k) & 1u) p = fr28_mul(p, tab[k]);
    const Fr28 step = tab[kYsumStepLog];
#pragma unroll 1
    for (uint32_t i = t;;) {
        uint32_t w[8];
        if (le) raw_from_le<8>(w, y32 + 32 * (size_t)i);
        else raw_from_be<8>(w, y32 + 32 * (size_t)i);
        acc = ysum_add(acc, fr28_mul(p, fr28_pack(w)));
        i += kYsumLanes;
        if (i >= n) break;
        p = fr28_mul(p, step);
    }
    return acc;
}

// the total of every share -> 32 canonical big-endian bytes
LWK_HD void ysum_bytes(uint8_t *out32, const Fr28 &total) {
    uint32_t w[8];
    fr28_unpack(w, fr28_canonical(LWK_FR28_MUL_CONST(total, ONE)));
    raw_to_be<8>(out32, w);
}

}  // namespace lwk
