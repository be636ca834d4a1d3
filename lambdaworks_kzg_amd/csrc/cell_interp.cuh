// cell_interp.cuh -- what the kernels that read EIP-7594 cells share (cells_verify.hip: the batch verification's column sums;
// recover.hip: the recovery's per-cell interpolation): an element's canonical integer from its bytes, c_k, and the 64-point inverse
// transform over a cell's coset with its scaling. Cell k's elements are the evaluations on h_k <w64>, h_k = w8192^bitrev7(k), in
// bit-reversed order -- exactly the order a decimation-in-time transform consumes.
#pragma once
#include "kernels.h"

namespace lwk {

// the canonical integer of a 32-byte element from its two 16-byte halves as they lie in memory
__device__ __forceinline__ void element_limbs(uint32_t t[8], const uint4 &first, const uint4 &second, int le) {
    if (le) {
        t[0] = first.x, t[1] = first.y, t[2] = first.z, t[3] = first.w;
        t[4] = second.x, t[5] = second.y, t[6] = second.z, t[7] = second.w;
    } else {
        t[7] = __builtin_bswap32(first.x), t[6] = __builtin_bswap32(first.y), t[5] = __builtin_bswap32(first.z), t[4] = __builtin_bswap32(first.w);
        t[3] = __builtin_bswap32(second.x), t[2] = __builtin_bswap32(second.y), t[1] = __builtin_bswap32(second.z), t[0] = __builtin_bswap32(second.w);
    }
}

// c_k = w128^bitrev7(k) = w4096^(32 bitrev7(k)), Montgomery form, from the forward twiddles w^e, e < 2048 (w^2048 = -1)
__device__ __forceinline__ Fr c_of_cell(const Fr *tw_fwd, uint32_t k) {
    const uint32_t e = 32 * (__brev(k & 127u) >> 25);
    return e < kBlobElems / 2 ? tw_fwd[e] : neg(tw_fwd[e - kBlobElems / 2]);
}

// stage s (0 .. 5) of the 64-point decimation-in-time inverse transform of buf[0 .. 63] in place: butterfly b of 32. The caller puts a
// barrier between the stages. buf holds canonical integers and keeps them (a Montgomery-form twiddle times a raw value is raw).
__device__ __forceinline__ void cell_idft64_stage(Fr *buf, const Fr *__restrict__ tw_inv, int s, uint32_t b) {
    const uint32_t half = 1u << s, q = b & (half - 1);
    const uint32_t i0 = ((b >> s) << (s + 1)) + q, i1 = i0 + half;
    // w_(2 half)^-q = w64^-(q 32 / half) = w4096^-(64 q (32 >> s))
    const Fr u = buf[i0], x = tw_inv[64 * q * (32u >> s)] * buf[i1];
    buf[i0] = u + x;
    buf[i1] = u - x;
}

// h_k^-t in Montgomery form, h_k = w8192^bitrev7(k): the exponent e = bitrev7(k) t < 8192; w8192^-e = w4096^-(e >> 1) (times
// w8192^-1 if e is odd; inv_omega8192_mont: that constant's limbs). Coefficient t of the transform above times this and 1/64 is
// coefficient t of the cell's interpolant.
__device__ __forceinline__ Fr cell_coeff_twist(const Fr *__restrict__ tw_inv, uint32_t k, uint32_t t, const uint32_t *inv_omega8192_mont) {
    const uint32_t e = (__brev(k) >> 25) * t, half_e = e >> 1;
    Fr sc = half_e < kBlobElems / 2 ? tw_inv[half_e] : neg(tw_inv[half_e - kBlobElems / 2]);
    if (e & 1u) {
        Fr c;
#pragma unroll
        for (int j = 0; j < 8; j++) c.l[j] = inv_omega8192_mont[j];
        sc = sc * c;
    }
    return sc;
}

}  // namespace lwk
