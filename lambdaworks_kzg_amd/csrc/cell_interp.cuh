// cell_interp.cuh -- what the kernels that read EIP-7594 cells share (cells_verify.hip: the column sums of a batch and of a call of
// groups, and the batch's scalars behind r; cells_verify_groups.hip: the grouped scalars; cells_verify_each.hip: the per-item
// interpolant; recover.hip: the recovery's per-cell interpolation): an element's canonical integer from its bytes, c_k, the 64-point
// inverse transform over a cell's coset with its scaling, the Fr constants of all of them (recover_consts.inc, its one home), and an
// item's scalars a_i, b_i once its kernel knows the item's power table and exponent. Cell k's elements are the evaluations on
// h_k <w64>, h_k = w8192^bitrev7(k), in bit-reversed order -- exactly the order a decimation-in-time transform consumes.
#pragma once
#include "kernels.h"
#include "glv.cuh"

namespace lwk {

namespace {   // (a copy per translation unit: the library is not built as relocatable device code)
#include "recover_consts.inc"
}  // namespace

// a constant of recover_consts.inc as a field element
__device__ __forceinline__ Fr const_fr(const uint32_t *limbs) {
    Fr c;
#pragma unroll
    for (int j = 0; j < 8; j++) c.l[j] = limbs[j];
    return c;
}

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
// w8192^-1 if e is odd). Coefficient t of the transform above times this and 1/64 is coefficient t of the cell's interpolant.
__device__ __forceinline__ Fr cell_coeff_twist(const Fr *__restrict__ tw_inv, uint32_t k, uint32_t t) {
    const uint32_t e = (__brev(k) >> 25) * t, half_e = e >> 1;
    Fr sc = half_e < kBlobElems / 2 ? tw_inv[half_e] : neg(tw_inv[half_e - kBlobElems / 2]);
    if (e & 1u) sc = sc * const_fr(kRecInvOmega8192Mont);
    return sc;
}

// h_k^-t / 64: what coefficient t of the transform above is multiplied by (recover.hip has its 1/64 in a table and takes the twist alone)
__device__ __forceinline__ Fr cell_coeff_scale(const Fr *__restrict__ tw_inv, uint32_t k, uint32_t t) {
    return cell_coeff_twist(tw_inv, k, t) * const_fr(kRecInv64Mont);
}

// scalar i of sc: raw as lo + hi z^2, the form k_vmsm_accumulate and the slices take (glv.cuh)
__device__ __forceinline__ void store_split(uint32_t *sc, size_t i, const uint32_t raw[8]) {
    uint32_t lo[4], hi[4];
    split_by_z2_barrett(lo, hi, raw);
#pragma unroll
    for (int q = 0; q < 4; q++) {
        sc[8 * i + q] = lo[q];
        sc[8 * i + 4 + q] = hi[q];
    }
}

// Item i's scalars behind r, for a lane that knows its table (tab[k] = r^(2^k), k < 32; tab[32]: the power the walk starts from) and
// its exponent e: a_i = tab[32] r^e into a_mont (Montgomery form, for the weights and the column sums), a_i and b_i = a_i c_(idx[i])
// split into sc_a / sc_b. idx[i] is below 128 (the caller's skip word or group flag keeps an unchecked index from coming here).
__device__ __forceinline__ void cell_item_scalars(const Fr *__restrict__ tab, uint32_t e, uint32_t i, const uint64_t *__restrict__ idx,
                                                  const Fr *__restrict__ tw_fwd, Fr *__restrict__ a_mont, uint32_t *__restrict__ sc_a,
                                                  uint32_t *__restrict__ sc_b) {
    Fr a = tab[32];
#pragma unroll 1
    for (int k = 0; k < 32; k++) {
        if ((e >> k) == 0) break;
        if ((e >> k) & 1u) a = a * tab[k];
    }
    a_mont[i] = a;
    const Fr b = a * c_of_cell(tw_fwd, (uint32_t)idx[i]);
    uint32_t raw[8];
    fe_to_raw<FrParams>(raw, a);
    store_split(sc_a, i, raw);
    fe_to_raw<FrParams>(raw, b);
    store_split(sc_b, i, raw);
}

}  // namespace lwk
