// cell_each.cuh -- the per-lane pieces of the per-item cell verification (cells_verify_each.hip) that need no LDS
// and no lane exchange, and the reduction tree over a workgroup's 64 points that it shares with the grouped verification
// (cells_verify_groups.hip; section 4q): the scalar product of an affine point over the endomorphism split, and the two scalars of an item -- c_k and a
// coefficient of its interpolant -- as the canonical integers that product takes. Host and device (tools/cell_each_check.hip holds them
// against g1.cuh's plain double-and-add on the host).
#pragma once
#include "g1.cuh"
#include "glv.cuh"

namespace lwk {

// [lo]Q + [hi](beta x_Q, -y_Q) for affine Q and two 128-bit scalars, sharing 128 doublings. beta: g1_beta_raw in Montgomery form.
// Complete: lo = hi = 0 gives the point at infinity. (The grouped cell verification takes its scalars already split, as
// k_cellv_scalars writes them: cells_verify_groups.hip.)
LWK_HD G1Xyzz glv_mul_affine_split(const Fp &qx, const Fp &qy, const Fp &beta, const uint32_t lo[4], const uint32_t hi[4]) {
    const Fp ex = beta * qx, ey = neg(qy);
    G1Xyzz acc = G1Xyzz::infinity();
#pragma unroll 1
    for (int bit = 127; bit >= 0; bit--) {
        acc = xyzz_dbl(acc);
        const uint32_t w = bit >> 5, sh = bit & 31;
        if ((lo[w] >> sh) & 1u) acc = xyzz_madd(acc, qx, qy);
        if ((hi[w] >> sh) & 1u) acc = xyzz_madd(acc, ex, ey);
    }
    return acc;
}

// [k]Q for affine Q and a canonical k < r: k = lo + hi z^2 (glv.cuh), so [k]Q = [lo]Q + [hi](beta x_Q, -y_Q)
LWK_HD G1Xyzz glv_mul_affine(const Fp &qx, const Fp &qy, const Fp &beta, const uint32_t k[8]) {
    uint32_t lo[4], hi[4];
    split_by_z2_barrett(lo, hi, k);
    return glv_mul_affine_split(qx, qy, beta, lo, hi);
}

#if defined(__HIPCC__)
// The one piece with LDS and barriers: the 64 partial points of a 64-lane workgroup (lane t holds acc) summed pairwise over six
// levels -- lane t takes lane t + d at every level d = 1, 2, .. 32 where t is a multiple of 2 d. Two lanes may hold equal or opposite
// points, or the point at infinity: the complete addition. sh: 64 points of LDS (12 KiB) that nobody reads any more; every lane of
// the workgroup calls this; lane 0's acc is the sum afterwards.
__device__ __forceinline__ void cell_each_tree_sum(G1Xyzz &acc, G1Xyzz *sh, uint32_t t) {
#pragma unroll 1
    for (uint32_t d = 1; d < 64u; d <<= 1) {
        if ((t & (2 * d - 1)) == d) sh[t] = acc;
        __syncthreads();
        if ((t & (2 * d - 1)) == 0) acc = xyzz_add(acc, sh[t + d]);
        __syncthreads();
    }
}
#endif

// c_k (cell_interp.cuh: c_of_cell, Montgomery form) as the canonical integer the product above takes
LWK_HD void cell_each_ck_raw(uint32_t raw[8], const Fr &ck_mont) { fe_to_raw<FrParams>(raw, ck_mont); }

// coefficient t of a cell's interpolant as a canonical integer: the transform's output (a canonical integer in an Fr's limbs) times
// its scale h_k^-t / 64 (Montgomery form) -- a Montgomery product of the two is the canonical product
LWK_HD void cell_each_coeff_raw(uint32_t raw[8], const Fr &scale_mont, const Fr &value_raw) {
    const Fr c = scale_mont * value_raw;
#pragma unroll
    for (int j = 0; j < 8; j++) raw[j] = c.l[j];
}

}  // namespace lwk
