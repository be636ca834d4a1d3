// cell_each.cuh -- the per-lane pieces of the per-item cell verification (cells_verify_each.hip) that need no LDS
// and no lane exchange: the scalar product of an affine point over the endomorphism split, and the two scalars of an item -- c_k and a
// coefficient of its interpolant -- as the canonical integers that product takes. Host and device (tools/cell_each_check.hip holds them
// against g1.cuh's plain double-and-add on the host).
#pragma once
#include "g1.cuh"
#include "glv.cuh"

namespace lwk {

// [k]Q for affine Q and a canonical k < r: k = lo + hi z^2 (glv.cuh), so [k]Q = [lo]Q + [hi](beta x_Q, -y_Q) -- two 128-bit scalars
// against Q and its image, sharing 128 doublings. beta: g1_beta_raw in Montgomery form. Complete: k = 0 gives the point at infinity.
LWK_HD G1Xyzz glv_mul_affine(const Fp &qx, const Fp &qy, const Fp &beta, const uint32_t k[8]) {
    uint32_t lo[4], hi[4];
    split_by_z2_barrett(lo, hi, k);
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
