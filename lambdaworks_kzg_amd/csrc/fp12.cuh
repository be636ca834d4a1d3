// fp12.cuh -- the BLS12-381 pairing tower and the optimal-ate pairing check over the device field (field.cuh's 12 x 32-bit Montgomery Fp),
// compiled for the device (verify_each.hip: one pairing check per verified item) and for the host (tools/pairing_dev_check.hip).
//
// Same tower and same construction as the host's pairing.hip:
//   Fp2 = Fp[u]/(u^2 + 1), Fp6 = Fp2[v]/(v^3 - (1 + u)), Fp12 = Fp6[w]/(w^2 - v);
//   Miller loop over |x| = 0xd201000000010000 against FIXED G2 points: the slope and constant term of every line (63 tangents + 5 chords)
//   come from a table made once per point (pairing.hip: fixed_q_lines), so a step is one Fp12 squaring and a sparse line product per pair;
//   final exponentiation = easy part (p^6 - 1)(p^2 + 1), hard part through the x-chain with cyclotomic squarings.
// The Frobenius constants are baked (fp12_consts.inc, tools/gen_pairing_consts.py). Every value is canonical (< p), so is_one is an
// exact comparison.
//
// On the device the Fp12 / Fp6 products are real functions (as the Fp product is, field.cuh: fe_mul_call): a pairing check is ~18k
// field products, and inlining every level of the tower would make a kernel of megabytes.
#pragma once
#include "field.cuh"
#include "fp2.h"

namespace lwk {

#define LWK_TOWER_FN static __host__ __device__ __noinline__

namespace fp12c {
#include "fp12_consts.inc"
}

constexpr int kPairingLines = 68;                      // lines of one Miller loop: 63 doublings + 5 additions
constexpr unsigned long long kPairingAbsX = 0xd201000000010000ull;  // |x|, x < 0

// one line of a fixed-Q Miller loop: l(P) = c0 + (-lambda x_P) v + (y_P) v w  (c0 = lambda x_T - y_T)
struct alignas(16) PairingLine {
    Fp2 lambda, c0;
};

// ---- Fp2 -----------------------------------------------------------------------------------------------------------------------

LWK_HD Fp2 f2add(const Fp2 &a, const Fp2 &b) { return {a.c0 + b.c0, a.c1 + b.c1}; }
LWK_HD Fp2 f2sub(const Fp2 &a, const Fp2 &b) { return {a.c0 - b.c0, a.c1 - b.c1}; }
LWK_HD Fp2 f2neg(const Fp2 &a) { return {neg(a.c0), neg(a.c1)}; }
LWK_HD Fp2 f2dbl(const Fp2 &a) { return f2add(a, a); }
LWK_HD Fp2 f2conj(const Fp2 &a) { return {a.c0, neg(a.c1)}; }
LWK_HD Fp2 f2zero() { return {Fp::zero(), Fp::zero()}; }
LWK_HD Fp2 f2one() { return {Fp::one(), Fp::zero()}; }
LWK_HD bool f2is_zero(const Fp2 &a) { return a.c0.is_zero() && a.c1.is_zero(); }
LWK_HD bool f2eq(const Fp2 &a, const Fp2 &b) { return a.c0 == b.c0 && a.c1 == b.c1; }
LWK_HD Fp2 f2mul(const Fp2 &a, const Fp2 &b) {  // three products
    Fp t0 = a.c0 * b.c0, t1 = a.c1 * b.c1;
    return {t0 - t1, (a.c0 + a.c1) * (b.c0 + b.c1) - t0 - t1};
}
LWK_HD Fp2 f2sqr(const Fp2 &a) {  // two products
    Fp m = a.c0 * a.c1;
    return {(a.c0 + a.c1) * (a.c0 - a.c1), m + m};
}
LWK_HD Fp2 f2mul_fp(const Fp2 &a, const Fp &s) { return {a.c0 * s, a.c1 * s}; }
LWK_HD Fp2 f2mul_xi(const Fp2 &a) { return {a.c0 - a.c1, a.c0 + a.c1}; }  // * (1 + u)
LWK_HD Fp2 f2inv(const Fp2 &a) {
    Fp n = inv(sqr(a.c0) + sqr(a.c1));
    return {a.c0 * n, neg(a.c1 * n)};
}
LWK_HD Fp fp_const(const uint32_t *l) {
    Fp r;
#pragma unroll
    for (int i = 0; i < 12; i++) r.l[i] = l[i];
    return r;
}
LWK_HD Fp2 gamma1(int k) { return {fp_const(fp12c::GAMMA1[k][0]), fp_const(fp12c::GAMMA1[k][1])}; }
LWK_HD Fp gamma2(int k) { return fp_const(fp12c::GAMMA2[k]); }

// ---- Fp6 -----------------------------------------------------------------------------------------------------------------------

struct Fp6 {
    Fp2 c0, c1, c2;
};
LWK_HD Fp6 f6add(const Fp6 &a, const Fp6 &b) { return {f2add(a.c0, b.c0), f2add(a.c1, b.c1), f2add(a.c2, b.c2)}; }
LWK_HD Fp6 f6sub(const Fp6 &a, const Fp6 &b) { return {f2sub(a.c0, b.c0), f2sub(a.c1, b.c1), f2sub(a.c2, b.c2)}; }
LWK_HD Fp6 f6neg(const Fp6 &a) { return {f2neg(a.c0), f2neg(a.c1), f2neg(a.c2)}; }
LWK_HD Fp6 f6mul_v(const Fp6 &a) { return {f2mul_xi(a.c2), a.c0, a.c1}; }
LWK_HD Fp6 f6zero() { return {f2zero(), f2zero(), f2zero()}; }
LWK_HD Fp6 f6one() { return {f2one(), f2zero(), f2zero()}; }
LWK_TOWER_FN Fp6 f6mul(const Fp6 &a, const Fp6 &b) {  // six Fp2 products (Karatsuba)
    Fp2 t0 = f2mul(a.c0, b.c0), t1 = f2mul(a.c1, b.c1), t2 = f2mul(a.c2, b.c2);
    Fp6 r;
    r.c0 = f2add(t0, f2mul_xi(f2sub(f2sub(f2mul(f2add(a.c1, a.c2), f2add(b.c1, b.c2)), t1), t2)));
    r.c1 = f2add(f2sub(f2sub(f2mul(f2add(a.c0, a.c1), f2add(b.c0, b.c1)), t0), t1), f2mul_xi(t2));
    r.c2 = f2add(f2sub(f2sub(f2mul(f2add(a.c0, a.c2), f2add(b.c0, b.c2)), t0), t2), t1);
    return r;
}
// f * (a + b v): five Fp2 products
LWK_TOWER_FN Fp6 f6mul_by_01(const Fp6 &f, const Fp2 &a, const Fp2 &b) {
    Fp2 t0 = f2mul(f.c0, a), t1 = f2mul(f.c1, b);
    Fp6 r;
    r.c0 = f2add(t0, f2mul_xi(f2sub(f2mul(f2add(f.c1, f.c2), b), t1)));
    r.c1 = f2sub(f2sub(f2mul(f2add(f.c0, f.c1), f2add(a, b)), t0), t1);
    r.c2 = f2add(t1, f2mul(f.c2, a));
    return r;
}
LWK_HD Fp6 f6inv(const Fp6 &a) {
    Fp2 c0 = f2sub(f2sqr(a.c0), f2mul_xi(f2mul(a.c1, a.c2)));
    Fp2 c1 = f2sub(f2mul_xi(f2sqr(a.c2)), f2mul(a.c0, a.c1));
    Fp2 c2 = f2sub(f2sqr(a.c1), f2mul(a.c0, a.c2));
    Fp2 t = f2inv(f2add(f2mul(a.c0, c0), f2mul_xi(f2add(f2mul(a.c2, c1), f2mul(a.c1, c2)))));
    return {f2mul(c0, t), f2mul(c1, t), f2mul(c2, t)};
}

// ---- Fp12 ----------------------------------------------------------------------------------------------------------------------

struct Fp12 {
    Fp6 c0, c1;
};
LWK_HD Fp12 f12one() { return {f6one(), f6zero()}; }
LWK_HD Fp12 f12conj(const Fp12 &a) { return {a.c0, f6neg(a.c1)}; }
LWK_TOWER_FN Fp12 f12mul(const Fp12 &a, const Fp12 &b) {  // three Fp6 products
    Fp6 t0 = f6mul(a.c0, b.c0), t1 = f6mul(a.c1, b.c1);
    return {f6add(t0, f6mul_v(t1)), f6sub(f6sub(f6mul(f6add(a.c0, a.c1), f6add(b.c0, b.c1)), t0), t1)};
}
// a^2 by the complex method over Fp6[w]/(w^2 - v): two Fp6 products
LWK_TOWER_FN Fp12 f12sqr(const Fp12 &a) {
    Fp6 ab = f6mul(a.c0, a.c1);
    Fp6 t = f6sub(f6sub(f6mul(f6add(a.c0, a.c1), f6add(a.c0, f6mul_v(a.c1))), ab), f6mul_v(ab));
    return {t, f6add(ab, ab)};
}
// f * l for l = (a + b v) + (c v) w, c in Fp: 36 Fp products instead of 54
LWK_TOWER_FN Fp12 f12mul_by_line(const Fp12 &f, const Fp2 &a, const Fp2 &b, const Fp &c) {
    Fp6 t0 = f6mul_by_01(f.c0, a, b);
    Fp6 t1 = {f2mul_xi(f2mul_fp(f.c1.c2, c)), f2mul_fp(f.c1.c0, c), f2mul_fp(f.c1.c1, c)};  // f.c1 * (c v)
    Fp2 bc = {b.c0 + c, b.c1};
    Fp6 cross = f6sub(f6sub(f6mul_by_01(f6add(f.c0, f.c1), a, bc), t0), t1);
    return {f6add(t0, f6mul_v(t1)), cross};
}
LWK_TOWER_FN Fp12 f12inv(const Fp12 &a) {  // one Fp inversion
    Fp6 t = f6inv(f6sub(f6mul(a.c0, a.c0), f6mul_v(f6mul(a.c1, a.c1))));
    return {f6mul(a.c0, t), f6neg(f6mul(a.c1, t))};
}
LWK_HD bool f12is_one(const Fp12 &a) {
    return f2eq(a.c0.c0, f2one()) && f2is_zero(a.c0.c1) && f2is_zero(a.c0.c2) && f2is_zero(a.c1.c0) && f2is_zero(a.c1.c1) &&
           f2is_zero(a.c1.c2);
}
LWK_HD bool f12eq(const Fp12 &a, const Fp12 &b) {
    return f2eq(a.c0.c0, b.c0.c0) && f2eq(a.c0.c1, b.c0.c1) && f2eq(a.c0.c2, b.c0.c2) && f2eq(a.c1.c0, b.c1.c0) &&
           f2eq(a.c1.c1, b.c1.c1) && f2eq(a.c1.c2, b.c1.c2);
}

// a^(p^2): the coefficient of w^(2i+j) (v^i w^j) is scaled by GAMMA2[2i+j]; Fp2 is fixed by x -> x^(p^2)
LWK_TOWER_FN Fp12 frob_p2(const Fp12 &a) {
    Fp12 r;
    r.c0.c0 = a.c0.c0;
    r.c0.c1 = f2mul_fp(a.c0.c1, gamma2(2));
    r.c0.c2 = f2mul_fp(a.c0.c2, gamma2(4));
    r.c1.c0 = f2mul_fp(a.c1.c0, gamma2(1));
    r.c1.c1 = f2mul_fp(a.c1.c1, gamma2(3));
    r.c1.c2 = f2mul_fp(a.c1.c2, gamma2(5));
    return r;
}
// a^p: Fp2 coefficients conjugated, the coefficient of w^(2i+j) scaled by GAMMA1[2i+j]
LWK_TOWER_FN Fp12 frob_p(const Fp12 &a) {
    Fp12 r;
    r.c0.c0 = f2conj(a.c0.c0);
    r.c0.c1 = f2mul(f2conj(a.c0.c1), gamma1(2));
    r.c0.c2 = f2mul(f2conj(a.c0.c2), gamma1(4));
    r.c1.c0 = f2mul(f2conj(a.c1.c0), gamma1(1));
    r.c1.c1 = f2mul(f2conj(a.c1.c1), gamma1(3));
    r.c1.c2 = f2mul(f2conj(a.c1.c2), gamma1(5));
    return r;
}

// a^2 for a in the cyclotomic subgroup (Granger-Scott): three Fp4 squarings, 9 Fp2 products. Coefficient order of this tower:
// g = (z0 + z4 v + z3 v^2) + (z2 + z1 v + z5 v^2) w
LWK_HD void fp4_sqr(const Fp2 &x, const Fp2 &y, Fp2 &t_even, Fp2 &t_odd) {  // (x + y s)^2, s^2 = xi
    Fp2 xy = f2mul(x, y);
    t_even = f2sub(f2sub(f2mul(f2add(x, y), f2add(f2mul_xi(y), x)), xy), f2mul_xi(xy));
    t_odd = f2dbl(xy);
}
LWK_HD Fp2 three_t_minus_two_z(const Fp2 &t, const Fp2 &z) {
    Fp2 d = f2sub(t, z);
    return f2add(f2dbl(d), t);
}
LWK_HD Fp2 three_t_plus_two_z(const Fp2 &t, const Fp2 &z) {
    Fp2 d = f2add(t, z);
    return f2add(f2dbl(d), t);
}
LWK_TOWER_FN Fp12 cyclotomic_sqr(const Fp12 &a) {
    Fp2 t0, t1, t2, t3, t4, t5;
    fp4_sqr(a.c0.c0, a.c1.c1, t0, t1);   // z0, z1
    fp4_sqr(a.c1.c0, a.c0.c2, t2, t3);   // z2, z3
    fp4_sqr(a.c0.c1, a.c1.c2, t4, t5);   // z4, z5
    Fp12 r;
    r.c0.c0 = three_t_minus_two_z(t0, a.c0.c0);
    r.c1.c1 = three_t_plus_two_z(t1, a.c1.c1);
    r.c1.c0 = three_t_plus_two_z(f2mul_xi(t5), a.c1.c0);
    r.c0.c2 = three_t_minus_two_z(t4, a.c0.c2);
    r.c0.c1 = three_t_minus_two_z(t2, a.c0.c1);
    r.c1.c2 = three_t_plus_two_z(t3, a.c1.c2);
    return r;
}

// a^x for the negative curve parameter, a in the cyclotomic subgroup (the inverse is the conjugate)
LWK_TOWER_FN Fp12 exp_by_x(const Fp12 &a) {
    Fp12 acc = a;  // bit 63
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {
        acc = cyclotomic_sqr(acc);
        if ((kPairingAbsX >> i) & 1) acc = f12mul(acc, a);
    }
    return f12conj(acc);
}

// f^((p^12 - 1) / r) == 1 ?  Easy part (p^6 - 1)(p^2 + 1); hard part by 3h = (x - 1)^2 (x + p)(x^2 + p^2 - 1) + 3 (pairing.hip)
LWK_TOWER_FN bool final_exponentiation_is_one(const Fp12 &f) {
    Fp12 t = f12mul(f12conj(f), f12inv(f));  // f^(p^6 - 1)
    t = f12mul(frob_p2(t), t);               // ^(p^2 + 1)
    Fp12 t0 = f12mul(exp_by_x(t), f12conj(t));     // t^(x - 1)
    Fp12 t1 = f12mul(exp_by_x(t0), f12conj(t0));   // t^((x - 1)^2)
    Fp12 t2 = f12mul(exp_by_x(t1), frob_p(t1));    // ^(x + p)
    Fp12 t3 = f12mul(f12mul(exp_by_x(exp_by_x(t2)), frob_p2(t2)), f12conj(t2));  // ^(x^2 + p^2 - 1)
    Fp12 tt = f12mul(t, t);
    return f12is_one(f12mul(f12mul(t3, tt), t));
}

// The Miller loop of e(P0, Q0) e(P1, Q1) against two fixed G2 points given by their line tables (kPairingLines each), one squaring per
// bit shared by both; use0 / use1 = false drops a pair (a point at infinity: its pairing is 1). Returns f already conjugated (x < 0).
LWK_TOWER_FN Fp12 miller_loop_fixed2(const Fp &px0, const Fp &py0, const PairingLine *l0, bool use0, const Fp &px1, const Fp &py1,
                                     const PairingLine *l1, bool use1) {
    Fp12 f = f12one();
    int k = 0;
#pragma unroll 1
    for (int bit = 62; bit >= 0; bit--) {
        const int steps = ((kPairingAbsX >> bit) & 1) ? 2 : 1;
        if (bit != 62) f = f12sqr(f);  // (f = 1 at the top: its square is 1)
#pragma unroll 1
        for (int s = 0; s < steps; s++, k++) {
            if (use0) {
                const PairingLine lc = l0[k];
                f = f12mul_by_line(f, lc.c0, f2neg(f2mul_fp(lc.lambda, px0)), py0);
            }
            if (use1) {
                const PairingLine lc = l1[k];
                f = f12mul_by_line(f, lc.c0, f2neg(f2mul_fp(lc.lambda, px1)), py1);
            }
        }
    }
    return f12conj(f);
}

// e(P0, Q0) e(P1, Q1) == 1 for affine P's (use = false: that P is the point at infinity)
LWK_HD bool pairing2_is_one(const Fp &px0, const Fp &py0, const PairingLine *l0, bool use0, const Fp &px1, const Fp &py1,
                            const PairingLine *l1, bool use1) {
    if (!use0 && !use1) return true;
    return final_exponentiation_is_one(miller_loop_fixed2(px0, py0, l0, use0, px1, py1, l1, use1));
}

}  // namespace lwk
