// fk20.cuh -- the per-lane pieces of the FK20 cell proof engine (fk20.hip, fk20_api.hip) that need no LDS and no
// lane exchange, host and device: the geometry of the window table over the 8192 transformed bases, the signed-digit recoding of an
// MSM scalar, the recoding of the 128 fixed roots over the endomorphism split, the product of an XYZZ point with such a root, and the
// steps of the two 128-point transforms over G1 as functions of a position, so that a host loop over the positions runs the same code
// as the 128 lanes of k_fk20_transforms (tools/fk20_check.hip holds all of it against g1.cuh's plain double-and-add).
#pragma once
#include "g1.cuh"
#include "glv.cuh"

namespace lwk {

constexpr int kFk20Points = 128;                 // transform length: one point per cell proof
constexpr int kFk20Terms = 64;                   // terms of one of the 128 MSMs
constexpr int kFk20Bases = kFk20Points * kFk20Terms;
constexpr int kFk20DefaultBits = 8;
constexpr int kFk20RootDigits = 132;             // bytes per recoded root: 130 digit pairs (a 128-bit half in NAF has up to 129) + padding
constexpr int kFk20Roots = 2 * kFk20Points;      // w^e for e < 128, then w^e / 128

// ---- the window table: rows d = 1 .. 2^(c-1) of [2^(c j)]B for every base B and window j ---------------------------------------------
// Digits are signed, -2^(c-1) .. 2^(c-1); the top window takes the carry and is never negated, so its value, at most 2^wtop (wtop = the
// bits of a 255-bit scalar it holds), must be one of the 2^(c-1) rows: widths with wtop <= c - 1 are supported (4, 6, 7, 8, 9).
struct Fk20Plan {
    int c, nw;
    uint32_t h;          // rows per (base, window)
    size_t rows;         // of the whole table
};
LWK_HD Fk20Plan fk20_plan(int bits) {
    Fk20Plan p{};
    if (bits < 4 || bits > 9) return p;
    const int nw = (255 + bits - 1) / bits, wtop = 255 - bits * (nw - 1);
    if (wtop > bits - 1) return p;
    p.c = bits;
    p.nw = nw;
    p.h = 1u << (bits - 1);
    p.rows = (size_t)kFk20Bases * nw * p.h;
    return p;
}
// row of multiple d (1 .. h) of window j of base Y^_i[m]: one MSM's 64 terms lie side by side
LWK_HD size_t fk20_row(const Fk20Plan &p, uint32_t i, uint32_t m, uint32_t j, uint32_t d) {
    return (((size_t)m * kFk20Terms + i) * p.nw + j) * p.h + (d - 1);
}

// the next digit of a canonical scalar: its low c bits leave k, the carry of the digit below comes in and this one's goes out.
// top: the last window, whose value (at most 2^(c-1), see above) is taken as it is
LWK_HD void fk20_next_digit(uint32_t k[8], int c, bool top, uint32_t &carry, uint32_t &mag, uint32_t &negative) {
    const uint32_t raw = (k[0] & ((1u << c) - 1u)) + carry;
#pragma unroll
    for (int w = 0; w < 7; w++) k[w] = (k[w] >> c) | (k[w + 1] << (32 - c));
    k[7] >>= c;
    negative = (!top && raw > (1u << (c - 1))) ? 1u : 0u;
    mag = negative ? (1u << c) - raw : raw;
    carry = negative;
}

// ---- the fixed roots --------------------------------------------------------------------------------------------------------------
// w128 = w4096^32 in Montgomery form (w4096 = 7^((r-1)/4096): fr_ops.hip's kOmegaRaw)
LWK_HD Fr fk20_w128() {
    const uint32_t omega_raw[8] = {0xa5d36306u, 0xe206da11u, 0x378fbf96u, 0x0ad1347bu, 0xe0f8245fu, 0xfc3e8acfu, 0xa0f704f4u, 0x564c0a11u};
    Fr w = fe_from_raw<FrParams>(omega_raw);
    for (int i = 0; i < 5; i++) w = sqr(w);
    return w;
}

// root `idx` as a canonical integer: w^idx for idx < 128, w^(idx - 128) / 128 beyond (the inverse transform's last level carries the scale)
inline void fk20_root_raw(uint32_t raw[8], int idx) {
    const Fr w = fk20_w128();
    Fr v = Fr::one();
    for (int e = 0; e < (idx & (kFk20Points - 1)); e++) v = v * w;
    if (idx >= kFk20Points) {
        const uint32_t n_raw[8] = {(uint32_t)kFk20Points, 0, 0, 0, 0, 0, 0, 0};
        v = v * inv(fe_from_raw<FrParams>(n_raw));
    }
    fe_to_raw<FrParams>(raw, v);
}

// a canonical k < r as digit pairs over the endomorphism split k = lo + hi z^2 (glv.cuh): both 128-bit halves in non-adjacent form,
// byte t = the two digits of weight 2^t: bits 0-1 lo's (0 none, 1 plus, 2 minus), bits 2-3 hi's
inline void fk20_recode_root(uint8_t digits[kFk20RootDigits], const uint32_t k[8]) {
    uint32_t half[2][4];
    split_by_z2_barrett(half[0], half[1], k);
    for (int t = 0; t < kFk20RootDigits; t++) digits[t] = 0;
    for (int s = 0; s < 2; s++) {
        uint32_t n[5] = {half[s][0], half[s][1], half[s][2], half[s][3], 0};
        for (int t = 0; t < kFk20RootDigits - 2; t++) {
            if (n[0] & 1u) {
                if ((n[0] & 3u) == 1u) {
                    digits[t] |= (uint8_t)(1u << (2 * s));
                    n[0] -= 1u;   // (odd: no borrow)
                } else {
                    digits[t] |= (uint8_t)(2u << (2 * s));
                    uint64_t cy = 1;   // n += 1
                    for (int i = 0; i < 5 && cy; i++) {
                        cy += n[i];
                        n[i] = (uint32_t)cy;
                        cy >>= 32;
                    }
                }
            }
            for (int i = 0; i < 4; i++) n[i] = (n[i] >> 1) | (n[i + 1] << 31);
            n[4] >>= 1;
        }
    }
}

LWK_HD F29<2> fk20_beta29() {
    uint32_t raw[12];
    g1_beta_raw(raw);
    return f29_from_raw32(raw);
}

LWK_HD G1Xyzz29 fk20_neg(const G1Xyzz29 &p) {
    G1Xyzz29 r = p;
    r.y = neg(p.y) * F29<1>::one();   // back below 2p
    return r;
}

// [k]P for the recoded root k and any P, complete: [lo]P + [hi](-phi(P)), phi(X, Y, ZZ, ZZZ) = (beta X, Y, ZZ, ZZZ), over 130 shared
// doublings; a digit adds or subtracts its point. P = O and k = 0 give O.
LWK_HD G1Xyzz29 fk20_mul_root(const G1Xyzz29 &p, const uint8_t *__restrict__ digits, const F29<2> &beta) {
    if (p.is_inf()) return G1Xyzz29::infinity();
    const F29<2> y_plus = p.y * F29<1>::one(), y_minus = neg(p.y) * F29<1>::one();
    const F29<2> x_phi = p.x * beta;
    G1Xyzz29 acc = G1Xyzz29::infinity();
#pragma unroll 1
    for (int t = kFk20RootDigits - 3; t >= 0; t--) {
        acc = xyzz_dbl(acc);
        const uint32_t code = digits[t];
        if (code & 3u) {
            G1Xyzz29 q = p;
            q.y = (code & 3u) == 1u ? y_plus : y_minus;
            acc = xyzz_add(acc, q);
        }
        if (code & 12u) {
            G1Xyzz29 q = p;
            q.x = x_phi;
            q.y = (code & 12u) == 4u ? y_minus : y_plus;   // -phi(P) carries -Y
            acc = xyzz_add(acc, q);
        }
    }
    return acc;
}

// ---- the two transforms, a position at a time ----------------------------------------------------------------------------------------
// Inverse (decimation in time): input E in bit-reversed positions, levels of half-width h = 1, 2, .. 64; position pos of a level first
// takes its root (fk20_inverse_root: 0 = none), then its sum or difference (fk20_inverse_out). The last level carries the 1/128 and
// leaves h_0 .. h_63 in positions 0 .. 63; the upper half, which FK20 discards, becomes O.
// Forward (decimation in frequency): levels h = 64, 32, .. 1; a position first takes its sum or difference (fk20_forward_out), then its
// root (fk20_forward_root). Output position k holds F[rev7(k)]: proof k.
LWK_HD int fk20_inverse_root(uint32_t pos, uint32_t h) {
    if (h == kFk20Points / 2) return kFk20Points + (int)((pos & h) ? ((kFk20Points - (pos & (h - 1))) & (kFk20Points - 1)) : 0);
    if (!(pos & h)) return 0;
    const uint32_t e = (pos & (h - 1)) * (kFk20Points / 2 / h);
    return (int)((kFk20Points - e) & (kFk20Points - 1));
}
LWK_HD G1Xyzz29 fk20_inverse_out(const G1Xyzz29 *x, uint32_t pos, uint32_t h) {
    if (h == kFk20Points / 2) return (pos & h) ? G1Xyzz29::infinity() : xyzz_add(x[pos], x[pos + h]);
    if (pos & h) return xyzz_add(x[pos - h], fk20_neg(x[pos]));
    return xyzz_add(x[pos], x[pos + h]);
}
LWK_HD G1Xyzz29 fk20_forward_out(const G1Xyzz29 *x, uint32_t pos, uint32_t h) {
    if (pos & h) return xyzz_add(x[pos - h], fk20_neg(x[pos]));
    return xyzz_add(x[pos], x[pos + h]);
}
LWK_HD int fk20_forward_root(uint32_t pos, uint32_t h) {
    if (!(pos & h)) return 0;
    return (int)((pos & (h - 1)) * (kFk20Points / 2 / h));
}

}  // namespace lwk
