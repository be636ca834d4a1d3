// pairing.hip -- host-side BLS12-381 optimal-ate pairing product check for the verify_* symbols.
//
// two pairings per verification stay on the host, as in the reference, whose
// KZG::verify calls BLS12381AtePairing::compute_batch from the un-vendored lambdaworks-math crate
// (call sites /root/reference/src/lib.rs:444,496,691; /root/reference/src/utils.rs:224-236). Nothing of
// that crate is available, so this is the textbook construction:
//   Fp2 = Fp[u]/(u^2+1), Fp6 = Fp2[v]/(v^3 - (1+u)), Fp12 = Fp6[w]/(w^2 - v);
//   Miller loop over |z| = 0xd201000000010000 with affine line functions on the M-type twist
//   y^2 = x^3 + 4(1+u), conjugation for z < 0;
//   final exponentiation = easy part (p^6-1)(p^2+1) by conjugation/inversion/Frobenius, hard part
//   (p^4-p^2+1)/r through the curve-parameter chain with Granger-Scott cyclotomic squarings.
// Only the accept/reject bit leaves this file, so no intermediate representation needs to match
// anything upstream.
#include "engine.h"
#include "knobs.h"
#include "fp2.h"
#include "hostfp.h"

#include <stdlib.h>
#include <string.h>

#include <stdio.h>

#include <chrono>
#include <memory>
#include <mutex>
#include <thread>
#include <vector>

namespace lwk {

unsigned host_threads();  // sha256_host.hip

namespace {

// the tower over the host representation (hostfp.h); inputs arrive as Fe-based Fp / Fp2 and are repacked at entry
struct H2 {
    HFp c0, c1;
};

inline H2 operator+(const H2 &a, const H2 &b) { return {a.c0 + b.c0, a.c1 + b.c1}; }
inline H2 operator-(const H2 &a, const H2 &b) { return {a.c0 - b.c0, a.c1 - b.c1}; }
static_assert(sizeof(H2) == 12 * sizeof(uint64_t), "fp_x86.S reads an Fp2 element as twelve consecutive limbs");
inline H2 operator*(const H2 &a, const H2 &b) {
#if defined(__x86_64__)
    if (hf_fp2_on_adx()) {  // three 768-bit products, two reductions (fp_x86.S)
        H2 r;
        lwk_fp2_mul_adx(r.c0.l, a.c0.l, b.c0.l);
        return r;
    }
#endif
    HFp t0 = a.c0 * b.c0, t1 = a.c1 * b.c1;
    return {t0 - t1, (a.c0 + a.c1) * (b.c0 + b.c1) - t0 - t1};
}
inline H2 mul_fp(const H2 &a, const HFp &s) { return {a.c0 * s, a.c1 * s}; }
inline H2 f2neg(const H2 &a) { return {neg(a.c0), neg(a.c1)}; }
inline H2 f2zero() { return {HFp::zero(), HFp::zero()}; }
inline H2 f2one() { return {HFp::one(), HFp::zero()}; }
inline bool f2is_zero(const H2 &a) { return a.c0.is_zero() && a.c1.is_zero(); }
inline bool f2eq(const H2 &a, const H2 &b) { return a.c0 == b.c0 && a.c1 == b.c1; }
inline H2 mul_xi(const H2 &a) { return {a.c0 - a.c1, a.c0 + a.c1}; }  // * (1 + u)
inline H2 f2inv(const H2 &a) {
    HFp n = inv(sqr(a.c0) + sqr(a.c1));
    return {a.c0 * n, neg(a.c1 * n)};
}

struct H6 {
    H2 c0, c1, c2;
};
inline H6 operator+(const H6 &a, const H6 &b) { return {a.c0 + b.c0, a.c1 + b.c1, a.c2 + b.c2}; }
inline H6 operator-(const H6 &a, const H6 &b) { return {a.c0 - b.c0, a.c1 - b.c1, a.c2 - b.c2}; }
inline H6 operator*(const H6 &a, const H6 &b) {
    H2 t0 = a.c0 * b.c0, t1 = a.c1 * b.c1, t2 = a.c2 * b.c2;
    H6 r;
    r.c0 = t0 + mul_xi((a.c1 + a.c2) * (b.c1 + b.c2) - t1 - t2);
    r.c1 = (a.c0 + a.c1) * (b.c0 + b.c1) - t0 - t1 + mul_xi(t2);
    r.c2 = (a.c0 + a.c2) * (b.c0 + b.c2) - t0 - t2 + t1;
    return r;
}
inline H6 f6neg(const H6 &a) { return {f2neg(a.c0), f2neg(a.c1), f2neg(a.c2)}; }
inline H6 mul_v(const H6 &a) { return {mul_xi(a.c2), a.c0, a.c1}; }
inline H6 f6zero() { return {f2zero(), f2zero(), f2zero()}; }
inline H6 f6one() { return {f2one(), f2zero(), f2zero()}; }
inline H6 f6inv(const H6 &a) {
    H2 c0 = a.c0 * a.c0 - mul_xi(a.c1 * a.c2);
    H2 c1 = mul_xi(a.c2 * a.c2) - a.c0 * a.c1;
    H2 c2 = a.c1 * a.c1 - a.c0 * a.c2;
    H2 t = f2inv(a.c0 * c0 + mul_xi(a.c2 * c1 + a.c1 * c2));
    return {c0 * t, c1 * t, c2 * t};
}

struct H12 {
    H6 c0, c1;
};
inline H12 operator*(const H12 &a, const H12 &b) {
    H6 t0 = a.c0 * b.c0, t1 = a.c1 * b.c1;
    return {t0 + mul_v(t1), (a.c0 + a.c1) * (b.c0 + b.c1) - t0 - t1};
}
// a^2 by the complex method over Fp6[w]/(w^2 - v): two Fp6 products instead of three
inline H12 f12sqr(const H12 &a) {
    H6 ab = a.c0 * a.c1;
    H6 t = (a.c0 + a.c1) * (a.c0 + mul_v(a.c1)) - ab - mul_v(ab);
    return {t, ab + ab};
}
// f * (a + b v) in Fp6: five Fp2 products
inline H6 f6mul_by_01(const H6 &f, const H2 &a, const H2 &b) {
    H2 t0 = f.c0 * a, t1 = f.c1 * b;
    H6 r;
    r.c0 = t0 + mul_xi((f.c1 + f.c2) * b - t1);
    r.c1 = (f.c0 + f.c1) * (a + b) - t0 - t1;
    r.c2 = t1 + f.c2 * a;
    return r;
}
// f * l for a line value l = (a + b v) + (c v) w with c in Fp (the shape `line` below produces): 36 Fp products, not 54
inline H12 f12mul_by_line(const H12 &f, const H2 &a, const H2 &b, const HFp &c) {
    H6 t0 = f6mul_by_01(f.c0, a, b);
    H6 t1 = {mul_xi(mul_fp(f.c1.c2, c)), mul_fp(f.c1.c0, c), mul_fp(f.c1.c1, c)};  // f.c1 * (c v)
    H2 bc = {b.c0 + c, b.c1};
    H6 cross = f6mul_by_01(f.c0 + f.c1, a, bc) - t0 - t1;
    return {t0 + mul_v(t1), cross};
}
inline H12 f12one() { return {f6one(), f6zero()}; }
inline H12 f12conj(const H12 &a) { return {a.c0, f6neg(a.c1)}; }
inline H12 f12inv(const H12 &a) {
    H6 t = f6inv(a.c0 * a.c0 - mul_v(a.c1 * a.c1));
    return {a.c0 * t, f6neg(a.c1 * t)};
}
inline bool f12is_one(const H12 &a) {
    return f2eq(a.c0.c0, f2one()) && f2is_zero(a.c0.c1) && f2is_zero(a.c0.c2) && f2is_zero(a.c1.c0) &&
           f2is_zero(a.c1.c1) && f2is_zero(a.c1.c2);
}

// big public exponents below are little-endian arrays of 32-bit limbs

// o = a * b (schoolbook), limbs little-endian
void big_mul(uint32_t *o, const uint32_t *a, int na, const uint32_t *b, int nb) {
    for (int i = 0; i < na + nb; i++) o[i] = 0;
    for (int i = 0; i < na; i++) {
        u64 c = 0;
        for (int j = 0; j < nb; j++) {
            c += (u64)a[i] * b[j] + o[i + j];
            o[i + j] = (uint32_t)c;
            c >>= 32;
        }
        o[i + nb] = (uint32_t)c;
    }
}
// a -= b (a >= b)
void big_sub(uint32_t *a, int na, const uint32_t *b, int nb) {
    long long br = 0;
    for (int i = 0; i < na; i++) {
        long long d = (long long)a[i] - (i < nb ? b[i] : 0) - br;
        br = d < 0;
        a[i] = (uint32_t)d;
    }
}
// q = a / d for an exact or inexact division by a multi-limb d, bit-by-bit (init-time only)
void big_div(uint32_t *q, uint32_t *a, int na, const uint32_t *d, int nd) {
    // schoolbook binary long division: remainder kept in r (na limbs)
    uint32_t r[64];
    for (int i = 0; i < 64; i++) r[i] = 0;
    for (int i = 0; i < na; i++) q[i] = 0;
    for (int bit = na * 32 - 1; bit >= 0; bit--) {
        // r = (r << 1) | a_bit
        uint32_t carry = (a[bit >> 5] >> (bit & 31)) & 1;
        for (int i = 0; i <= nd; i++) {
            uint32_t nc = r[i] >> 31;
            r[i] = (r[i] << 1) | carry;
            carry = nc;
        }
        // if r >= d: r -= d, q_bit = 1
        bool ge = true;
        if (r[nd] == 0) {
            for (int i = nd - 1; i >= 0; i--) {
                if (r[i] > d[i]) break;
                if (r[i] < d[i]) { ge = false; break; }
            }
        }
        if (ge) {
            big_sub(r, nd + 1, d, nd);
            q[bit >> 5] |= 1u << (bit & 31);
        }
    }
}

template <class T, class MulF>
T pow_big(const T &a, const T &one, const uint32_t *e, int n, MulF mul) {
    T acc = one;
    bool started = false;
    for (int i = n * 32 - 1; i >= 0; i--) {
        if (started) acc = mul(acc, acc);
        if ((e[i >> 5] >> (i & 31)) & 1) {
            acc = started ? mul(acc, a) : a;
            started = true;
        }
    }
    return acc;
}

struct Consts {
    H2 gamma[6];      // xi^(k (p^2-1)/6), k = 0..5 (they lie in HFp)
    H2 gamma1[6];     // xi^(k (p-1)/6), k = 0..5
    uint32_t hard[48]; // (p^4 - p^2 + 1) / r
    int hard_n;
    bool ready = false;
};
Consts g_c;
std::mutex g_c_mu;

void init_consts() {
    std::lock_guard<std::mutex> lk(g_c_mu);
    if (g_c.ready) return;
    uint32_t p[12], r[8];
    for (int i = 0; i < 12; i++) p[i] = FpParams::MOD[i];
    for (int i = 0; i < 8; i++) r[i] = FrParams::MOD[i];
    uint32_t p2[24], p4[48];
    big_mul(p2, p, 12, p, 12);
    big_mul(p4, p2, 24, p2, 24);
    // hard = (p^4 - p^2 + 1) / r
    uint32_t num[48];
    memcpy(num, p4, sizeof num);
    big_sub(num, 48, p2, 24);
    {
        u64 c = 1;
        for (int i = 0; i < 48 && c; i++) {
            c += num[i];
            num[i] = (uint32_t)c;
            c >>= 32;
        }
    }
    big_div(g_c.hard, num, 48, r, 8);
    g_c.hard_n = 48;
    // e6 = (p^2 - 1) / 6
    uint32_t e6n[24], six[1] = {6}, e6[24];
    memcpy(e6n, p2, sizeof e6n);
    e6n[0] -= 1;  // p^2 is odd
    big_div(e6, e6n, 24, six, 1);
    H2 xi = {HFp::one(), HFp::one()};
    auto m2 = [](const H2 &a, const H2 &b) { return a * b; };
    H2 g1 = pow_big<H2>(xi, f2one(), e6, 24, m2);
    g_c.gamma[0] = f2one();
    for (int k = 1; k < 6; k++) g_c.gamma[k] = g_c.gamma[k - 1] * g1;
    // e1 = (p - 1) / 6 for the p-power Frobenius
    uint32_t e1n[12], e1[12];
    memcpy(e1n, p, sizeof e1n);
    e1n[0] -= 1;
    big_div(e1, e1n, 12, six, 1);
    H2 h1 = pow_big<H2>(xi, f2one(), e1, 12, m2);
    g_c.gamma1[0] = f2one();
    for (int k = 1; k < 6; k++) g_c.gamma1[k] = g_c.gamma1[k - 1] * h1;
    g_c.ready = true;
}

// a^(p^2): coefficient of v^i w^j (= w^(2i+j)) is scaled by gamma[2i+j]; H2 is fixed by x -> x^(p^2)
H12 frob_p2(const H12 &a) {
    H12 r;
    r.c0.c0 = a.c0.c0;
    r.c0.c1 = a.c0.c1 * g_c.gamma[2];
    r.c0.c2 = a.c0.c2 * g_c.gamma[4];
    r.c1.c0 = a.c1.c0 * g_c.gamma[1];
    r.c1.c1 = a.c1.c1 * g_c.gamma[3];
    r.c1.c2 = a.c1.c2 * g_c.gamma[5];
    return r;
}

// a^p: H2 coefficients are conjugated, the coefficient of w^(2i+j) is scaled by gamma1[2i+j]
H12 frob_p(const H12 &a) {
    auto cj = [](const H2 &c) { return H2{c.c0, neg(c.c1)}; };
    H12 r;
    r.c0.c0 = cj(a.c0.c0);
    r.c0.c1 = cj(a.c0.c1) * g_c.gamma1[2];
    r.c0.c2 = cj(a.c0.c2) * g_c.gamma1[4];
    r.c1.c0 = cj(a.c1.c0) * g_c.gamma1[1];
    r.c1.c1 = cj(a.c1.c1) * g_c.gamma1[3];
    r.c1.c2 = cj(a.c1.c2) * g_c.gamma1[5];
    return r;
}

// a^2 for a in the cyclotomic subgroup (after the easy part of the final exponentiation): Granger-Scott, "Faster
// squaring in the cyclotomic subgroup of sixth degree extensions" -- three Fp4 squarings (9 Fp2 products with the
// Karatsuba-style square below) instead of a full Fp12 product (18). Coefficient order of this tower:
// g = (z0 + z4 v + z3 v^2) + (z2 + z1 v + z5 v^2) w.
H12 cyclotomic_sqr(const H12 &a) {
    const H2 &z0 = a.c0.c0, &z4 = a.c0.c1, &z3 = a.c0.c2, &z2 = a.c1.c0, &z1 = a.c1.c1, &z5 = a.c1.c2;
    // (x + y s)^2 in Fp4 = Fp2[s]/(s^2 - xi):  t_even = x^2 + xi y^2,  t_odd = 2 x y
    auto fp4_sqr = [](const H2 &x, const H2 &y, H2 &t_even, H2 &t_odd) {
        H2 xy = x * y;
        t_even = (x + y) * (mul_xi(y) + x) - xy - mul_xi(xy);
        t_odd = xy + xy;
    };
    H2 t0, t1, t2, t3, t4, t5;
    fp4_sqr(z0, z1, t0, t1);
    fp4_sqr(z2, z3, t2, t3);
    fp4_sqr(z4, z5, t4, t5);
    auto three_t_minus_two_z = [](const H2 &t, const H2 &z) { H2 d = t - z; return d + d + t; };
    auto three_t_plus_two_z = [](const H2 &t, const H2 &z) { H2 d = t + z; return d + d + t; };
    H12 r;
    r.c0.c0 = three_t_minus_two_z(t0, z0);
    r.c1.c1 = three_t_plus_two_z(t1, z1);
    r.c1.c0 = three_t_plus_two_z(mul_xi(t5), z2);
    r.c0.c2 = three_t_minus_two_z(t4, z3);
    r.c0.c1 = three_t_minus_two_z(t2, z4);
    r.c1.c2 = three_t_plus_two_z(t3, z5);
    return r;
}

// a^x for the (negative) curve parameter x = -0xd201000000010000, a in the cyclotomic subgroup
// (where the inverse is the conjugate). LWKZG_PAIRING_GENERIC_SQR=1 squares with the generic product (cross-check).
H12 exp_by_x(const H12 &a) {
    const int generic = knobs().pairing_generic_sqr ? 1 : 0;
    H12 acc = a;  // bit 63
    for (int i = 62; i >= 0; i--) {
        acc = generic ? acc * acc : cyclotomic_sqr(acc);
        if (i == 62 || i == 60 || i == 57 || i == 48 || i == 16) acc = acc * a;
    }
    return f12conj(acc);
}

// Is f^((p^12 - 1) / r) == 1 ?  Easy part (p^6 - 1)(p^2 + 1) by conjugation / inversion / Frobenius; for the
// hard part h = (p^4 - p^2 + 1) / r the identity  3 h = (x - 1)^2 (x + p) (x^2 + p^2 - 1) + 3  (BLS12 family)
// gives f^(3h) with five exponentiations by x. The result lies in the order-r subgroup and gcd(3, r) = 1,
// so f^(3h) == 1 exactly when f^h == 1. LWKZG_PAIRING_NAIVE=1 switches to the plain 1268-bit exponentiation
// (kept as the cross-check the x-chain was validated against).
bool final_exponentiation_is_one(const H12 &f) {
    H12 t = f12conj(f) * f12inv(f);  // f^(p^6 - 1)
    t = frob_p2(t) * t;               // ^(p^2 + 1)
    const int naive = knobs().pairing_naive ? 1 : 0;
    if (naive) {
        auto m12 = [](const H12 &a, const H12 &b) { return a * b; };
        return f12is_one(pow_big<H12>(t, f12one(), g_c.hard, g_c.hard_n, m12));
    }
    H12 t0 = exp_by_x(t) * f12conj(t);             // t^(x-1)
    H12 t1 = exp_by_x(t0) * f12conj(t0);           // t^((x-1)^2)
    H12 t2 = exp_by_x(t1) * frob_p(t1);            // ^(x+p)
    H12 t3 = exp_by_x(exp_by_x(t2)) * frob_p2(t2) * f12conj(t2);  // ^(x^2+p^2-1)
    return f12is_one(t3 * t * t * t);
}

struct G2A {
    H2 x, y;
};

// line through T (tangent if double) evaluated at P, scaled by w^3 (killed by the final exponentiation):
//   l = (lambda x_T - y_T) + (-lambda x_P) v + (y_P) v w
H12 line(const H2 &lambda, const G2A &t, const HFp &xp, const HFp &yp) {
    H12 l;
    l.c0.c0 = lambda * t.x - t.y;
    l.c0.c1 = f2neg(mul_fp(lambda, xp));
    l.c0.c2 = f2zero();
    l.c1.c0 = f2zero();
    l.c1.c1 = {yp, HFp::zero()};
    l.c1.c2 = f2zero();
    return l;
}

const u64 kAbsZ = 0xd201000000010000ull;  // |z|, z < 0

// The G2 arguments of the verifications are the two setup points, the same on every call: the slope and the constant
// term of every line of their Miller loops (63 tangents + 5 chords) depend on Q alone and are computed once per
// distinct Q -- with them a step needs no G2 arithmetic and no inversion, only the evaluation at P.
struct LineCoeff {
    H2 lambda, c0;  // l(P) = c0 + (-lambda x_P) v + (y_P) v w,  c0 = lambda x_T - y_T
};
struct FixedQ {
    H2 x, y;
    std::vector<LineCoeff> lines;  // in the order the loop consumes them
};

thread_local bool tl_keep_lines = true;   // false: this thread's pairings leave the cache alone (pairing_product_is_one_uncached)

std::shared_ptr<const FixedQ> fixed_q_lines(const G2A &q) {
    static std::mutex mu;
    static std::vector<std::shared_ptr<const FixedQ>> cache;  // a handful of entries: linear search
    {
        std::lock_guard<std::mutex> lk(mu);
        for (auto &e : cache)
            if (f2eq(e->x, q.x) && f2eq(e->y, q.y)) return e;
    }
    auto fq = std::make_shared<FixedQ>();
    fq->x = q.x;
    fq->y = q.y;
    G2A t = q;
    for (int bit = 62; bit >= 0; bit--) {
        H2 xx = t.x * t.x;
        H2 lambda = (xx + xx + xx) * f2inv(t.y + t.y);  // tangent: 3 x^2 / (2 y)
        fq->lines.push_back({lambda, lambda * t.x - t.y});
        H2 x3 = lambda * lambda - t.x - t.x;
        t = {x3, lambda * (t.x - x3) - t.y};
        if ((kAbsZ >> bit) & 1) {
            lambda = (t.y - q.y) * f2inv(t.x - q.x);  // chord through T and Q (T != +-Q for points of order r inside the loop)
            fq->lines.push_back({lambda, lambda * t.x - t.y});
            x3 = lambda * lambda - t.x - q.x;
            t = {x3, lambda * (t.x - x3) - t.y};
        }
    }
    std::lock_guard<std::mutex> lk(mu);
    if (tl_keep_lines && cache.size() < 8) cache.push_back(fq);  // beyond that (the test hook with arbitrary points) nothing is kept
    return fq;
}

}  // namespace

// the 68 lines of Q's Miller loop (in the order the loop consumes them) as the device tower takes them: out[2 k] = lambda,
// out[2 k + 1] = c0 (fp12.cuh: PairingLine; verify_each.hip uploads them once per context). Q: affine, of order r.
void pairing_line_table_host(const Fp2 &qx, const Fp2 &qy, Fp2 *out) {
    const G2A q = {{HFp::from_fe(qx.c0), HFp::from_fe(qx.c1)}, {HFp::from_fe(qy.c0), HFp::from_fe(qy.c1)}};
    std::shared_ptr<const FixedQ> fq = fixed_q_lines(q);
    for (size_t k = 0; k < fq->lines.size(); k++) {
        const LineCoeff &lc = fq->lines[k];
        out[2 * k] = {lc.lambda.c0.to_fe(), lc.lambda.c1.to_fe()};
        out[2 * k + 1] = {lc.c0.c0.to_fe(), lc.c0.c1.to_fe()};
    }
}

// prod_i e(P_i, Q_i) == 1 for affine, non-infinity inputs (callers drop pairs with an infinity: e = 1)
bool pairing_product_is_one(const G1Affine *ps, const Fp2 *qx, const Fp2 *qy, int n) {
    init_consts();
    if (n == 0) return true;
    const u64 z = kAbsZ;
    G2A t[4], q[4];
    HFp px[4], py[4];
    if (n > 4) return false;
    for (int i = 0; i < n; i++) {
        q[i] = {{HFp::from_fe(qx[i].c0), HFp::from_fe(qx[i].c1)}, {HFp::from_fe(qy[i].c0), HFp::from_fe(qy[i].c1)}};
        t[i] = q[i];
        px[i] = HFp::from_fe(ps[i].x);
        py[i] = HFp::from_fe(ps[i].y);
    }
    H12 f = f12one();
    const int on_the_fly = knobs().pairing_no_precomp ? 1 : 0;  // =1: the loop below that walks T itself (cross-check)
    if (!on_the_fly) {
        const auto t0 = std::chrono::steady_clock::now();
        std::shared_ptr<const FixedQ> fq[4];
        for (int i = 0; i < n; i++) fq[i] = fixed_q_lines(q[i]);
        // Miller loop over the pairs [lo, hi): one squaring per bit shared by them
        auto miller = [&](int lo, int hi) {
            H12 g = f12one();
            size_t k = 0;
            auto step = [&]() {
                for (int i = lo; i < hi; i++) {
                    const LineCoeff &lc = fq[i]->lines[k];
                    g = f12mul_by_line(g, lc.c0, f2neg(mul_fp(lc.lambda, px[i])), py[i]);
                }
                k++;
            };
            for (int bit = 62; bit >= 0; bit--) {
                g = f12sqr(g);
                step();
                if ((z >> bit) & 1) step();
            }
            return g;
        };
        static const bool two_threads = host_threads() >= 2 && !knobs().pairing_one_thread;
        if (n == 2 && two_threads) {
            // the two pairings of a verification on two threads: each pays its own squarings (36 of the 74 field products
            // of a step), but the loop takes 0.26 ms instead of 0.40 ms
            H12 g1;
            SideTask side([&]() { g1 = miller(1, 2); });  // (runs inline when no thread can be had)
            H12 g0 = miller(0, 1);
            side.join();
            f = g0 * g1;
        } else {
            f = miller(0, n);
        }
        const bool timing = knobs().timing;
        if (!timing) return final_exponentiation_is_one(f12conj(f));  // z < 0
        const auto t1 = std::chrono::steady_clock::now();
        const bool verdict = final_exponentiation_is_one(f12conj(f));
        const auto t2 = std::chrono::steady_clock::now();
        fprintf(stderr, "[lambdaworks_kzg_amd] pairing product of %d: Miller loop %.3f ms, final exponentiation %.3f ms\n", n,
                std::chrono::duration<double, std::milli>(t1 - t0).count(), std::chrono::duration<double, std::milli>(t2 - t1).count());
        return verdict;
    }
    // all denominators of a step are inverted together (Montgomery's trick): one Fp inversion per step, not one per pairing
    auto batch_inv = [&](H2 *d) {
        H2 pre[4];
        pre[0] = d[0];
        for (int i = 1; i < n; i++) pre[i] = pre[i - 1] * d[i];
        H2 inv = f2inv(pre[n - 1]);
        for (int i = n - 1; i >= 1; i--) {
            H2 di = d[i];
            d[i] = inv * pre[i - 1];
            inv = inv * di;
        }
        d[0] = inv;
    };
    for (int bit = 62; bit >= 0; bit--) {
        f = f * f;
        H2 den[4];
        for (int i = 0; i < n; i++) den[i] = t[i].y + t[i].y;
        batch_inv(den);
        for (int i = 0; i < n; i++) {
            // tangent: lambda = 3 x^2 / (2 y)
            H2 xx = t[i].x * t[i].x;
            H2 lambda = (xx + xx + xx) * den[i];
            f = f * line(lambda, t[i], px[i], py[i]);
            H2 x3 = lambda * lambda - t[i].x - t[i].x;
            H2 y3 = lambda * (t[i].x - x3) - t[i].y;
            t[i] = {x3, y3};
        }
        if ((z >> bit) & 1) {
            for (int i = 0; i < n; i++) den[i] = t[i].x - q[i].x;
            batch_inv(den);
            for (int i = 0; i < n; i++) {
                // chord through T and Q (T != +-Q for points of order r inside the loop)
                H2 lambda = (t[i].y - q[i].y) * den[i];
                f = f * line(lambda, t[i], px[i], py[i]);
                H2 x3 = lambda * lambda - t[i].x - q[i].x;
                H2 y3 = lambda * (t[i].x - x3) - t[i].y;
                t[i] = {x3, y3};
            }
        }
    }
    f = f12conj(f);  // z < 0
    return final_exponentiation_is_one(f);
}

// the same for G2 points that no later call will see again (lwkzg_trusted_setup_check walks all 65 of a setup): their line tables are used
// once and not kept, so the handful of cached ones stay those of the verifications
bool pairing_product_is_one_uncached(const G1Affine *ps, const Fp2 *qx, const Fp2 *qy, int n) {
    tl_keep_lines = false;
    const bool r = pairing_product_is_one(ps, qx, qy, n);
    tl_keep_lines = true;
    return r;
}

// test hook (CPU-only): compressed inputs, host decompression, no subgroup checks on G2
bool pairing_check_compressed(const uint8_t *g1s, const uint8_t *g2s, int n, bool *ok) {
    G1Affine ps[4];
    Fp2 qx[4], qy[4];
    int m = 0;
    if (n > 4) return false;
    for (int i = 0; i < n; i++) {
        G1Affine p;
        int rc = g1_decompress_nocheck(p, g1s + 48 * i);
        if (rc == 2) return false;
        bool inf2 = false;
        Fp2 x, y;
        if (!g2_decompress(x, y, inf2, g2s + 96 * i)) return false;
        if (rc == 1 || inf2) continue;  // e(O, Q) = e(P, O) = 1
        ps[m] = p;
        qx[m] = x;
        qy[m] = y;
        m++;
    }
    *ok = pairing_product_is_one(ps, qx, qy, m);
    return true;
}

}  // namespace lwk
