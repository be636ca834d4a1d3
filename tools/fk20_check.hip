// fk20_check.hip -- the host+device pieces of the FK20 cell proof engine (csrc/fk20.cuh), compiled for the HOST and held against
// g1.cuh's plain double-and-add and complete addition. Pure host code: runs without a GPU (tests/test_fk20_cpu.py builds and runs it).
//   1. fk20_mul_root: the fixed-root product of an XYZZ point over the endomorphism split, for all 256 recoded roots (w^e and w^e / 128),
//      for a point with ZZ != 1 and for P = O; the same recoding for 0, 1, r - 1 and random scalars; w^128 = 1 and 128 (1/128) = 1
//   2. fk20_next_digit: the signed window digits of every supported width rebuild the scalar (0, 1, r - 1, 2^248 - 1 and its
//      neighbours, whose carry runs into the top window, random scalars), no digit exceeds its rows, the top one is never negated
//   3. the whole inverse and forward 128-point G1 transforms run through fk20_inverse_* / fk20_forward_* position by position, on points
//      [a_j]G with points at infinity, a doubling and a cancellation among the first butterflies, against the O(n^2) sums of the a_j;
//      and the forward transform of h_0 = h_32 = G, which doubles in one butterfly and cancels in another
//   hipcc -O1 -std=c++17 --cuda-host-only -I lambdaworks_kzg_amd/csrc tools/fk20_check.hip -o /tmp/fk20_check
// This program is also the place for a sanitizer run of that code (add -fsanitize=address,undefined to the line above).
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "fk20.cuh"
#include <vector>
using namespace lwk;

static uint64_t sm(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Scalar {
    uint32_t l[8];
};

static Scalar random_scalar(uint64_t &seed) {
    Scalar s;
    for (int i = 0; i < 8; i++) s.l[i] = (uint32_t)sm(seed);
    s.l[7] &= 0x3fffffffu;   // < 2^254 < r
    return s;
}

static int bad = 0;
static G1Affine g;
static F29<2> beta;

static G1Xyzz29 lift(const G1Xyzz &p) {   // a saturated XYZZ point in the hot-loop form
    if (p.is_inf()) return G1Xyzz29::infinity();
    const G1Affine29 a = affine_to_29(xyzz_to_affine(p));
    return G1Xyzz29::from_affine(a.x, a.y);
}

static G1Xyzz29 times_g(const Fr &a) {   // [a]G by the plain double-and-add
    uint32_t raw[8];
    fe_to_raw<FrParams>(raw, a);
    return lift(xyzz_mul_affine<8>(g, raw));
}

static bool same(const G1Xyzz29 &a, const G1Xyzz29 &b) {
    uint8_t x[48], y[48];
    g1_compress(x, a);
    g1_compress(y, b);
    return memcmp(x, y, 48) == 0;
}

static void check_product(const G1Xyzz29 &p, const Scalar &k, const char *what, int idx) {
    uint8_t digits[kFk20RootDigits];
    fk20_recode_root(digits, k.l);
    const G1Xyzz29 got = fk20_mul_root(p, digits, beta);
    G1Xyzz29 want = G1Xyzz29::infinity();
    if (!p.is_inf()) want = lift(xyzz_mul_affine<8>(xyzz_to_affine(p), k.l));
    if (!same(got, want) && bad++ < 5) printf("fixed-root product mismatch: %s %d\n", what, idx);
}

static void inverse_host(std::vector<G1Xyzz29> &x, const std::vector<uint8_t> &roots) {
    std::vector<G1Xyzz29> out(kFk20Points);
    for (uint32_t h = 1; h < (uint32_t)kFk20Points; h <<= 1) {
        for (uint32_t pos = 0; pos < (uint32_t)kFk20Points; pos++) {
            const int root = fk20_inverse_root(pos, h);
            if (root) x[pos] = fk20_mul_root(x[pos], &roots[(size_t)root * kFk20RootDigits], beta);
        }
        for (uint32_t pos = 0; pos < (uint32_t)kFk20Points; pos++) out[pos] = fk20_inverse_out(x.data(), pos, h);
        x = out;
    }
}

static void forward_host(std::vector<G1Xyzz29> &x, const std::vector<uint8_t> &roots) {
    std::vector<G1Xyzz29> out(kFk20Points);
    for (uint32_t h = kFk20Points / 2; h >= 1; h >>= 1) {
        for (uint32_t pos = 0; pos < (uint32_t)kFk20Points; pos++) {
            out[pos] = fk20_forward_out(x.data(), pos, h);
            const int root = fk20_forward_root(pos, h);
            if (root) out[pos] = fk20_mul_root(out[pos], &roots[(size_t)root * kFk20RootDigits], beta);
        }
        x = out;
    }
}

static uint32_t rev7(uint32_t k) {
    uint32_t q = 0;
    for (int b = 0; b < 7; b++) q |= ((k >> b) & 1u) << (6 - b);
    return q;
}

int main() {
    uint64_t seed = 20;
    const char *ghex = "97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb";
    uint8_t gb[48];
    for (int i = 0; i < 48; i++) {
        unsigned v;
        sscanf(ghex + 2 * i, "%2x", &v);
        gb[i] = (uint8_t)v;
    }
    if (g1_decompress_nocheck(g, gb) != 0) {
        printf("generator does not decompress\n");
        return 1;
    }
    beta = fk20_beta29();
    const G1Affine29 g29 = affine_to_29(g);
    // a point whose ZZ is not one: 2G + G, left as the formulas leave it
    G1Xyzz29 p3 = xyzz_madd(xyzz_dbl(G1Xyzz29::from_affine(g29.x, g29.y)), g29.x, g29.y);
    if (p3.is_inf() || (p3.zz * F29<1>::one() - F29<2>::one()).is_zero()) {
        printf("the test point is affine\n");
        bad++;
    }

    // ---- 1. the fixed roots
    std::vector<uint8_t> roots((size_t)kFk20Roots * kFk20RootDigits);
    std::vector<Fr> root_fr(kFk20Roots);
    for (int idx = 0; idx < kFk20Roots; idx++) {
        Scalar k;
        fk20_root_raw(k.l, idx);
        root_fr[idx] = fe_from_raw<FrParams>(k.l);
        fk20_recode_root(&roots[(size_t)idx * kFk20RootDigits], k.l);
        check_product(p3, k, "root", idx);
        check_product(G1Xyzz29::infinity(), k, "root at infinity", idx);
    }
    {
        Fr w128 = root_fr[1], acc = Fr::one();
        for (int i = 0; i < 128; i++) acc = acc * w128;
        Fr half = root_fr[1];
        for (int i = 0; i < 6; i++) half = sqr(half);   // w^64 = -1
        const uint32_t n_raw[8] = {128, 0, 0, 0, 0, 0, 0, 0};
        if (!(acc - Fr::one()).is_zero() || !(half + Fr::one()).is_zero() ||
            !(root_fr[128] * fe_from_raw<FrParams>(n_raw) - Fr::one()).is_zero()) {
            printf("the root table is not w128^e, w128^e / 128\n");
            bad++;
        }
    }
    {
        std::vector<Scalar> ks;
        Scalar z = {}, one = {}, m;
        one.l[0] = 1;
        for (int i = 0; i < 8; i++) m.l[i] = FrParams::MOD[i];
        m.l[0] -= 1;   // r - 1
        ks.push_back(z);
        ks.push_back(one);
        ks.push_back(m);
        for (int j = 0; j < 60; j++) ks.push_back(random_scalar(seed));
        for (size_t j = 0; j < ks.size(); j++) check_product(p3, ks[j], "scalar", (int)j);
    }

    // ---- 2. the window digits
    {
        std::vector<Scalar> ks;
        Scalar z = {}, one = {}, m, c248 = {};
        one.l[0] = 1;
        for (int i = 0; i < 8; i++) m.l[i] = FrParams::MOD[i];
        m.l[0] -= 1;
        for (int i = 0; i < 7; i++) c248.l[i] = 0xffffffffu;
        c248.l[7] = 0x00ffffffu;   // 2^248 - 1: every window below the top one carries
        ks.push_back(z);
        ks.push_back(one);
        ks.push_back(m);
        ks.push_back(c248);
        Scalar c = c248;
        c.l[0] -= 1;
        ks.push_back(c);
        c = c248;
        c.l[7] = 0x72ffffffu;   // the same below the largest top digit a scalar < r can have
        ks.push_back(c);
        for (int j = 0; j < 2000; j++) ks.push_back(random_scalar(seed));
        const int widths[5] = {4, 6, 7, 8, 9};
        for (int wi = 0; wi < 5; wi++) {
            const Fk20Plan plan = fk20_plan(widths[wi]);
            if (plan.c != widths[wi]) {
                printf("width %d has no plan\n", widths[wi]);
                bad++;
                continue;
            }
            uint32_t step_raw[8] = {1u << plan.c, 0, 0, 0, 0, 0, 0, 0};
            const Fr step = fe_from_raw<FrParams>(step_raw);
            for (size_t j = 0; j < ks.size(); j++) {
                uint32_t k[8], carry = 0;
                memcpy(k, ks[j].l, 32);
                Fr sum = Fr::zero(), weight = Fr::one();
                bool ok = true;
                for (int win = 0; win < plan.nw; win++) {
                    uint32_t mag, negative;
                    fk20_next_digit(k, plan.c, win == plan.nw - 1, carry, mag, negative);
                    if (mag > plan.h || (win == plan.nw - 1 && (negative || carry))) ok = false;
                    uint32_t mag_raw[8] = {mag, 0, 0, 0, 0, 0, 0, 0};
                    const Fr term = fe_from_raw<FrParams>(mag_raw) * weight;
                    sum = negative ? sum - term : sum + term;
                    weight = weight * step;
                }
                if ((!ok || !(sum - fe_from_raw<FrParams>(ks[j].l)).is_zero()) && bad++ < 5)
                    printf("window digits mismatch: width %d, scalar %zu\n", plan.c, j);
            }
        }
        if (fk20_plan(5).c || fk20_plan(10).c || fk20_plan(99).c || fk20_plan(0).c) {
            printf("an unsupported width has a plan\n");
            bad++;
        }
    }

    // ---- 3. the transforms
    {
        std::vector<Fr> a(kFk20Points);
        for (int j = 0; j < kFk20Points; j++) {
            Scalar s = random_scalar(seed);
            a[j] = fe_from_raw<FrParams>(s.l);
        }
        // E[m] sits at position rev7(m): positions 0, 1 hold E[0], E[64]; 2, 3 hold E[32], E[96]; 4, 5 hold E[16], E[80]
        a[64] = a[0];          // the first butterfly doubles
        a[96] = neg(a[32]);    // the second cancels in its sum
        a[16] = Fr::zero();    // points at infinity on either side of a butterfly, and on both
        a[72] = Fr::zero();
        a[8] = Fr::zero();
        a[40] = a[104];        // the fourth cancels in its difference
        std::vector<G1Xyzz29> x(kFk20Points);
        for (uint32_t m = 0; m < (uint32_t)kFk20Points; m++) x[rev7(m)] = times_g(a[m]);
        inverse_host(x, roots);
        std::vector<Fr> hs(kFk20Terms);
        for (int u = 0; u < kFk20Terms; u++) {
            Fr acc = Fr::zero();
            for (int m = 0; m < kFk20Points; m++) acc = acc + a[m] * root_fr[(kFk20Points - (m * u) % kFk20Points) % kFk20Points];
            hs[u] = acc * root_fr[kFk20Points];
            if (!same(x[u], times_g(hs[u])) && bad++ < 5) printf("inverse transform mismatch at %d\n", u);
        }
        for (int u = kFk20Terms; u < kFk20Points; u++)
            if (!x[u].is_inf() && bad++ < 5) printf("inverse transform: position %d is not at infinity\n", u);
        forward_host(x, roots);
        for (uint32_t k = 0; k < (uint32_t)kFk20Points; k++) {
            Fr acc = Fr::zero();
            for (uint32_t u = 0; u < (uint32_t)kFk20Terms; u++) acc = acc + hs[u] * root_fr[(u * rev7(k)) % kFk20Points];
            if (!same(x[k], times_g(acc)) && bad++ < 5) printf("forward transform mismatch at %u\n", k);
        }
        // h_0 = h_32 = G: proof k = [1 + (w^32)^rev7(k)]G, 2G for 32 values of k and O for 32
        for (int u = 0; u < kFk20Points; u++) x[u] = G1Xyzz29::infinity();
        x[0] = x[32] = G1Xyzz29::from_affine(g29.x, g29.y);
        forward_host(x, roots);
        int twos = 0, infs = 0;
        for (uint32_t k = 0; k < (uint32_t)kFk20Points; k++) {
            const Fr want = Fr::one() + root_fr[(32 * rev7(k)) % kFk20Points];
            if (!same(x[k], times_g(want)) && bad++ < 5) printf("edge transform mismatch at %u\n", k);
            if (x[k].is_inf()) infs++;
            else if (same(x[k], xyzz_dbl(G1Xyzz29::from_affine(g29.x, g29.y)))) twos++;
        }
        if ((twos != 32 || infs != 32) && bad++ < 5) printf("edge transform: %d doubled, %d cancelled, 32 of each expected\n", twos, infs);
    }
    if (bad) printf("FAIL %d\n", bad);
    else printf("ok: fixed-root products (%d roots), window digits and both 128-point G1 transforms agree with the plain routes\n", kFk20Roots);
    return bad != 0;
}
