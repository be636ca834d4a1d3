// cell_each_check.hip -- the per-lane pieces of the per-item cell verification (csrc/cell_each.cuh), compiled for the HOST and held
// against g1.cuh's plain double-and-add. Pure host code: runs without a GPU (tests/test_cell_verify_each_cpu.py builds and runs it).
//   1. glv_mul_affine: [k]Q over the endomorphism split (two 128-bit scalars against Q and its image, 128 shared doublings) ==
//      xyzz_mul_affine<8> on compressed bytes, for Q the generator and a second point, and k = 0, 1, z^2 - 1, z^2, z^2 + 1, 2^128 - 1,
//      2^128, r - 1, every c_k (k < 128) and a few thousand random scalars below r
//   2. cell_each_ck_raw / cell_each_coeff_raw: the canonical integers they hand to that product == the plain conversions
//   hipcc -O1 -std=c++17 --cuda-host-only -I lambdaworks_kzg_amd/csrc tools/cell_each_check.hip -o /tmp/cell_each_check
// This program is also the place for a sanitizer run of that code (add -fsanitize=address,undefined to the line above).
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include "cell_each.cuh"
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

static Scalar small(uint32_t v) {
    Scalar s = {};
    s.l[0] = v;
    return s;
}

int main() {
    uint64_t seed = 7594;
    int bad = 0;
    const char *ghex = "97f1d3a73197d7942695638c4fa9ac0fc3688c4f9774b905a14e3a3f171bac586c55e83ff97a1aeffb3af00adb22c6bb";
    uint8_t gb[48];
    for (int i = 0; i < 48; i++) {
        unsigned v;
        sscanf(ghex + 2 * i, "%2x", &v);
        gb[i] = (uint8_t)v;
    }
    G1Affine g;
    if (g1_decompress_nocheck(g, gb) != 0) {
        printf("generator does not decompress\n");
        return 1;
    }
    const uint32_t second_k[8] = {0x9e3779b9u, 0x7f4a7c15u, 0xf39cc060u, 0x5cedc834u, 0x1082276bu, 0xf3a27251u, 0xf86c6a11u, 0x0d0c7a54u};
    const G1Affine second = xyzz_to_affine(xyzz_mul_affine<8>(g, second_k));
    uint32_t braw[12];
    g1_beta_raw(braw);
    const Fp beta = fe_from_raw<FpParams>(braw);

    std::vector<Scalar> ks;
    const uint32_t zsq[4] = {0x00000000u, 0x00000001u, 0x0001a402u, 0xac45a401u};
    ks.push_back(small(0));
    ks.push_back(small(1));
    for (int d = -1; d <= 1; d++) {   // z^2 - 1, z^2, z^2 + 1
        Scalar s = {};
        for (int i = 0; i < 4; i++) s.l[i] = zsq[i];
        if (d < 0) {
            s.l[0] = 0xffffffffu;   // (the low limb of z^2 is zero: borrow from the next)
            s.l[1] -= 1;
        }
        if (d > 0) s.l[0] = 1;
        ks.push_back(s);
    }
    {
        Scalar s = {};
        for (int i = 0; i < 4; i++) s.l[i] = 0xffffffffu;   // 2^128 - 1
        ks.push_back(s);
        Scalar p = {};
        p.l[4] = 1;   // 2^128
        ks.push_back(p);
        Scalar m;
        for (int i = 0; i < 8; i++) m.l[i] = FrParams::MOD[i];   // r - 1
        m.l[0] -= 1;
        ks.push_back(m);
    }
    // c_k = w128^bitrev7(k), w128 = w4096^32
    const uint32_t omega_raw[8] = {0xa5d36306u, 0xe206da11u, 0x378fbf96u, 0x0ad1347bu, 0xe0f8245fu, 0xfc3e8acfu, 0xa0f704f4u, 0x564c0a11u};
    Fr w128 = fe_from_raw<FrParams>(omega_raw);
    for (int i = 0; i < 5; i++) w128 = sqr(w128);
    {
        Fr chk = w128;
        for (int i = 0; i < 6; i++) chk = sqr(chk);   // w128^64 = -1
        if (!(chk + Fr::one()).is_zero()) {
            printf("w128 is not a primitive 128th root of unity\n");
            bad++;
        }
    }
    std::vector<Fr> pw(128);
    pw[0] = Fr::one();
    for (int j = 1; j < 128; j++) pw[j] = pw[j - 1] * w128;
    for (uint32_t k = 0; k < 128; k++) {
        uint32_t q = 0;
        for (int bit = 0; bit < 7; bit++) q |= ((k >> bit) & 1u) << (6 - bit);
        Scalar s, plain;
        cell_each_ck_raw(s.l, pw[q]);
        fe_to_raw<FrParams>(plain.l, pw[q]);
        if (memcmp(s.l, plain.l, 32) != 0 || raw_geq<8>(s.l, FrParams::MOD)) {
            if (bad++ < 5) printf("c_k conversion mismatch at k = %u\n", k);
        }
        ks.push_back(s);
    }
    for (int j = 0; j < 2000; j++) {
        Scalar s;
        for (int i = 0; i < 8; i++) s.l[i] = (uint32_t)sm(seed);
        s.l[7] &= 0x3fffffffu;   // < 2^254 < r
        if (j % 97 == 0) s.l[7] = s.l[6] = s.l[5] = s.l[4] = 0;   // the high half empty
        if (j % 89 == 0) s.l[0] = s.l[1] = s.l[2] = s.l[3] = 0;
        ks.push_back(s);
    }
    // ---- 1. the two-base product against the plain one
    const G1Affine pts[2] = {g, second};
    for (size_t j = 0; j < ks.size(); j++)
        for (int p = 0; p < 2; p++) {
            if (p == 1 && j >= 8 + 128 + 300) break;   // the second point: the edge values, every c_k and 300 random scalars
            uint8_t o1[48], o2[48];
            g1_compress(o1, glv_mul_affine(pts[p].x, pts[p].y, beta, ks[j].l));
            g1_compress(o2, xyzz_mul_affine<8>(pts[p], ks[j].l));
            if (memcmp(o1, o2, 48) != 0 && bad++ < 5) printf("two-base product mismatch: scalar %zu, point %d\n", j, p);
        }
    // ---- 2. a coefficient as a canonical integer: (Montgomery scale) x (raw value) is the raw product
    for (int j = 0; j < 2000; j++) {
        uint32_t a[8], v[8];
        for (int i = 0; i < 8; i++) {
            a[i] = (uint32_t)sm(seed);
            v[i] = (uint32_t)sm(seed);
        }
        a[7] &= 0x3fffffffu;
        v[7] &= 0x3fffffffu;
        if (j == 0) memset(v, 0, sizeof v);
        if (j == 1) {
            for (int i = 0; i < 8; i++) v[i] = FrParams::MOD[i];
            v[0] -= 1;
        }
        const Fr scale = fe_from_raw<FrParams>(a);
        Fr value;
        for (int i = 0; i < 8; i++) value.l[i] = v[i];
        uint32_t got[8], want[8];
        cell_each_coeff_raw(got, scale, value);
        fe_to_raw<FrParams>(want, scale * fe_from_raw<FrParams>(v));
        if ((memcmp(got, want, 32) != 0 || raw_geq<8>(got, FrParams::MOD)) && bad++ < 5) printf("coefficient conversion mismatch at case %d\n", j);
    }
    if (bad) printf("FAIL %d\n", bad);
    else printf("ok: two-base scalar products (%zu scalars) and scalar conversions agree with the plain routes\n", ks.size());
    return bad != 0;
}
