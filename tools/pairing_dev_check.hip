// pairing_dev_check.hip -- the device pairing (fp12.cuh: tower, Miller loop against line tables, final exponentiation) compiled for the
// HOST and driven by tests/test_pairing_device_math_cpu.py without a GPU. Commands, one per line of the file named by argv[1]:
//   selftest N                 N random Fp12 elements: a * a^-1 == 1; on cyclotomic elements the Granger-Scott square == the generic
//                              square == the product; frob_p applied 12 times == id, frob_p twice == frob_p2. Prints "selftest ok".
//   lines X0 X1 Y0 Y1          the 68 lines of Q = (X0 + X1 u, Y0 + Y1 u) (canonical big-endian hex) by this file's own affine G2 walk
//                              on the tower: prints lambda.c0 | lambda.c1 | c0.c0 | c0.c1 of every line as one hex string
//   q K X0 X1 Y0 Y1            Q_K (K = 0, 1) for the pairs below, lines by the same walk
//   pair P PI                  compressed G1 points (hex): prints 1 if e(P, Q_0) e(-PI, Q_1) == 1, else 0 (pairing2_is_one)
//   hipcc -O1 -std=c++17 --cuda-host-only -I lambdaworks_kzg_amd/csrc tools/pairing_dev_check.hip -o /tmp/pairing_dev_check
#include <stdio.h>
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "g1.cuh"
#include "fp12.cuh"
using namespace lwk;

static uint64_t sm(uint64_t &s) {
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static Fp rnd_fp(uint64_t &s) {
    uint32_t raw[12];
    for (int i = 0; i < 12; i++) raw[i] = (uint32_t)sm(s);
    return fe_from_raw<FpParams>(raw);  // reduced
}
static Fp2 rnd_fp2(uint64_t &s) { return {rnd_fp(s), rnd_fp(s)}; }
static Fp12 rnd_fp12(uint64_t &s) {
    Fp12 a;
    Fp2 *c[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
    for (auto *p : c) *p = rnd_fp2(s);
    return a;
}

static bool hex_bytes(const char *h, uint8_t *out, size_t n) {
    if (strlen(h) != 2 * n) return false;
    for (size_t i = 0; i < n; i++) {
        unsigned v;
        if (sscanf(h + 2 * i, "%2x", &v) != 1) return false;
        out[i] = (uint8_t)v;
    }
    return true;
}
static Fp fp_hex(const char *h) {
    uint8_t b[48];
    uint32_t raw[12];
    if (!hex_bytes(h, b, 48)) {
        fprintf(stderr, "bad field element %s\n", h);
        exit(2);
    }
    raw_from_be<12>(raw, b);
    return fe_from_raw<FpParams>(raw);
}
static void print_fp(const Fp &a) {
    uint32_t raw[12];
    uint8_t b[48];
    fe_to_raw<FpParams>(raw, a);
    raw_to_be<12>(b, raw);
    for (int i = 0; i < 48; i++) printf("%02x", b[i]);
}

// the lines of Q's Miller loop by an affine walk T <- 2T (+ Q) over |x|: tangent slope 3 x^2 / (2 y), chord slope (y_T - y_Q) / (x_T - x_Q)
static void walk_lines(const Fp2 &qx, const Fp2 &qy, PairingLine *out) {
    Fp2 tx = qx, ty = qy;
    int k = 0;
    for (int bit = 62; bit >= 0; bit--) {
        Fp2 xx = f2sqr(tx);
        Fp2 lambda = f2mul(f2add(f2dbl(xx), xx), f2inv(f2dbl(ty)));
        out[k++] = {lambda, f2sub(f2mul(lambda, tx), ty)};
        Fp2 x3 = f2sub(f2sub(f2sqr(lambda), tx), tx);
        ty = f2sub(f2mul(lambda, f2sub(tx, x3)), ty);
        tx = x3;
        if ((kPairingAbsX >> bit) & 1) {
            lambda = f2mul(f2sub(ty, qy), f2inv(f2sub(tx, qx)));
            out[k++] = {lambda, f2sub(f2mul(lambda, tx), ty)};
            x3 = f2sub(f2sub(f2sqr(lambda), tx), qx);
            ty = f2sub(f2mul(lambda, f2sub(tx, x3)), ty);
            tx = x3;
        }
    }
}

static bool selftest(int n) {
    uint64_t s = 0x5eed;
    for (int it = 0; it < n; it++) {
        const Fp12 a = rnd_fp12(s);
        if (!f12is_one(f12mul(a, f12inv(a)))) return fprintf(stderr, "a * a^-1 != 1\n"), false;
        Fp12 c = f12mul(f12conj(a), f12inv(a));  // a^(p^6 - 1)
        c = f12mul(frob_p2(c), c);               //  ^(p^2 + 1): cyclotomic
        const Fp12 cc = f12mul(c, c);
        if (!f12eq(cyclotomic_sqr(c), cc)) return fprintf(stderr, "cyclotomic square != product\n"), false;
        if (!f12eq(f12sqr(c), cc) || !f12eq(f12sqr(a), f12mul(a, a))) return fprintf(stderr, "square != product\n"), false;
        if (!f12eq(f12mul(c, f12conj(c)), f12one())) return fprintf(stderr, "conjugate is not the inverse on the cyclotomic subgroup\n"), false;
        Fp12 f = a;
        for (int k = 0; k < 12; k++) {
            f = frob_p(f);
            if (k == 0 && !f12eq(frob_p(f), frob_p2(a))) return fprintf(stderr, "frob_p^2 != frob_p2\n"), false;
            if (k < 11 && f12eq(f, a)) return fprintf(stderr, "frob_p^%d == id\n", k + 1), false;
        }
        if (!f12eq(f, a)) return fprintf(stderr, "frob_p^12 != id\n"), false;
        // exp_by_x twice against x^2 as one exponent (x^2 > 0): square-and-multiply with the generic product
        const unsigned long long ax = kPairingAbsX;
        Fp12 e = c;  // c^|x|
        for (int i = 62; i >= 0; i--) {
            e = f12mul(e, e);
            if ((ax >> i) & 1) e = f12mul(e, c);
        }
        if (!f12eq(exp_by_x(c), f12conj(e))) return fprintf(stderr, "exp_by_x != c^x\n"), false;
    }
    return true;
}

int main(int argc, char **argv) {
    if (argc != 2) {
        fprintf(stderr, "usage: %s COMMANDS_FILE\n", argv[0]);
        return 2;
    }
    FILE *fin = fopen(argv[1], "r");
    if (!fin) return 2;
    static PairingLine q[2][kPairingLines];
    char line[4096];
    while (fgets(line, sizeof line, fin)) {
        char cmd[32], a[256], b[256], c[256], d[256], e[256];
        int m = sscanf(line, "%31s %255s %255s %255s %255s %255s", cmd, a, b, c, d, e);
        if (m <= 0) continue;
        std::string k = cmd;
        if (k == "selftest" && m == 2) {
            printf(selftest(atoi(a)) ? "selftest ok\n" : "selftest FAILED\n");
        } else if (k == "lines" && m == 5) {
            PairingLine t[kPairingLines];
            walk_lines({fp_hex(a), fp_hex(b)}, {fp_hex(c), fp_hex(d)}, t);
            for (int i = 0; i < kPairingLines; i++) {
                print_fp(t[i].lambda.c0);
                print_fp(t[i].lambda.c1);
                print_fp(t[i].c0.c0);
                print_fp(t[i].c0.c1);
            }
            printf("\n");
        } else if (k == "q" && m == 6) {
            walk_lines({fp_hex(b), fp_hex(c)}, {fp_hex(d), fp_hex(e)}, q[atoi(a) & 1]);
        } else if (k == "pair" && m == 3) {
            uint8_t pb[48], pib[48];
            if (!hex_bytes(a, pb, 48) || !hex_bytes(b, pib, 48)) return 2;
            G1Affine p, pi;
            const int rp = g1_decompress_nocheck(p, pb), rpi = g1_decompress_nocheck(pi, pib);
            if (rp == 2 || rpi == 2) {
                printf("invalid\n");
                continue;
            }
            const bool ok = pairing2_is_one(p.x, p.y, q[0], rp == 0, pi.x, neg(pi.y), q[1], rpi == 0);
            printf("%d\n", ok ? 1 : 0);
        } else {
            fprintf(stderr, "bad command: %s", line);
            return 2;
        }
        fflush(stdout);
    }
    return 0;
}
