// The arithmetic of k_verify_ysum (lambdaworks_kzg_amd/csrc/verify_ysum.cuh) compiled for the host: the kernel's 256 lanes run one after
// the other, their shares are added by the kernel's tree, and the bytes are compared with sum r^i y_i on the plain 32-bit field
// (field.cuh). Sizes at the lane, wave and workgroup edges and beyond one term per lane; both byte orders; random y_i and the worst
// case y_i = r - 1 everywhere. Prints "ok: <cases>" or the mismatches.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "verify_ysum.cuh"
using namespace lwk;

static uint64_t sm = 0x4b5a47;
static uint32_t rnd32() {   // SplitMix64
    uint64_t z = (sm += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}
static Fr rnd_fr() {
    uint32_t t[8];
    for (int k = 0; k < 8; k++) t[k] = rnd32();
    t[7] &= 0x3fffffffu;
    return fe_from_raw<FrParams>(t);
}

static void as_the_kernel(const uint8_t *y32, int le, const Fr *pw, uint8_t *out32, uint32_t n) {
    Fr28 tab[33];
    for (int t = 0; t < 33; t++) tab[t] = fr28_from_mont256(pw[t]);
    std::vector<Fr28> part(kYsumLanes);
    for (uint32_t t = 0; t < (uint32_t)kYsumLanes; t++) part[t] = ysum_lane(tab, y32, le, t, n);
    for (int d = kYsumLanes / 2; d >= 1; d >>= 1)
        for (int t = 0; t < d; t++) part[t] = ysum_add(part[t], part[t + d]);
    ysum_bytes(out32, part[0]);
}

int main() {
    int bad = 0, cases = 0;
    const uint32_t ns[] = {1, 2, 3, 63, 64, 65, 255, 256, 257, 300, 511, 512, 513, 1025, 4096, 20000};
    for (int le = 0; le < 2; le++)
        for (uint32_t n : ns)
            for (int worst = 0; worst < 2; worst++)
                for (int shifted = 0; shifted < 2; shifted++) {
                    const Fr r = rnd_fr();
                    Fr pw[33], sq = r;
                    for (int k = 0; k < 32; k++) {
                        pw[k] = sq;
                        sq = sq * sq;
                    }
                    const Fr first = shifted ? rnd_fr() : Fr::one();   // r^first: any element will do
                    pw[32] = first;
                    std::vector<uint8_t> y(32 * (size_t)n);
                    Fr sum = Fr::zero(), rp = first;
                    for (uint32_t i = 0; i < n; i++) {
                        const Fr f = worst ? neg(Fr::one()) : rnd_fr();
                        uint32_t c[8];
                        fe_to_raw<FrParams>(c, f);
                        if (le) raw_to_le<8>(&y[32 * (size_t)i], c);
                        else raw_to_be<8>(&y[32 * (size_t)i], c);
                        sum = sum + rp * f;
                        rp = rp * r;
                    }
                    uint32_t want_raw[8];
                    fe_to_raw<FrParams>(want_raw, sum);
                    uint8_t want[32], got[32];
                    raw_to_be<8>(want, want_raw);
                    as_the_kernel(y.data(), le, pw, got, n);
                    cases++;
                    if (memcmp(want, got, 32)) {
                        bad++;
                        printf("MISMATCH le=%d n=%u worst=%d shifted=%d\n", le, n, worst, shifted);
                    }
                }
    if (!bad) printf("ok: %d cases\n", cases);
    return bad != 0;
}
