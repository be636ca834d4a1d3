// carve_check.cpp -- lambdaworks_kzg_amd/csrc/carve.h on the host, built with -fsanitize=address,undefined (tests/test_carve_cpu.py).
// For every capacity given on the command line a list of pieces (sizes 0, 1, 255, 256, 257 and multiples of the capacity) is carved
// twice: from a null base (the size probe) and from a real block of exactly the probed size. Every pointer must be 256-byte aligned,
// the pieces must lie in order inside the block without overlapping, and both passes must report the same total. Every byte of every
// piece is written, so a piece that left the block would be the sanitizer's finding too. Prints one line per capacity; exit status 1
// on the first violation.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "carve.h"

namespace {

struct Pieces {
    uint8_t *bytes0, *bytes1;
    uint32_t *words;
    uint64_t *longs;
    uint8_t *p255, *p256, *p257;
    double *tail;
};

std::vector<size_t> sizes_for(size_t cap) { return {0, 1, cap * 4, cap * 8 + 8, 255, 256, 257, cap * 33}; }

size_t carve(Pieces &p, uint8_t *base, size_t cap) {
    const std::vector<size_t> sz = sizes_for(cap);
    lwk::Carver cv(base);
    cv.take(p.bytes0, sz[0]);
    cv.take(p.bytes1, sz[1]);
    cv.take(p.words, sz[2]);
    cv.take(p.longs, sz[3]);
    cv.take(p.p255, sz[4]);
    cv.take(p.p256, sz[5]);
    cv.take(p.p257, sz[6]);
    cv.take(p.tail, sz[7]);
    return cv.bytes();
}

bool check(size_t cap) {
    Pieces probe, real;
    const size_t total = carve(probe, nullptr, cap);
    uint8_t *block = (uint8_t *)aligned_alloc(256, total);   // (every piece is a multiple of 256 bytes, so the total is one)
    if (!block) return false;
    const size_t again = carve(real, block, cap);
    const std::vector<size_t> sz = sizes_for(cap);
    const uint8_t *at[] = {real.bytes0, real.bytes1, (uint8_t *)real.words, (uint8_t *)real.longs, real.p255, real.p256, real.p257,
                           (uint8_t *)real.tail};
    const uint8_t *at_probe[] = {probe.bytes0, probe.bytes1, (uint8_t *)probe.words, (uint8_t *)probe.longs, probe.p255, probe.p256,
                                 probe.p257, (uint8_t *)probe.tail};
    bool ok = again == total;
    const uint8_t *end = block;   // where the previous piece ended
    for (size_t k = 0; k < sz.size() && ok; k++) {
        ok = ok && (uintptr_t)at[k] % 256 == 0;
        ok = ok && at[k] >= end && at[k] - end < 256 && at[k] + sz[k] <= block + total;   // right behind its predecessor, inside the block
        ok = ok && (uintptr_t)at_probe[k] == (uintptr_t)(at[k] - block);       // the probe hands out the same offsets
        memset((void *)at[k], (int)k, sz[k]);
        end = at[k] + sz[k];
    }
    free(block);
    printf("cap %zu: %zu bytes %s\n", cap, total, ok ? "ok" : "BAD");
    return ok;
}

}  // namespace

int main(int argc, char **argv) {
    for (int i = 1; i < argc; i++)
        if (!check(strtoull(argv[i], nullptr, 10))) return 1;
    return 0;
}
