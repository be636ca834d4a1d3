// sha256_host_check.cpp -- the host SHA-256 routines of lambdaworks_kzg_amd/csrc/sha256_host.hip compiled as plain C++ with
// -fsanitize=address,undefined (tests/test_sha256_host_cpu.py): for every length given on the command line, the digests of the first
// `len` bytes of a fixed message by sha256_host (always the portable compression), by sha256_fast (the SHA extensions when the CPU has
// them) and by sha256_fast_prefixed with the message cut after 0, 1, 32 and 63 bytes, one line each: "len name hex".
#include <stdio.h>
#include <stdlib.h>

#include "sha256_host.hip"

namespace lwk {
const Knobs &knobs() {
    static const Knobs k;
    return k;
}
}  // namespace lwk

static void line(size_t len, const char *name, const uint8_t d[32]) {
    printf("%zu %s ", len, name);
    for (int k = 0; k < 32; k++) printf("%02x", d[k]);
    printf("\n");
}

int main(int argc, char **argv) {
    std::vector<uint8_t> m(4096);
    for (size_t i = 0; i < m.size(); i++) m[i] = (uint8_t)(i * 7 + 3);
    for (int a = 1; a < argc; a++) {
        const size_t len = strtoull(argv[a], nullptr, 10);
        if (len > m.size()) return 1;
        uint8_t d[32];
        lwk::sha256_host(d, len ? m.data() : nullptr, len);
        line(len, "host", d);
        lwk::sha256_fast(d, len ? m.data() : nullptr, len);
        line(len, "fast", d);
        for (size_t cut : {(size_t)0, (size_t)1, (size_t)32, (size_t)63}) {
            if (cut > len) continue;
            lwk::sha256_fast_prefixed(d, cut ? m.data() : nullptr, cut, len > cut ? m.data() + cut : nullptr, len - cut);
            line(len, "prefixed", d);
        }
    }
    return 0;
}
