// setup_text.h -- the text of a c-kzg-4844 trusted setup, host only (no HIP in here: tests/setup_text_check.cpp compiles it alone, under
// AddressSanitizer and UndefinedBehaviorSanitizer).
//
// Both layouts are a stream of tokens separated by ANY whitespace, which is what c-kzg's fscanf reads:
//     n1 n2 | n1 x 96 hex digits: G1, Lagrange form | n2 x 192 hex digits: G2, monomial                 (c-kzg-4844 1.x)
//     n1 n2 | n1 x 96 hex digits: G1, Lagrange form | n2 x 192 hex digits: G2 | n1 x 96: G1, monomial    (c-kzg-4844 2.x)
// and they are told apart by the token count alone: 2 + n1 + n2, or 2 + 2 n1 + n2.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <utility>
#include <vector>

namespace lwk {

constexpr size_t kSetupTextG1 = 4096, kSetupTextG2 = 65;   // the one size this engine is built for

struct SetupText {
    bool three_sections = false;
    std::vector<uint8_t> g1_lagrange;   // kSetupTextG1 x 48
    std::vector<uint8_t> g2_monomial;   // kSetupTextG2 x 96
    std::vector<uint8_t> g1_monomial;   // kSetupTextG1 x 48, three-section layout only
    char error[160] = {0};              // what was wrong, when parse returns false
};

inline int setup_text_hex(int ch) {
    if (ch >= '0' && ch <= '9') return ch - '0';
    if (ch >= 'a' && ch <= 'f') return ch - 'a' + 10;
    if (ch >= 'A' && ch <= 'F') return ch - 'A' + 10;
    return -1;
}
inline bool setup_text_space(char ch) { return ch == ' ' || ch == '\t' || ch == '\n' || ch == '\r' || ch == '\v' || ch == '\f'; }

// a decimal count of any length: digits only (an optional '+' in front, as the line loader takes); saturates instead of wrapping
inline bool setup_text_count(const char *p, size_t len, size_t *v) {
    size_t k = 0;
    if (len && p[0] == '+') k = 1;
    if (k == len) return false;
    size_t acc = 0;
    for (; k < len; k++) {
        if (p[k] < '0' || p[k] > '9') return false;
        if (acc < ((size_t)1 << 32)) acc = acc * 10 + (size_t)(p[k] - '0');   // (beyond 2^32 the value no longer matters: it fits no layout)
    }
    *v = acc;
    return true;
}

// true: `out` holds the sections. false: out.error says why (every such case is the caller's C_KZG_BADARGS)
inline bool setup_text_parse(const char *text, size_t size, SetupText &out) {
    std::vector<std::pair<size_t, size_t>> tok;   // (offset, length)
    tok.reserve(2 + 2 * kSetupTextG1 + kSetupTextG2);
    const size_t most = 2 + 2 * kSetupTextG1 + kSetupTextG2;
    size_t pos = 0;
    while (pos < size) {
        while (pos < size && setup_text_space(text[pos])) pos++;
        if (pos == size) break;
        const size_t start = pos;
        while (pos < size && !setup_text_space(text[pos])) pos++;
        if (tok.size() <= most) tok.push_back({start, pos - start});   // (one past `most` is enough to know that there are too many)
    }
    if (tok.size() < 2) {
        snprintf(out.error, sizeof out.error, "trusted setup text: %zu tokens, no header", tok.size());
        return false;
    }
    size_t n1 = 0, n2 = 0;
    if (!setup_text_count(text + tok[0].first, tok[0].second, &n1) || !setup_text_count(text + tok[1].first, tok[1].second, &n2)) {
        snprintf(out.error, sizeof out.error, "trusted setup text: the header is not two decimal counts");
        return false;
    }
    if (n1 != kSetupTextG1 || n2 != kSetupTextG2) {
        snprintf(out.error, sizeof out.error, "trusted setup text announces %zu/%zu points; this engine needs 4096/65", n1, n2);
        return false;
    }
    const size_t points = tok.size() - 2;
    if (points != n1 + n2 && points != 2 * n1 + n2) {
        snprintf(out.error, sizeof out.error, "trusted setup text: %zu%s point tokens fit neither layout (%zu: c-kzg 1.x, %zu: 2.x)",
                 points > 2 * n1 + n2 ? 2 * n1 + n2 : points, points > 2 * n1 + n2 ? "+" : "", n1 + n2, 2 * n1 + n2);
        return false;
    }
    out.three_sections = points == 2 * n1 + n2;
    out.g1_lagrange.assign(n1 * 48, 0);
    out.g2_monomial.assign(n2 * 96, 0);
    out.g1_monomial.assign(out.three_sections ? n1 * 48 : 0, 0);
    for (size_t i = 0; i < points; i++) {
        const bool is_g2 = i >= n1 && i < n1 + n2;
        const size_t nb = is_g2 ? 96 : 48;
        uint8_t *dst = i < n1 ? &out.g1_lagrange[i * 48] : is_g2 ? &out.g2_monomial[(i - n1) * 96] : &out.g1_monomial[(i - n1 - n2) * 48];
        const char *section = i < n1 ? "g1 lagrange" : is_g2 ? "g2" : "g1 monomial";
        const size_t index = i < n1 ? i : is_g2 ? i - n1 : i - n1 - n2;
        const size_t o = tok[2 + i].first, l = tok[2 + i].second;
        if (l != 2 * nb) {
            snprintf(out.error, sizeof out.error, "trusted setup text: %s point %zu has %zu characters, expected %zu", section, index, l, 2 * nb);
            return false;
        }
        for (size_t k = 0; k < nb; k++) {
            const int h = setup_text_hex((unsigned char)text[o + 2 * k]), lo = setup_text_hex((unsigned char)text[o + 2 * k + 1]);
            if (h < 0 || lo < 0) {
                snprintf(out.error, sizeof out.error, "trusted setup text: %s point %zu is not hex", section, index);
                return false;
            }
            dst[k] = (uint8_t)(h * 16 + lo);
        }
    }
    return true;
}

// the library's Lagrange form is in the blob's own (bit-reversed domain) order: out[i] = in[bitrev12(i)], 48 bytes each. An involution:
// the same call takes the library's order back to the natural one
inline void setup_text_bitrev48(uint8_t *out, const uint8_t *in) {
    for (size_t i = 0; i < kSetupTextG1; i++) {
        size_t r = 0;
        for (int b = 0; b < 12; b++) r |= ((i >> b) & 1u) << (11 - b);
        for (int k = 0; k < 48; k++) out[48 * i + k] = in[48 * r + k];
    }
}

}  // namespace lwk
