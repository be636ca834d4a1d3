// Stand-alone check of lambdaworks_kzg_amd/csrc/setup_text.h (the whitespace-token parser of the two c-kzg-4844 trusted setup layouts),
// built by tests/test_setup_text_cpu.py under AddressSanitizer and UndefinedBehaviorSanitizer. The points are synthetic bytes: the parser
// only tells hex of the right length, it does not know a curve. Every input is handed over in a heap block of exactly its size, so a read
// past the end is the sanitizer's to report.
#include "setup_text.h"

#include <stdlib.h>
#include <string.h>

#include <string>

using namespace lwk;

static int failures = 0;
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);   \
            failures++;                                                \
        }                                                              \
    } while (0)

static uint8_t byte_of(int section, size_t point, size_t k) {   // a different string for every (section, point)
    uint32_t h = (uint32_t)(section + 1) * 0x9E3779B1u ^ (uint32_t)point * 0x85EBCA6Bu;
    h ^= h >> 15;
    h *= 0xC2B2AE35u;
    h += (uint32_t)k * 0x27D4EB2Fu;
    h ^= h >> 13;
    h *= 0x165667B1u;
    return (uint8_t)(h >> 24);
}

static std::string hex_point(int section, size_t point, size_t nb, bool upper) {
    static const char *lo = "0123456789abcdef", *up = "0123456789ABCDEF";
    std::string s;
    for (size_t k = 0; k < nb; k++) {
        const uint8_t b = byte_of(section, point, k);
        s += (upper ? up : lo)[b >> 4];
        s += (upper ? up : lo)[b & 15];
    }
    return s;
}

// the tokens of one layout; sep(i) is what follows token i
template <class Sep>
static std::string build(bool three, Sep sep, const char *n1 = "4096", const char *n2 = "65") {
    std::string s;
    size_t i = 0;
    auto put = [&](const std::string &tok) {
        s += tok;
        s += sep(i++);
    };
    put(n1);
    put(n2);
    for (size_t p = 0; p < kSetupTextG1; p++) put(hex_point(0, p, 48, (p & 1) != 0));
    for (size_t p = 0; p < kSetupTextG2; p++) put(hex_point(1, p, 96, false));
    if (three)
        for (size_t p = 0; p < kSetupTextG1; p++) put(hex_point(2, p, 48, false));
    return s;
}

static bool parse(const std::string &text, SetupText &t) {
    char *block = (char *)malloc(text.size() ? text.size() : 1);   // exactly the text: no terminator behind it
    memcpy(block, text.data(), text.size());
    const bool ok = setup_text_parse(block, text.size(), t);
    free(block);
    return ok;
}

static void expect_sections(const SetupText &t, bool three) {
    CHECK(t.three_sections == three);
    CHECK(t.g1_lagrange.size() == kSetupTextG1 * 48 && t.g2_monomial.size() == kSetupTextG2 * 96);
    CHECK(t.g1_monomial.size() == (three ? kSetupTextG1 * 48 : 0));
    bool same = true;
    for (size_t p = 0; p < kSetupTextG1 && same; p++)
        for (size_t k = 0; k < 48; k++) {
            same = same && t.g1_lagrange[48 * p + k] == byte_of(0, p, k);
            if (three) same = same && t.g1_monomial[48 * p + k] == byte_of(2, p, k);
        }
    for (size_t p = 0; p < kSetupTextG2 && same; p++)
        for (size_t k = 0; k < 96; k++) same = same && t.g2_monomial[96 * p + k] == byte_of(1, p, k);
    CHECK(same);
}

int main() {
    auto lf = [](size_t) { return std::string("\n"); };
    auto crlf = [](size_t) { return std::string("\r\n"); };
    auto mixed = [](size_t i) { return std::string(i % 3 == 0 ? "\t" : i % 3 == 1 ? "   " : " \n\t\r\n "); };
    auto space = [](size_t) { return std::string(" "); };
    for (int three = 0; three < 2; three++) {
        {   // one token per line, trailing newline
            SetupText t;
            CHECK(parse(build(three != 0, lf), t));
            expect_sections(t, three != 0);
        }
        {   // no trailing newline
            std::string s = build(three != 0, lf);
            s.pop_back();
            SetupText t;
            CHECK(parse(s, t));
            expect_sections(t, three != 0);
        }
        {   // CRLF
            SetupText t;
            CHECK(parse(build(three != 0, crlf), t));
            expect_sections(t, three != 0);
        }
        {   // tabs, runs of blanks, blank lines; leading whitespace
            SetupText t;
            CHECK(parse(" \n\t" + build(three != 0, mixed), t));
            expect_sections(t, three != 0);
        }
        {   // one line, single spaces (what fscanf accepts)
            SetupText t;
            CHECK(parse(build(three != 0, space), t));
            expect_sections(t, three != 0);
        }
        {   // truncated in the middle of the last token
            std::string s = build(three != 0, lf);
            s.resize(s.size() - 1 - 40);
            SetupText t;
            CHECK(!parse(s, t));
            CHECK(strstr(t.error, "characters") != nullptr);
        }
        {   // truncated in the middle of a token further up: the count fits no layout, or the cut token is short
            std::string s = build(three != 0, lf);
            s.resize(s.size() / 2 + 17);
            SetupText t;
            CHECK(!parse(s, t));
            CHECK(t.error[0] != 0);
        }
        {   // one token too many / too few
            SetupText t;
            CHECK(!parse(build(three != 0, lf) + hex_point(0, 0, 48, false) + "\n", t));
            CHECK(strstr(t.error, "neither layout") != nullptr);
            std::string s = build(three != 0, lf);
            s.resize(s.size() - (three ? 97 : 193));
            SetupText u;
            CHECK(!parse(s, u));
            CHECK(strstr(u.error, "neither layout") != nullptr);
        }
    }
    {   // an empty file, whitespace only, a lone count
        SetupText t;
        CHECK(!parse("", t));
        CHECK(!parse(" \n\r\n\t", t));
        CHECK(!parse("4096", t));
        CHECK(!parse("4096\n", t));
    }
    {   // counts of 20 digits (past 2^64), other counts, counts that are no numbers
        SetupText t;
        CHECK(!parse(build(false, lf, "99999999999999999999", "65"), t));
        CHECK(strstr(t.error, "4096/65") != nullptr);
        CHECK(!parse(build(false, lf, "4096", "18446744073709551681"), t));   // 2^64 + 65: must not wrap to 65
        CHECK(!parse(build(false, lf, "00000000000000004096", "00000000000000000065") + "zz\n", t));
        SetupText z;
        CHECK(parse(build(false, lf, "00000000000000004096", "00000000000000000065"), z));   // (20 digits that ARE 4096 / 65)
        CHECK(!parse(build(false, lf, "4095", "65"), t));
        CHECK(!parse(build(false, lf, "4096", "64"), t));
        CHECK(!parse(build(false, lf, "0x1000", "65"), t));
        CHECK(!parse(build(false, lf, "-4096", "65"), t));
        CHECK(!parse(build(false, lf, "+", "65"), t));
    }
    {   // a token that is not hex, one of the wrong length (G1 length where G2 belongs)
        std::string s = build(true, lf);
        const size_t at = s.find(hex_point(0, 7, 48, true));
        CHECK(at != std::string::npos);
        s[at + 5] = 'g';
        SetupText t;
        CHECK(!parse(s, t));
        CHECK(strstr(t.error, "g1 lagrange point 7 is not hex") != nullptr);
        std::string u = build(true, lf);
        const size_t g2 = u.find(hex_point(1, 3, 96, false));
        u.erase(g2, 96);
        SetupText v;
        CHECK(!parse(u, v));
        CHECK(strstr(v.error, "g2 point 3 has 96 characters") != nullptr);
        std::string w = build(true, lf);
        const size_t m = w.find(hex_point(2, 4095, 48, false));
        w[m + 95] = '\x80';
        SetupText x;
        CHECK(!parse(w, x));
        CHECK(strstr(x.error, "g1 monomial point 4095 is not hex") != nullptr);
    }
    {   // the permutation is an involution and moves what it should
        std::vector<uint8_t> a(kSetupTextG1 * 48), b(a.size()), c(a.size());
        for (size_t i = 0; i < a.size(); i++) a[i] = (uint8_t)(i * 2654435761u >> 13);
        setup_text_bitrev48(b.data(), a.data());
        setup_text_bitrev48(c.data(), b.data());
        CHECK(a == c);
        CHECK(memcmp(&b[48 * 1], &a[48 * 2048], 48) == 0 && memcmp(&b[48 * 4095], &a[48 * 4095], 48) == 0 && memcmp(&b[48 * 6], &a[48 * 1536], 48) == 0);
    }
    if (failures) return 1;
    printf("setup_text ok\n");
    return 0;
}
