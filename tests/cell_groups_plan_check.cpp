// The host's plan of a grouped cell verification (lambdaworks_kzg_amd/csrc/cell_groups_plan.h) as a stand-alone program, built under
// AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_cell_groups_cpu.py. Every case prints one line, "<name> ok" or
// "<name> FAILED: ..."; the exit status is the number of failures.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "cell_groups_plan.h"

using namespace lwk;

namespace {

int failures = 0;

void report(const char *name, bool ok, const std::string &why = "") {
    if (!ok) failures++;
    printf("%s %s%s\n", name, ok ? "ok" : "FAILED: ", ok ? "" : why.c_str());
}

typedef std::vector<uint32_t> U32;

std::string show(const U32 &v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); i++) s += (i ? " " : "") + std::to_string(v[i]);
    return s + "]";
}

#define EXPECT(field, ...)                                                        \
    do {                                                                          \
        const U32 want_ = __VA_ARGS__;                                            \
        const auto &field_ = field;                                               \
        const U32 got_(field_.begin(), field_.end());                             \
        if (got_ != want_) why += std::string(" " #field " = ") + show(got_);     \
    } while (0)

// items as (commitment tag, index); the arrays in heap blocks of exactly their size, so that a read past either end is the sanitizer's
struct Call {
    std::vector<uint8_t> comms;
    std::vector<uint64_t> idx;
    std::vector<uint64_t> off{0};
    void item(uint8_t tag, uint64_t k) {
        uint8_t c[48];
        memset(c, tag, 48);
        comms.insert(comms.end(), c, c + 48);
        idx.push_back(k);
    }
    void close() { off.push_back(idx.size()); }
    void plan(GroupsPlan &p) {
        std::vector<uint8_t> c(comms);
        std::vector<uint64_t> i(idx), o(off);
        c.shrink_to_fit(), i.shrink_to_fit(), o.shrink_to_fit();
        plan_groups(p, c.data(), i.data(), i.size(), o.data(), o.size() - 1);
    }
};

U32 slice_words(const GroupsPlan &p) {
    U32 w;
    for (const GroupSlice &s : p.slices) w.insert(w.end(), {s.group, s.sum, s.first, s.count});
    return w;
}

void offsets_cases() {
    const uint64_t good[] = {0, 0, 2, 2, 5, 5}, first[] = {1, 2}, last[] = {0, 2}, down[] = {0, 3, 2, 4}, one[] = {0};
    std::string why;
    if (!group_offsets_valid(good, 5, 5)) why += " empty groups at the front, in the middle and at the end refused";
    if (group_offsets_valid(first, 1, 2)) why += " offsets[0] != 0 accepted";
    if (group_offsets_valid(last, 1, 3)) why += " offsets[g] != n accepted";
    if (group_offsets_valid(down, 3, 4)) why += " descending offsets accepted";
    if (group_offsets_valid(nullptr, 1, 0)) why += " NULL offsets accepted";
    if (group_offsets_valid(one, 0, 1)) why += " g == 0 with n > 0 accepted";
    if (!group_offsets_valid(nullptr, 0, 0)) why += " g == 0 with n == 0 refused";
    if (!group_offsets_valid(one, 0, 0)) why += " g == 0 with n == 0 and offsets refused";
    report("offsets", why.empty(), why);
}

// groups: {} {A5 B5} {} {B7 A7 B9} {}: B is row 1 of group 1 and row 0 of group 3 -- rows restart per group
void empty_groups_and_rows() {
    Call c;
    c.close();
    c.item(0xa, 5), c.item(0xb, 5), c.close();
    c.close();
    c.item(0xb, 7), c.item(0xa, 7), c.item(0xb, 9), c.close();
    c.close();
    GroupsPlan p;
    c.plan(p);
    std::string why;
    if (p.g != 5 || p.n != 5 || p.m_total != 4) why += " g, n, m_total";
    EXPECT(p.item_off, {0, 0, 2, 2, 5, 5});
    EXPECT(p.row_base, {0, 0, 2, 2, 4, 4});
    EXPECT(p.dead, {0, 0, 0, 0, 0});
    EXPECT(p.item_group, {1, 1, 3, 3, 3});
    EXPECT(p.rows, {0, 1, 0, 1, 0});
    EXPECT(p.perm_row, {0, 1, 2, 4, 3});
    EXPECT(p.row_off, {0, 1, 2, 4, 5});
    if (p.distinct.size() != 48 * 5) why += " distinct size";
    else {
        const uint8_t want[5] = {0xa, 0xb, 0xb, 0xa, 0xc0};
        for (int q = 0; q < 5; q++)
            if (p.distinct[48 * q] != want[q] || p.distinct[48 * q + 47] != (q < 4 ? want[q] : 0)) why += " distinct " + std::to_string(q);
    }
    if (p.col_off.size() != 128 * 5 + 1) why += " col_off size";
    else {
        // group 1: both items in column 5; group 3: items 2, 3 in column 7, item 4 in column 9
        const uint32_t at[][2] = {{0, 0}, {128, 0}, {128 + 5, 0}, {128 + 6, 2}, {256, 2}, {384, 2}, {384 + 7, 2}, {384 + 8, 4}, {384 + 9, 4},
                                  {384 + 10, 5}, {512, 5}, {640, 5}};
        for (auto &a : at)
            if (p.col_off[a[0]] != a[1]) why += " col_off[" + std::to_string(a[0]) + "] = " + std::to_string(p.col_off[a[0]]);
    }
    EXPECT(p.perm_col, {0, 1, 2, 3, 4});
    EXPECT(p.slice_off, {0, 0, 0, 0, 1, 2, 3, 3, 3, 3, 4, 5, 6, 6, 6, 6});
    EXPECT(slice_words(p), {1, 0, 0, 2, 1, 1, 0, 2, 1, 2, 0, 2, 3, 0, 2, 3, 3, 1, 2, 3, 3, 2, 2, 2});
    report("empty groups and rows that restart", why.empty(), why);
}

// a commitment repeated inside a group: one row, and a repeated item keeps both of its places
void repeats_inside_a_group() {
    Call c;
    c.item(0xa, 3), c.item(0xb, 3), c.item(0xa, 4), c.item(0xb, 3), c.close();
    GroupsPlan p;
    c.plan(p);
    std::string why;
    EXPECT(p.rows, {0, 1, 0, 1});
    EXPECT(p.row_base, {0, 2});
    EXPECT(p.perm_row, {0, 2, 1, 3});
    EXPECT(p.row_off, {0, 2, 4});
    EXPECT(p.perm_col, {0, 1, 3, 2});
    if (p.col_off[3] != 0 || p.col_off[4] != 3 || p.col_off[5] != 4 || p.col_off[128] != 4) why += " col_off";
    if (p.distinct[0] != 0xa || p.distinct[48] != 0xb || p.distinct[96] != 0xc0 || p.distinct[97] != 0 || p.distinct[144] != 0xc0) why += " distinct";
    EXPECT(slice_words(p), {0, 0, 0, 4, 0, 1, 0, 4, 0, 2, 0, 2});
    report("repeats inside a group", why.empty(), why);
}

// group sizes 0, 1, 64, 65, 128, 129, every item its own commitment: the slices of all three sums
void slice_tables() {
    const uint32_t sizes[] = {0, 1, 64, 65, 128, 129};
    Call c;
    uint8_t tag = 0;
    for (uint32_t m : sizes) {
        for (uint32_t i = 0; i < m; i++) c.item(tag = (uint8_t)(tag + 1), i % 128);   // (387 items: a tag comes again only in another group)
        c.close();
    }
    GroupsPlan p;
    c.plan(p);
    std::string why;
    U32 want_off{0}, want;
    uint32_t lo = 0, rb = 0, gi = 0;
    for (uint32_t m : sizes) {
        const uint32_t rows = p.row_base[gi + 1] - p.row_base[gi];
        if (rows != m) why += " rows of group " + std::to_string(gi);
        for (uint32_t s = 0; s < 3; s++) {
            const uint32_t first = s == 2 ? rb : lo, count = s == 2 ? rows : m;
            for (uint32_t at = 0; at < count; at += 64) want.insert(want.end(), {gi, s, first + at, count - at < 64 ? count - at : 64});
            want_off.push_back((uint32_t)want.size() / 4);
        }
        lo += m, rb += rows, gi++;
    }
    EXPECT(p.slice_off, want_off);
    EXPECT(slice_words(p), want);
    U32 per_sum;
    for (size_t q = 0; q + 1 < p.slice_off.size(); q++) per_sum.push_back(p.slice_off[q + 1] - p.slice_off[q]);
    EXPECT(per_sum, {0, 0, 0, 1, 1, 1, 1, 1, 1, 2, 2, 2, 2, 2, 2, 3, 3, 3});
    if (p.slices.size() > plan_max_slices(p.n, p.g)) why += " more slices than plan_max_slices";
    for (const GroupSlice &s : p.slices)
        if (s.count == 0 || s.count > 64 || s.first + s.count > (s.sum == 2 ? p.m_total : p.n)) why += " a slice out of range";
    report("slice tables", why.empty(), why);
}

// a bad index kills its group alone: no rows, no columns, no slices, and the lists of the groups behind it stay dense
void dead_flag() {
    Call c;
    c.item(0xa, 1), c.close();
    c.item(0xb, 2), c.item(0xc, 128), c.close();
    c.item(0xd, 3), c.item(0xb, 3), c.close();
    c.item(0xe, ~(uint64_t)0), c.close();
    GroupsPlan p;
    c.plan(p);
    std::string why;
    EXPECT(p.dead, {0, 1, 0, 1});
    EXPECT(p.row_base, {0, 1, 1, 3, 3});
    EXPECT(p.rows, {0, 0, 0, 0, 1, 0});
    EXPECT(p.item_group, {0, 1, 1, 2, 2, 3});
    EXPECT(p.perm_row, {0, 3, 4});
    EXPECT(p.row_off, {0, 1, 2, 3});
    EXPECT(p.perm_col, {0, 3, 4});
    if (p.col_off.size() != 513 || p.col_off[128] != 1 || p.col_off[256] != 1 || p.col_off[256 + 3] != 1 || p.col_off[256 + 4] != 3 || p.col_off[512] != 3)
        why += " col_off";
    if (p.m_total != 3 || p.distinct[0] != 0xa || p.distinct[48] != 0xd || p.distinct[96] != 0xb || p.distinct[144] != 0xc0) why += " distinct";
    EXPECT(p.slice_off, {0, 1, 2, 3, 3, 3, 3, 4, 5, 6, 6, 6, 6});
    EXPECT(slice_words(p), {0, 0, 0, 1, 0, 1, 0, 1, 0, 2, 0, 1, 2, 0, 3, 2, 2, 1, 3, 2, 2, 2, 1, 2});
    report("dead flag", why.empty(), why);
}

}  // namespace

int main() {
    offsets_cases();
    empty_groups_and_rows();
    repeats_inside_a_group();
    slice_tables();
    dead_flag();
    return failures;
}
