// The slice rule that the host's plan and the device's slice table share (lambdaworks_kzg_amd/csrc/cell_groups_plan.h: plan_slice_count,
// plan_slice) as a stand-alone program, built under AddressSanitizer and UndefinedBehaviorSanitizer by
// tests/test_cell_groups_async_cpu.py. table_from_rule() is what k_seg_slice_table (cell_group.hip) does, one sum after the other:
// from the offsets, row_base and one flag per group -- never from the commitments -- the counts, their exclusive scan and every sum's
// slices. Every case holds it against plan_groups' own slices and prints "<name> ok" or "<name> FAILED: ..."; the exit status is the
// number of failures.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "cell_groups_plan.h"

using namespace lwk;

namespace {

int failures = 0;

void report(const std::string &name, const std::string &why) {
    if (!why.empty()) failures++;
    printf("%s %s%s\n", name.c_str(), why.empty() ? "ok" : "FAILED:", why.c_str());
}

struct Table {
    std::vector<GroupSlice> slices;
    std::vector<uint32_t> slice_off;
};

Table table_from_rule(const std::vector<uint32_t> &item_off, const std::vector<uint32_t> &row_base, const std::vector<uint32_t> &flag) {
    const size_t g = flag.size();
    Table t;
    t.slice_off.assign(3 * g + 1, 0);
    for (size_t q = 0; q < 3 * g; q++) {
        const uint32_t j = (uint32_t)(q / 3), s = (uint32_t)(q % 3);
        uint32_t first = 0, terms = 0;
        if (!flag[j]) {
            const std::vector<uint32_t> &off = s < 2 ? item_off : row_base;
            first = off[j];
            terms = off[j + 1] - first;
        }
        const uint32_t cnt = plan_slice_count(terms);
        for (uint32_t k = 0; k < cnt; k++) t.slices.push_back(plan_slice(j, s, first, terms, k));
        t.slice_off[q + 1] = t.slice_off[q] + cnt;
    }
    return t;
}

// groups of these sizes; item i of the call has commitment tag (i / repeat) -- repeat > 1 gives a group fewer rows than items -- and
// column i % 128, or an index of 128 where i == bad
void one_case(const std::string &name, const std::vector<uint32_t> &sizes, uint32_t repeat, long bad = -1) {
    std::vector<uint8_t> comms;
    std::vector<uint64_t> idx, off{0};
    for (uint32_t m : sizes) {
        for (uint32_t k = 0; k < m; k++) {
            const size_t i = idx.size();
            uint8_t c[48];
            memset(c, 0, 48);
            const uint32_t tag = (uint32_t)(i / repeat);
            memcpy(c + 8, &tag, 4);
            comms.insert(comms.end(), c, c + 48);
            idx.push_back((long)i == bad ? 128 : i % 128);
        }
        off.push_back(idx.size());
    }
    comms.shrink_to_fit(), idx.shrink_to_fit(), off.shrink_to_fit();
    GroupsPlan p;
    plan_groups(p, comms.data(), idx.data(), idx.size(), off.data(), sizes.size());
    const std::vector<uint32_t> flag(p.dead.begin(), p.dead.end());
    const Table t = table_from_rule(p.item_off, p.row_base, flag);
    std::string why;
    if (t.slice_off != p.slice_off) why += " slice_off differs";
    if (t.slices.size() != p.slices.size()) why += " " + std::to_string(t.slices.size()) + " slices, the plan has " + std::to_string(p.slices.size());
    else
        for (size_t k = 0; k < t.slices.size(); k++) {
            const GroupSlice &a = t.slices[k], &b = p.slices[k];
            if (a.group != b.group || a.sum != b.sum || a.first != b.first || a.count != b.count) {
                why += " slice " + std::to_string(k) + " differs";
                break;
            }
        }
    if (t.slices.size() > plan_max_slices(p.n, p.g)) why += " more slices than plan_max_slices";
    // what the rule promises on its own: every term of every live sum in exactly one slice, in order, none longer than 64
    for (size_t q = 0; q < 3 * sizes.size(); q++) {
        const uint32_t j = (uint32_t)(q / 3);
        const uint32_t first = q % 3 < 2 ? p.item_off[j] : p.row_base[j];
        const uint32_t terms = flag[j] ? 0 : (q % 3 < 2 ? p.item_off[j + 1] : p.row_base[j + 1]) - first;
        uint32_t at = first;
        for (uint32_t k = t.slice_off[q]; k < t.slice_off[q + 1]; k++) {
            const GroupSlice &s = t.slices[k];
            if (s.first != at || s.count == 0 || s.count > kPlanSliceTerms || s.group != j || s.sum != q % 3) why += " sum " + std::to_string(q) + " is not covered in order";
            at += s.count;
        }
        if (at != first + terms) why += " sum " + std::to_string(q) + " covers " + std::to_string(at - first) + " of " + std::to_string(terms);
    }
    report(name, why);
}

}  // namespace

int main() {
    std::string why;
    const uint32_t counts[][2] = {{0, 0}, {1, 1}, {2, 1}, {63, 1}, {64, 1}, {65, 2}, {128, 2}, {129, 3}, {130, 3}, {8192, 128}};
    for (auto &c : counts)
        if (plan_slice_count(c[0]) != c[1]) why += " plan_slice_count(" + std::to_string(c[0]) + ")";
    const GroupSlice last = plan_slice(7, 2, 1000, 130, 2), full = plan_slice(7, 2, 1000, 130, 1);
    if (last.group != 7 || last.sum != 2 || last.first != 1128 || last.count != 2) why += " the short last slice";
    if (full.first != 1064 || full.count != 64) why += " a full slice";
    report("the rule", why);

    one_case("boundary sizes with empty groups", {0, 1, 2, 63, 0, 64, 65, 130, 0}, 1);
    one_case("boundary sizes with repeated commitments", {0, 1, 2, 63, 0, 64, 65, 130, 0}, 3);
    one_case("sixty-five groups of one", std::vector<uint32_t>(65, 1), 1);
    one_case("257 items in uneven groups", {100, 156, 0, 1}, 2);             // a boundary inside a 256-lane workgroup, a group across two
    one_case("1025 items in uneven groups", {3, 700, 0, 321, 1}, 5);         // group 3 straddles the scan's 1024-item chunk
    one_case("a bad index first", {3, 65, 64}, 1, 1);
    one_case("a bad index last", {64, 65, 3}, 1, 131);
    return failures;
}
