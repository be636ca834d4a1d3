// cell_groups_plan.h -- the host's plan of a cell proof verification: the grouping of one batch (group_items: cells_verify_api.hip and,
// per range, the grouped call) and the plan of a call of g groups (cells_verify_groups.hip). Host only and free
// of HIP: tests/cell_groups_plan_check.cpp compiles it as it stands. The slice rule (plan_slice_count, plan_slice) is also the device's:
// a cell verifier's grouped call cuts its slice table by it in a kernel (cell_group.hip: k_seg_slice_table; section 4r), and
// tests/cell_groups_slice_rule_check.cpp holds the two against each other.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <unordered_map>
#include <vector>

namespace lwk {

constexpr size_t kPlanCellsPerBlob = 128;   // kernels.h: kCellsPerBlob (cells_verify_api.hip holds the two against each other)
constexpr uint32_t kPlanSliceTerms = 64;    // terms of one slice of one sum: one lane each of a 64-lane workgroup
constexpr size_t kPwWords = 33;             // field-element slots of a group's power table: r^(2^k), k < 32, then 1

// what the host derives from the commitments and the indices of one batch
struct Grouping {
    size_t m = 0;
    std::vector<uint8_t> distinct;    // 48 m: the distinct commitments as given, in order of first occurrence
    std::vector<uint32_t> rows;       // n
    std::vector<uint32_t> perm_row, row_off, perm_col, col_off;   // n, m + 1, n, 129
};

// false: an index is not below 128 (nothing of g is to be read then)
inline bool group_items(Grouping &g, const uint8_t *comms, const uint64_t *idx, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (idx[i] >= (uint64_t)kPlanCellsPerBlob) return false;
    g.rows.resize(n);
    std::unordered_map<std::string, uint32_t> seen;
    for (size_t i = 0; i < n; i++) {
        auto it = seen.emplace(std::string((const char *)comms + 48 * i, 48), (uint32_t)g.m);
        if (it.second) {
            g.distinct.insert(g.distinct.end(), comms + 48 * i, comms + 48 * i + 48);
            g.m++;
        }
        g.rows[i] = it.first->second;
    }
    auto sort_by = [n](std::vector<uint32_t> &perm, std::vector<uint32_t> &off, size_t groups, auto key) {
        off.assign(groups + 1, 0);
        for (size_t i = 0; i < n; i++) off[key(i) + 1]++;
        for (size_t j = 0; j < groups; j++) off[j + 1] += off[j];
        std::vector<uint32_t> at(off.begin(), off.end() - 1);
        perm.resize(n);
        for (size_t i = 0; i < n; i++) perm[at[key(i)]++] = (uint32_t)i;
    };
    sort_by(g.perm_row, g.row_off, g.m, [&](size_t i) { return (size_t)g.rows[i]; });
    sort_by(g.perm_col, g.col_off, kPlanCellsPerBlob, [&](size_t i) { return (size_t)idx[i]; });
    return true;
}

// ---- a call of g groups ----------------------------------------------------------------------------------------------------------------
// One slice of one sum of one group: up to kPlanSliceTerms consecutive terms. sum 0 (P) and 1 (RLP) count the group's items, first an
// item of the call; sum 2 (RLC) counts the group's distinct commitments, first a row of the call's concatenated rows.
struct GroupSlice {
    uint32_t group, sum, first, count;
};

// The rule both sides cut by (plan_groups below; k_seg_slice_table of cell_group.hip on the device): a sum of `count` terms from term
// `first` on is plan_slice_count(count) slices, slice s of them plan_slice(.., s) -- kPlanSliceTerms terms each but the last.
#if defined(__HIPCC__) || defined(__CUDACC__)
#define LWK_PLAN_HD __host__ __device__ __forceinline__
#else
#define LWK_PLAN_HD inline
#endif
LWK_PLAN_HD uint32_t plan_slice_count(uint32_t count) { return count / kPlanSliceTerms + (count % kPlanSliceTerms ? 1u : 0u); }
LWK_PLAN_HD GroupSlice plan_slice(uint32_t group, uint32_t sum, uint32_t first, uint32_t count, uint32_t s) {
    const uint32_t at = s * kPlanSliceTerms;
    return GroupSlice{group, sum, first + at, count - at < kPlanSliceTerms ? count - at : kPlanSliceTerms};
}

struct GroupsPlan {
    size_t g = 0, n = 0, m_total = 0;
    std::vector<uint32_t> item_off;     // g + 1: the call's offsets
    std::vector<uint32_t> row_base;     // g + 1: group j's rows are row_base[j] .. row_base[j + 1] - 1 of the concatenated rows
    std::vector<uint32_t> dead;         // g: an index of the group is not below 128; it has no rows, no columns and no slices
    std::vector<uint32_t> item_group;   // n
    std::vector<uint32_t> rows;         // n: GROUP-LOCAL rows, as the group's own transcript numbers them (0 for a dead group's items)
    std::vector<uint8_t> distinct;      // 48 n: the groups' distinct commitments one after the other, then infinity encodings
    std::vector<uint32_t> perm_row, row_off;   // items of the call by concatenated row: m_total + 1 offsets (dead groups' items in no row)
    std::vector<uint32_t> perm_col, col_off;   // items of the call by (group, column): 128 g + 1 offsets, list 128 j + k
    std::vector<GroupSlice> slices;
    std::vector<uint32_t> slice_off;    // 3 g + 1: the slices of sum s of group j are slice_off[3 j + s] .. slice_off[3 j + s + 1] - 1
};

// the call-level checks of the offsets: g + 1 ascending values from 0 to n (g == 0 only with n == 0)
inline bool group_offsets_valid(const uint64_t *off, size_t g, size_t n) {
    if (g == 0) return n == 0;
    if (!off || off[0] != 0 || off[g] != (uint64_t)n) return false;
    for (size_t j = 0; j < g; j++)
        if (off[j] > off[j + 1]) return false;
    return true;
}

// the plan of a call whose offsets are valid. comms / idx: the call's n commitments and indices (host memory)
inline void plan_groups(GroupsPlan &p, const uint8_t *comms, const uint64_t *idx, size_t n, const uint64_t *off, size_t g) {
    p = GroupsPlan();
    p.g = g, p.n = n;
    p.item_off.resize(g + 1);
    for (size_t j = 0; j <= g; j++) p.item_off[j] = (uint32_t)off[j];
    p.row_base.assign(g + 1, 0);
    p.dead.assign(g, 0);
    p.item_group.resize(n);
    p.rows.assign(n, 0);
    p.distinct.reserve(48 * n);
    p.perm_row.reserve(n);
    p.perm_col.reserve(n);
    p.row_off.assign(1, 0);
    p.col_off.assign(1, 0);
    p.col_off.reserve(kPlanCellsPerBlob * g + 1);
    p.slice_off.assign(1, 0);
    auto cut = [&p](uint32_t group, uint32_t sum, uint32_t first, uint32_t count) {
        for (uint32_t k = 0, slices = plan_slice_count(count); k < slices; k++) p.slices.push_back(plan_slice(group, sum, first, count, k));
        p.slice_off.push_back((uint32_t)p.slices.size());
    };
    for (size_t j = 0; j < g; j++) {
        const uint32_t lo = p.item_off[j], cnt = p.item_off[j + 1] - lo;
        for (uint32_t i = 0; i < cnt; i++) p.item_group[lo + i] = (uint32_t)j;
        Grouping gr;
        p.dead[j] = cnt != 0 && !group_items(gr, comms + 48 * (size_t)lo, idx + lo, cnt);
        if (p.dead[j] || cnt == 0) {
            p.row_base[j + 1] = p.row_base[j];
            p.col_off.insert(p.col_off.end(), kPlanCellsPerBlob, (uint32_t)p.perm_col.size());
            for (uint32_t s = 0; s < 3; s++) cut((uint32_t)j, s, 0, 0);
            continue;
        }
        const uint32_t rb = p.row_base[j];
        p.row_base[j + 1] = rb + (uint32_t)gr.m;
        p.distinct.insert(p.distinct.end(), gr.distinct.begin(), gr.distinct.end());
        for (uint32_t i = 0; i < cnt; i++) p.rows[lo + i] = gr.rows[i];
        const uint32_t cb = (uint32_t)p.perm_col.size();   // == perm_row.size(): a dead group's items are in neither list
        for (uint32_t i = 0; i < cnt; i++) p.perm_row.push_back(lo + gr.perm_row[i]);
        for (size_t r = 1; r <= gr.m; r++) p.row_off.push_back(cb + gr.row_off[r]);
        for (uint32_t i = 0; i < cnt; i++) p.perm_col.push_back(lo + gr.perm_col[i]);
        for (size_t k = 1; k <= kPlanCellsPerBlob; k++) p.col_off.push_back(cb + gr.col_off[k]);
        cut((uint32_t)j, 0, lo, cnt);
        cut((uint32_t)j, 1, lo, cnt);
        cut((uint32_t)j, 2, rb, (uint32_t)gr.m);
    }
    p.m_total = p.row_base[g];
    p.distinct.resize(48 * n, 0);
    for (size_t q = p.m_total; q < n; q++) p.distinct[48 * q] = 0xc0;
}

// the most slices a call of n items in g groups cuts into (scratch sizing): every sum of every group one more than its full slices
inline size_t plan_max_slices(size_t n, size_t g) { return 3 * (n / kPlanSliceTerms + g); }

}  // namespace lwk
