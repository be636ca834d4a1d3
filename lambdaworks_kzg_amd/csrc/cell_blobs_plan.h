// cell_blobs_plan.h -- the grouping of the expanded items of whole blobs in closed form (cells_verify_blobs.hip).
// Blob b of a call stands for the 128 items (commitments[b], k, ., .), i = 128 b + k, so everything cell_groups_plan.h derives from
// 128 n commitments and indices follows from n-entry tables: the host makes the tables (plan_blobs), and every 128 n-entry list is a
// function of its own position and the tables (blob_item_lists, blob_col_off, blob_pad_word: the bodies of k_blob_items, and plain
// host functions too). Host only and free of HIP: tests/cell_blobs_plan_check.cpp holds the lists against group_items and plan_groups
// on the expanded arrays, under the sanitizers.
#pragma once
#include "cell_groups_plan.h"

namespace lwk {

// per blob, from the n commitments and the groups' offsets in blobs
struct BlobTables {
    size_t groups = 1;
    std::vector<uint32_t> brow;      // n: blob b's row, local to its group
    std::vector<uint32_t> bperm;     // n: the blobs in the order (group, row, blob)
    std::vector<uint32_t> bgroup;    // n: blob b's group (a grouped call)
    std::vector<uint32_t> row_off;   // rows + 1: the concatenated rows' offsets in ITEMS (perm_row's)
};

// comms: the nb commitments (host memory); boff: g + 1 valid offsets in blobs. A batch (grouped == false, g == 1, boff = {0, nb}) gets
// m and distinct of gr; a grouped call gets what the pipeline reads of p: g, n, m_total, item_off, row_base, dead (nobody is: every
// index is below 128), slices, slice_off and the 48 m_total bytes of distinct
inline void plan_blobs(BlobTables &t, Grouping &gr, GroupsPlan &p, const uint8_t *comms, size_t nb, const uint64_t *boff, size_t g,
                       bool grouped) {
    t = BlobTables();
    t.groups = g;
    t.brow.resize(nb);
    t.bperm.resize(nb);
    t.row_off.assign(1, 0);
    std::vector<uint8_t> distinct;
    std::vector<uint32_t> row_base(g + 1, 0);
    for (size_t j = 0; j < g; j++) {
        const size_t lo = (size_t)boff[j], hi = (size_t)boff[j + 1];
        std::unordered_map<std::string, uint32_t> seen;
        uint32_t m = 0;
        for (size_t b = lo; b < hi; b++) {
            auto it = seen.emplace(std::string((const char *)comms + 48 * b, 48), m);
            if (it.second) {
                distinct.insert(distinct.end(), comms + 48 * b, comms + 48 * b + 48);
                m++;
            }
            t.brow[b] = it.first->second;
        }
        std::vector<uint32_t> off(m + 1, 0);   // the group's blobs counting-sorted by row
        for (size_t b = lo; b < hi; b++) off[t.brow[b] + 1]++;
        for (uint32_t r = 0; r < m; r++) off[r + 1] += off[r];
        std::vector<uint32_t> at(off.begin(), off.end() - 1);
        for (size_t b = lo; b < hi; b++) t.bperm[lo + at[t.brow[b]]++] = (uint32_t)b;
        for (uint32_t r = 1; r <= m; r++) t.row_off.push_back((uint32_t)((lo + off[r]) * kPlanCellsPerBlob));
        row_base[j + 1] = row_base[j] + m;
    }
    if (!grouped) {
        gr = Grouping();
        gr.m = row_base[g];
        gr.distinct.swap(distinct);
        return;
    }
    t.bgroup.resize(nb);
    p = GroupsPlan();
    p.g = g, p.n = nb * kPlanCellsPerBlob, p.m_total = row_base[g];
    p.item_off.resize(g + 1);
    for (size_t j = 0; j <= g; j++) p.item_off[j] = (uint32_t)(boff[j] * kPlanCellsPerBlob);
    p.dead.assign(g, 0);
    p.slice_off.assign(1, 0);
    auto cut = [&p](uint32_t group, uint32_t sum, uint32_t first, uint32_t count) {   // (plan_groups' rule)
        for (uint32_t k = 0, slices = plan_slice_count(count); k < slices; k++) p.slices.push_back(plan_slice(group, sum, first, count, k));
        p.slice_off.push_back((uint32_t)p.slices.size());
    };
    for (size_t j = 0; j < g; j++) {
        for (size_t b = (size_t)boff[j]; b < (size_t)boff[j + 1]; b++) t.bgroup[b] = (uint32_t)j;
        const uint32_t lo = p.item_off[j], cnt = p.item_off[j + 1] - lo;
        cut((uint32_t)j, 0, cnt ? lo : 0, cnt);
        cut((uint32_t)j, 1, cnt ? lo : 0, cnt);
        cut((uint32_t)j, 2, cnt ? row_base[j] : 0, row_base[j + 1] - row_base[j]);
    }
    p.row_base.swap(row_base);
    p.distinct.swap(distinct);
}

// ---- the 128 n-entry lists, a word at a time ---------------------------------------------------------------------------------------------
// bgroup / item_off (the groups' offsets in items, g + 1): a grouped call's; nullptr for a batch, which is one group of all nb blobs
struct BlobItemLists {
    uint64_t *idx;
    uint32_t *rows, *perm_row, *perm_col, *item_group;   // item_group: nullptr for a batch
};

// the words of item i = 128 b + k: its row, its index, its group, and its places in the two sorted lists --
//   perm_row[128 p + k] = 128 bperm[p] + k     a row's items are its blobs' items, in order
//   perm_col[128 lo + k cnt + (b - lo)] = i    group j (blobs lo .. lo + cnt) keeps column k's list at 128 lo + k cnt: b ascending
// (the last is below 128 (lo + cnt) <= 128 nb for b in its group's range)
LWK_PLAN_HD void blob_item_lists(const BlobItemLists &l, size_t i, const uint32_t *brow, const uint32_t *bperm, const uint32_t *bgroup,
                                 const uint32_t *item_off, uint32_t nb) {
    const uint32_t b = (uint32_t)(i >> 7), k = (uint32_t)(i & 127);
    const uint32_t j = bgroup ? bgroup[b] : 0u;
    const uint32_t lo = bgroup ? item_off[j] >> 7 : 0u, cnt = bgroup ? (item_off[j + 1] >> 7) - lo : nb;
    l.rows[i] = brow[b];
    l.idx[i] = k;
    l.perm_row[i] = (bperm[b] << 7) | k;
    l.perm_col[((size_t)lo << 7) + (size_t)k * cnt + (b - lo)] = (uint32_t)i;
    if (l.item_group) l.item_group[i] = j;
}

// col_off[q], q <= 128 g: list 128 j + k starts at 128 lo + k cnt; the last entry closes the lists at 128 nb
LWK_PLAN_HD uint32_t blob_col_off(size_t q, const uint32_t *item_off, uint32_t nb, uint32_t g) {
    if (q == (size_t)g << 7) return nb << 7;
    const uint32_t j = (uint32_t)(q >> 7), k = (uint32_t)(q & 127);
    const uint32_t lo = item_off ? item_off[j] >> 7 : 0u, cnt = item_off ? (item_off[j + 1] >> 7) - lo : nb;
    return (lo << 7) + k * cnt;
}

// word q of the commitment set behind the distinct commitments: infinity encodings, 0xc0 and 47 zero bytes in twelve words each
LWK_PLAN_HD uint32_t blob_pad_word(size_t q) { return q % 12 == 0 ? 0xc0u : 0u; }

}  // namespace lwk
