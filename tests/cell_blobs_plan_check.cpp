// The closed-form grouping of the expanded items of whole blobs (lambdaworks_kzg_amd/csrc/cell_blobs_plan.h) as a stand-alone program,
// built under AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_blob_cell_verify_cpu.py. A case is a list of groups of
// blobs, a blob its commitment's tag. The tables of plan_blobs and the lists that blob_item_lists / blob_col_off / blob_pad_word write
// (the bodies of k_blob_items, here in loops over exactly sized heap blocks) are held against what cell_groups_plan.h makes of the 128 n
// expanded commitments and indices: group_items for a batch, plan_groups for a grouped call. Every case prints one line, "<name> ok"
// or "<name> FAILED: ..."; the exit status is the number of failures.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "cell_blobs_plan.h"

using namespace lwk;

namespace {

int failures = 0;

void report(const std::string &name, const std::string &why) {
    if (!why.empty()) failures++;
    printf("%s %s%s\n", name.c_str(), why.empty() ? "ok" : "FAILED:", why.c_str());
}

typedef std::vector<uint32_t> U32;
typedef std::vector<std::vector<uint8_t>> Groups;   // per group its blobs' commitment tags

template <class A, class B>
void same(std::string &why, const char *what, const A &got, const B &want) {
    if (got.size() != want.size()) {
        why += std::string(" ") + what + " has " + std::to_string(got.size()) + " entries, not " + std::to_string(want.size());
        return;
    }
    for (size_t i = 0; i < got.size(); i++)
        if ((uint64_t)got[i] != (uint64_t)want[i]) {
            why += std::string(" ") + what + "[" + std::to_string(i) + "] = " + std::to_string((uint64_t)got[i]) + ", not " +
                   std::to_string((uint64_t)want[i]);
            return;
        }
}

struct Lists {
    std::vector<uint64_t> idx;
    U32 rows, perm_row, perm_col, item_group, col_off;
    std::vector<uint8_t> comm_in;
};

// what k_blob_items leaves: every store of its three loops, on blocks of exactly the size the pipeline's buffers promise
void write_lists(Lists &l, const BlobTables &t, const std::vector<uint8_t> &distinct, size_t m, const U32 *item_off, size_t nb) {
    const size_t n = 128 * nb;
    l.idx.assign(n, ~(uint64_t)0);
    l.rows.assign(n, ~0u), l.perm_row.assign(n, ~0u), l.perm_col.assign(n, ~0u);
    l.item_group.assign(item_off ? n : 0, ~0u);
    l.col_off.assign(128 * t.groups + 1, ~0u);
    l.comm_in.assign(48 * n, 0xee);
    memcpy(l.comm_in.data(), distinct.data(), 48 * m);
    const BlobItemLists out{l.idx.data(), l.rows.data(), l.perm_row.data(), l.perm_col.data(), item_off ? l.item_group.data() : nullptr};
    for (size_t i = 0; i < n; i++)
        blob_item_lists(out, i, t.brow.data(), t.bperm.data(), item_off ? t.bgroup.data() : nullptr, item_off ? item_off->data() : nullptr, (uint32_t)nb);
    for (size_t q = 0; q <= 128 * t.groups; q++) l.col_off[q] = blob_col_off(q, item_off ? item_off->data() : nullptr, (uint32_t)nb, (uint32_t)t.groups);
    for (size_t q = 12 * m; q < 12 * n; q++) {
        const uint32_t w = blob_pad_word(q);
        memcpy(&l.comm_in[4 * q], &w, 4);
    }
}

void expand(std::vector<uint8_t> &comms, std::vector<uint64_t> &idx, std::vector<uint64_t> &item_off, std::vector<uint8_t> &blob_comms,
            std::vector<uint64_t> &blob_off, const Groups &groups) {
    blob_off.assign(1, 0), item_off.assign(1, 0);
    for (const auto &grp : groups) {
        for (uint8_t tag : grp) {
            uint8_t c[48];
            memset(c, tag, 48);
            blob_comms.insert(blob_comms.end(), c, c + 48);
            for (uint64_t k = 0; k < 128; k++) {
                comms.insert(comms.end(), c, c + 48);
                idx.push_back(k);
            }
        }
        blob_off.push_back(blob_off.back() + grp.size());
        item_off.push_back(128 * blob_off.back());
    }
    comms.shrink_to_fit(), idx.shrink_to_fit(), blob_comms.shrink_to_fit();
}

U32 slice_words(const GroupsPlan &p) {
    U32 w;
    for (const GroupSlice &s : p.slices) w.insert(w.end(), {s.group, s.sum, s.first, s.count});
    return w;
}

void grouped_case(const std::string &name, const Groups &groups) {
    std::vector<uint8_t> comms, blob_comms;
    std::vector<uint64_t> idx, item_off, blob_off;
    expand(comms, idx, item_off, blob_comms, blob_off, groups);
    const size_t nb = blob_off.back(), g = groups.size();
    GroupsPlan want, got;
    plan_groups(want, comms.data(), idx.data(), idx.size(), item_off.data(), g);
    BlobTables t;
    Grouping unused;
    plan_blobs(t, unused, got, blob_comms.data(), nb, blob_off.data(), g, true);
    std::string why;
    if (got.g != want.g || got.n != want.n || got.m_total != want.m_total) why += " g, n or m_total";
    same(why, "item_off", got.item_off, want.item_off);
    same(why, "row_base", got.row_base, want.row_base);
    same(why, "dead", got.dead, want.dead);
    same(why, "slice_off", got.slice_off, want.slice_off);
    same(why, "slices", slice_words(got), slice_words(want));
    same(why, "row_off", t.row_off, want.row_off);
    if (got.distinct.size() != 48 * got.m_total) why += " distinct size";
    Lists l;
    write_lists(l, t, got.distinct, got.m_total, &got.item_off, nb);
    same(why, "idx", l.idx, idx);
    same(why, "rows", l.rows, want.rows);
    same(why, "item_group", l.item_group, want.item_group);
    same(why, "perm_row", l.perm_row, want.perm_row);
    same(why, "perm_col", l.perm_col, want.perm_col);
    same(why, "col_off", l.col_off, want.col_off);
    same(why, "comm_in", l.comm_in, want.distinct);
    report("groups: " + name, why);
}

void batch_case(const std::string &name, const std::vector<uint8_t> &tags) {
    std::vector<uint8_t> comms, blob_comms;
    std::vector<uint64_t> idx, item_off, blob_off;
    expand(comms, idx, item_off, blob_comms, blob_off, Groups{tags});
    const size_t nb = tags.size();
    Grouping want, got;
    std::string why;
    if (!group_items(want, comms.data(), idx.data(), idx.size())) why += " group_items refused";
    BlobTables t;
    GroupsPlan unused;
    plan_blobs(t, got, unused, blob_comms.data(), nb, blob_off.data(), 1, false);
    if (got.m != want.m) why += " m";
    same(why, "distinct", got.distinct, want.distinct);
    same(why, "row_off", t.row_off, want.row_off);
    Lists l;
    write_lists(l, t, got.distinct, got.m, nullptr, nb);
    same(why, "idx", l.idx, idx);
    same(why, "rows", l.rows, want.rows);
    same(why, "perm_row", l.perm_row, want.perm_row);
    same(why, "perm_col", l.perm_col, want.perm_col);
    same(why, "col_off", l.col_off, want.col_off);
    std::vector<uint8_t> padded(48 * idx.size(), 0);   // as cell_batch_sums pads the distinct commitments
    memcpy(padded.data(), want.distinct.data(), 48 * want.m);
    for (size_t j = want.m; j < idx.size(); j++) padded[48 * j] = 0xc0;
    same(why, "comm_in", l.comm_in, padded);
    report("batch: " + name, why);
}

}  // namespace

int main() {
    batch_case("one blob", {0xa});
    batch_case("the same blob twice", {0xa, 0xa});
    batch_case("A B A", {0xa, 0xb, 0xa});
    batch_case("B A A C B A C", {0xb, 0xa, 0xa, 0xc, 0xb, 0xa, 0xc});
    std::vector<uint8_t> many;
    for (int b = 0; b < 65; b++) many.push_back((uint8_t)(1 + b % 3));
    batch_case("65 blobs of three commitments", many);
    grouped_case("one blob", {{0xa}});
    grouped_case("[0, 1, 1, 3, 6]", {{0xa}, {}, {0xb, 0xc}, {0xd, 0xe, 0xf}});
    grouped_case("empty groups at the front, in the middle and at the end", {{}, {0xa, 0xb}, {}, {}, {0xb}, {}});
    grouped_case("rows restart per group", {{0xa, 0xb, 0xa}, {0xb, 0xa, 0xb, 0xb}, {0xa, 0xa}});
    grouped_case("everything in one group", {{0xb, 0xa, 0xa, 0xc, 0xb}});
    grouped_case("one group per blob", {{0xa}, {0xa}, {0xb}, {0xa}});
    std::vector<uint8_t> wide;                     // 70 distinct commitments in one group: two slices of the row sum
    for (int b = 0; b < 70; b++) wide.push_back((uint8_t)(1 + b));
    grouped_case("70 rows in a group", {{0x90}, wide, {0x91, 0x91}});
    return failures;
}
