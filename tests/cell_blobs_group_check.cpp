// The blob-level grouping of a cell verifier's blob calls (lambdaworks_kzg_amd/csrc/cell_blobs_group.h) as a stand-alone program, built
// under AddressSanitizer and UndefinedBehaviorSanitizer by tests/test_blob_cell_verify_async_cpu.py. The steps that k_blob_group runs
// between its barriers are run here lane after lane -- in ascending, descending and strided lane order, so that both ends of the
// claim-or-lower protocol of the table are taken -- on exactly sized heap blocks, with the two scans as plain loops; the expansion
// (the bodies of k_blob_items_dev) follows on blocks of the sizes the verifier's buffers promise. Everything is held against
// plan_blobs and the lists blob_item_lists writes from ITS tables (cell_blobs_plan.h); the order inside a row's list and inside a
// (group, column) list is not defined, so those are compared as sets. Every case prints one line, "<name> ok" or "<name> FAILED: ...";
// the exit status is the number of failures.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "cell_blobs_group.h"

using namespace lwk;

namespace {

int failures = 0;

void report(const std::string &name, const std::string &why) {
    if (!why.empty()) failures++;
    printf("%s %s%s\n", name.c_str(), why.empty() ? "ok" : "FAILED:", why.c_str());
}

typedef std::vector<uint32_t> U32;
typedef std::vector<std::vector<uint32_t>> Groups;   // per group its blobs' commitment tags

struct PlainAtomics {   // one lane at a time
    static uint32_t cas(uint32_t *p, uint32_t expect, uint32_t v) {
        const uint32_t old = *p;
        if (old == expect) *p = v;
        return old;
    }
    static void min(uint32_t *p, uint32_t v) {
        if (v < *p) *p = v;
    }
    static uint32_t add(uint32_t *p, uint32_t v) {
        const uint32_t old = *p;
        *p += v;
        return old;
    }
    static void bit_or(uint32_t *p, uint32_t v) { *p |= v; }
};

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

// the lists [off[q], off[q + 1]) of two permutations hold the same entries, list by list
void same_lists(std::string &why, const char *what, const U32 &got, const U32 &want, const U32 &off) {
    if (got.size() != want.size()) {
        why += std::string(" ") + what + " size";
        return;
    }
    for (size_t q = 0; q + 1 < off.size(); q++) {
        if (off[q] > off[q + 1] || off[q + 1] > got.size()) {
            why += std::string(" ") + what + ": offsets out of range at " + std::to_string(q);
            return;
        }
        U32 a(got.begin() + off[q], got.begin() + off[q + 1]), b(want.begin() + off[q], want.begin() + off[q + 1]);
        std::sort(a.begin(), a.end()), std::sort(b.begin(), b.end());
        if (a != b) {
            why += std::string(" ") + what + ": list " + std::to_string(q) + " differs";
            return;
        }
    }
}

struct Tables {   // what k_blob_group leaves, on blocks of exactly the promised sizes
    U32 brow, bgroup, bperm, brow_off, bfirst, row_base, head;
    std::vector<uint8_t> distinct;
};

// order: 0 ascending, 1 descending, 2 strided (lane 7 k mod lanes; 7 and 512 are coprime)
uint32_t lane_at(uint32_t k, int order) {
    const uint32_t lanes = kBlobGroupCap;
    return order == 0 ? k : order == 1 ? lanes - 1 - k : (uint32_t)((7ull * k + 3) % lanes);
}

void run_group(Tables &t, const std::vector<uint8_t> &comms, const U32 *item_off, size_t nb, size_t g, uint64_t seed, uint32_t hash_mask,
               int order) {
    t.brow.assign(nb, ~0u), t.bgroup.assign(nb, ~0u), t.bperm.assign(nb, ~0u), t.brow_off.assign(nb + 1, ~0u), t.bfirst.assign(nb, ~0u);
    t.row_base.assign(item_off ? g + 1 : 0, ~0u), t.head.assign(kBlobHeadWords, ~0u);
    t.distinct.assign(48 * nb, 0xee);
    const BlobGroupOut o{t.brow.data(),   t.bgroup.data(),   t.bperm.data(), t.brow_off.data(), t.bfirst.data(), item_off ? t.row_base.data() : nullptr,
                         t.distinct.data(), t.head.data()};
    std::unique_ptr<BlobGroupShared> sh(new BlobGroupShared);
    memset(sh.get(), 0xee, sizeof(BlobGroupShared));
    const uint32_t lanes = kBlobGroupCap, n32 = (uint32_t)nb, g32 = (uint32_t)g;
    const uint32_t *off = item_off ? item_off->data() : nullptr;
    for (uint32_t k = 0; k < lanes; k++) blob_group_clear(*sh, lane_at(k, order), lanes, n32, o);
    for (uint32_t k = 0; k < lanes; k++) blob_group_insert<PlainAtomics>(*sh, lane_at(k, order), n32, comms.data(), off, g32, seed, hash_mask);
    uint32_t run = 0;   // the kernel's first scan
    for (uint32_t b = 0; b < lanes; b++) {
        sh->pre[b] = run;
        run += blob_group_flag(*sh, b, n32);
    }
    sh->pre[lanes] = run;
    sh->pre[nb] = run;
    const uint32_t total = run;
    for (uint32_t k = 0; k < lanes; k++) blob_group_first(*sh, lane_at(k, order), lanes, n32, comms.data(), off, g32, o);
    for (uint32_t k = 0; k < lanes; k++) blob_group_rows<PlainAtomics>(*sh, lane_at(k, order), n32, off, g32, o);
    const uint32_t rows = total < n32 ? total : n32;   // the kernel's second scan, in place
    uint32_t placed = 0;
    for (uint32_t r = 0; r < rows; r++) {
        const uint32_t c = sh->cnt[r];
        sh->cnt[r] = placed;
        t.brow_off[r] = placed;
        placed += c;
    }
    sh->cnt[rows] = placed;
    t.brow_off[rows] = placed;
    for (uint32_t k = 0; k < lanes; k++) blob_group_scatter<PlainAtomics>(*sh, lane_at(k, order), n32, o);
}

struct Lists {
    std::vector<uint64_t> idx;
    U32 rows, perm_row, perm_col, item_group, col_off, row_off, first_item;
    std::vector<uint8_t> comm_in;
};

void size_lists(Lists &l, size_t nb, size_t g, bool grouped, const std::vector<uint8_t> &distinct, size_t m) {
    const size_t n = 128 * nb;
    l.idx.assign(n, ~(uint64_t)0);
    l.rows.assign(n, ~0u), l.perm_row.assign(n, ~0u), l.perm_col.assign(n, ~0u);
    l.item_group.assign(grouped ? n : 0, ~0u);
    l.col_off.assign(128 * g + 1, ~0u);
    l.row_off.assign(m + 1, ~0u), l.first_item.assign(m, ~0u);
    l.comm_in.assign(48 * n, 0xee);
    memcpy(l.comm_in.data(), distinct.data(), 48 * m);
}

// every store of k_blob_items_dev
void write_lists_dev(Lists &l, const Tables &t, const U32 *item_off, size_t nb, size_t g) {
    const size_t n = 128 * nb;
    uint32_t m = t.head[kBlobHeadM];
    if (m > nb) m = (uint32_t)nb;
    size_lists(l, nb, g, item_off != nullptr, t.distinct, m);
    const uint32_t *off = item_off ? item_off->data() : nullptr;
    const BlobItemLists out{l.idx.data(), l.rows.data(), l.perm_row.data(), l.perm_col.data(), item_off ? l.item_group.data() : nullptr};
    for (size_t i = 0; i < n; i++) blob_item_lists(out, i, t.brow.data(), t.bperm.data(), item_off ? t.bgroup.data() : nullptr, off, (uint32_t)nb);
    for (size_t q = 0; q <= 128 * g; q++) l.col_off[q] = blob_col_off(q, off, (uint32_t)nb, (uint32_t)g);
    for (uint32_t r = 0; r <= m; r++) l.row_off[r] = blob_row_off_items(t.brow_off.data(), r);
    for (uint32_t r = 0; r < m; r++) l.first_item[r] = blob_first_item(t.bfirst.data(), r);
    for (size_t q = 12 * (size_t)m; q < 12 * n; q++) {
        const uint32_t w = blob_pad_word(q);
        memcpy(&l.comm_in[4 * q], &w, 4);
    }
}

// the host plan's lists (k_blob_items' stores from plan_blobs' tables)
void write_lists_plan(Lists &l, const BlobTables &t, const std::vector<uint8_t> &distinct, size_t m, const U32 *item_off, size_t nb, size_t g) {
    const size_t n = 128 * nb;
    size_lists(l, nb, g, item_off != nullptr, distinct, m);
    const uint32_t *off = item_off ? item_off->data() : nullptr;
    const BlobItemLists out{l.idx.data(), l.rows.data(), l.perm_row.data(), l.perm_col.data(), item_off ? l.item_group.data() : nullptr};
    for (size_t i = 0; i < n; i++) blob_item_lists(out, i, t.brow.data(), t.bperm.data(), item_off ? t.bgroup.data() : nullptr, off, (uint32_t)nb);
    for (size_t q = 0; q <= 128 * g; q++) l.col_off[q] = blob_col_off(q, off, (uint32_t)nb, (uint32_t)g);
    l.row_off = t.row_off;
    for (size_t q = 12 * m; q < 12 * n; q++) {
        const uint32_t w = blob_pad_word(q);
        memcpy(&l.comm_in[4 * q], &w, 4);
    }
}

// a tag's 48 bytes: distinct tags differ in several words, equal tags are equal
void tag_bytes(uint8_t out[48], uint32_t tag) {
    uint64_t x = 0x9e3779b97f4a7c15ull * (tag + 1);
    for (int k = 0; k < 6; k++) {
        x ^= x >> 29, x *= 0xbf58476d1ce4e5b9ull, x ^= x >> 32;
        memcpy(out + 8 * k, &x, 8);
    }
}

void one_case(const std::string &name, const Groups &groups, bool grouped) {
    std::vector<uint8_t> comms;
    std::vector<uint64_t> blob_off(1, 0);
    for (const auto &grp : groups) {
        for (uint32_t tag : grp) {
            uint8_t c[48];
            tag_bytes(c, tag);
            comms.insert(comms.end(), c, c + 48);
        }
        blob_off.push_back(blob_off.back() + grp.size());
    }
    comms.shrink_to_fit();
    const size_t nb = blob_off.back(), g = groups.size();
    BlobTables want;
    Grouping gr;
    GroupsPlan plan;
    plan_blobs(want, gr, plan, comms.data(), nb, blob_off.data(), g, grouped);
    const size_t m = grouped ? plan.m_total : gr.m;
    const std::vector<uint8_t> &distinct = grouped ? plan.distinct : gr.distinct;
    const U32 *item_off = grouped ? &plan.item_off : nullptr;
    // what the plan does not keep: the rows' first blobs, and the rows' offsets in blobs
    U32 row_base(g + 1, 0), first(m, ~0u), brow_off;
    for (size_t j = 0, rows = 0; j < g; j++) {
        for (size_t b = blob_off[j]; b < blob_off[j + 1]; b++) {
            const uint32_t r = (uint32_t)rows + want.brow[b];
            if (first[r] == ~0u) first[r] = (uint32_t)b;
        }
        uint32_t mj = 0;
        for (size_t b = blob_off[j]; b < blob_off[j + 1]; b++) mj = std::max(mj, want.brow[b] + 1);
        rows += mj;
        row_base[j + 1] = (uint32_t)rows;
    }
    for (uint32_t w : want.row_off) brow_off.push_back(w >> 7);
    Lists lw;
    write_lists_plan(lw, want, distinct, m, item_off, nb, g);

    std::string why;
    for (uint32_t mask : {0xffffffffu, 0u})
        for (int order = 0; order < 3 && why.empty(); order++) {
            Tables t;
            run_group(t, comms, item_off, nb, g, 0x0123456789abcdefull + 977 * (uint64_t)order, mask, order);
            if (t.head[kBlobHeadM] != m || t.head[kBlobHeadBad] != 0 || t.head[kBlobHeadErr] != 0)
                why += " head = (" + std::to_string(t.head[0]) + ", " + std::to_string(t.head[1]) + ", " + std::to_string(t.head[2]) + ")";
            same(why, "brow", t.brow, want.brow);
            if (grouped) {
                same(why, "bgroup", t.bgroup, want.bgroup);
                same(why, "row_base", t.row_base, row_base);
                if (plan.row_base != row_base) why += " (the check's own row_base)";
            }
            same(why, "distinct", std::vector<uint8_t>(t.distinct.begin(), t.distinct.begin() + 48 * std::min(m, nb)), distinct);
            same(why, "bfirst", U32(t.bfirst.begin(), t.bfirst.begin() + std::min(m, nb)), first);
            same(why, "brow_off", U32(t.brow_off.begin(), t.brow_off.begin() + std::min(m, nb) + 1), brow_off);
            if (why.empty()) same_lists(why, "bperm", t.bperm, want.bperm, brow_off);
            if (!why.empty()) break;
            Lists l;
            write_lists_dev(l, t, item_off, nb, g);
            same(why, "idx", l.idx, lw.idx);
            same(why, "rows", l.rows, lw.rows);
            same(why, "item_group", l.item_group, lw.item_group);
            same(why, "col_off", l.col_off, lw.col_off);
            same(why, "row_off", l.row_off, lw.row_off);
            same(why, "comm_in", l.comm_in, lw.comm_in);
            U32 first_items;
            for (uint32_t b : first) first_items.push_back(128 * b);
            same(why, "first_item", l.first_item, first_items);
            if (why.empty()) same_lists(why, "perm_row", l.perm_row, lw.perm_row, lw.row_off);
            if (why.empty()) same_lists(why, "perm_col", l.perm_col, lw.perm_col, lw.col_off);
            if (!why.empty()) why += " (hash_mask " + std::to_string(mask) + ", lane order " + std::to_string(order) + ")";
        }
    report(std::string(grouped ? "groups: " : "batch: ") + name, why);
}

}  // namespace

int main() {
    const Groups seven = {{}, {1, 0, 0}, {}, {2, 1, 0, 2}, {}};
    one_case("one blob", {{0}}, false);
    one_case("one blob", {{0}}, true);
    one_case("1 0 0 2 1 0 2", {{1, 0, 0, 2, 1, 0, 2}}, false);
    one_case("1 0 0 2 1 0 2 in [0, 3, 0, 4, 0]", seven, true);
    one_case("rows restart per group", {{10, 11, 10}, {11, 10, 11, 11}, {10, 10}}, true);
    std::vector<uint32_t> wide;
    for (uint32_t b = 0; b < 70; b++) wide.push_back(100 + b);
    one_case("70 distinct commitments", {wide}, false);
    one_case("70 distinct commitments in one group", {wide}, true);
    Groups full(5);   // 512 blobs of 300 distinct commitments in 5 groups, one of them empty
    const size_t sizes[5] = {200, 0, 100, 12, 200};
    uint32_t x = 12345;
    for (size_t j = 0, b = 0; j < 5; j++)
        for (size_t k = 0; k < sizes[j]; k++, b++) {
            x = x * 1664525u + 1013904223u;
            full[j].push_back(b < 300 ? (uint32_t)b : (x >> 8) % 300);
        }
    one_case("512 blobs of 300 commitments in 5 groups", full, true);
    std::vector<uint32_t> flat;
    for (const auto &grp : full) flat.insert(flat.end(), grp.begin(), grp.end());
    one_case("512 blobs of 300 commitments", {flat}, false);
    return failures;
}
