// The slot hash and the compare of the grouping kernels (lambdaworks_kzg_amd/csrc/cell_group.cuh) compiled for the host, driven through a
// sequential emulation of cell_group.hip's steps -- insert (claim, compare against the claimant's input bytes, lower the slot), the scan
// in index order, the histograms, the offsets and the scatter -- and held against a plain std::map: rows, m, the distinct commitments,
// first_item, row_off and col_off exactly, the groups of perm_row / perm_col as sets. The items are inserted in a shuffled order, as the
// lanes of a launch arrive in any order. Also: the table size rule, two seeds giving two different slot assignments but one result, and
// the mask 0 / 1 chains. Prints "ok: <cases>" or the mismatches.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <set>
#include <string>
#include <vector>
#include "cell_group.cuh"
using namespace lwk;

static uint64_t sm = 0x43454c4c47525550ull;
static uint64_t rnd64() {   // SplitMix64
    uint64_t z = (sm += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

struct Out {
    uint32_t m = 0, bad = kGroupEmpty;
    std::vector<uint32_t> rows, first_item, perm_row, row_off, perm_col, col_off, slot_of;
    std::vector<uint8_t> distinct;
    bool error = false;
};

// cell_group.hip, one lane after the other (in `order`)
static Out as_the_kernels(const std::vector<uint64_t> &comms /* 6 n words: 8-byte aligned, as the kernels ask */, const std::vector<uint64_t> &idx,
                          uint64_t seed, uint32_t hash_mask, const std::vector<uint32_t> &order) {
    const uint8_t *bytes = (const uint8_t *)comms.data();
    const uint32_t n = (uint32_t)idx.size();
    const size_t slots = group_table_slots(n);
    const uint32_t mask = (uint32_t)(slots - 1);
    Out o;
    std::vector<uint32_t> table(slots, kGroupEmpty), slot_row(slots, kGroupEmpty), row_cnt(n, 0), col_cnt(kGroupColumns, 0);
    o.slot_of.assign(n, 0);
    for (uint32_t i : order) {   // k_group_insert
        if (idx[i] >= kGroupColumns && i < o.bad) o.bad = i;
        uint64_t key[6];
        group_load48(key, bytes + 48 * (size_t)i);
        uint32_t s = group_slot_hash(key, seed, hash_mask) & mask, found = kGroupEmpty;
        for (uint32_t probe = 0; probe <= mask; probe++, s = (s + 1) & mask) {
            const uint32_t c = table[s];
            if (c == kGroupEmpty) {
                table[s] = i;
                found = s;
                break;
            }
            if (group_equal48(key, bytes + 48 * (size_t)c)) {
                table[s] = std::min(table[s], i);
                found = s;
                break;
            }
        }
        if (found == kGroupEmpty) o.error = true, found = 0;
        o.slot_of[i] = found;
    }
    o.first_item.assign(n, 0);
    o.distinct.assign(48 * (size_t)n, 0);
    for (uint32_t i = 0; i < n; i++)   // k_group_scan
        if (table[o.slot_of[i]] == i) {
            slot_row[o.slot_of[i]] = o.m;
            o.first_item[o.m] = i;
            memcpy(&o.distinct[48 * (size_t)o.m], bytes + 48 * (size_t)i, 48);
            o.m++;
        }
    o.rows.assign(n, 0);
    for (uint32_t i = 0; i < n; i++) {   // k_group_rows
        uint32_t row = slot_row[o.slot_of[i]];
        if (row >= n) o.error = true, row = 0;
        o.rows[i] = row;
        row_cnt[row]++;
        if (idx[i] < kGroupColumns) col_cnt[idx[i]]++;
        if (i >= o.m) o.distinct[48 * (size_t)i] = 0xc0;
    }
    o.row_off.assign(o.m + 1, 0);   // k_group_offsets
    for (uint32_t j = 0; j < o.m; j++) o.row_off[j + 1] = o.row_off[j] + row_cnt[j];
    o.col_off.assign(kGroupColumns + 1, 0);
    for (uint32_t k = 0; k < kGroupColumns; k++) o.col_off[k + 1] = o.col_off[k] + col_cnt[k];
    o.perm_row.assign(n, kGroupEmpty);
    o.perm_col.assign(n, kGroupEmpty);
    for (uint32_t i : order) {   // k_group_scatter: the counters counted down
        o.perm_row[o.row_off[o.rows[i]] + --row_cnt[o.rows[i]]] = i;
        if (idx[i] < kGroupColumns) o.perm_col[o.col_off[idx[i]] + --col_cnt[idx[i]]] = i;
    }
    o.first_item.resize(o.m);
    return o;
}

// group_items of cells_verify_api.hip, with a plain map
static Out plain(const std::vector<uint64_t> &comms, const std::vector<uint64_t> &idx) {
    const uint8_t *bytes = (const uint8_t *)comms.data();
    const uint32_t n = (uint32_t)idx.size();
    Out o;
    std::map<std::string, uint32_t> seen;
    o.distinct.assign(48 * (size_t)n, 0);
    for (uint32_t i = 0; i < n; i++) {
        if (idx[i] >= kGroupColumns && o.bad == kGroupEmpty) o.bad = i;
        auto it = seen.emplace(std::string((const char *)bytes + 48 * (size_t)i, 48), o.m);
        if (it.second) {
            memcpy(&o.distinct[48 * (size_t)o.m], bytes + 48 * (size_t)i, 48);
            o.first_item.push_back(i);
            o.m++;
        }
        o.rows.push_back(it.first->second);
    }
    for (uint32_t j = o.m; j < n; j++) o.distinct[48 * (size_t)j] = 0xc0;
    o.row_off.assign(o.m + 1, 0);
    o.col_off.assign(kGroupColumns + 1, 0);
    for (uint32_t i = 0; i < n; i++) {
        o.row_off[o.rows[i] + 1]++;
        if (idx[i] < kGroupColumns) o.col_off[idx[i] + 1]++;
    }
    for (uint32_t j = 0; j < o.m; j++) o.row_off[j + 1] += o.row_off[j];
    for (uint32_t k = 0; k < kGroupColumns; k++) o.col_off[k + 1] += o.col_off[k];
    return o;
}

static bool groups_hold(const std::vector<uint32_t> &perm, const std::vector<uint32_t> &off, const std::vector<uint64_t> &key_of, uint32_t groups) {
    std::set<uint32_t> all;
    for (uint32_t g = 0; g < groups; g++)
        for (uint32_t s = off[g]; s < off[g + 1]; s++) {
            if (perm[s] >= key_of.size() || key_of[perm[s]] != g || !all.insert(perm[s]).second) return false;
        }
    size_t members = 0;
    for (uint64_t k : key_of) members += k < groups;
    return all.size() == members;
}

static int check(const char *name, const std::vector<uint64_t> &comms, const std::vector<uint64_t> &idx, uint64_t seed, uint32_t hash_mask) {
    const uint32_t n = (uint32_t)idx.size();
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; i++) order[i] = i;
    for (uint32_t i = n; i > 1; i--) std::swap(order[i - 1], order[rnd64() % i]);
    const Out got = as_the_kernels(comms, idx, seed, hash_mask, order), want = plain(comms, idx);
    std::vector<uint64_t> rows64(got.rows.begin(), got.rows.end());
    const bool ok = !got.error && got.m == want.m && got.bad == want.bad && got.rows == want.rows && got.first_item == want.first_item &&
                    got.distinct == want.distinct && got.row_off == want.row_off && got.col_off == want.col_off &&
                    groups_hold(got.perm_row, got.row_off, rows64, got.m) && groups_hold(got.perm_col, got.col_off, idx, kGroupColumns);
    if (!ok) printf("MISMATCH %s n=%u seed=%llx mask=%x (m %u / %u, error %d)\n", name, n, (unsigned long long)seed, hash_mask, got.m, want.m, got.error);
    return ok ? 0 : 1;
}

int main() {
    int bad = 0, cases = 0;
    for (size_t cap : {1, 2, 31, 32, 33, 255, 256, 257, 4097, 8192}) {
        const size_t s = group_table_slots(cap);
        cases++;
        if (s < 2 * cap || (s & (s - 1)) || s < 64) bad++, printf("MISMATCH table size %zu for %zu\n", s, cap);
    }
    const uint32_t ns[] = {1, 2, 255, 256, 257, 300, 1025, 4097};
    for (uint32_t n : ns)
        for (int shape = 0; shape < 5; shape++) {
            std::vector<uint64_t> comms(6 * (size_t)n), idx(n);
            const uint32_t distinct = shape == 0 ? 1 : shape == 1 ? n : 37;
            std::vector<uint64_t> pool(6 * (size_t)distinct);
            for (auto &w : pool) w = rnd64();
            for (uint32_t i = 0; i < n; i++) {
                const uint32_t d = shape < 3 ? (shape == 1 ? i : (uint32_t)(rnd64() % distinct)) : i;
                for (int k = 0; k < 6; k++) comms[6 * (size_t)i + k] = shape < 3 ? pool[6 * (size_t)d + k] : 0x1111111111111111ull * (k + 1);
                uint8_t *b = (uint8_t *)&comms[6 * (size_t)i];
                if (shape == 3) memcpy(b + 44, &i, 4);          // equal except in the last four bytes
                if (shape == 4) b[0] = (uint8_t)(i % 200);      // equal except in the first byte (200 distinct at most)
                idx[i] = shape == 0 ? 77 : shape == 1 ? i % 128 : rnd64() % 128;
            }
            for (int variant = 0; variant < 4; variant++) {
                std::vector<uint64_t> ix = idx;
                if (variant == 2 && n > 2) ix[n - 2] = 128, ix[1] = 1ull << 63;
                if (variant == 3) ix[n - 1] = ~0ull;
                const uint64_t seed = variant == 1 ? 0 : rnd64();
                const uint32_t masks[] = {0xffffffffu, 0u, 1u};
                for (uint32_t mask : masks) {
                    if (mask != 0xffffffffu && n > 300) continue;   // one chain is quadratic: small n only
                    cases++;
                    bad += check("grouping", comms, ix, seed, mask);
                }
            }
        }
    // two seeds: another placement of the same keys, the same result (checked above); the placement itself does differ
    {
        std::vector<uint64_t> comms(6 * 300), idx(300, 5);
        for (auto &w : comms) w = rnd64();
        std::vector<uint32_t> order(300);
        for (uint32_t i = 0; i < 300; i++) order[i] = i;
        const Out a = as_the_kernels(comms, idx, 1, 0xffffffffu, order), b = as_the_kernels(comms, idx, 2, 0xffffffffu, order);
        cases++;
        if (a.slot_of == b.slot_of || a.rows != b.rows) bad++, printf("MISMATCH seeds\n");
        const Out c = as_the_kernels(comms, idx, 1, 0u, order);
        cases++;
        for (uint32_t i = 0; i < 300; i++)
            if (c.slot_of[i] != i) {   // mask 0, inserted in index order, all distinct: one chain from slot 0
                bad++, printf("MISMATCH chain at %u\n", i);
                break;
            }
    }
    if (!bad) printf("ok: %d cases\n", cases);
    return bad != 0;
}
