// recover_sets.h -- the index sets of the EIP-7594 recovery calls on the host: one list of 64 .. 128 ascending cell
// indices -> a RecoverSet, and the lists of a call, one per blob (mixed) or one for all (shared set) -> its distinct sets, a set id and a
// cell offset per blob, or the first blob whose list is at fault. Plain C++, no HIP header: tests/recover_sets_check.cpp compiles it for
// the host.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <array>
#include <map>
#include <vector>

namespace lwk {

constexpr size_t kRecoverCells = 128;                  // cells per blob (kernels.h: kCellsPerBlob)
constexpr size_t kRecoverMinCells = kRecoverCells / 2;

// the index set of one blob: k[i] = the index of the i-th given cell (ascending), and bit q of `given` = the cell at position
// q = bitrev7(k), whose c_k is w128^q, is among them. The shared-set kernels take it by value
struct RecoverSet {
    uint8_t k[kRecoverCells];
    uint32_t given[kRecoverCells / 32];
};

enum RecoverListFault { kRecoverListGood = 0, kRecoverListCount, kRecoverListIndex, kRecoverListOrder };

// one list -> its set. *at (optional): the place in the list the fault was found at
inline RecoverListFault recover_set_of(RecoverSet &set, const uint64_t *idx, size_t num_cells, size_t *at = nullptr) {
    if (num_cells < kRecoverMinCells || num_cells > kRecoverCells) return kRecoverListCount;
    memset(&set, 0, sizeof set);
    for (size_t i = 0; i < num_cells; i++) {
        if (at) *at = i;
        if (idx[i] >= (uint64_t)kRecoverCells) return kRecoverListIndex;
        if (i > 0 && idx[i] <= idx[i - 1]) return kRecoverListOrder;
        const uint32_t k = (uint32_t)idx[i];
        uint32_t q = 0;
        for (int b = 0; b < 7; b++) q |= ((k >> b) & 1u) << (6 - b);
        set.k[i] = (uint8_t)k;
        set.given[q >> 5] |= 1u << (q & 31u);
    }
    return kRecoverListGood;
}

// the lists of a call, blob after blob in idx. sets: the distinct ones in order of first occurrence (two lists are the same set
// exactly when their masks are equal); set_of[b]: blob b's set; cell_off[b]: the cells in front of blob b's (n + 1 entries, the last
// one the call's total)
struct RecoverSets {
    std::vector<RecoverSet> sets;
    std::vector<uint32_t> set_of;
    std::vector<size_t> cell_off;
    RecoverListFault fault = kRecoverListGood;
    size_t bad_blob = 0, bad_at = 0;   // with a fault: the first blob whose list has one, and the place in that list
};

inline bool recover_sets_of(RecoverSets &out, const uint64_t *idx, const size_t *num_cells, size_t n) {
    out = RecoverSets();
    out.set_of.reserve(n);
    out.cell_off.reserve(n + 1);
    out.cell_off.push_back(0);
    std::map<std::array<uint32_t, 4>, uint32_t> ids;
    size_t off = 0;
    for (size_t b = 0; b < n; b++) {
        RecoverSet set;
        out.bad_at = 0;
        out.fault = recover_set_of(set, idx + off, num_cells[b], &out.bad_at);
        if (out.fault != kRecoverListGood) {
            out.bad_blob = b;
            return false;
        }
        const std::array<uint32_t, 4> mask = {set.given[0], set.given[1], set.given[2], set.given[3]};
        const auto ins = ids.emplace(mask, (uint32_t)out.sets.size());
        const size_t id = ins.first->second;
        if (id == out.sets.size()) out.sets.push_back(set);
        out.set_of.push_back((uint32_t)id);
        off += num_cells[b];
        out.cell_off.push_back(off);
    }
    return true;
}

// a shared-set call of n blobs as the call it is: one list -> one set, every blob's id 0 and num_cells cells per blob. A fault is the
// list's, as recover_set_of reports it (bad_blob says nothing)
inline bool recover_sets_shared(RecoverSets &out, const uint64_t *idx, size_t num_cells, size_t n) {
    out = RecoverSets();
    RecoverSet set;
    out.fault = recover_set_of(set, idx, num_cells, &out.bad_at);
    if (out.fault != kRecoverListGood) return false;
    out.sets.push_back(set);
    out.set_of.assign(n, 0);
    for (size_t b = 0; b <= n; b++) out.cell_off.push_back(b * num_cells);
    return true;
}

}  // namespace lwk
