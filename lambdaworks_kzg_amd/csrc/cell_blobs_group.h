// cell_blobs_group.h -- the grouping of the commitments of whole blobs on the device (cell_blobs_group.hip): what
// plan_blobs (cell_blobs_plan.h) makes on the host, for a cell verifier that never brings the commitments down. A call has at most
// kBlobGroupCap blobs (one extension chunk), so ONE workgroup does all of it with the table, the scans and the counting sort in its
// LDS: a lane per blob, the steps below between the workgroup's barriers. The steps are written once, free of HIP, over a block of
// shared words (BlobGroupShared: the kernel's LDS, a plain struct on the host) and an atomics policy: tests/cell_blobs_group_check.cpp
// runs them lane after lane, in several lane orders, against plan_blobs under the sanitizers.
//
// The key of a blob is (its group, its 48 commitment bytes) under the verifier's seeded SipHash (cell_group.cuh: group_slot_hash_seg;
// a transaction pool's inputs are as adversarial as gossip). A slot holds a BLOB INDEX, as cell_group.hip's slots hold item indices:
// claimed by CAS(empty -> b); a later arrival compares its bytes against the INPUT bytes of the blob it found there and on equality
// lowers the slot with an atomic minimum, so that the slot ends at the key's first occurrence. Groups are contiguous blob ranges, so
// one scan of the first-occurrence flags in blob order numbers the CONCATENATED rows, and a group's rows start at the count of flags
// in front of its first blob (k_group_scan / k_seg_rows' rule).
#pragma once
#include "cell_blobs_plan.h"
#include "cell_group.cuh"

namespace lwk {

constexpr uint32_t kBlobGroupCap = 512;                      // blobs of one call: kCellsChunk, one extension chunk
constexpr uint32_t kBlobGroupSlots = 2 * kBlobGroupCap;      // never more than half full: every probe chain ends
constexpr uint32_t kBlobHeadM = 0, kBlobHeadBad = 1, kBlobHeadErr = 2, kBlobHeadWords = 4;   // (kernels.h: kGroupHead*)

// the workgroup's words: 20 KiB
struct BlobGroupShared {
    uint32_t table[kBlobGroupSlots];      // slot -> the lowest blob of the slot's key, or kGroupEmpty
    uint32_t slot_row[kBlobGroupSlots];   // slot -> the key's concatenated row
    uint32_t slot_of[kBlobGroupCap];      // blob -> its slot, or kGroupEmpty (a probe that ran out: never, with a table half full)
    uint32_t crow[kBlobGroupCap];         // blob -> its concatenated row, or kGroupEmpty
    uint32_t pre[kBlobGroupCap + 1];      // the exclusive scan of the first-occurrence flags; pre[nb] = M
    uint32_t cnt[kBlobGroupCap + 1];      // row -> its blobs; scanned in place: row -> the blobs in front of it (cnt[M]: all)
    uint32_t cur[kBlobGroupCap];          // row -> the places of its list taken so far
    uint32_t err;
};

// what the grouping leaves in device memory. Capacities for nb blobs in g groups: brow, bgroup, bperm nb; brow_off nb + 1; bfirst nb;
// row_base g + 1 (nullptr for a batch); distinct 48 nb; head kBlobHeadWords
struct BlobGroupOut {
    uint32_t *brow;       // blob b's row, local to its group
    uint32_t *bgroup;     // blob b's group
    uint32_t *bperm;      // the blobs in the order (group, row); the order inside a row is not defined
    uint32_t *brow_off;   // M + 1: the concatenated rows' offsets in bperm (in BLOBS)
    uint32_t *bfirst;     // M: the first blob of every concatenated row
    uint32_t *row_base;   // g + 1: the groups' first concatenated rows; row_base[g] = M
    uint8_t *distinct;    // the groups' distinct commitments one after the other, in order of first occurrence
    uint32_t *head;       // [kBlobHeadM] = M, [kBlobHeadBad] = 0 (every index of a blob's items is below 128), [kBlobHeadErr]
};

// the group of blob b: item_off (the groups' offsets in ITEMS, 128 per blob, g + 1 valid values; nullptr: one group of all nb blobs)
LWK_GROUP_HD uint32_t blob_group_of(const uint32_t *item_off, uint32_t g, uint32_t b) {
    if (!item_off) return 0;
    uint32_t lo = 0, hi = g;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if ((item_off[mid] >> 7) <= b) lo = mid;
        else hi = mid;
    }
    return lo;
}
LWK_GROUP_HD uint32_t blob_group_lo(const uint32_t *item_off, uint32_t j) { return item_off ? item_off[j] >> 7 : 0u; }
LWK_GROUP_HD uint32_t blob_group_hi(const uint32_t *item_off, uint32_t j, uint32_t nb) { return item_off ? item_off[j + 1] >> 7 : nb; }

// ---- the steps, one call per lane each, a barrier between two steps. lanes: kBlobGroupCap in the kernel -----------------------------------
// step 0: the table empty, the counters zero, bperm the identity (a place no lane takes below stays a subscript in range)
LWK_GROUP_HD void blob_group_clear(BlobGroupShared &sh, uint32_t lane, uint32_t lanes, uint32_t nb, const BlobGroupOut &o) {
    for (uint32_t s = lane; s < kBlobGroupSlots; s += lanes) sh.table[s] = kGroupEmpty, sh.slot_row[s] = kGroupEmpty;
    for (uint32_t r = lane; r <= kBlobGroupCap; r += lanes) sh.cnt[r] = 0;
    for (uint32_t r = lane; r < kBlobGroupCap; r += lanes) sh.cur[r] = 0, sh.crow[r] = kGroupEmpty, sh.slot_of[r] = kGroupEmpty;
    for (uint32_t b = lane; b < nb; b += lanes) o.bperm[b] = b;
    if (lane == 0) sh.err = 0;
}

// step 1: blob b into the table (cell_group.hip: group_probe, on a table in LDS and over blobs)
template <class Atomics>
LWK_GROUP_HD void blob_group_insert(BlobGroupShared &sh, uint32_t b, uint32_t nb, const uint8_t *comms, const uint32_t *item_off, uint32_t g,
                                    uint64_t seed, uint32_t hash_mask) {
    if (b >= nb) return;
    const uint32_t j = blob_group_of(item_off, g, b), lo = blob_group_lo(item_off, j), hi = blob_group_hi(item_off, j, nb);
    uint64_t key[6];
    group_load48(key, comms + 48 * (size_t)b);
    uint32_t s = group_slot_hash_seg(key, j, seed, hash_mask) & (kBlobGroupSlots - 1), found = kGroupEmpty;
    for (uint32_t probe = 0; probe < kBlobGroupSlots; probe++, s = (s + 1) & (kBlobGroupSlots - 1)) {
        const uint32_t c = Atomics::cas(&sh.table[s], kGroupEmpty, b);
        if (c == kGroupEmpty) {   // claimed
            found = s;
            break;
        }
        if (c >= nb) break;       // (no lane writes such a word)
        if (c >= lo && c < hi && group_equal48(key, comms + 48 * (size_t)c)) {   // (the group is asked before c's bytes are read)
            Atomics::min(&sh.table[s], b);
            found = s;
            break;
        }
    }
    if (found == kGroupEmpty) Atomics::bit_or(&sh.err, 1u);
    sh.slot_of[b] = found;
}

// step 2: is blob b its key's first occurrence? The caller scans the flags in blob order into sh.pre (pre[nb] = M)
LWK_GROUP_HD uint32_t blob_group_flag(const BlobGroupShared &sh, uint32_t b, uint32_t nb) {
    if (b >= nb) return 0;
    const uint32_t s = sh.slot_of[b];
    return s != kGroupEmpty && sh.table[s] == b ? 1u : 0u;
}

// step 3: a first occurrence names its row, its first blob and its bytes; the groups' first rows
LWK_GROUP_HD void blob_group_first(BlobGroupShared &sh, uint32_t lane, uint32_t lanes, uint32_t nb, const uint8_t *comms,
                                   const uint32_t *item_off, uint32_t g, const BlobGroupOut &o) {
    if (blob_group_flag(sh, lane, nb)) {
        const uint32_t row = sh.pre[lane];   // < nb: at most one flag per blob
        sh.slot_row[sh.slot_of[lane]] = row;
        o.bfirst[row] = lane;
        const uint64_t *src = (const uint64_t *)(comms + 48 * (size_t)lane);
        uint64_t *dst = (uint64_t *)(o.distinct + 48 * (size_t)row);
        for (int k = 0; k < 6; k++) dst[k] = src[k];
    }
    if (o.row_base)   // (right for an empty group and for groups at the very end, whose offset is nb)
        for (uint32_t q = lane; q <= g; q += lanes) {
            const uint32_t at = blob_group_lo(item_off, q);
            o.row_base[q] = sh.pre[at <= nb ? at : nb];
        }
}

// step 4: blob b's rows -- concatenated (for the sort) and local to its group -- and its group; the rows' counts
template <class Atomics>
LWK_GROUP_HD void blob_group_rows(BlobGroupShared &sh, uint32_t b, uint32_t nb, const uint32_t *item_off, uint32_t g, const BlobGroupOut &o) {
    if (b >= nb) return;
    const uint32_t j = blob_group_of(item_off, g, b), first = sh.pre[blob_group_lo(item_off, j)], s = sh.slot_of[b];
    uint32_t crow = s != kGroupEmpty ? sh.slot_row[s] : kGroupEmpty;
    if (crow >= nb || crow < first) {   // only behind a failed insertion: keep every subscript in range, report
        Atomics::bit_or(&sh.err, 2u);
        crow = kGroupEmpty;
    } else {
        Atomics::add(&sh.cnt[crow], 1u);
    }
    sh.crow[b] = crow;
    o.brow[b] = crow != kGroupEmpty ? crow - first : 0u;
    o.bgroup[b] = j;
}

// (between 4 and 5 the caller scans sh.cnt[0 .. M) in place, exclusively, cnt[M] = the total, and writes o.brow_off[0 .. M] from it)

// step 5: blob b takes the next place of its row's list; the head words
template <class Atomics>
LWK_GROUP_HD void blob_group_scatter(BlobGroupShared &sh, uint32_t b, uint32_t nb, const BlobGroupOut &o) {
    if (b == 0) {
        o.head[kBlobHeadM] = sh.pre[nb];
        o.head[kBlobHeadBad] = 0;
        o.head[kBlobHeadErr] = sh.err;
        o.head[3] = 0;
    }
    if (b >= nb) return;
    const uint32_t crow = sh.crow[b];
    if (crow >= nb) return;
    const uint32_t at = sh.cnt[crow] + Atomics::add(&sh.cur[crow], 1u);
    if (at < nb) o.bperm[at] = b;
}

// ---- the expansion: what the 128 nb-entry lists need beside blob_item_lists / blob_col_off / blob_pad_word (cell_blobs_plan.h) -----------
// word r of the rows' offsets and of their first items, in ITEMS: a row's list is its blobs' items, a row's first item its first blob's
LWK_GROUP_HD uint32_t blob_row_off_items(const uint32_t *brow_off, uint32_t r) { return brow_off[r] << 7; }
LWK_GROUP_HD uint32_t blob_first_item(const uint32_t *bfirst, uint32_t r) { return bfirst[r] << 7; }

}  // namespace lwk
