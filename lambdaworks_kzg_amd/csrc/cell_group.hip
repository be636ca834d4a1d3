// cell_group.hip -- the items of a cell proof batch grouped on the device: what group_items
// (cells_verify_api.hip) does on the host -- commitments de-duplicated by byte equality in order of first occurrence, the items
// counting-sorted by row and by column -- as six latency-shaped launches, so that an asynchronous cell verifier
// (cells_verify_async.hip) never brings the commitments to the host to learn m. lwkzg_cell_group_device is the test hook.
//
//   k_group_insert    one lane per item: its 48 bytes into an open-addressing table in HBM. A slot holds an ITEM INDEX: claimed by
//                     atomicCAS(empty -> i); a later arrival compares its bytes against the INPUT bytes at the index it found there
//                     (immutable: no lane ever waits for another lane's store) and on equality lowers the slot with atomicMin, else
//                     probes on. Every index a slot ever holds carries the slot's key, so one word serves as claim and as first
//                     occurrence. The table has >= 2 n slots, every probe loop is bounded by the table size, and a loop that runs
//                     out raises the error word instead of spinning. The lowest index >= 128 is recorded here too.
//   k_group_scan      ONE workgroup walks the items in index order, 1024 at a time: is_first[i] = (table[slot_of[i]] == i), an
//                     exclusive scan of the flags is the row id; the first item of row j writes slot_row, first_item[j], distinct[j]; m.
//   k_group_rows      rows[i] = slot_row[slot_of[i]], the histograms of both lists (rows: atomics in HBM; columns: 128 bins in LDS,
//                     flushed once per workgroup), and the infinity encodings behind the m-th distinct commitment.
//   k_group_offsets   two workgroups: the exclusive scans row_off[m + 1] and col_off[129].
//   k_group_scatter   perm_row / perm_col: a lane takes the next free place of its group from the group's counter, counted down.
//                     The order inside a group is whatever the atomics gave: every consumer sums field elements exactly.
// An index >= 128 is never a bin or a subscript here: such an item is left out of the column list, and the verifier's skip word keeps
// everything that reads idx[] as a subscript from running.
// The second half of the file is the same for a call of g groups (k_seg_*: the segmented grouping and the slice table of a cell
// verifier's grouped calls; lwkzg_cell_group_segmented_device is its test hook). What the two do alike is
// written once: the probe of the table (group_probe), and k_group_scan and k_group_offsets, which both launch as they are. What they
// do differently stays two kernels: the batch keeps a row for every item, whatever its index, and bins columns in LDS; a group with a
// bad index has no rows at all, and its bins are (group, column) pairs in HBM.
#include "abi_guard.h"
#include "carve.h"
#include "cell_group.cuh"
#include "cell_groups_plan.h"
#include "kernels.h"

#include <vector>

namespace lwk {

namespace {

constexpr int kGroupLanes = 256;    // the per-item kernels
constexpr int kScanLanes = 1024;    // the single-workgroup scans
constexpr int kScanWaves = kScanLanes / 64;

// exclusive scan of v over the workgroup's kScanLanes lanes (all of them call it); *total: the sum. wave_tot: kScanWaves words of LDS
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *wave_tot, uint32_t *total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= (uint32_t)d) inc += up;
    }
    if (lane == 63) wave_tot[wave] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kScanWaves; w++) {
        const uint32_t t = wave_tot[w];
        before += (uint32_t)w < wave ? t : 0u;
        all += t;
    }
    __syncthreads();   // wave_tot is free for the next chunk
    *total = all;
    return before + inc - v;
}

// Item i (key: its 48 bytes) into the table, probing from slot s: the slot it claimed or shares with the items of its key, or
// kGroupEmpty where the probe ran out or met a word no lane of this launch writes. may_share(c): may item c be of i's row at all (a
// segmented grouping: only an item of i's group) -- asked before c's bytes are read.
template <class MayShare>
__device__ __forceinline__ uint32_t group_probe(const uint8_t *__restrict__ comms, uint32_t *__restrict__ table, const uint64_t key[6], uint32_t s,
                                                uint32_t i, uint32_t n, uint32_t slot_mask, MayShare may_share) {
    uint32_t found = kGroupEmpty;
#pragma unroll 1
    for (uint32_t probe = 0; probe <= slot_mask; probe++, s = (s + 1) & slot_mask) {
        const uint32_t c = atomicCAS(&table[s], kGroupEmpty, i);
        if (c == kGroupEmpty) {   // claimed
            found = s;
            break;
        }
        if (c >= n) break;        // (no lane writes such a word: the table is not this launch's)
        if (may_share(c) && group_equal48(key, comms + 48 * (size_t)c)) {
            atomicMin(&table[s], i);
            found = s;
            break;
        }
    }
    return found;
}

}  // namespace

__global__ __launch_bounds__(kGroupLanes) void k_group_insert(const uint8_t *__restrict__ comms, const uint64_t *__restrict__ idx,
                                                              uint32_t *__restrict__ table, uint32_t *__restrict__ slot_of,
                                                              uint32_t *__restrict__ head, uint32_t n, uint32_t slot_mask, uint64_t seed,
                                                              uint32_t hash_mask) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (idx[i] >= (uint64_t)kGroupColumns) atomicMax(&head[kGroupHeadBad], ~i);
    uint64_t key[6];
    group_load48(key, comms + 48 * (size_t)i);
    uint32_t found = group_probe(comms, table, key, group_slot_hash(key, seed, hash_mask) & slot_mask, i, n, slot_mask,
                                 [](uint32_t) { return true; });
    if (found == kGroupEmpty) {
        atomicOr(&head[kGroupHeadErr], 1u);
        found = 0;
    }
    slot_of[i] = found;
}

// pre (nullptr for the batch): the flags' exclusive scan itself, pre[i] for i <= n -- what the segmented grouping reads a group's first
// row off. An item without a slot (slot_of[i] == kGroupEmpty: only the segmented insertion leaves one) is nobody's first occurrence.
__global__ __launch_bounds__(kScanLanes) void k_group_scan(const uint8_t *__restrict__ comms, const uint32_t *__restrict__ table,
                                                           const uint32_t *__restrict__ slot_of, uint32_t *__restrict__ slot_row,
                                                           uint32_t *__restrict__ first_item, uint8_t *__restrict__ distinct,
                                                           uint32_t *__restrict__ pre, uint32_t *__restrict__ head, uint32_t n) {
    __shared__ uint32_t wave_tot[kScanWaves];
    uint32_t run = 0;
#pragma unroll 1
    for (uint32_t base = 0; base < n; base += kScanLanes) {   // (n is the same for every lane: they all meet the barriers)
        const uint32_t i = base + threadIdx.x;
        uint32_t s = kGroupEmpty, flag = 0;
        if (i < n) {
            s = slot_of[i];
            flag = s != kGroupEmpty && table[s] == i ? 1u : 0u;
        }
        uint32_t total;
        const uint32_t before = block_exclusive_scan(flag, wave_tot, &total);
        if (pre && i < n) pre[i] = run + before;
        if (flag) {
            const uint32_t row = run + before;   // < n: at most one flag per item
            slot_row[s] = row;
            first_item[row] = i;
            const uint64_t *src = (const uint64_t *)(comms + 48 * (size_t)i);
            uint64_t *dst = (uint64_t *)(distinct + 48 * (size_t)row);
#pragma unroll
            for (int k = 0; k < 6; k++) dst[k] = src[k];
        }
        run += total;
    }
    if (threadIdx.x == 0) {
        head[kGroupHeadM] = run;
        if (pre) pre[n] = run;
    }
}

__global__ __launch_bounds__(kGroupLanes) void k_group_rows(const uint64_t *__restrict__ idx, const uint32_t *__restrict__ slot_of,
                                                            const uint32_t *__restrict__ slot_row, uint32_t *__restrict__ rows,
                                                            uint32_t *__restrict__ row_cnt, uint32_t *__restrict__ col_cnt,
                                                            uint8_t *__restrict__ distinct, uint32_t *__restrict__ head, uint32_t n) {
    __shared__ uint32_t bins[kGroupColumns];
    if (threadIdx.x < kGroupColumns) bins[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        uint32_t row = slot_row[slot_of[i]];
        if (row >= n) {   // only behind a failed insertion (the slot is nobody's): keep every subscript in range, report
            atomicOr(&head[kGroupHeadErr], 2u);
            row = 0;
        }
        rows[i] = row;
        atomicAdd(&row_cnt[row], 1u);
        const uint64_t k = idx[i];
        if (k < (uint64_t)kGroupColumns) atomicAdd(&bins[(uint32_t)k], 1u);
        if (i >= head[kGroupHeadM]) {   // the padding the two-set launches take: infinity
            uint64_t *dst = (uint64_t *)(distinct + 48 * (size_t)i);
            dst[0] = 0xc0ull;   // (little-endian: byte 0)
#pragma unroll
            for (int q = 1; q < 6; q++) dst[q] = 0;
        }
    }
    __syncthreads();
    if (threadIdx.x < kGroupColumns && bins[threadIdx.x]) atomicAdd(&col_cnt[threadIdx.x], bins[threadIdx.x]);
}

// workgroup 0: row_off[0 .. m] from row_cnt; workgroup 1: col_off[0 .. cols] from col_cnt (cols: 128 for the batch, 128 g for a call
// of g groups)
__global__ __launch_bounds__(kScanLanes) void k_group_offsets(const uint32_t *__restrict__ row_cnt, const uint32_t *__restrict__ col_cnt,
                                                              uint32_t *__restrict__ row_off, uint32_t *__restrict__ col_off,
                                                              const uint32_t *__restrict__ head, uint32_t n, uint32_t cols) {
    __shared__ uint32_t wave_tot[kScanWaves];
    const bool by_col = blockIdx.x != 0;
    const uint32_t *cnt = by_col ? col_cnt : row_cnt;
    uint32_t *off = by_col ? col_off : row_off;
    uint32_t len = by_col ? cols : head[kGroupHeadM];
    if (len > n && !by_col) len = n;
    uint32_t run = 0;
#pragma unroll 1
    for (uint32_t base = 0; base < len; base += kScanLanes) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < len ? cnt[i] : 0u;
        uint32_t total;
        const uint32_t before = block_exclusive_scan(v, wave_tot, &total);
        if (i < len) off[i] = run + before;
        run += total;
    }
    if (threadIdx.x == 0) off[len] = run;
}

__global__ __launch_bounds__(kGroupLanes) void k_group_scatter(const uint64_t *__restrict__ idx, const uint32_t *__restrict__ rows,
                                                               const uint32_t *__restrict__ row_off, const uint32_t *__restrict__ col_off,
                                                               uint32_t *__restrict__ row_cnt, uint32_t *__restrict__ col_cnt,
                                                               uint32_t *__restrict__ perm_row, uint32_t *__restrict__ perm_col, uint32_t n) {
    __shared__ uint32_t bins[kGroupColumns], first[kGroupColumns];
    if (threadIdx.x < kGroupColumns) bins[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    uint32_t col = kGroupColumns, rank = 0;
    if (i < n) {
        const uint32_t row = rows[i];   // < n (k_group_rows)
        const uint32_t at = row_off[row] + atomicSub(&row_cnt[row], 1u) - 1u;
        if (at < n) perm_row[at] = i;
        const uint64_t k = idx[i];
        if (k < (uint64_t)kGroupColumns) {
            col = (uint32_t)k;
            rank = atomicAdd(&bins[col], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < kGroupColumns && bins[threadIdx.x])   // this workgroup's run of places in the column, taken from the top
        first[threadIdx.x] = atomicSub(&col_cnt[threadIdx.x], bins[threadIdx.x]) - bins[threadIdx.x];
    __syncthreads();
    if (col < kGroupColumns) {
        const uint32_t at = col_off[col] + first[col] + rank;
        if (at < n) perm_col[at] = i;
    }
}

void launch_cell_group(const uint8_t *comms48, const uint64_t *idx, size_t n, size_t slots, uint64_t seed, uint32_t hash_mask,
                       const CellGroupBufs &g, hipStream_t st) {
    const uint32_t n32 = (uint32_t)n;
    const dim3 per_item((unsigned)((n + kGroupLanes - 1) / kGroupLanes));
    hipMemsetAsync(g.table, 0xff, slots * 4, st);
    hipMemsetAsync(g.row_cnt, 0, n * 4, st);
    hipMemsetAsync(g.col_cnt, 0, (kGroupColumns + kGroupHeadWords) * 4, st);
    prof_launch("k_group_insert", st, k_group_insert, per_item, dim3(kGroupLanes), 0, comms48, idx, g.table, g.slot_of, g.head, n32,
                (uint32_t)(slots - 1), seed, hash_mask);
    prof_launch("k_group_scan", st, k_group_scan, dim3(1), dim3(kScanLanes), 0, comms48, (const uint32_t *)g.table, (const uint32_t *)g.slot_of,
                g.slot_row, g.first_item, g.distinct, (uint32_t *)nullptr, g.head, n32);
    prof_launch("k_group_rows", st, k_group_rows, per_item, dim3(kGroupLanes), 0, idx, (const uint32_t *)g.slot_of, (const uint32_t *)g.slot_row,
                g.rows, g.row_cnt, g.col_cnt, g.distinct, g.head, n32);
    prof_launch("k_group_offsets", st, k_group_offsets, dim3(2), dim3(kScanLanes), 0, (const uint32_t *)g.row_cnt, (const uint32_t *)g.col_cnt,
                g.row_off, g.col_off, (const uint32_t *)g.head, n32, kGroupColumns);
    prof_launch("k_group_scatter", st, k_group_scatter, per_item, dim3(kGroupLanes), 0, idx, (const uint32_t *)g.rows, (const uint32_t *)g.row_off,
                (const uint32_t *)g.col_off, g.row_cnt, g.col_cnt, g.perm_row, g.perm_col, n32);
}

// ---- the segmented grouping: a call of g groups ---------------------------------------------------------------------
// What plan_groups (cell_groups_plan.h) makes on the host, for a verifier that never brings the commitments down. The key of an item is
// (its group, its 48 bytes): the same commitment in two groups is two rows. Groups are contiguous item ranges, so ONE scan of the
// first-occurrence flags over all items in index order numbers the CONCATENATED rows directly, and a group's rows start at the count of
// flags in front of its first item.
//   k_seg_mark        one lane per item: its group (a binary search of the offsets), and the group's bad word where its index is >= 128
//   k_seg_insert      k_group_insert with the group in the slot hash and in the equality test. Whether the item found in a slot is of
//                     the same group is read off the OFFSETS (immutable), not off another lane's store. The items of a group with a
//                     bad word take no slot.
//   k_group_scan      as above, and it keeps the flags' exclusive scan pre[i] (pre[n] = M)
//   k_seg_rows        the concatenated row of every item (kept in slot_of), its group-local row, both histograms (in HBM: the bins are
//                     (group, column) pairs), row_base[j] = pre[item_off[j]] -- right for an empty group and for groups at the very
//                     end, whose offset is n -- and the infinity encodings behind the M-th distinct commitment
//   k_group_offsets   as above: the exclusive scans row_off[M + 1] and col_off[128 g + 1]
//   k_seg_scatter     perm_row / perm_col, places counted down from the counters as in k_group_scatter
// An index >= 128 is never a bin or a subscript: its whole group has no slot, row, column or place in a list.
namespace {

// the group of item i: item_off[j] <= i < item_off[j + 1] (offsets valid, i < n: item_off[0] = 0 <= i < n = item_off[g])
__device__ __forceinline__ uint32_t seg_group_of(const uint32_t *__restrict__ item_off, uint32_t g, uint32_t i) {
    uint32_t lo = 0, hi = g;
#pragma unroll 1
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (item_off[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}

}  // namespace

__global__ __launch_bounds__(kGroupLanes) void k_seg_mark(const uint64_t *__restrict__ idx, const uint32_t *__restrict__ item_off,
                                                          uint32_t *__restrict__ item_group, uint32_t *__restrict__ gbad, uint32_t n,
                                                          uint32_t g) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = seg_group_of(item_off, g, i);
    item_group[i] = j;
    if (idx[i] >= (uint64_t)kGroupColumns) atomicOr(&gbad[j], 1u);
}

__global__ __launch_bounds__(kGroupLanes) void k_seg_insert(const uint8_t *__restrict__ comms, const uint32_t *__restrict__ item_off,
                                                            const uint32_t *__restrict__ item_group, const uint32_t *__restrict__ gbad,
                                                            uint32_t *__restrict__ table, uint32_t *__restrict__ slot_of,
                                                            uint32_t *__restrict__ head, uint32_t n, uint32_t slot_mask, uint64_t seed,
                                                            uint32_t hash_mask) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = item_group[i];
    if (gbad[j]) {   // (k_seg_mark is complete: the word is final)
        slot_of[i] = kGroupEmpty;
        return;
    }
    const uint32_t lo = item_off[j], hi = item_off[j + 1];
    uint64_t key[6];
    group_load48(key, comms + 48 * (size_t)i);
    const uint32_t found = group_probe(comms, table, key, group_slot_hash_seg(key, j, seed, hash_mask) & slot_mask, i, n, slot_mask,
                                       [lo, hi](uint32_t c) { return c >= lo && c < hi; });
    if (found == kGroupEmpty) atomicOr(&head[kGroupHeadErr], 1u);   // (the item is in no row; host function 1 fails the call)
    slot_of[i] = found;
}

// lanes 0 .. max(n, g + 1) - 1
__global__ __launch_bounds__(kGroupLanes) void k_seg_rows(const uint64_t *__restrict__ idx, const uint32_t *__restrict__ item_off,
                                                          const uint32_t *__restrict__ item_group, uint32_t *__restrict__ slot_of,
                                                          const uint32_t *__restrict__ slot_row, const uint32_t *__restrict__ pre,
                                                          uint32_t *__restrict__ rows, uint32_t *__restrict__ row_base,
                                                          uint32_t *__restrict__ row_cnt, uint32_t *__restrict__ col_cnt,
                                                          uint8_t *__restrict__ distinct, uint32_t *__restrict__ head, uint32_t n, uint32_t g) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= g) {
        const uint32_t at = item_off[i];
        row_base[i] = pre[at <= n ? at : n];
    }
    if (i >= n) return;
    const uint32_t s = slot_of[i];
    uint32_t crow = kGroupEmpty, local = 0;
    if (s != kGroupEmpty) {
        const uint32_t j = item_group[i], first = pre[item_off[j]];
        crow = slot_row[s];
        if (crow >= n || crow < first) {   // only behind a failed insertion elsewhere: keep every subscript in range, report
            atomicOr(&head[kGroupHeadErr], 2u);
            crow = kGroupEmpty;
        } else {
            local = crow - first;
            atomicAdd(&row_cnt[crow], 1u);
            const uint64_t k = idx[i];
            if (k < (uint64_t)kGroupColumns) atomicAdd(&col_cnt[(size_t)kGroupColumns * j + (uint32_t)k], 1u);
        }
    }
    slot_of[i] = crow;   // from here on the item's CONCATENATED row (only lane i reads slot_of[i] in this launch)
    rows[i] = local;
    if (i >= head[kGroupHeadM]) {   // the padding the two-set launches take: infinity
        uint64_t *dst = (uint64_t *)(distinct + 48 * (size_t)i);
        dst[0] = 0xc0ull;   // (little-endian: byte 0)
#pragma unroll
        for (int q = 1; q < 6; q++) dst[q] = 0;
    }
}

__global__ __launch_bounds__(kGroupLanes) void k_seg_scatter(const uint64_t *__restrict__ idx, const uint32_t *__restrict__ item_group,
                                                             const uint32_t *__restrict__ crow_of, const uint32_t *__restrict__ row_off,
                                                             const uint32_t *__restrict__ col_off, uint32_t *__restrict__ row_cnt,
                                                             uint32_t *__restrict__ col_cnt, uint32_t *__restrict__ perm_row,
                                                             uint32_t *__restrict__ perm_col, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t crow = crow_of[i];
    if (crow >= n) return;   // an item of a group with a bad word (or behind a failed insertion): in neither list
    uint32_t at = row_off[crow] + atomicSub(&row_cnt[crow], 1u) - 1u;
    if (at < n) perm_row[at] = i;
    const uint64_t k = idx[i];
    if (k >= (uint64_t)kGroupColumns) return;
    const size_t bin = (size_t)kGroupColumns * item_group[i] + (uint32_t)k;
    at = col_off[bin] + atomicSub(&col_cnt[bin], 1u) - 1u;
    if (at < n) perm_col[at] = i;
}

// ---- the slice table of a call of g groups, on the device -------------------------------------------------------------------------------------
// One workgroup over the 3 g sums in order: sum 3 j + s of a group without a flag has plan_slice_count(terms) slices -- terms the
// group's items (s < 2) or its distinct commitments (s == 2) -- an exclusive scan of the counts is slice_off, and the sum's lane writes
// its slices by plan_slice: the rule plan_groups cuts by (cell_groups_plan.h). A flagged group has none. slice_off[3 g]: the live count.
__global__ __launch_bounds__(kScanLanes) void k_seg_slice_table(const uint32_t *__restrict__ item_off, const uint32_t *__restrict__ row_base,
                                                                const uint32_t *__restrict__ gflag, GroupSlice *__restrict__ slices,
                                                                uint32_t *__restrict__ slice_off, uint32_t sums, uint32_t max_slices) {
    __shared__ uint32_t wave_tot[kScanWaves];
    uint32_t run = 0;
#pragma unroll 1
    for (uint32_t base = 0; base < sums; base += kScanLanes) {
        const uint32_t q = base + threadIdx.x, j = q / 3, s = q - 3 * j;
        uint32_t first = 0, terms = 0;
        if (q < sums && !gflag[j]) {
            const uint32_t *off = s < 2 ? item_off : row_base;
            first = off[j];
            terms = off[j + 1] - first;
        }
        const uint32_t cnt = plan_slice_count(terms);
        uint32_t total;
        const uint32_t before = block_exclusive_scan(cnt, wave_tot, &total);
        if (q < sums) {
            slice_off[q] = run + before;
#pragma unroll 1
            for (uint32_t k = 0; k < cnt; k++) {
                const uint32_t at = run + before + k;
                if (at < max_slices) slices[at] = plan_slice(j, s, first, terms, k);
            }
        }
        run += total;
    }
    if (threadIdx.x == 0) slice_off[sums] = run < max_slices ? run : max_slices;
}

void launch_cell_group_seg(const uint8_t *comms48, const uint64_t *idx, size_t n, size_t g, size_t slots, uint64_t seed, uint32_t hash_mask,
                           const CellGroupSegBufs &s, hipStream_t st) {
    const uint32_t n32 = (uint32_t)n, g32 = (uint32_t)g;
    const dim3 per_item((unsigned)((n + kGroupLanes - 1) / kGroupLanes));
    const size_t lanes = n > g + 1 ? n : g + 1;
    hipMemsetAsync(s.table, 0xff, slots * 4, st);
    hipMemsetAsync(s.row_cnt, 0, n * 4, st);
    hipMemsetAsync(s.head, 0, (kGroupHeadWords + kGroupColumns * g) * 4, st);   // (col_cnt behind it: one piece)
    hipMemsetAsync(s.gbad, 0, g * 4, st);
    prof_launch("k_seg_mark", st, k_seg_mark, per_item, dim3(kGroupLanes), 0, idx, (const uint32_t *)s.item_off, s.item_group, s.gbad, n32, g32);
    prof_launch("k_seg_insert", st, k_seg_insert, per_item, dim3(kGroupLanes), 0, comms48, (const uint32_t *)s.item_off,
                (const uint32_t *)s.item_group, (const uint32_t *)s.gbad, s.table, s.slot_of, s.head, n32, (uint32_t)(slots - 1), seed,
                hash_mask);
    // (the two shared kernels keep this call's names in the profile)
    prof_launch("k_seg_scan", st, k_group_scan, dim3(1), dim3(kScanLanes), 0, comms48, (const uint32_t *)s.table, (const uint32_t *)s.slot_of,
                s.slot_row, s.first_item, s.distinct, s.pre, s.head, n32);
    prof_launch("k_seg_rows", st, k_seg_rows, dim3((unsigned)((lanes + kGroupLanes - 1) / kGroupLanes)), dim3(kGroupLanes), 0, idx,
                (const uint32_t *)s.item_off, (const uint32_t *)s.item_group, s.slot_of, (const uint32_t *)s.slot_row, (const uint32_t *)s.pre,
                s.rows, s.row_base, s.row_cnt, s.col_cnt, s.distinct, s.head, n32, g32);
    prof_launch("k_seg_offsets", st, k_group_offsets, dim3(2), dim3(kScanLanes), 0, (const uint32_t *)s.row_cnt, (const uint32_t *)s.col_cnt,
                s.row_off, s.col_off, (const uint32_t *)s.head, n32, (uint32_t)(kGroupColumns * g));
    prof_launch("k_seg_scatter", st, k_seg_scatter, per_item, dim3(kGroupLanes), 0, idx, (const uint32_t *)s.item_group, (const uint32_t *)s.slot_of,
                (const uint32_t *)s.row_off, (const uint32_t *)s.col_off, s.row_cnt, s.col_cnt, s.perm_row, s.perm_col, n32);
}

void launch_cell_group_slice_table(const uint32_t *item_off, const uint32_t *row_base, const uint32_t *gflag, GroupSlice *slices,
                                   uint32_t *slice_off, size_t g, size_t max_slices, hipStream_t st) {
    prof_launch("k_seg_slice_table", st, k_seg_slice_table, dim3(1), dim3(kScanLanes), 0, item_off, row_base, gflag, slices, slice_off,
                (uint32_t)(3 * g), (uint32_t)max_slices);
}

namespace {

size_t hook_carve(CellGroupBufs &g, uint8_t *base, size_t n, size_t slots) {
    Carver cv(base);
    cell_group_carve(g, cv, n, slots);
    cv.take(g.rows, n * 4);
    cv.take(g.perm_row, n * 4);
    cv.take(g.row_off, (n + 1) * 4);
    cv.take(g.perm_col, n * 4);
    cv.take(g.col_off, (kGroupColumns + 1) * 4);
    cv.take(g.distinct, n * 48);
    return cv.bytes();
}

// where a hook's answers go on the host (row_base .. slice_off: the segmented hook's alone)
struct HookOut {
    uint32_t *rows, *m_out, *first_item, *perm_row, *row_off, *perm_col, *col_off, *row_base, *bad_words, *slices, *slice_off;
    uint8_t *distinct48;
};

// what both hooks bring down, enqueued on st: the head words and the seven outputs a grouping of n items over `cols` column lists has,
// from where g has them; the first error
hipError_t hook_copies_down(uint32_t head[kGroupHeadWords], const HookOut &o, const CellGroupBufs &g, size_t n, size_t cols, hipStream_t st) {
    const struct { void *dst; const void *src; size_t bytes; } copies[8] = {
        {head, g.head, kGroupHeadWords * 4}, {o.rows, g.rows, n * 4},           {o.distinct48, g.distinct, n * 48}, {o.first_item, g.first_item, n * 4},
        {o.perm_row, g.perm_row, n * 4},     {o.row_off, g.row_off, (n + 1) * 4}, {o.perm_col, g.perm_col, n * 4},    {o.col_off, g.col_off, (cols + 1) * 4}};
    hipError_t e = hipSuccess;
    for (int k = 0; k < 8 && e == hipSuccess; k++) e = hipMemcpyAsync(copies[k].dst, copies[k].src, copies[k].bytes, hipMemcpyDeviceToHost, st);
    return e;
}

C_KZG_RET cell_group_hook(const HookOut &o, uint32_t *bad_index, const uint8_t *comms, const uint64_t *idx, size_t n, uint64_t seed,
                          uint32_t hash_mask, hipStream_t st) {
    if (n == 0 || n >= 0x7fffffffu || !o.rows || !o.m_out || !o.distinct48 || !o.first_item || !o.perm_row || !o.row_off || !o.perm_col ||
        !o.col_off || !bad_index || !comms || !idx)
        return C_KZG_BADARGS;
    const size_t slots = group_table_slots(n);
    CellGroupBufs g;
    const size_t bytes = hook_carve(g, nullptr, n, slots);
    uint8_t *dev = nullptr;
    if (hipMalloc((void **)&dev, bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("lwkzg_cell_group_device: no device memory for %zu bytes", bytes);
        return C_KZG_MALLOC;
    }
    DevBlock block{dev};
    hook_carve(g, dev, n, slots);
    LWK_HIP(hipMemsetAsync(g.perm_row, 0xff, n * 4, st));   // (a place no lane wrote shows as such)
    LWK_HIP(hipMemsetAsync(g.perm_col, 0xff, n * 4, st));
    launch_cell_group(comms, idx, n, slots, seed, hash_mask, g, st);
    LWK_HIP(hipGetLastError());
    uint32_t head[kGroupHeadWords];
    LWK_HIP(hook_copies_down(head, o, g, n, kGroupColumns, st));
    LWK_HIP(hipStreamSynchronize(st));
    *o.m_out = head[kGroupHeadM];
    *bad_index = ~head[kGroupHeadBad];
    if (head[kGroupHeadErr] || head[kGroupHeadM] == 0 || head[kGroupHeadM] > n) {
        set_error("lwkzg_cell_group_device: the grouping failed (error word %u, m = %u)", head[kGroupHeadErr], head[kGroupHeadM]);
        return C_KZG_ERROR;
    }
    return C_KZG_OK;
}

C_KZG_RET cell_group_seg_hook(const HookOut &o, const uint32_t *gflag, const uint8_t *comms, const uint64_t *idx, size_t n,
                              const uint64_t *offsets, size_t g, uint64_t seed, uint32_t hash_mask, hipStream_t st) {
    if (n == 0 || g == 0 || n >= 0x7fffffffu || g > 0x40000000u || !o.rows || !o.m_out || !o.distinct48 || !o.first_item || !o.perm_row ||
        !o.row_off || !o.perm_col || !o.col_off || !o.row_base || !o.bad_words || !comms || !idx || !group_offsets_valid(offsets, g, n) ||
        (o.slices != nullptr) != (o.slice_off != nullptr))
        return C_KZG_BADARGS;
    const size_t slots = group_table_slots(n), max_slices = plan_max_slices(n, g);
    CellGroupBufs gb;
    CellGroupSegBufs sb;
    uint32_t *d_gflag, *d_slice_off;
    GroupSlice *d_slices;
    auto carve = [&](uint8_t *base) {
        const size_t used = hook_carve(gb, base, n, slots);
        Carver cv(base ? base + used : nullptr);
        cell_group_seg_carve(sb, gb, cv, n, g);
        cv.take(d_gflag, g * 4);
        cv.take(d_slice_off, (3 * g + 1) * 4);
        cv.take(d_slices, max_slices * sizeof(GroupSlice));
        return used + cv.bytes();
    };
    const size_t bytes = carve(nullptr);
    uint8_t *dev = nullptr;
    if (hipMalloc((void **)&dev, bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("lwkzg_cell_group_segmented_device: no device memory for %zu bytes", bytes);
        return C_KZG_MALLOC;
    }
    DevBlock block{dev};
    carve(dev);
    std::vector<uint32_t> off32(g + 1);
    for (size_t j = 0; j <= g; j++) off32[j] = (uint32_t)offsets[j];
    LWK_HIP(hipMemcpyAsync(sb.item_off, off32.data(), (g + 1) * 4, hipMemcpyHostToDevice, st));
    LWK_HIP(hipMemsetAsync(sb.perm_row, 0xff, n * 4, st));   // (a place no lane wrote shows as such)
    LWK_HIP(hipMemsetAsync(sb.perm_col, 0xff, n * 4, st));
    launch_cell_group_seg(comms, idx, n, g, slots, seed, hash_mask, sb, st);
    if (o.slices) {
        if (gflag) LWK_HIP(hipMemcpyAsync(d_gflag, gflag, g * 4, hipMemcpyHostToDevice, st));
        launch_cell_group_slice_table(sb.item_off, sb.row_base, gflag ? d_gflag : sb.gbad, d_slices, d_slice_off, g, max_slices, st);
        LWK_HIP(hipMemcpyAsync(o.slices, d_slices, max_slices * sizeof(GroupSlice), hipMemcpyDeviceToHost, st));
        LWK_HIP(hipMemcpyAsync(o.slice_off, d_slice_off, (3 * g + 1) * 4, hipMemcpyDeviceToHost, st));
    }
    LWK_HIP(hipGetLastError());
    uint32_t head[kGroupHeadWords];
    CellGroupBufs down = gb;   // (sb's outputs are gb's, but for its own head and its 128 g column lists)
    down.head = sb.head, down.col_off = sb.col_off;
    LWK_HIP(hook_copies_down(head, o, down, n, kGroupColumns * g, st));
    LWK_HIP(hipMemcpyAsync(o.row_base, sb.row_base, (g + 1) * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(o.bad_words, sb.gbad, g * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipStreamSynchronize(st));
    *o.m_out = head[kGroupHeadM];
    if (head[kGroupHeadErr] || head[kGroupHeadM] > n) {
        set_error("lwkzg_cell_group_segmented_device: the grouping failed (error word %u, M = %u)", head[kGroupHeadErr], head[kGroupHeadM]);
        return C_KZG_ERROR;
    }
    return C_KZG_OK;
}

}  // namespace

}  // namespace lwk

using namespace lwk;

extern "C" C_KZG_RET lwkzg_cell_group_segmented_device(uint32_t *rows, uint32_t *m_out, uint8_t *distinct48, uint32_t *first_item,
                                                       uint32_t *perm_row, uint32_t *row_off, uint32_t *perm_col, uint32_t *col_off,
                                                       uint32_t *row_base, uint32_t *bad_words, uint32_t *slices_out, uint32_t *slice_off_out,
                                                       const uint32_t *gflag, const void *commitments48_dev, const void *cell_indices_dev,
                                                       size_t n, const uint64_t *group_offsets, size_t g, uint64_t seed, uint32_t hash_mask,
                                                       void *stream) {
    return guarded("lwkzg_cell_group_segmented_device", [&] {
        const HookOut o{rows, m_out, first_item, perm_row, row_off, perm_col, col_off, row_base, bad_words, slices_out, slice_off_out, distinct48};
        return cell_group_seg_hook(o, gflag, (const uint8_t *)commitments48_dev, (const uint64_t *)cell_indices_dev, n, group_offsets, g, seed,
                                   hash_mask, (hipStream_t)stream);
    });
}

extern "C" C_KZG_RET lwkzg_cell_group_device(uint32_t *rows, uint32_t *m_out, uint8_t *distinct48, uint32_t *first_item, uint32_t *perm_row,
                                             uint32_t *row_off, uint32_t *perm_col, uint32_t *col_off, uint32_t *bad_index,
                                             const void *commitments48_dev, const void *cell_indices_dev, size_t n, uint64_t seed,
                                             uint32_t hash_mask, void *stream) {
    return guarded("lwkzg_cell_group_device", [&] {
        const HookOut o{rows, m_out, first_item, perm_row, row_off, perm_col, col_off, nullptr, nullptr, nullptr, nullptr, distinct48};
        return cell_group_hook(o, bad_index, (const uint8_t *)commitments48_dev, (const uint64_t *)cell_indices_dev, n, seed, hash_mask,
                               (hipStream_t)stream);
    });
}
