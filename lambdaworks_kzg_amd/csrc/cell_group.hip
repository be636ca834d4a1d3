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
#include "abi_guard.h"
#include "carve.h"
#include "cell_group.cuh"
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
    uint32_t s = group_slot_hash(key, seed, hash_mask) & slot_mask;
    uint32_t found = kGroupEmpty;
#pragma unroll 1
    for (uint32_t probe = 0; probe <= slot_mask; probe++, s = (s + 1) & slot_mask) {
        const uint32_t c = atomicCAS(&table[s], kGroupEmpty, i);
        if (c == kGroupEmpty) {   // claimed
            found = s;
            break;
        }
        if (c >= n) break;        // (no lane writes such a word: the table is not this launch's)
        if (group_equal48(key, comms + 48 * (size_t)c)) {
            atomicMin(&table[s], i);
            found = s;
            break;
        }
    }
    if (found == kGroupEmpty) {
        atomicOr(&head[kGroupHeadErr], 1u);
        found = 0;
    }
    slot_of[i] = found;
}

__global__ __launch_bounds__(kScanLanes) void k_group_scan(const uint8_t *__restrict__ comms, const uint32_t *__restrict__ table,
                                                           const uint32_t *__restrict__ slot_of, uint32_t *__restrict__ slot_row,
                                                           uint32_t *__restrict__ first_item, uint8_t *__restrict__ distinct,
                                                           uint32_t *__restrict__ head, uint32_t n) {
    __shared__ uint32_t wave_tot[kScanWaves];
    uint32_t run = 0;
#pragma unroll 1
    for (uint32_t base = 0; base < n; base += kScanLanes) {   // (n is the same for every lane: they all meet the barriers)
        const uint32_t i = base + threadIdx.x;
        uint32_t s = 0, flag = 0;
        if (i < n) {
            s = slot_of[i];
            flag = table[s] == i ? 1u : 0u;
        }
        uint32_t total;
        const uint32_t before = block_exclusive_scan(flag, wave_tot, &total);
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
    if (threadIdx.x == 0) head[kGroupHeadM] = run;
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

// workgroup 0: row_off[0 .. m] from row_cnt; workgroup 1: col_off[0 .. 128] from col_cnt
__global__ __launch_bounds__(kScanLanes) void k_group_offsets(const uint32_t *__restrict__ row_cnt, const uint32_t *__restrict__ col_cnt,
                                                              uint32_t *__restrict__ row_off, uint32_t *__restrict__ col_off,
                                                              const uint32_t *__restrict__ head, uint32_t n) {
    __shared__ uint32_t wave_tot[kScanWaves];
    const bool cols = blockIdx.x != 0;
    const uint32_t *cnt = cols ? col_cnt : row_cnt;
    uint32_t *off = cols ? col_off : row_off;
    uint32_t len = cols ? kGroupColumns : head[kGroupHeadM];
    if (len > n && !cols) len = n;
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
    {
        ProfScope p("k_group_insert", st);
        hipLaunchKernelGGL(k_group_insert, per_item, dim3(kGroupLanes), 0, st, comms48, idx, g.table, g.slot_of, g.head, n32,
                           (uint32_t)(slots - 1), seed, hash_mask);
    }
    {
        ProfScope p("k_group_scan", st);
        hipLaunchKernelGGL(k_group_scan, dim3(1), dim3(kScanLanes), 0, st, comms48, (const uint32_t *)g.table, (const uint32_t *)g.slot_of,
                           g.slot_row, g.first_item, g.distinct, g.head, n32);
    }
    {
        ProfScope p("k_group_rows", st);
        hipLaunchKernelGGL(k_group_rows, per_item, dim3(kGroupLanes), 0, st, idx, (const uint32_t *)g.slot_of, (const uint32_t *)g.slot_row,
                           g.rows, g.row_cnt, g.col_cnt, g.distinct, g.head, n32);
    }
    {
        ProfScope p("k_group_offsets", st);
        hipLaunchKernelGGL(k_group_offsets, dim3(2), dim3(kScanLanes), 0, st, (const uint32_t *)g.row_cnt, (const uint32_t *)g.col_cnt,
                           g.row_off, g.col_off, (const uint32_t *)g.head, n32);
    }
    ProfScope p("k_group_scatter", st);
    hipLaunchKernelGGL(k_group_scatter, per_item, dim3(kGroupLanes), 0, st, idx, (const uint32_t *)g.rows, (const uint32_t *)g.row_off,
                       (const uint32_t *)g.col_off, g.row_cnt, g.col_cnt, g.perm_row, g.perm_col, n32);
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

C_KZG_RET cell_group_hook(uint32_t *rows, uint32_t *m_out, uint8_t *distinct48, uint32_t *first_item, uint32_t *perm_row, uint32_t *row_off,
                          uint32_t *perm_col, uint32_t *col_off, uint32_t *bad_index, const uint8_t *comms, const uint64_t *idx, size_t n,
                          uint64_t seed, uint32_t hash_mask, hipStream_t st) {
    if (n == 0 || n >= 0x7fffffffu || !rows || !m_out || !distinct48 || !first_item || !perm_row || !row_off || !perm_col || !col_off ||
        !bad_index || !comms || !idx)
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
    LWK_HIP(hipMemcpyAsync(head, g.head, sizeof head, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(rows, g.rows, n * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(distinct48, g.distinct, n * 48, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(first_item, g.first_item, n * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(perm_row, g.perm_row, n * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(row_off, g.row_off, (n + 1) * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(perm_col, g.perm_col, n * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(col_off, g.col_off, (kGroupColumns + 1) * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipStreamSynchronize(st));
    *m_out = head[kGroupHeadM];
    *bad_index = ~head[kGroupHeadBad];
    if (head[kGroupHeadErr] || head[kGroupHeadM] == 0 || head[kGroupHeadM] > n) {
        set_error("lwkzg_cell_group_device: the grouping failed (error word %u, m = %u)", head[kGroupHeadErr], head[kGroupHeadM]);
        return C_KZG_ERROR;
    }
    return C_KZG_OK;
}

}  // namespace

}  // namespace lwk

using namespace lwk;

extern "C" C_KZG_RET lwkzg_cell_group_device(uint32_t *rows, uint32_t *m_out, uint8_t *distinct48, uint32_t *first_item, uint32_t *perm_row,
                                             uint32_t *row_off, uint32_t *perm_col, uint32_t *col_off, uint32_t *bad_index,
                                             const void *commitments48_dev, const void *cell_indices_dev, size_t n, uint64_t seed,
                                             uint32_t hash_mask, void *stream) {
    return guarded("lwkzg_cell_group_device", [&] {
        return cell_group_hook(rows, m_out, distinct48, first_item, perm_row, row_off, perm_col, col_off, bad_index,
                               (const uint8_t *)commitments48_dev, (const uint64_t *)cell_indices_dev, n, seed, hash_mask, (hipStream_t)stream);
    });
}
