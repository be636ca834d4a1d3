// cell_blobs_group.hip -- the commitments of whole blobs grouped on the device, and the lists of their 128 n expanded items written
// from tables that never left it: what plan_blobs and k_blob_items (cells_verify_blobs.hip) do for the
// synchronous calls with the commitments on the host, for the cell verifier's blob calls (cells_verify_async.hip), which bring
// nothing down to learn m. lwkzg_blob_group_device is the test hook.
//
//   k_blob_group       ONE workgroup of kBlobGroupCap lanes, a lane per blob, everything in LDS (cell_blobs_group.h has the steps):
//                      the table of (group, 48 bytes) -> first blob under the seeded SipHash, the scan of the first-occurrence flags
//                      (the concatenated rows, the groups' first rows, M), the rows' counts, their scan and the counting sort of the
//                      blobs by (group, row). One launch where the item-level grouping of cell_group.hip takes five to seven: the
//                      table has 1024 slots, not 2 x 128 n, and nothing of it is in HBM.
//   k_blob_items_dev   k_blob_items with m, the tables and the offsets read from device memory: every 128 n-entry list of the call by
//                      the closed forms of cell_blobs_plan.h, the rows' offsets and first items in ITEMS, the column offsets, and the
//                      infinity encodings behind the M distinct commitments.
// No index of an expanded item is >= 128, so the bad-index words are zero by construction.
#include "abi_guard.h"
#include "carve.h"
#include "cell_blobs_group.h"
#include "cell_groups_plan.h"
#include "kernels.h"

#include <vector>

namespace lwk {

namespace {

constexpr int kBlobGroupWaves = kBlobGroupCap / 64;

struct LdsAtomics {   // (ds_* atomics: the words are the workgroup's)
    static __device__ __forceinline__ uint32_t cas(uint32_t *p, uint32_t expect, uint32_t v) { return atomicCAS(p, expect, v); }
    static __device__ __forceinline__ void min(uint32_t *p, uint32_t v) { atomicMin(p, v); }
    static __device__ __forceinline__ uint32_t add(uint32_t *p, uint32_t v) { return atomicAdd(p, v); }
    static __device__ __forceinline__ void bit_or(uint32_t *p, uint32_t v) { atomicOr(p, v); }
};

// exclusive scan of v over the workgroup's kBlobGroupCap lanes (all of them call it); *total: the sum. wave_tot: kBlobGroupWaves words
__device__ __forceinline__ uint32_t blob_block_scan(uint32_t v, uint32_t *wave_tot, uint32_t *total) {
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
    for (int w = 0; w < kBlobGroupWaves; w++) {
        const uint32_t t = wave_tot[w];
        before += (uint32_t)w < wave ? t : 0u;
        all += t;
    }
    __syncthreads();   // wave_tot is free for the next scan
    *total = all;
    return before + inc - v;
}

}  // namespace

// nb <= kBlobGroupCap (the launcher's check); item_off: g + 1 offsets in items, or nullptr for one group of all blobs
__global__ __launch_bounds__(kBlobGroupCap) void k_blob_group(const uint8_t *__restrict__ comms, const uint32_t *__restrict__ item_off,
                                                              uint32_t nb, uint32_t g, uint64_t seed, uint32_t hash_mask, BlobGroupOut o) {
    __shared__ BlobGroupShared sh;
    __shared__ uint32_t wave_tot[kBlobGroupWaves];
    const uint32_t b = threadIdx.x;
    if (nb > kBlobGroupCap) nb = kBlobGroupCap;   // (never: every subscript below stays inside the workgroup's words)
    blob_group_clear(sh, b, kBlobGroupCap, nb, o);
    __syncthreads();
    blob_group_insert<LdsAtomics>(sh, b, nb, comms, item_off, g, seed, hash_mask);
    __syncthreads();
    uint32_t total;
    const uint32_t flag = blob_group_flag(sh, b, nb);
    const uint32_t before = blob_block_scan(flag, wave_tot, &total);
    sh.pre[b] = before;
    if (b == 0) sh.pre[kBlobGroupCap] = total;
    __syncthreads();
    if (b == 0) sh.pre[nb] = total;   // (no flag at or behind nb: pre[nb] was the total already unless nb == kBlobGroupCap)
    __syncthreads();
    blob_group_first(sh, b, kBlobGroupCap, nb, comms, item_off, g, o);
    __syncthreads();
    blob_group_rows<LdsAtomics>(sh, b, nb, item_off, g, o);
    __syncthreads();
    const uint32_t rows = total < nb ? total : nb;
    const uint32_t mine = b < rows ? sh.cnt[b] : 0u;
    uint32_t placed;
    const uint32_t in_front = blob_block_scan(mine, wave_tot, &placed);   // (its barriers stand between the reads and the writes of cnt)
    if (b < rows) {
        sh.cnt[b] = in_front;
        o.brow_off[b] = in_front;
    }
    if (b == 0) {
        sh.cnt[rows] = placed;
        o.brow_off[rows] = placed;
    }
    __syncthreads();
    blob_group_scatter<LdsAtomics>(sh, b, nb, o);
}

// Grid-stride, a plain store per word. bgroup / item_off: nullptr for a batch (one group, g == 1). head: where k_blob_group left M
__global__ __launch_bounds__(256) void k_blob_items_dev(const uint32_t *__restrict__ brow, const uint32_t *__restrict__ bperm,
                                                        const uint32_t *__restrict__ bgroup, const uint32_t *__restrict__ item_off,
                                                        const uint32_t *__restrict__ brow_off, const uint32_t *__restrict__ bfirst,
                                                        const uint32_t *__restrict__ head, uint32_t nb, uint32_t g,
                                                        uint32_t *__restrict__ comm_words, uint32_t *__restrict__ col_off,
                                                        uint32_t *__restrict__ row_off, uint32_t *__restrict__ first_item, BlobItemLists lists) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const size_t n = (size_t)nb * kGroupColumns;
    uint32_t m = head[kBlobHeadM];
    if (m > nb) m = nb;   // (never: the words below stay inside the lists)
    for (size_t i = t; i < n; i += stride) blob_item_lists(lists, i, brow, bperm, bgroup, item_off, nb);
    for (size_t q = t; q <= (size_t)g * kGroupColumns; q += stride) col_off[q] = blob_col_off(q, item_off, nb, g);
    for (size_t r = t; r <= m; r += stride) row_off[r] = blob_row_off_items(brow_off, (uint32_t)r);
    for (size_t r = t; r < m; r += stride) first_item[r] = blob_first_item(bfirst, (uint32_t)r);
    for (size_t q = 12 * (size_t)m + t; q < 12 * n; q += stride) comm_words[q] = blob_pad_word(q);
}

hipError_t launch_cell_blobs_group(const uint8_t *comms48, const uint32_t *item_off, size_t nb, size_t g, uint64_t seed, uint32_t hash_mask,
                                   const BlobGroupOut &o, hipStream_t st) {
    if (nb == 0 || nb > kBlobGroupCap || g == 0) return hipErrorInvalidValue;
    prof_launch("k_blob_group", st, k_blob_group, dim3(1), dim3(kBlobGroupCap), 0, comms48, item_off, (uint32_t)nb, (uint32_t)g, seed, hash_mask, o);
    return hipGetLastError();
}

hipError_t launch_cell_blobs_items(const BlobGroupOut &o, const uint32_t *item_off, size_t nb, size_t g, const BlobItemsOut &x, hipStream_t st) {
    if (nb == 0 || nb > kBlobGroupCap || g == 0) return hipErrorInvalidValue;
    const size_t blocks = (nb * kGroupColumns + 255) / 256;
    prof_launch("k_blob_items_dev", st, k_blob_items_dev, dim3((unsigned)blocks), dim3(256), 0, (const uint32_t *)o.brow, (const uint32_t *)o.bperm,
                item_off ? (const uint32_t *)o.bgroup : nullptr, item_off, (const uint32_t *)o.brow_off, (const uint32_t *)o.bfirst,
                (const uint32_t *)o.head, (uint32_t)nb, (uint32_t)g, (uint32_t *)o.distinct, x.col_off, x.row_off, x.first_item,
                BlobItemLists{x.idx, x.rows, x.perm_row, x.perm_col, item_off ? x.item_group : nullptr});
    return hipGetLastError();
}

namespace {

// where the hook's answers go on the host
struct BlobHookOut {
    uint32_t *rows, *m_out, *first_item, *perm_row, *row_off, *perm_col, *col_off, *row_base, *bad_words, *slices, *slice_off, *item_group;
    uint64_t *idx;
    uint8_t *distinct48;
};

C_KZG_RET blob_group_hook(const BlobHookOut &h, const uint8_t *comms, size_t nb, const uint64_t *offsets, size_t g, uint64_t seed,
                          uint32_t hash_mask, hipStream_t st) {
    if (nb == 0 || nb > kBlobGroupCap || g == 0 || g > 0x40000000u || !h.rows || !h.m_out || !h.distinct48 || !h.first_item || !h.perm_row ||
        !h.row_off || !h.perm_col || !h.col_off || !h.row_base || !h.bad_words || !comms || !group_offsets_valid(offsets, g, nb) ||
        (h.slices != nullptr) != (h.slice_off != nullptr))
        return C_KZG_BADARGS;
    const size_t n = nb * kGroupColumns, max_slices = plan_max_slices(n, g);
    BlobGroupOut o;
    BlobItemsOut x;
    uint32_t *d_item_off, *d_gbad, *d_slice_off;
    GroupSlice *d_slices;
    auto carve = [&](uint8_t *base) {
        Carver cv(base);
        cv.take(o.brow, nb * 4);
        cv.take(o.bgroup, nb * 4);
        cv.take(o.bperm, nb * 4);
        cv.take(o.brow_off, (nb + 1) * 4);
        cv.take(o.bfirst, nb * 4);
        cv.take(o.row_base, (g + 1) * 4);
        cv.take(o.distinct, n * 48);
        cv.take(o.head, kBlobHeadWords * 4);
        cv.take(x.idx, n * 8);
        cv.take(x.rows, n * 4);
        cv.take(x.perm_row, n * 4);
        cv.take(x.perm_col, n * 4);
        cv.take(x.item_group, n * 4);
        cv.take(x.col_off, (kGroupColumns * g + 1) * 4);
        cv.take(x.row_off, (n + 1) * 4);
        cv.take(x.first_item, n * 4);
        cv.take(d_item_off, (g + 1) * 4);
        cv.take(d_gbad, g * 4);
        cv.take(d_slice_off, (3 * g + 1) * 4);
        cv.take(d_slices, max_slices * sizeof(GroupSlice));
        return cv.bytes();
    };
    const size_t bytes = carve(nullptr);
    uint8_t *dev = nullptr;
    if (hipMalloc((void **)&dev, bytes) != hipSuccess) {
        (void)hipGetLastError();
        set_error("lwkzg_blob_group_device: no device memory for %zu bytes", bytes);
        return C_KZG_MALLOC;
    }
    DevBlock block{dev};
    carve(dev);
    std::vector<uint32_t> off32(g + 1);
    for (size_t j = 0; j <= g; j++) off32[j] = (uint32_t)(offsets[j] * kGroupColumns);
    LWK_HIP(hipMemcpyAsync(d_item_off, off32.data(), (g + 1) * 4, hipMemcpyHostToDevice, st));
    LWK_HIP(hipMemsetAsync(d_gbad, 0, g * 4, st));
    LWK_HIP(hipMemsetAsync(x.perm_row, 0xff, n * 4, st));   // (a place no lane wrote shows as such)
    LWK_HIP(hipMemsetAsync(x.perm_col, 0xff, n * 4, st));
    LWK_HIP(launch_cell_blobs_group(comms, d_item_off, nb, g, seed, hash_mask, o, st));
    LWK_HIP(launch_cell_blobs_items(o, d_item_off, nb, g, x, st));
    if (h.slices) {
        launch_cell_group_slice_table(d_item_off, o.row_base, d_gbad, d_slices, d_slice_off, g, max_slices, st);
        LWK_HIP(hipMemcpyAsync(h.slices, d_slices, max_slices * sizeof(GroupSlice), hipMemcpyDeviceToHost, st));
        LWK_HIP(hipMemcpyAsync(h.slice_off, d_slice_off, (3 * g + 1) * 4, hipMemcpyDeviceToHost, st));
    }
    LWK_HIP(hipGetLastError());
    uint32_t head[kBlobHeadWords];
    const struct { void *dst; const void *src; size_t bytes; } copies[] = {
        {head, o.head, sizeof head},           {h.rows, x.rows, n * 4},         {h.distinct48, o.distinct, n * 48},
        {h.first_item, x.first_item, n * 4},   {h.perm_row, x.perm_row, n * 4}, {h.row_off, x.row_off, (n + 1) * 4},
        {h.perm_col, x.perm_col, n * 4},       {h.col_off, x.col_off, (kGroupColumns * g + 1) * 4},
        {h.row_base, o.row_base, (g + 1) * 4}, {h.bad_words, d_gbad, g * 4},    {h.item_group, x.item_group, n * 4},
        {h.idx, x.idx, n * 8}};
    for (const auto &c : copies)
        if (c.dst) LWK_HIP(hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipStreamSynchronize(st));
    *h.m_out = head[kBlobHeadM];
    if (head[kBlobHeadErr] || head[kBlobHeadBad] || head[kBlobHeadM] == 0 || head[kBlobHeadM] > nb) {
        set_error("lwkzg_blob_group_device: the grouping failed (error word %u, M = %u)", head[kBlobHeadErr], head[kBlobHeadM]);
        return C_KZG_ERROR;
    }
    return C_KZG_OK;
}

}  // namespace

}  // namespace lwk

using namespace lwk;

extern "C" C_KZG_RET lwkzg_blob_group_device(uint32_t *rows, uint32_t *m_out, uint8_t *distinct48, uint32_t *first_item, uint32_t *perm_row,
                                             uint32_t *row_off, uint32_t *perm_col, uint32_t *col_off, uint32_t *row_base, uint32_t *bad_words,
                                             uint32_t *slices_out, uint32_t *slice_off_out, uint32_t *item_group_out, uint64_t *cell_indices_out,
                                             const void *commitments48_dev, size_t n_blobs, const uint64_t *group_offsets, size_t g, uint64_t seed,
                                             uint32_t hash_mask, void *stream) {
    return guarded("lwkzg_blob_group_device", [&] {
        const BlobHookOut h{rows,      m_out,         first_item,     perm_row,         row_off,   perm_col, col_off, row_base,
                            bad_words, slices_out,    slice_off_out,  item_group_out,   cell_indices_out, distinct48};
        return blob_group_hook(h, (const uint8_t *)commitments48_dev, n_blobs, group_offsets, g, seed, hash_mask, (hipStream_t)stream);
    });
}
