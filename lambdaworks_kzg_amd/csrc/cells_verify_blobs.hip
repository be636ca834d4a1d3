// cells_verify_blobs.hip -- do the 128 cell proofs of whole blobs belong to the blobs and their commitments? lwkzg_verify_blob_cell_kzg_proofs_batch
// (+ _device), lwkzg_blob_cell_verify_partials, lwkzg_verify_blob_cell_kzg_proofs_groups (+ _device), lwkzg_blob_cell_verify_groups_partials.
// DESIGN.md section 4s.
//
// The answers are DEFINED by the calls over items: with cells_b the 128 cells the compute call gives for blob b, the expanded items of a
// call are (commitments[b], k, cells_b[k], cell_proofs[128 b + k]) in the order i = 128 b + k, and the batch call / the grouped call over
// them is what answers. Nobody builds those items: this file is the front (cells_verify_blobs.h) of the two pipelines.
//   host     arguments and offsets checked; the n commitments (the device forms bring them down: 48 n bytes) de-duplicated per group
//            in order of first occurrence -- per blob its row, the blobs in order of their rows, per row its first item
//   device   under the pipeline's lock: the blobs to coefficients (the front of the compute call: launch_parse_be_reduce, or
//            launch_blob_evaluations_to_coefficients with a status word per blob), launch_cells_extend in chunks of kCellsChunk blobs into
//            the settings' scratch (the host forms upload slices of kHostSlice blobs in front of it); k_blob_items writes every
//            128 n-entry list of the call from the n-entry tables -- the grouping is closed form: item 128 b + k has blob b's row and
//            column k, and column k's list is the items 128 b + k (cell_blobs_plan.h: the tables and the kernel's bodies, which
//            tests/cell_blobs_plan_check.cpp holds against cell_groups_plan.h on the expanded items without a GPU)
//   device   the pipeline as it is (cells_verify_api.hip, cells_verify_groups.hip); behind its validation k_blob_fold_status gives the
//            items of a rejected blob the mode's bad-input code, so that the call (batch) or exactly the blob's group (groups) answers it
// The scratch (Ctx::blobv, grow-only, freed with the settings): 256 KiB of cells + 16 bytes of tables per blob, and the host forms'
// upload slice (128 KiB per blob, at most kHostSlice of them). No proofs are computed, so the cell proof engine does not matter.
// The forms that do not block are the cell verifier's blob calls (cells_verify_async.hip): they share the two
// device steps at the end of the front below (launch_blob_cells, launch_blob_fold_status) and group on the device instead of here.
#include "abi_guard.h"
#include "cell_blobs_plan.h"
#include "cells_verify_blobs.h"
#include "knobs.h"

#include <string.h>

#include <vector>

namespace lwk {

namespace {

constexpr size_t kMaxBlobs = (size_t)0x7fffffff / kCellsPerBlob;   // the pipelines count items in 31 bits

// ---- the lists of the expanded items -------------------------------------------------------------------------------------------------------
// Every 128 n-entry list of the call from the n-entry tables (cell_blobs_plan.h has the closed forms): rows, idx, perm_row, perm_col and
// the item -> group words per item, col_off per (group, column), and the infinity encodings behind the m distinct commitments, up to n
// entries of the commitment set. Grid-stride, a plain store per word. bgroup / item_off: nullptr for a batch (one group, g == 1).
__global__ __launch_bounds__(256) void k_blob_items(const uint32_t *__restrict__ brow, const uint32_t *__restrict__ bperm,
                                                    const uint32_t *__restrict__ bgroup, const uint32_t *__restrict__ item_off, uint32_t nb,
                                                    uint32_t m, uint32_t g, uint32_t *__restrict__ comm_words, uint32_t *__restrict__ col_off,
                                                    BlobItemLists lists) {
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    const size_t n = (size_t)nb * kCellsPerBlob;
    for (size_t i = t; i < n; i += stride) blob_item_lists(lists, i, brow, bperm, bgroup, item_off, nb);
    for (size_t q = t; q <= (size_t)g * kCellsPerBlob; q += stride) col_off[q] = blob_col_off(q, item_off, nb, g);
    for (size_t q = 12 * (size_t)m + t; q < 12 * n; q += stride) comm_words[q] = blob_pad_word(q);
}

// the items of a blob whose status word is set take bad_code (a plain store per item; the other items' words stay)
__global__ __launch_bounds__(256) void k_blob_fold_status(int32_t *__restrict__ words, const int32_t *__restrict__ bstatus, uint32_t nb,
                                                          int bad_code) {
    const size_t stride = (size_t)gridDim.x * blockDim.x, n = (size_t)nb * kCellsPerBlob;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        if (bstatus[i >> 7] != 0) words[i] = bad_code;
}

unsigned grid_for(size_t work) {
    const size_t blocks = (work + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : blocks > 4096 ? 4096 : blocks);
}

// where the coefficient step of cells_chunks reads the blobs (device memory at src): the front of the compute call
CoefficientStep coefficient_step(Ctx *c, const uint8_t *src, int mode, hipStream_t st) {
    const ModeRules rules = mode_rules(mode);
    return [=](size_t off, size_t m, int32_t *stt) {
        const uint8_t *in = src + off * (size_t)kBlobBytes;
        if (!rules.evaluation_form) launch_parse_be_reduce(in, c->ws.scalars, m * kBlobElems, st);
        else launch_blob_evaluations_to_coefficients(in, c->ws.scalars, c->tw28_inv, stt, m, st, rules.le());
    };
}

// ---- the settings' scratch -----------------------------------------------------------------------------------------------------------------
struct BlobvBufs {
    uint8_t *cells, *stage;
    int32_t *status;
    uint32_t *brow, *bperm, *bgroup;
};

size_t carve(BlobvBufs &b, uint8_t *base, size_t cap) {
    Carver cv(base);
    cv.take(b.cells, cap * kBlobCellBytes);
    cv.take(b.stage, min_sz(cap, kHostSlice) * (size_t)kBlobBytes);
    cv.take(b.status, cap * 4);
    cv.take(b.brow, cap * 4);
    cv.take(b.bperm, cap * 4);
    cv.take(b.bgroup, cap * 4);
    return cv.bytes();
}

// grow-only, kept with the settings object: first 8 blobs, then doubling; no allocation in steady state (caller holds c->mu)
C_KZG_RET reserve(Ctx *c, size_t nb, BlobvBufs &b) {
    if (c->blobv.cap < nb) {
        size_t bytes = 0;
        C_KZG_RET rc = grow_reserve(c->blobv, nb, 8, [&](size_t cap) { BlobvBufs probe; return bytes = carve(probe, nullptr, cap); }, nullptr);
        if (rc == C_KZG_MALLOC) set_error("verify_blob_cell_kzg_proofs: no memory for the cells of %zu blobs (%zu bytes on the device)", nb, bytes);
        if (rc != C_KZG_OK) return rc;
    }
    carve(b, c->blobv.dev, c->blobv.cap);
    return C_KZG_OK;
}

template <class T>
hipError_t upload(T *dst, const std::vector<T> &src, hipStream_t st) {
    return src.empty() ? hipSuccess : hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, st);
}

// ---- the front -----------------------------------------------------------------------------------------------------------------------------
struct BlobFront : CellFront {
    const uint8_t *blobs = nullptr, *proofs = nullptr;   // host or device memory (device_inputs)
    size_t nb = 0;
    int mode = 0;
    bool device_inputs = false, grouped = false;
    BlobTables t;   // cell_blobs_plan.h
    mutable const int32_t *d_status = nullptr;

    // the host side: comms are the nb commitments in host memory, boff the g + 1 offsets in blobs (valid)
    void plan_blobs(const uint8_t *comms, const uint64_t *boff, size_t g_count) { lwk::plan_blobs(t, g, plan, comms, nb, boff, g_count, grouped); }

    C_KZG_RET items(Ctx *c, hipStream_t st, const CellvBufs &b, const CellFrontGroupLists *gl, const uint8_t *&cells_out,
                    const uint8_t *&proofs_out) const override {
        BlobvBufs bb;
        C_KZG_RET rc = reserve(c, nb, bb);
        if (rc != C_KZG_OK) return rc;
        d_status = bb.status;
        if (device_inputs) {
            if ((rc = launch_blob_cells(c, bb.cells, bb.status, blobs, nb, mode, st)) != C_KZG_OK) return rc;
            proofs_out = proofs;
        } else {
            const CoefficientStep coefficients = coefficient_step(c, bb.stage, mode, st);
            for (size_t off = 0; off < nb; off += kHostSlice) {   // (the stream orders a slice's upload behind its predecessor's parse)
                const size_t m = min_sz(kHostSlice, nb - off);
                LWK_HIP(hipMemcpyAsync(bb.stage, blobs + off * (size_t)kBlobBytes, m * (size_t)kBlobBytes, hipMemcpyHostToDevice, st));
                if ((rc = cells_chunks(c, bb.cells + off * kBlobCellBytes, nullptr, m, mode, st, bb.status + off, coefficients, nb)) != C_KZG_OK)
                    return rc;
            }
            LWK_HIP(hipMemcpyAsync(b.proofs, proofs, 48 * kProofsPerBlob * nb, hipMemcpyHostToDevice, st));
            proofs_out = b.proofs;
        }
        cells_out = bb.cells;
        // the n-entry tables go up; every 128 n-entry list is written where it is read
        const std::vector<uint8_t> &distinct = grouped ? plan.distinct : g.distinct;
        const size_t m = grouped ? plan.m_total : g.m;
        LWK_HIP(upload(b.comm_in, distinct, st));
        LWK_HIP(upload(bb.brow, t.brow, st));
        LWK_HIP(upload(bb.bperm, t.bperm, st));
        LWK_HIP(upload(b.row_off, t.row_off, st));
        if (grouped) {
            LWK_HIP(upload(bb.bgroup, t.bgroup, st));
            LWK_HIP(upload(gl->item_off, plan.item_off, st));
            LWK_HIP(upload(gl->slice_off, plan.slice_off, st));
            LWK_HIP(upload(gl->slices, plan.slices, st));
        }
        prof_launch("k_blob_items", st, k_blob_items, dim3(grid_for(nb * kCellsPerBlob)), dim3(256), 0, (const uint32_t *)bb.brow,
                    (const uint32_t *)bb.bperm, grouped ? (const uint32_t *)bb.bgroup : nullptr,
                    grouped ? (const uint32_t *)gl->item_off : nullptr, (uint32_t)nb, (uint32_t)m, (uint32_t)t.groups, (uint32_t *)b.comm_in,
                    b.col_off, BlobItemLists{b.idx, b.rows, b.perm_row, b.perm_col, grouped ? gl->item_group : nullptr});
        LWK_HIP(hipGetLastError());
        return C_KZG_OK;
    }

    void fold_status(int32_t *words, int bad_code, hipStream_t st) const override {
        (void)launch_blob_fold_status(words, d_status, nb, mode, bad_code, st);   // (a failed launch: the pipeline's hipGetLastError)
    }
};

}  // namespace

// cells_verify_blobs.h: the two device steps, shared with the cell verifier's blob calls
C_KZG_RET launch_blob_cells(Ctx *c, uint8_t *cells, int32_t *bstatus, const uint8_t *blobs_dev, size_t nb, int mode, hipStream_t st) {
    return cells_chunks(c, cells, nullptr, nb, mode, st, bstatus, coefficient_step(c, blobs_dev, mode, st), nb);
}

hipError_t launch_blob_fold_status(int32_t *words, const int32_t *bstatus, size_t nb, int mode, int bad_code, hipStream_t st) {
    if (!mode_rules(mode).evaluation_form) return hipSuccess;   // reference mode reduces: no blob is rejected
    prof_launch("k_blob_fold_status", st, k_blob_fold_status, dim3(grid_for(nb * kCellsPerBlob)), dim3(256), 0, words, bstatus, (uint32_t)nb, bad_code);
    return hipPeekAtLastError();   // (left standing for the pipeline's own hipGetLastError)
}

namespace {

// the n commitments on the host: the caller's array, or (device form) brought down on the call's stream
C_KZG_RET host_commitments(const uint8_t *&comms, std::vector<uint8_t> &down, const void *given, size_t nb, const KZGSettings *s,
                           bool device_inputs, hipStream_t caller) {
    comms = (const uint8_t *)given;
    if (!device_inputs) return C_KZG_OK;
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = caller ? caller : c->stream;
    down.resize(48 * nb);
    LWK_HIP(hipMemcpyAsync(down.data(), given, 48 * nb, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipStreamSynchronize(st));
    comms = down.data();
    return C_KZG_OK;
}

// the verdict (ok) and / or the partials of the batch call over the expanded items
C_KZG_RET blob_batch_impl(bool *ok, uint8_t *partials, const void *blobs, const void *commitments, const void *cell_proofs, size_t nb,
                          const KZGSettings *s, bool device_inputs, hipStream_t caller) {
    if (!s) return C_KZG_BADARGS;
    if (nb == 0) {
        if (ok) *ok = true;   // the batch call's answer to no items
        return C_KZG_OK;
    }
    if (!blobs || !commitments || !cell_proofs) {
        set_error("verify_blob_cell_kzg_proofs_batch: NULL argument");
        return C_KZG_BADARGS;
    }
    if (nb > kMaxBlobs) {
        set_error("verify_blob_cell_kzg_proofs_batch: more than %zu blobs", kMaxBlobs);
        return C_KZG_BADARGS;
    }
    BlobFront f;
    f.blobs = (const uint8_t *)blobs, f.proofs = (const uint8_t *)cell_proofs, f.nb = nb, f.mode = mode_of(s), f.device_inputs = device_inputs;
    const uint8_t *comms;
    std::vector<uint8_t> down;
    C_KZG_RET rc = host_commitments(comms, down, commitments, nb, s, device_inputs, caller);
    if (rc != C_KZG_OK) return rc;
    const uint64_t boff[2] = {0, (uint64_t)nb};
    f.plan_blobs(comms, boff, 1);
    return cell_batch_front(ok, partials, nb * kCellsPerBlob, s, caller, f);
}

// the answers (ok_out, rc_out) or the partials of the grouped call over the expanded items; the offsets count BLOBS
C_KZG_RET blob_groups_impl(uint8_t *ok_out, int32_t *rc_out, uint8_t *partials_out, const void *blobs, const void *commitments,
                           const void *cell_proofs, size_t nb, const uint64_t *offsets, size_t g, const KZGSettings *s, bool device_inputs,
                           hipStream_t caller) {
    // the call-level checks: before any device work, and nothing is written
    if (!s) return C_KZG_BADARGS;
    const bool no_output = partials_out ? false : !ok_out || !rc_out;
    if ((g > 0 && (no_output || !offsets)) || (nb > 0 && (!blobs || !commitments || !cell_proofs))) {
        set_error("verify_blob_cell_kzg_proofs_groups: NULL argument");
        return C_KZG_BADARGS;
    }
    if (nb > kMaxBlobs || g > (size_t)0x3fffffff || !group_offsets_valid(offsets, g, nb)) {
        set_error("verify_blob_cell_kzg_proofs_groups: group_offsets must be %zu ascending values from 0 to %zu (blobs)", g + 1, nb);
        return C_KZG_BADARGS;
    }
    if (g == 0) return C_KZG_OK;
    std::vector<uint64_t> item_off(g + 1);
    for (size_t j = 0; j <= g; j++) item_off[j] = offsets[j] * kCellsPerBlob;
    BlobFront f;
    f.blobs = (const uint8_t *)blobs, f.proofs = (const uint8_t *)cell_proofs, f.nb = nb, f.mode = mode_of(s), f.device_inputs = device_inputs;
    f.grouped = true;
    if (nb > 0) {   // (empty groups alone: the grouped call answers them without a front)
        const uint8_t *comms;
        std::vector<uint8_t> down;
        C_KZG_RET rc = host_commitments(comms, down, commitments, nb, s, device_inputs, caller);
        if (rc != C_KZG_OK) return rc;
        f.plan_blobs(comms, offsets, g);
    }
    return cell_groups_front(ok_out, rc_out, partials_out, nb * kCellsPerBlob, item_off.data(), g, s, caller, f);
}

}  // namespace

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_verify_blob_cell_kzg_proofs_batch(bool *ok, const Blob *blobs, const Bytes48 *commitments, const Bytes48 *cell_proofs, size_t n,
                                                  const KZGSettings *s) {
    if (!ok) return C_KZG_BADARGS;
    *ok = false;
    return guarded("lwkzg_verify_blob_cell_kzg_proofs_batch",
                   [&] { return blob_batch_impl(ok, nullptr, blobs, commitments, cell_proofs, n, s, false, nullptr); });
}

C_KZG_RET lwkzg_verify_blob_cell_kzg_proofs_batch_device(bool *ok, const void *blobs_dev, const void *commitments48_dev,
                                                         const void *cell_proofs48_dev, size_t n, const KZGSettings *s, void *stream) {
    if (!ok) return C_KZG_BADARGS;
    *ok = false;
    return guarded("lwkzg_verify_blob_cell_kzg_proofs_batch_device", [&] {
        return blob_batch_impl(ok, nullptr, blobs_dev, commitments48_dev, cell_proofs48_dev, n, s, true, (hipStream_t)stream);
    });
}

C_KZG_RET lwkzg_blob_cell_verify_partials(uint8_t *out, const Blob *blobs, const Bytes48 *commitments, const Bytes48 *cell_proofs, size_t n,
                                          const KZGSettings *s) {
    if (!out && n) return C_KZG_BADARGS;
    return guarded("lwkzg_blob_cell_verify_partials",
                   [&] { return blob_batch_impl(nullptr, out, blobs, commitments, cell_proofs, n, s, false, nullptr); });
}

C_KZG_RET lwkzg_verify_blob_cell_kzg_proofs_groups(uint8_t *ok_out, int32_t *rc_out, const Blob *blobs, const Bytes48 *commitments,
                                                   const Bytes48 *cell_proofs, size_t n, const uint64_t *group_offsets, size_t g,
                                                   const KZGSettings *s) {
    return guarded("lwkzg_verify_blob_cell_kzg_proofs_groups", [&] {
        return blob_groups_impl(ok_out, rc_out, nullptr, blobs, commitments, cell_proofs, n, group_offsets, g, s, false, nullptr);
    });
}

C_KZG_RET lwkzg_verify_blob_cell_kzg_proofs_groups_device(uint8_t *ok_out, int32_t *rc_out, const void *blobs_dev, const void *commitments48_dev,
                                                          const void *cell_proofs48_dev, size_t n, const uint64_t *group_offsets, size_t g,
                                                          const KZGSettings *s, void *stream) {
    return guarded("lwkzg_verify_blob_cell_kzg_proofs_groups_device", [&] {
        return blob_groups_impl(ok_out, rc_out, nullptr, blobs_dev, commitments48_dev, cell_proofs48_dev, n, group_offsets, g, s, true,
                                (hipStream_t)stream);
    });
}

C_KZG_RET lwkzg_blob_cell_verify_groups_partials(uint8_t *out, const Blob *blobs, const Bytes48 *commitments, const Bytes48 *cell_proofs, size_t n,
                                                 const uint64_t *group_offsets, size_t g, const KZGSettings *s) {
    if (!out && g) return C_KZG_BADARGS;
    return guarded("lwkzg_blob_cell_verify_groups_partials", [&] {
        return blob_groups_impl(nullptr, nullptr, out, blobs, commitments, cell_proofs, n, group_offsets, g, s, false, nullptr);
    });
}

}  // extern "C"
