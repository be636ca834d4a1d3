// cells_api.hip -- EIP-7594 compute_cells_and_kzg_proofs: lwkzg_compute_cells_and_kzg_proofs (+ _batch, _batch_device).
//
// A chunk of blobs at a time, all on one stream:
//   parse       the blob's coefficients in ws.scalars, as the proof calls read it (reference mode: big-endian coefficients reduced mod r;
//               c-kzg mode: the inverse transform of the range-checked little-endian evaluations)
//   extension   cells.hip: two forward transforms per blob through ws.fr and ws.scalars2, the cells written in the mode's byte order
//   quotients   cells.hip: the 128 monomial quotients q_k of each blob straight into the scalar slots of ws.scalars2
//   MSM         the engine's own launch set over 128 scalar sets per blob: 8 blobs fill its 1024 slots
// With the settings' FK20 engine on (fk20_api.hip) and a call at or above its threshold, fk20_proofs replaces the last two steps and a
// chunk is 512 blobs.
// Everything behind the parse is cells_from_coefficients, which the recovery (recover_api.hip) shares.
// The cells-only call (no proofs) takes chunks of 512 blobs: the two transforms per blob are what bounds it.
// The _columns forms want c of the 128 columns: the same pipeline with the list handed to the exit of the
// extension and to the quotients by value, c scalar sets per blob and the chunks of cells_columns_plan.h; all 128 is the full call.
#include "abi_guard.h"
#include "cells_common.h"

#include <string.h>

#include <vector>

namespace lwk {

void cells_from_coefficients(Ctx *c, uint8_t *cells, uint8_t *proofs48, size_t m, int mode, hipStream_t st, bool fk20, const CellColumns *cols,
                             uint32_t ncols) {
    Workspace &w = c->ws;
    const int le = mode_rules(mode).le();
    const size_t sets = m * (cols ? ncols : kProofsPerBlob);
    if (cells) launch_cells_extend(w.scalars, c->tw_fwd, c->tw28_fwd, w.fr, (Fr *)w.scalars2, cells, le, m, st, cols, ncols);
    if (proofs48 && fk20) {
        // (launches only without the hook's copy; behind the extension: both write ws.scalars2). A column call: every point is made, the
        // wanted ones are compressed
        (void)fk20_proofs(c, cols ? nullptr : proofs48, m, st);
        if (cols) launch_fk20_columns_compress(c->fk20.pts, *cols, ncols, proofs48, m, st);
    } else if (proofs48) {
        if (cols) launch_cells_quotients_columns(w.scalars, c->tw_fwd, w.scalars2, *cols, ncols, m, st);
        else launch_cells_quotients(w.scalars, c->tw_fwd, w.scalars2, sets, st);
        const bool lg = coefficients_to_msm_form(c, mode, sets, st);   // (scratch: ws.scalars, whose coefficients nobody reads from here on)
        msm_stages(c, w.scalars2, proofs48, sets, st, 0, false, lg);
    }
}

bool columns_from_list(ColumnsUse &u, const uint64_t *columns, size_t num_columns, const char *call) {
    if (!columns || num_columns < 1 || num_columns > kProofsPerBlob) {
        set_error("%s: no column list, or %zu columns wanted where 1 .. %zu can be", call, num_columns, kProofsPerBlob);
        return false;
    }
    for (size_t i = 0; i < num_columns; i++) {
        if (columns[i] >= kProofsPerBlob) {
            set_error("%s: column index %llu (at %zu) is not below %zu", call, (unsigned long long)columns[i], i, kProofsPerBlob);
            return false;
        }
        if (i && columns[i] <= columns[i - 1]) {
            set_error("%s: the columns are not strictly ascending (at %zu)", call, i);
            return false;
        }
        u.cols.k[i] = (uint8_t)columns[i];
    }
    for (size_t i = num_columns; i < kProofsPerBlob; i++) u.cols.k[i] = 0;
    u.c = (uint32_t)num_columns;
    return true;
}

ColumnsCall columns_call(const Ctx *c, const ColumnsUse &u, bool cells, bool proofs) {
    const Fk20State &f = c->primary->fk20;
    ColumnsCall q;
    q.c = u.c, q.cells = cells, q.proofs = proofs, q.pair_scratch = u.pair_scratch;
    q.fk20_on = f.engine == LWKZG_CELL_PROOFS_FK20, q.min_blobs = f.min_blobs;
    return q;
}

C_KZG_RET cells_chunks(Ctx *c, uint8_t *cells_out, uint8_t *proofs48, size_t n, int mode, hipStream_t st, int32_t *status,
                       const CoefficientStep &coefficients, size_t n_call, const ColumnsUse &use) {
    // (the caller holds this context's lock, under which the engine is switched)
    const ColumnsCall q = columns_call(c, use, cells_out != nullptr, proofs48 != nullptr);
    const bool fk20 = columns_fk20(q, n_call);
    const size_t chunk = columns_chunk(q, fk20);
    C_KZG_RET rc = ctx_reserve(c, columns_reserve(q, fk20, n));
    if (rc != C_KZG_OK) return rc;
    const CellColumns *cols = use.all() ? nullptr : &use.cols;   // all 128: the full calls' kernels
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = min_sz(chunk, n - off);
        int32_t *stt = status ? status + off : c->ws.status;
        LWK_HIP(hipMemsetAsync(stt, 0, m * 4, st));
        coefficients(off, m, stt);
        cells_from_coefficients(c, cells_out ? cells_out + off * use.c * kCellBytes : nullptr, proofs48 ? proofs48 + 48 * use.c * off : nullptr, m,
                                mode, st, fk20, cols, use.c);
    }
    LWK_HIP(hipGetLastError());
    return C_KZG_OK;
}

C_KZG_RET cells_host_slices(Ctx *c, const uint8_t *in, size_t in_bytes_per_blob, uint8_t *cells_out, uint8_t *proofs48, size_t n, int mode,
                            size_t *first_bad, const char *no_memory, const char *rejected, const SliceRun &run, const ColumnsUse *use) {
    std::vector<size_t> in_end(n + 1);
    for (size_t b = 0; b <= n; b++) in_end[b] = b * in_bytes_per_blob;
    return cells_host_slices_ragged(c, in, in_end.data(), cells_out, proofs48, n, mode, first_bad, no_memory, rejected,
                                    [&](uint8_t *d_cells, uint8_t *d_proofs, const uint8_t *d_in, size_t, size_t m, hipStream_t st,
                                        int32_t *d_status) { return run(d_cells, d_proofs, d_in, m, st, d_status); }, use);
}

C_KZG_RET cells_host_slices_ragged(Ctx *c, const uint8_t *in, const size_t *in_end, uint8_t *cells_out, uint8_t *proofs48, size_t n, int mode,
                                   size_t *first_bad, const char *no_memory, const char *rejected, const SliceRunAt &run,
                                   const ColumnsUse *use) {
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t ncols = use ? use->c : kProofsPerBlob;
    const size_t blob_cell_bytes = cells_out ? ncols * kCellBytes : 0, blob_proof_bytes = proofs48 ? ncols * 48 : 0;   // per blob, compact
    size_t slice = min_sz(n, kHostSlice);
    if (use) {   // the plan's slice: whole chunks of the engine this call's n takes
        const ColumnsCall q = columns_call(c, *use, cells_out != nullptr, proofs48 != nullptr);
        slice = columns_host_slice(columns_chunk(q, columns_fk20(q, n)), (in_end[n] + n - 1) / n + blob_cell_bytes + blob_proof_bytes + 4, n);
    }
    size_t in_bytes = 0;   // of the largest slice
    for (size_t off = 0; off < n; off += slice) {
        const size_t b = in_end[min_sz(off + slice, n)] - in_end[off];
        if (b > in_bytes) in_bytes = b;
    }
    in_bytes = (in_bytes + 15) & ~(size_t)15;   // (what follows the input in the block stays 16-byte aligned)
    const size_t cell_bytes = slice * blob_cell_bytes, proof_bytes = slice * blob_proof_bytes;
    const size_t total = in_bytes + cell_bytes + proof_bytes + slice * 4;
    LWK_HIP(hipSetDevice(c->device));
    uint8_t *d = nullptr;
    if (hipMalloc((void **)&d, total) != hipSuccess) {
        (void)hipGetLastError();
        set_error(no_memory, total);
        return C_KZG_MALLOC;
    }
    DevBlock block{d};
    uint8_t *d_in = d, *d_cells = cells_out ? d + in_bytes : nullptr;
    uint8_t *d_proofs = proofs48 ? d + in_bytes + cell_bytes : nullptr;
    int32_t *d_status = (int32_t *)(d + in_bytes + cell_bytes + proof_bytes);
    // the outputs go to host staging first: a rejected blob anywhere leaves the caller's buffers untouched
    std::vector<uint8_t> h_cells(n * blob_cell_bytes), h_proofs(n * blob_proof_bytes);
    std::vector<int32_t> h_status(n);
    hipStream_t st = c->stream;
    {
        WsUse wsu(c, st);
        for (size_t off = 0; off < n; off += slice) {
            const size_t m = min_sz(slice, n - off);
            LWK_HIP(hipMemcpyAsync(d_in, in + in_end[off], in_end[off + m] - in_end[off], hipMemcpyHostToDevice, st));
            C_KZG_RET rc = run(d_cells, d_proofs, d_in, off, m, st, d_status);
            if (rc != C_KZG_OK) return rc;
            LWK_HIP(hipMemcpyAsync(h_status.data() + off, d_status, m * 4, hipMemcpyDeviceToHost, st));
            if (cells_out) LWK_HIP(hipMemcpyAsync(h_cells.data() + off * blob_cell_bytes, d_cells, m * blob_cell_bytes, hipMemcpyDeviceToHost, st));
            if (proofs48) LWK_HIP(hipMemcpyAsync(h_proofs.data() + off * blob_proof_bytes, d_proofs, m * blob_proof_bytes, hipMemcpyDeviceToHost, st));
            LWK_HIP(hipStreamSynchronize(st));
        }
    }
    for (size_t i = 0; i < n; i++)
        if (h_status[i] != 0) {
            if (first_bad) *first_bad = i;
            set_error(rejected, i, h_status[i]);
            return map_rc((C_KZG_RET)h_status[i], mode);
        }
    if (cells_out) memcpy(cells_out, h_cells.data(), h_cells.size());
    if (proofs48) memcpy(proofs48, h_proofs.data(), h_proofs.size());
    return C_KZG_OK;
}

namespace {

// the device pipeline on st (caller holds the context's lock and the workspace); status: n words, 0 or the mode's rejection code
C_KZG_RET cells_device(Ctx *c, uint8_t *cells, uint8_t *proofs48, const uint8_t *blobs, size_t n, int mode, hipStream_t st, int32_t *status,
                       size_t n_call, const ColumnsUse &use = ColumnsUse()) {
    return cells_chunks(c, cells, proofs48, n, mode, st, status, [&](size_t off, size_t m, int32_t *stt) {
        const uint8_t *b = blobs + off * (size_t)kBlobBytes;
        if (!mode_rules(mode).evaluation_form) launch_parse_be_reduce(b, c->ws.scalars, m * kBlobElems, st);
        else launch_blob_evaluations_to_coefficients(b, c->ws.scalars, c->tw28_inv, stt, m, st, mode_rules(mode).le());
    }, n_call, use);
}

C_KZG_RET cells_batch_impl(Cell *cells, KZGProof *proofs, const Blob *blobs, size_t n, const KZGSettings *s, size_t *first_bad) {
    if (!s) return C_KZG_BADARGS;
    const int mode = mode_of(s);
    if (n == 0) return C_KZG_OK;
    if (!blobs || (!cells && !proofs)) {
        set_error("compute_cells_and_kzg_proofs: no blobs, or neither cells nor proofs wanted");
        return map_rc(C_KZG_BADARGS, mode);
    }
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    if (proofs) ensure_lagrange(c, mode);
    return cells_host_slices(c, (const uint8_t *)blobs, kBlobBytes, (uint8_t *)cells, (uint8_t *)proofs, n, mode, first_bad,
                             "compute_cells_and_kzg_proofs: no device memory for %zu bytes of staging", "blob %zu rejected (status %d)",
                             [&](uint8_t *d_cells, uint8_t *d_proofs, const uint8_t *d_blobs, size_t m, hipStream_t st, int32_t *d_status) {
                                 return cells_device(c, d_cells, d_proofs, d_blobs, m, mode, st, d_status, n);
                             });
}

// the argument errors of a column call, its list included: C_KZG_BADARGS in every mode, before any device work
bool columns_arguments(ColumnsUse &use, const void *cells, const void *proofs, const void *blobs, const uint64_t *columns, size_t num_columns,
                       const char *call) {
    if (!blobs || (!cells && !proofs)) {
        set_error("%s: no blobs, or neither cells nor proofs wanted", call);
        return false;
    }
    return columns_from_list(use, columns, num_columns, call);
}

C_KZG_RET cells_columns_impl(Cell *cells, KZGProof *proofs, const Blob *blobs, size_t n, const uint64_t *columns, size_t num_columns,
                             const KZGSettings *s, size_t *first_bad) {
    if (!s) return C_KZG_BADARGS;
    if (n == 0) return C_KZG_OK;
    ColumnsUse use;
    if (!columns_arguments(use, cells, proofs, blobs, columns, num_columns, "compute_cells_and_kzg_proofs_columns")) return C_KZG_BADARGS;
    const int mode = mode_of(s);
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    if (proofs) ensure_lagrange(c, mode);
    return cells_host_slices(c, (const uint8_t *)blobs, kBlobBytes, (uint8_t *)cells, (uint8_t *)proofs, n, mode, first_bad,
                             "compute_cells_and_kzg_proofs_columns: no device memory for %zu bytes of staging", "blob %zu rejected (status %d)",
                             [&](uint8_t *d_cells, uint8_t *d_proofs, const uint8_t *d_blobs, size_t m, hipStream_t st, int32_t *d_status) {
                                 return cells_device(c, d_cells, d_proofs, d_blobs, m, mode, st, d_status, n, use);
                             }, &use);
}

}  // namespace

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_compute_cells_and_kzg_proofs(Cell *cells, KZGProof *proofs, const Blob *blob, const KZGSettings *s) {
    return guarded("lwkzg_compute_cells_and_kzg_proofs", [&] { return cells_batch_impl(cells, proofs, blob, 1, s, nullptr); });
}

C_KZG_RET lwkzg_compute_cells_and_kzg_proofs_batch(Cell *cells, KZGProof *proofs, const Blob *blobs, size_t n, const KZGSettings *s,
                                                   size_t *first_bad) {
    return guarded("lwkzg_compute_cells_and_kzg_proofs_batch", [&] { return cells_batch_impl(cells, proofs, blobs, n, s, first_bad); });
}

C_KZG_RET lwkzg_compute_cells_and_kzg_proofs_batch_device(void *cells_dev, void *proofs48_dev, const void *blobs_dev, size_t n,
                                                          const KZGSettings *s, void *stream, int32_t *status_dev) {
    return guarded("lwkzg_compute_cells_and_kzg_proofs_batch_device", [&]() -> C_KZG_RET {
        if (!s) return C_KZG_BADARGS;
        const int mode = mode_of(s);
        if (n == 0) return C_KZG_OK;
        if (!blobs_dev || (!cells_dev && !proofs48_dev)) {
            set_error("lwkzg_compute_cells_and_kzg_proofs_batch_device: no blobs, or neither cells nor proofs wanted");
            return map_rc(C_KZG_BADARGS, mode);
        }
        Ctx *c = ctx_of(s);
        if (!c) return C_KZG_ERROR;
        if (proofs48_dev) ensure_lagrange(c, mode);
        std::lock_guard<std::mutex> lk(c->mu);
        LWK_HIP(hipSetDevice(c->device));
        hipStream_t st = stream ? (hipStream_t)stream : c->stream;
        WsUse wsu(c, st);
        return cells_device(c, (uint8_t *)cells_dev, (uint8_t *)proofs48_dev, (const uint8_t *)blobs_dev, n, mode, st, status_dev, n);
    });
}

C_KZG_RET lwkzg_compute_cells_and_kzg_proofs_columns(Cell *cells, KZGProof *proofs, const Blob *blobs, size_t n, const uint64_t *columns,
                                                     size_t num_columns, const KZGSettings *s, size_t *first_bad) {
    return guarded("lwkzg_compute_cells_and_kzg_proofs_columns",
                   [&] { return cells_columns_impl(cells, proofs, blobs, n, columns, num_columns, s, first_bad); });
}

C_KZG_RET lwkzg_compute_cells_and_kzg_proofs_columns_device(void *cells_dev, void *proofs48_dev, const void *blobs_dev, size_t n,
                                                            const uint64_t *columns, size_t num_columns, const KZGSettings *s, void *stream,
                                                            int32_t *status_dev) {
    return guarded("lwkzg_compute_cells_and_kzg_proofs_columns_device", [&]() -> C_KZG_RET {
        if (!s) return C_KZG_BADARGS;
        if (n == 0) return C_KZG_OK;
        ColumnsUse use;
        if (!columns_arguments(use, cells_dev, proofs48_dev, blobs_dev, columns, num_columns, "lwkzg_compute_cells_and_kzg_proofs_columns_device"))
            return C_KZG_BADARGS;
        const int mode = mode_of(s);
        Ctx *c = ctx_of(s);
        if (!c) return C_KZG_ERROR;
        if (proofs48_dev) ensure_lagrange(c, mode);
        std::lock_guard<std::mutex> lk(c->mu);
        LWK_HIP(hipSetDevice(c->device));
        hipStream_t st = stream ? (hipStream_t)stream : c->stream;
        WsUse wsu(c, st);
        return cells_device(c, (uint8_t *)cells_dev, (uint8_t *)proofs48_dev, (const uint8_t *)blobs_dev, n, mode, st, status_dev, n, use);
    });
}

}  // extern "C"
