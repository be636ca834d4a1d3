// cells_api.hip -- EIP-7594 compute_cells_and_kzg_proofs: lwkzg_compute_cells_and_kzg_proofs (+ _batch, _batch_device).
//
// A chunk of blobs at a time, all on one stream:
//   parse       the blob's coefficients in ws.scalars, as the proof calls read it (reference mode: big-endian coefficients reduced mod r;
//               c-kzg mode: the inverse transform of the range-checked little-endian evaluations)
//   extension   cells.hip: two forward transforms per blob through ws.fr and ws.scalars2, the cells written in the mode's byte order
//   quotients   cells.hip: the 128 monomial quotients q_k of each blob straight into the scalar slots of ws.scalars2
//   MSM         the engine's own launch set over 128 scalar sets per blob: 8 blobs fill its 1024 slots
// Everything behind the parse is cells_from_coefficients, which the recovery (recover_api.hip) shares.
// The cells-only call (no proofs) takes chunks of 512 blobs: the two transforms per blob are what bounds it.
#include "engine.h"

#include <string.h>

#include <vector>

namespace lwk {

namespace {

constexpr size_t kBlobCellBytes = (size_t)kCellsPerBlob * kCellElems * 32;   // 256 KiB: the 128 cells of one blob
constexpr size_t kProofsPerBlob = kCellsPerBlob;
constexpr size_t kProofChunk = kMaxChunk / kProofsPerBlob;                   // 8 blobs = one launch set of 1024 MSMs
constexpr size_t kCellsChunk = kMaxChunk / 2;                                // two transforms per blob in the workspace's 1024 slots
constexpr size_t kHostSlice = 64;                                            // blobs per upload / download of the host-pointer form
static_assert(kProofChunk * kProofsPerBlob == kMaxChunk, "a chunk of blobs fills a launch set");

size_t min_sz(size_t a, size_t b) { return a < b ? a : b; }

}  // namespace

void cells_from_coefficients(Ctx *c, uint8_t *cells, uint8_t *proofs48, size_t m, int mode, hipStream_t st) {
    Workspace &w = c->ws;
    const int le = mode == LWKZG_MODE_CKZG;
    if (cells) launch_cells_extend(w.scalars, c->tw_fwd, c->tw28_fwd, w.fr, (Fr *)w.scalars2, cells, le, m, st);
    if (proofs48) {
        launch_cells_quotients(w.scalars, c->tw_fwd, w.scalars2, m * kProofsPerBlob, st);
        const bool lg = coefficients_to_msm_form(c, mode, m * kProofsPerBlob, st);
        msm_stages(c, w.scalars2, proofs48, m * kProofsPerBlob, st, 0, false, lg);
    }
}

namespace {

// the device pipeline on st (caller holds the context's lock and the workspace); status: n words, 0 or the mode's rejection code
C_KZG_RET cells_device(Ctx *c, uint8_t *cells, uint8_t *proofs48, const uint8_t *blobs, size_t n, int mode, hipStream_t st, int32_t *status) {
    const size_t chunk = proofs48 ? kProofChunk : kCellsChunk;
    C_KZG_RET rc = ctx_reserve(c, (proofs48 ? kProofsPerBlob : 2) * min_sz(n, chunk));
    if (rc != C_KZG_OK) return rc;
    Workspace &w = c->ws;
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = min_sz(chunk, n - off);
        int32_t *stt = status ? status + off : w.status;
        const uint8_t *b = blobs + off * (size_t)kBlobBytes;
        LWK_HIP(hipMemsetAsync(stt, 0, m * 4, st));
        if (mode == LWKZG_MODE_REFERENCE) launch_parse_be_reduce(b, w.scalars, m * kBlobElems, st);
        else launch_blob_evaluations_to_coefficients(b, w.scalars, c->tw28_inv, stt, m, st);
        cells_from_coefficients(c, cells ? cells + off * kBlobCellBytes : nullptr, proofs48 ? proofs48 + 48 * kProofsPerBlob * off : nullptr, m, mode,
                                st);
    }
    LWK_HIP(hipGetLastError());
    return C_KZG_OK;
}

// host pointers: slices of up to kHostSlice blobs go up, through the device pipeline and back; the outputs are written only when every
// blob is good
C_KZG_RET cells_host(Ctx *c, uint8_t *cells, uint8_t *proofs48, const uint8_t *blobs, size_t n, int mode, size_t *first_bad) {
    const size_t slice = min_sz(n, kHostSlice);
    const size_t cell_bytes = cells ? slice * kBlobCellBytes : 0, proof_bytes = proofs48 ? slice * kProofsPerBlob * 48 : 0;
    const size_t total = slice * (size_t)kBlobBytes + cell_bytes + proof_bytes + slice * 4;
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    uint8_t *d = nullptr;
    if (hipMalloc((void **)&d, total) != hipSuccess) {
        (void)hipGetLastError();
        set_error("compute_cells_and_kzg_proofs: no device memory for %zu bytes of staging", total);
        return C_KZG_MALLOC;
    }
    struct Free {
        uint8_t *p;
        ~Free() { hipFree(p); }
    } fr{d};
    uint8_t *d_blobs = d, *d_cells = cells ? d + slice * (size_t)kBlobBytes : nullptr;
    uint8_t *d_proofs = proofs48 ? d + slice * (size_t)kBlobBytes + cell_bytes : nullptr;
    int32_t *d_status = (int32_t *)(d + slice * (size_t)kBlobBytes + cell_bytes + proof_bytes);
    // the outputs go to host staging first: a rejected blob anywhere leaves the caller's buffers untouched
    std::vector<uint8_t> h_cells(cells ? n * kBlobCellBytes : 0), h_proofs(proofs48 ? n * kProofsPerBlob * 48 : 0);
    std::vector<int32_t> h_status(n);
    hipStream_t st = c->stream;
    {
        WsUse wsu(c, st);
        for (size_t off = 0; off < n; off += slice) {
            const size_t m = min_sz(slice, n - off);
            LWK_HIP(hipMemcpyAsync(d_blobs, blobs + off * (size_t)kBlobBytes, m * (size_t)kBlobBytes, hipMemcpyHostToDevice, st));
            C_KZG_RET rc = cells_device(c, d_cells, d_proofs, d_blobs, m, mode, st, d_status);
            if (rc != C_KZG_OK) return rc;
            LWK_HIP(hipMemcpyAsync(h_status.data() + off, d_status, m * 4, hipMemcpyDeviceToHost, st));
            if (cells) LWK_HIP(hipMemcpyAsync(h_cells.data() + off * kBlobCellBytes, d_cells, m * kBlobCellBytes, hipMemcpyDeviceToHost, st));
            if (proofs48)
                LWK_HIP(hipMemcpyAsync(h_proofs.data() + off * kProofsPerBlob * 48, d_proofs, m * kProofsPerBlob * 48, hipMemcpyDeviceToHost, st));
            LWK_HIP(hipStreamSynchronize(st));
        }
    }
    for (size_t i = 0; i < n; i++)
        if (h_status[i] != 0) {
            if (first_bad) *first_bad = i;
            set_error("blob %zu rejected (status %d)", i, h_status[i]);
            return map_rc((C_KZG_RET)h_status[i], mode);
        }
    if (cells) memcpy(cells, h_cells.data(), h_cells.size());
    if (proofs48) memcpy(proofs48, h_proofs.data(), h_proofs.size());
    return C_KZG_OK;
}

// nothing may unwind across the C ABI
template <class F>
C_KZG_RET cells_guarded(const char *what, F &&f) {
    try {
        return f();
    } catch (const std::bad_alloc &) {
        set_error("%s: out of host memory", what);
        return C_KZG_MALLOC;
    } catch (...) {
        set_error("%s: unexpected exception", what);
        return C_KZG_ERROR;
    }
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
    return cells_host(c, (uint8_t *)cells, (uint8_t *)proofs, (const uint8_t *)blobs, n, mode, first_bad);
}

}  // namespace

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_compute_cells_and_kzg_proofs(Cell *cells, KZGProof *proofs, const Blob *blob, const KZGSettings *s) {
    return cells_guarded("lwkzg_compute_cells_and_kzg_proofs", [&] { return cells_batch_impl(cells, proofs, blob, 1, s, nullptr); });
}

C_KZG_RET lwkzg_compute_cells_and_kzg_proofs_batch(Cell *cells, KZGProof *proofs, const Blob *blobs, size_t n, const KZGSettings *s,
                                                   size_t *first_bad) {
    return cells_guarded("lwkzg_compute_cells_and_kzg_proofs_batch", [&] { return cells_batch_impl(cells, proofs, blobs, n, s, first_bad); });
}

C_KZG_RET lwkzg_compute_cells_and_kzg_proofs_batch_device(void *cells_dev, void *proofs48_dev, const void *blobs_dev, size_t n,
                                                          const KZGSettings *s, void *stream, int32_t *status_dev) {
    return cells_guarded("lwkzg_compute_cells_and_kzg_proofs_batch_device", [&]() -> C_KZG_RET {
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
        return cells_device(c, (uint8_t *)cells_dev, (uint8_t *)proofs48_dev, (const uint8_t *)blobs_dev, n, mode, st, status_dev);
    });
}

}  // extern "C"
