// recover_api.hip -- EIP-7594 recover_cells_and_kzg_proofs: lwkzg_recover_cells_and_kzg_proofs (+ _batch, _batch_device).
// DESIGN.md section 4j.
//
// n blobs seen through ONE index set of 64 .. 128 cells. The host checks the indices (below 128, strictly ascending) before any device
// work; then, all on one stream:
//   setup         recover.hip: the call's table (the vanishing polynomial of the missing cells at the roots and on the coset)
//   per chunk     the status words cleared; recover.hip: the given cells -> the blob's 4096 coefficients in ws.scalars through
//                 ws.scalars2 (256 KiB per blob); cells_from_coefficients (cells_api.hip): extension, quotients, MSM
// Chunks as cells_api.hip has them: 8 blobs with proofs (one launch set of 1024 MSMs), 512 without.
#include "engine.h"

#include <string.h>

#include <vector>

namespace lwk {

namespace {

constexpr size_t kCellBytes = (size_t)kCellElems * 32;
constexpr size_t kBlobCellBytes = (size_t)kCellsPerBlob * kCellBytes;   // 256 KiB: the 128 cells of one blob
constexpr size_t kProofsPerBlob = kCellsPerBlob;
constexpr size_t kProofChunk = kMaxChunk / kProofsPerBlob;               // 8 blobs = one launch set of 1024 MSMs
constexpr size_t kCellsChunk = kMaxChunk / 2;                            // two transforms (and 256 KiB of scratch) per blob in 1024 slots
constexpr size_t kHostSlice = 64;                                        // blobs per upload / download of the host-pointer forms
constexpr size_t kMinCells = kCellsPerBlob / 2;

size_t min_sz(size_t a, size_t b) { return a < b ? a : b; }

C_KZG_RET bad_input(int mode) { return mode == LWKZG_MODE_CKZG ? C_KZG_BADARGS : C_KZG_ERROR; }

// everything that is decidable without a GPU, in both modes: C_KZG_BADARGS
bool check_arguments(RecoverSet &set, const void *out_cells, const void *out_proofs, const uint64_t *idx, const void *cells, size_t num_cells) {
    if (!idx || !cells) {
        set_error("recover_cells_and_kzg_proofs: NULL argument");
        return false;
    }
    if (!out_cells && !out_proofs) {
        set_error("recover_cells_and_kzg_proofs: neither cells nor proofs wanted");
        return false;
    }
    if (num_cells < kMinCells || num_cells > (size_t)kCellsPerBlob) {
        set_error("recover_cells_and_kzg_proofs: %zu cells given, %zu .. %d are needed", num_cells, kMinCells, kCellsPerBlob);
        return false;
    }
    memset(&set, 0, sizeof set);
    for (size_t i = 0; i < num_cells; i++) {
        if (idx[i] >= (uint64_t)kCellsPerBlob) {
            set_error("recover_cells_and_kzg_proofs: cell index %zu is not below %d", i, kCellsPerBlob);
            return false;
        }
        if (i > 0 && idx[i] <= idx[i - 1]) {
            set_error("recover_cells_and_kzg_proofs: the cell indices are not strictly ascending (at %zu)", i);
            return false;
        }
        const uint32_t k = (uint32_t)idx[i];
        uint32_t q = 0;
        for (int b = 0; b < 7; b++) q |= ((k >> b) & 1u) << (6 - b);
        set.k[i] = (uint8_t)k;
        set.given[q >> 5] |= 1u << (q & 31u);
    }
    return true;
}

// the device pipeline on st (caller holds the context's lock and the workspace); status: n words, 0 or the mode's rejection code
C_KZG_RET recover_device(Ctx *c, uint8_t *cells_out, uint8_t *proofs48, const RecoverSet &set, const uint8_t *cells_in, size_t num_cells,
                         size_t n, int mode, hipStream_t st, int32_t *status) {
    const size_t chunk = proofs48 ? kProofChunk : kCellsChunk;
    C_KZG_RET rc = ctx_reserve(c, (proofs48 ? kProofsPerBlob : 2) * min_sz(n, chunk));
    if (rc != C_KZG_OK) return rc;
    Workspace &w = c->ws;
    const int le = mode == LWKZG_MODE_CKZG, bad = (int)bad_input(mode);
    launch_recover_setup(set, c->tw_fwd, c->recover_tab, st);
    for (size_t off = 0; off < n; off += chunk) {
        const size_t m = min_sz(chunk, n - off);
        int32_t *stt = status ? status + off : w.status;
        LWK_HIP(hipMemsetAsync(stt, 0, m * 4, st));
        launch_recover_coefficients(cells_in + off * num_cells * kCellBytes, set, num_cells, c->tw_fwd, c->tw_inv, c->recover_tab,
                                    (Fr *)w.scalars2, w.scalars, stt, bad, le, m, st);
        cells_from_coefficients(c, cells_out ? cells_out + off * kBlobCellBytes : nullptr,
                                proofs48 ? proofs48 + 48 * kProofsPerBlob * off : nullptr, m, mode, st);
    }
    LWK_HIP(hipGetLastError());
    return C_KZG_OK;
}

// host pointers: slices of up to kHostSlice blobs go up, through the device pipeline and back; the outputs are written only when every
// blob is good
C_KZG_RET recover_host(Ctx *c, uint8_t *cells_out, uint8_t *proofs48, const RecoverSet &set, const uint8_t *cells_in, size_t num_cells, size_t n,
                       int mode, size_t *first_bad) {
    const size_t slice = min_sz(n, kHostSlice);
    const size_t in_bytes = slice * num_cells * kCellBytes;
    const size_t cell_bytes = cells_out ? slice * kBlobCellBytes : 0, proof_bytes = proofs48 ? slice * kProofsPerBlob * 48 : 0;
    const size_t total = in_bytes + cell_bytes + proof_bytes + slice * 4;
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    uint8_t *d = nullptr;
    if (hipMalloc((void **)&d, total) != hipSuccess) {
        (void)hipGetLastError();
        set_error("recover_cells_and_kzg_proofs: no device memory for %zu bytes of staging", total);
        return C_KZG_MALLOC;
    }
    struct Free {
        uint8_t *p;
        ~Free() { hipFree(p); }
    } fr{d};
    uint8_t *d_in = d, *d_cells = cells_out ? d + in_bytes : nullptr;
    uint8_t *d_proofs = proofs48 ? d + in_bytes + cell_bytes : nullptr;
    int32_t *d_status = (int32_t *)(d + in_bytes + cell_bytes + proof_bytes);
    // the outputs go to host staging first: a rejected blob anywhere leaves the caller's buffers untouched
    std::vector<uint8_t> h_cells(cells_out ? n * kBlobCellBytes : 0), h_proofs(proofs48 ? n * kProofsPerBlob * 48 : 0);
    std::vector<int32_t> h_status(n);
    hipStream_t st = c->stream;
    {
        WsUse wsu(c, st);
        for (size_t off = 0; off < n; off += slice) {
            const size_t m = min_sz(slice, n - off);
            LWK_HIP(hipMemcpyAsync(d_in, cells_in + off * num_cells * kCellBytes, m * num_cells * kCellBytes, hipMemcpyHostToDevice, st));
            C_KZG_RET rc = recover_device(c, d_cells, d_proofs, set, d_in, num_cells, m, mode, st, d_status);
            if (rc != C_KZG_OK) return rc;
            LWK_HIP(hipMemcpyAsync(h_status.data() + off, d_status, m * 4, hipMemcpyDeviceToHost, st));
            if (cells_out) LWK_HIP(hipMemcpyAsync(h_cells.data() + off * kBlobCellBytes, d_cells, m * kBlobCellBytes, hipMemcpyDeviceToHost, st));
            if (proofs48)
                LWK_HIP(hipMemcpyAsync(h_proofs.data() + off * kProofsPerBlob * 48, d_proofs, m * kProofsPerBlob * 48, hipMemcpyDeviceToHost, st));
            LWK_HIP(hipStreamSynchronize(st));
        }
    }
    for (size_t i = 0; i < n; i++)
        if (h_status[i] != 0) {
            if (first_bad) *first_bad = i;
            set_error("recover_cells_and_kzg_proofs: blob %zu rejected: a cell element is not below r, or its cells are inconsistent", i);
            return map_rc((C_KZG_RET)h_status[i], mode);
        }
    if (cells_out) memcpy(cells_out, h_cells.data(), h_cells.size());
    if (proofs48) memcpy(proofs48, h_proofs.data(), h_proofs.size());
    return C_KZG_OK;
}

// nothing may unwind across the C ABI
template <class F>
C_KZG_RET recover_guarded(const char *what, F &&f) {
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

C_KZG_RET recover_batch_impl(Cell *cells_out, KZGProof *proofs, const uint64_t *idx, const Cell *cells, size_t num_cells, size_t n,
                             const KZGSettings *s, size_t *first_bad) {
    if (!s) return C_KZG_BADARGS;
    if (n == 0) return C_KZG_OK;
    RecoverSet set;
    if (!check_arguments(set, cells_out, proofs, idx, cells, num_cells)) return C_KZG_BADARGS;
    const int mode = mode_of(s);
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    if (proofs) ensure_lagrange(c, mode);
    return recover_host(c, (uint8_t *)cells_out, (uint8_t *)proofs, set, (const uint8_t *)cells, num_cells, n, mode, first_bad);
}

}  // namespace

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs(Cell *recovered_cells, KZGProof *recovered_proofs, const uint64_t *cell_indices, const Cell *cells,
                                             size_t num_cells, const KZGSettings *s) {
    return recover_guarded("lwkzg_recover_cells_and_kzg_proofs",
                           [&] { return recover_batch_impl(recovered_cells, recovered_proofs, cell_indices, cells, num_cells, 1, s, nullptr); });
}

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_batch(Cell *recovered_cells, KZGProof *recovered_proofs, const uint64_t *cell_indices,
                                                   const Cell *cells, size_t num_cells, size_t n, const KZGSettings *s, size_t *first_bad) {
    return recover_guarded("lwkzg_recover_cells_and_kzg_proofs_batch", [&] {
        return recover_batch_impl(recovered_cells, recovered_proofs, cell_indices, cells, num_cells, n, s, first_bad);
    });
}

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_batch_device(void *recovered_cells_dev, void *recovered_proofs48_dev, const uint64_t *cell_indices,
                                                          const void *cells_dev, size_t num_cells, size_t n, const KZGSettings *s, void *stream,
                                                          int32_t *status_dev) {
    return recover_guarded("lwkzg_recover_cells_and_kzg_proofs_batch_device", [&]() -> C_KZG_RET {
        if (!s) return C_KZG_BADARGS;
        if (n == 0) return C_KZG_OK;
        RecoverSet set;
        if (!check_arguments(set, recovered_cells_dev, recovered_proofs48_dev, cell_indices, cells_dev, num_cells)) return C_KZG_BADARGS;
        const int mode = mode_of(s);
        Ctx *c = ctx_of(s);
        if (!c) return C_KZG_ERROR;
        if (recovered_proofs48_dev) ensure_lagrange(c, mode);
        std::lock_guard<std::mutex> lk(c->mu);
        LWK_HIP(hipSetDevice(c->device));
        hipStream_t st = stream ? (hipStream_t)stream : c->stream;
        WsUse wsu(c, st);
        return recover_device(c, (uint8_t *)recovered_cells_dev, (uint8_t *)recovered_proofs48_dev, set, (const uint8_t *)cells_dev, num_cells, n,
                              mode, st, status_dev);
    });
}

}  // extern "C"
