// recover_api.hip -- EIP-7594 recover_cells_and_kzg_proofs: lwkzg_recover_cells_and_kzg_proofs (+ _batch, _batch_device).
// DESIGN.md section 4j.
//
// n blobs seen through ONE index set of 64 .. 128 cells. The host checks the indices (below 128, strictly ascending) before any device
// work; then, all on one stream:
//   setup         recover.hip: the call's table (the vanishing polynomial of the missing cells at the roots and on the coset)
//   per chunk     the status words cleared; recover.hip: the given cells -> the blob's 4096 coefficients in ws.scalars through
//                 ws.scalars2 (256 KiB per blob); cells_from_coefficients (cells_api.hip): extension, quotients, MSM
// Chunks as cells_api.hip has them: 8 blobs with proofs (one launch set of 1024 MSMs), 512 without.
#include "abi_guard.h"
#include "cells_common.h"

#include <string.h>

#include <vector>

namespace lwk {

namespace {

constexpr size_t kMinCells = kCellsPerBlob / 2;

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
                         size_t n, int mode, hipStream_t st, int32_t *status, size_t n_call) {
    const int le = mode == LWKZG_MODE_CKZG, bad = (int)bad_input(mode);
    launch_recover_setup(set, c->tw_fwd, c->recover_tab, st);
    return cells_chunks(c, cells_out, proofs48, n, mode, st, status, [&](size_t off, size_t m, int32_t *stt) {
        launch_recover_coefficients(cells_in + off * num_cells * kCellBytes, set, num_cells, c->tw_fwd, c->tw_inv, c->recover_tab,
                                    (Fr *)c->ws.scalars2, c->ws.scalars, stt, bad, le, m, st);
    }, n_call);
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
    return cells_host_slices(c, (const uint8_t *)cells, num_cells * kCellBytes, (uint8_t *)cells_out, (uint8_t *)proofs, n, mode, first_bad,
                             "recover_cells_and_kzg_proofs: no device memory for %zu bytes of staging",
                             "recover_cells_and_kzg_proofs: blob %zu rejected: a cell element is not below r, or its cells are inconsistent",
                             [&](uint8_t *d_cells, uint8_t *d_proofs, const uint8_t *d_in, size_t m, hipStream_t st, int32_t *d_status) {
                                 return recover_device(c, d_cells, d_proofs, set, d_in, num_cells, m, mode, st, d_status, n);
                             });
}

}  // namespace

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs(Cell *recovered_cells, KZGProof *recovered_proofs, const uint64_t *cell_indices, const Cell *cells,
                                             size_t num_cells, const KZGSettings *s) {
    return guarded("lwkzg_recover_cells_and_kzg_proofs",
                   [&] { return recover_batch_impl(recovered_cells, recovered_proofs, cell_indices, cells, num_cells, 1, s, nullptr); });
}

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_batch(Cell *recovered_cells, KZGProof *recovered_proofs, const uint64_t *cell_indices,
                                                   const Cell *cells, size_t num_cells, size_t n, const KZGSettings *s, size_t *first_bad) {
    return guarded("lwkzg_recover_cells_and_kzg_proofs_batch", [&] {
        return recover_batch_impl(recovered_cells, recovered_proofs, cell_indices, cells, num_cells, n, s, first_bad);
    });
}

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_batch_device(void *recovered_cells_dev, void *recovered_proofs48_dev, const uint64_t *cell_indices,
                                                          const void *cells_dev, size_t num_cells, size_t n, const KZGSettings *s, void *stream,
                                                          int32_t *status_dev) {
    return guarded("lwkzg_recover_cells_and_kzg_proofs_batch_device", [&]() -> C_KZG_RET {
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
                              mode, st, status_dev, n);
    });
}

}  // extern "C"
