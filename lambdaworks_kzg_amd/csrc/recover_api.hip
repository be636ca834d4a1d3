// recover_api.hip -- EIP-7594 recover_cells_and_kzg_proofs: lwkzg_recover_cells_and_kzg_proofs (+ _batch, _batch_device), and
// lwkzg_recover_cells_and_kzg_proofs_mixed (+ _device), where every blob has an index set of its own. DESIGN.md section 4j.
//
// n blobs seen through ONE index set of 64 .. 128 cells. The host checks the indices (below 128, strictly ascending) before any device
// work; then, all on one stream:
//   setup         recover.hip: the call's table (the vanishing polynomial of the missing cells at the roots and on the coset)
//   per chunk     the status words cleared; recover.hip: the given cells -> the blob's 4096 coefficients in ws.scalars through
//                 ws.scalars2 (256 KiB per blob); cells_from_coefficients (cells_api.hip): extension, quotients, MSM
// Chunks as cells_api.hip has them: 8 blobs with proofs (one launch set of 1024 MSMs), 512 without.
// The mixed form is the same pipeline: the setup makes one table per DISTINCT set of the call (recover_sets.h de-duplicates them) in a
// grow-only device buffer of the context, and a chunk's coefficient step hands its blobs' set ids and cell offsets to the kernels by
// value, kRecoverGroup blobs to a launch.
#include "abi_guard.h"
#include "carve.h"
#include "cells_common.h"

#include <stdio.h>
#include <string.h>

#include <vector>

namespace lwk {

namespace {

constexpr size_t kMinCells = kRecoverMinCells;

// a faulty index list as the error text; `blob`: its place in a mixed call, nullptr for the shared-set calls
void set_list_error(RecoverListFault f, size_t num_cells, size_t at, const size_t *blob) {
    char where[40] = "";
    if (blob) snprintf(where, sizeof where, " (blob %zu)", *blob);
    if (f == kRecoverListCount)
        set_error("recover_cells_and_kzg_proofs: %zu cells given, %zu .. %d are needed%s", num_cells, kMinCells, kCellsPerBlob, where);
    else if (f == kRecoverListIndex) set_error("recover_cells_and_kzg_proofs: cell index %zu is not below %d%s", at, kCellsPerBlob, where);
    else set_error("recover_cells_and_kzg_proofs: the cell indices are not strictly ascending (at %zu)%s", at, where);
}

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
    size_t at = 0;
    const RecoverListFault f = recover_set_of(set, idx, num_cells, &at);
    if (f != kRecoverListGood) set_list_error(f, num_cells, at, nullptr);
    return f == kRecoverListGood;
}

// the same for the mixed calls; first_bad (optional) gets the blob whose list is at fault
bool check_mixed_arguments(RecoverSets &sets, const void *out_cells, const void *out_proofs, const uint64_t *idx, const void *cells,
                           const size_t *num_cells, size_t n, size_t *first_bad) {
    if (!idx || !cells || !num_cells) {
        set_error("recover_cells_and_kzg_proofs_mixed: NULL argument");
        return false;
    }
    if (!out_cells && !out_proofs) {
        set_error("recover_cells_and_kzg_proofs_mixed: neither cells nor proofs wanted");
        return false;
    }
    if (recover_sets_of(sets, idx, num_cells, n)) return true;
    set_list_error(sets.fault, num_cells[sets.bad_blob], sets.bad_at, &sets.bad_blob);
    if (first_bad) *first_bad = sets.bad_blob;
    return false;
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

// The device block of a mixed call's distinct sets: grow-only, kept with the settings object (first 64 sets, 1 MiB, then doubling); no
// allocation in steady state. Written by k_recover_mixed_setup alone, in stream order behind whatever read it last (caller holds c->mu
// and the workspace, whose event orders the streams)
size_t carve_sets(RecoverSetsDev &d, uint8_t *base, size_t cap) {
    Carver cv(base);
    cv.take(d.tab, cap * kRecoverTabElems * sizeof(Fr));
    cv.take(d.k, cap * kCellsPerBlob);
    cv.take(d.given, cap * (kCellsPerBlob / 8));
    return cv.bytes();
}

C_KZG_RET mixed_setup(Ctx *c, const RecoverSets &sets, RecoverSetsDev &dev, hipStream_t st) {
    C_KZG_RET rc = grow_reserve(c->recover_sets, sets.sets.size(), 64, [](size_t cap) { RecoverSetsDev probe; return carve_sets(probe, nullptr, cap); },
                                "recover_cells_and_kzg_proofs_mixed: no device memory for %zu index sets (%zu bytes)");
    if (rc != C_KZG_OK) return rc;
    carve_sets(dev, c->recover_sets.dev, c->recover_sets.cap);
    for (size_t first = 0; first < sets.sets.size(); first += kRecoverSetupGroup) {
        const size_t m = min_sz(kRecoverSetupGroup, sets.sets.size() - first);
        RecoverMasks masks;
        for (size_t j = 0; j < m; j++) memcpy(masks.given[j], sets.sets[first + j].given, sizeof masks.given[j]);
        launch_recover_mixed_setup(masks, first, m, c->tw_fwd, dev, st);
    }
    return C_KZG_OK;
}

// the device pipeline of blobs b0 .. b0 + n of a mixed call on st (caller holds the context's lock and the workspace; the sets are on the
// device); cells_in: the cells of blob b0 on
C_KZG_RET mixed_device(Ctx *c, uint8_t *cells_out, uint8_t *proofs48, const RecoverSets &sets, const RecoverSetsDev &dev, const uint8_t *cells_in,
                       size_t b0, size_t n, int mode, hipStream_t st, int32_t *status, size_t n_call) {
    const int le = mode == LWKZG_MODE_CKZG, bad = (int)bad_input(mode);
    return cells_chunks(c, cells_out, proofs48, n, mode, st, status, [&](size_t off, size_t m, int32_t *stt) {
        // the chunk's blobs b0 + off .. + m, a group at a time: the chunk's scratch, coefficients and status words are blob-major
        for (size_t g0 = 0; g0 < m; g0 += kRecoverGroup) {
            const size_t gm = min_sz(kRecoverGroup, m - g0), first = b0 + off + g0;
            RecoverGroup grp;
            for (size_t j = 0; j < gm; j++) {
                grp.set[j] = sets.set_of[first + j];
                grp.cell0[j] = (uint32_t)(sets.cell_off[first + j] - sets.cell_off[first]);
            }
            launch_recover_mixed_coefficients(cells_in + (sets.cell_off[first] - sets.cell_off[b0]) * kCellBytes, grp,
                                              sets.cell_off[first + gm] - sets.cell_off[first], c->tw_fwd, c->tw_inv, dev,
                                              (Fr *)c->ws.scalars2 + g0 * (size_t)kCellElems * kCellsPerBlob,
                                              c->ws.scalars + g0 * (size_t)kBlobElems * 8, stt + g0, bad, le, gm, st);
        }
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

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_mixed(Cell *recovered_cells, KZGProof *recovered_proofs, const uint64_t *cell_indices,
                                                   const Cell *cells, const size_t *num_cells, size_t n, const KZGSettings *s, size_t *first_bad) {
    return guarded("lwkzg_recover_cells_and_kzg_proofs_mixed", [&]() -> C_KZG_RET {
        if (!s) return C_KZG_BADARGS;
        if (n == 0) return C_KZG_OK;
        RecoverSets sets;
        if (!check_mixed_arguments(sets, recovered_cells, recovered_proofs, cell_indices, cells, num_cells, n, first_bad)) return C_KZG_BADARGS;
        const int mode = mode_of(s);
        Ctx *c = ctx_of(s);
        if (!c) return C_KZG_ERROR;
        if (recovered_proofs) ensure_lagrange(c, mode);
        std::vector<size_t> in_end(n + 1);
        for (size_t b = 0; b <= n; b++) in_end[b] = sets.cell_off[b] * kCellBytes;
        RecoverSetsDev dev;
        return cells_host_slices_ragged(
            c, (const uint8_t *)cells, in_end.data(), (uint8_t *)recovered_cells, (uint8_t *)recovered_proofs, n, mode, first_bad,
            "recover_cells_and_kzg_proofs_mixed: no device memory for %zu bytes of staging",
            "recover_cells_and_kzg_proofs_mixed: blob %zu rejected: a cell element is not below r, or its cells are inconsistent",
            [&](uint8_t *d_cells, uint8_t *d_proofs, const uint8_t *d_in, size_t off, size_t m, hipStream_t st, int32_t *d_status) {
                if (off == 0) {   // the call's sets, once, in front of its first slice
                    C_KZG_RET rc = mixed_setup(c, sets, dev, st);
                    if (rc != C_KZG_OK) return rc;
                }
                return mixed_device(c, d_cells, d_proofs, sets, dev, d_in, off, m, mode, st, d_status, n);
            });
    });
}

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_mixed_device(void *recovered_cells_dev, void *recovered_proofs48_dev, const uint64_t *cell_indices,
                                                          const void *cells_dev, const size_t *num_cells, size_t n, const KZGSettings *s,
                                                          void *stream, int32_t *status_dev) {
    return guarded("lwkzg_recover_cells_and_kzg_proofs_mixed_device", [&]() -> C_KZG_RET {
        if (!s) return C_KZG_BADARGS;
        if (n == 0) return C_KZG_OK;
        RecoverSets sets;
        if (!check_mixed_arguments(sets, recovered_cells_dev, recovered_proofs48_dev, cell_indices, cells_dev, num_cells, n, nullptr))
            return C_KZG_BADARGS;
        const int mode = mode_of(s);
        Ctx *c = ctx_of(s);
        if (!c) return C_KZG_ERROR;
        if (recovered_proofs48_dev) ensure_lagrange(c, mode);
        std::lock_guard<std::mutex> lk(c->mu);
        LWK_HIP(hipSetDevice(c->device));
        hipStream_t st = stream ? (hipStream_t)stream : c->stream;
        WsUse wsu(c, st);
        RecoverSetsDev dev;
        C_KZG_RET rc = mixed_setup(c, sets, dev, st);
        if (rc != C_KZG_OK) return rc;
        return mixed_device(c, (uint8_t *)recovered_cells_dev, (uint8_t *)recovered_proofs48_dev, sets, dev, (const uint8_t *)cells_dev, 0, n, mode,
                            st, status_dev, n);
    });
}

}  // extern "C"
