// recover_api.hip -- EIP-7594 recover_cells_and_kzg_proofs: lwkzg_recover_cells_and_kzg_proofs (+ _batch, _batch_device), n blobs seen
// through ONE index set, and lwkzg_recover_cells_and_kzg_proofs_mixed (+ _device), where every blob has an index set of its own.
// DESIGN.md section 4j.
//
// One argument check, one host driver and one device driver behind the five entry points: to the host a shared-set call is a mixed
// call with one distinct set (recover_sets.h). The host checks the lists (64 .. 128 indices, below 128, strictly ascending) before any
// device work; then, all on one stream:
//   setup         recover.hip: one table per DISTINCT set of the call (the vanishing polynomial of the missing cells at the roots and on
//                 the coset)
//   per chunk     the status words cleared; recover.hip: the given cells -> the blob's 4096 coefficients in ws.scalars through
//                 ws.scalars2 (256 KiB per blob); cells_from_coefficients (cells_api.hip): extension, quotients, MSM
// Chunks as cells_api.hip has them: 8 blobs with proofs (one launch set of 1024 MSMs), 512 without.
// The _columns forms (shared set) hand a list of wanted columns to what is behind the coefficients; the setup,
// the coefficient step and the consistency check do not know of it.
// The two kinds of call differ in how the sets reach the kernels, in two places (recover_setup and the coefficient step of
// recover_device). A shared-set call hands its kernels the set by value and keeps its table in the context's recover_tab: a chunk is one
// launch of each kernel. A mixed call keeps its sets' tables, lists and masks in a grow-only device buffer of the context and hands a
// chunk's set ids and cell offsets to the kernels by value, kRecoverGroup blobs to a launch. (A cells-only shared-set call of 1024 blobs
// through the mixed kernels was measured 2 % slower, two launches per chunk where one does: profiles/recover_one_kernel_set_timing.md.)
#include "abi_guard.h"
#include "carve.h"
#include "cells_common.h"

#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

namespace lwk {

namespace {

constexpr size_t kMinCells = kRecoverMinCells;

// the lists of a call as its entry point got them: one for every blob (mixed; num_cells: n counts) or one for all of them (num_cells:
// its one count)
struct Lists {
    bool mixed;
    const uint64_t *idx;
    const size_t *num_cells;
    const char *call() const { return mixed ? "recover_cells_and_kzg_proofs_mixed" : "recover_cells_and_kzg_proofs"; }
};

// a faulty index list as the error text; `blob`: its place in a mixed call, nullptr for the shared-set calls
void set_list_error(RecoverListFault f, size_t num_cells, size_t at, const size_t *blob) {
    char where[40] = "";
    if (blob) snprintf(where, sizeof where, " (blob %zu)", *blob);
    if (f == kRecoverListCount)
        set_error("recover_cells_and_kzg_proofs: %zu cells given, %zu .. %d are needed%s", num_cells, kMinCells, kCellsPerBlob, where);
    else if (f == kRecoverListIndex) set_error("recover_cells_and_kzg_proofs: cell index %zu is not below %d%s", at, kCellsPerBlob, where);
    else set_error("recover_cells_and_kzg_proofs: the cell indices are not strictly ascending (at %zu)%s", at, where);
}

// everything that is decidable without a GPU, in both modes: C_KZG_BADARGS. A mixed call's faulty list names its blob, in first_bad
// (optional) too
bool check_arguments(RecoverSets &sets, const Lists &l, const void *out_cells, const void *out_proofs, const void *cells, size_t n,
                     size_t *first_bad) {
    if (!l.idx || !cells || !l.num_cells) {
        set_error("%s: NULL argument", l.call());
        return false;
    }
    if (!out_cells && !out_proofs) {
        set_error("%s: neither cells nor proofs wanted", l.call());
        return false;
    }
    if (l.mixed ? recover_sets_of(sets, l.idx, l.num_cells, n) : recover_sets_shared(sets, l.idx, *l.num_cells, n)) return true;
    set_list_error(sets.fault, l.num_cells[sets.bad_blob], sets.bad_at, l.mixed ? &sets.bad_blob : nullptr);
    if (l.mixed && first_bad) *first_bad = sets.bad_blob;
    return false;
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

// the call's tables on st: a shared-set call's one table in the context's recover_tab (its kernels take the set itself by value), a
// mixed call's sets in the block above, dev its pieces
C_KZG_RET recover_setup(Ctx *c, const Lists &l, const RecoverSets &sets, RecoverSetsDev &dev, hipStream_t st) {
    if (!l.mixed) {
        launch_recover_setup(sets.sets[0], c->tw_fwd, c->recover_tab, st);
        return C_KZG_OK;
    }
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

// the device pipeline of blobs b0 .. b0 + n of a call on st (caller holds the context's lock and the workspace; recover_setup has run);
// cells_in: the cells of blob b0 on; status: n words, 0 or the mode's rejection code; use: the wanted columns, which reach only what
// is behind the coefficients
C_KZG_RET recover_device(Ctx *c, uint8_t *cells_out, uint8_t *proofs48, const Lists &l, const RecoverSets &sets, const RecoverSetsDev &dev,
                         const uint8_t *cells_in, size_t b0, size_t n, int mode, hipStream_t st, int32_t *status, size_t n_call,
                         const ColumnsUse &use) {
    const int le = mode_rules(mode).le(), bad = (int)bad_input(mode);
    return cells_chunks(c, cells_out, proofs48, n, mode, st, status, [&](size_t off, size_t m, int32_t *stt) {
        if (!l.mixed) {   // the whole chunk in one launch of each kernel
            launch_recover_coefficients(cells_in + off * *l.num_cells * kCellBytes, sets.sets[0], *l.num_cells, c->tw_fwd, c->tw_inv,
                                        c->recover_tab, (Fr *)c->ws.scalars2, c->ws.scalars, stt, bad, le, m, st);
            return;
        }
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
    }, n_call, use);
}

// the wanted columns of a call as its entry point got them: a list (the _columns forms) or none (all 128)
struct Wanted {
    bool listed = false;
    const uint64_t *columns = nullptr;
    size_t num_columns = 0;
};

// use for the call: the recovery's scratch is two workspace slots per blob whatever is wanted; a list is checked behind the full call's
// own arguments (C_KZG_BADARGS)
bool wanted_columns(ColumnsUse &use, const Wanted &w) {
    use.pair_scratch = true;
    return !w.listed || columns_from_list(use, w.columns, w.num_columns, "recover_cells_and_kzg_proofs_columns");
}

// host pointers: slices of 64 blobs (a column call: the plan's slice) up and back (cells_api.hip), the call's sets made once, in front of
// its first slice
C_KZG_RET recover_host(Cell *cells_out, KZGProof *proofs, const Lists &l, const Cell *cells, size_t n, const KZGSettings *s, size_t *first_bad,
                       const Wanted &wanted = Wanted()) {
    if (!s) return C_KZG_BADARGS;
    if (n == 0) return C_KZG_OK;
    RecoverSets sets;
    if (!check_arguments(sets, l, cells_out, proofs, cells, n, first_bad)) return C_KZG_BADARGS;
    ColumnsUse use;
    if (!wanted_columns(use, wanted)) return C_KZG_BADARGS;
    const int mode = mode_of(s);
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    if (proofs) ensure_lagrange(c, mode);
    std::vector<size_t> in_end(n + 1);
    for (size_t b = 0; b <= n; b++) in_end[b] = sets.cell_off[b] * kCellBytes;
    const std::string no_memory = std::string(l.call()) + ": no device memory for %zu bytes of staging";
    const std::string rejected = std::string(l.call()) + ": blob %zu rejected: a cell element is not below r, or its cells are inconsistent";
    RecoverSetsDev dev{};
    return cells_host_slices_ragged(
        c, (const uint8_t *)cells, in_end.data(), (uint8_t *)cells_out, (uint8_t *)proofs, n, mode, first_bad, no_memory.c_str(), rejected.c_str(),
        [&](uint8_t *d_cells, uint8_t *d_proofs, const uint8_t *d_in, size_t off, size_t m, hipStream_t st, int32_t *d_status) {
            if (off == 0) {
                C_KZG_RET rc = recover_setup(c, l, sets, dev, st);
                if (rc != C_KZG_OK) return rc;
            }
            return recover_device(c, d_cells, d_proofs, l, sets, dev, d_in, off, m, mode, st, d_status, n, use);
        }, wanted.listed ? &use : nullptr);
}

// device pointers, on the caller's stream or the context's
C_KZG_RET recover_on_device(void *cells_out, void *proofs48, const Lists &l, const void *cells, size_t n, const KZGSettings *s, void *stream,
                            int32_t *status, const Wanted &wanted = Wanted()) {
    if (!s) return C_KZG_BADARGS;
    if (n == 0) return C_KZG_OK;
    RecoverSets sets;
    if (!check_arguments(sets, l, cells_out, proofs48, cells, n, nullptr)) return C_KZG_BADARGS;
    ColumnsUse use;
    if (!wanted_columns(use, wanted)) return C_KZG_BADARGS;
    const int mode = mode_of(s);
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    if (proofs48) ensure_lagrange(c, mode);
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    WsUse wsu(c, st);
    RecoverSetsDev dev{};
    C_KZG_RET rc = recover_setup(c, l, sets, dev, st);
    if (rc != C_KZG_OK) return rc;
    return recover_device(c, (uint8_t *)cells_out, (uint8_t *)proofs48, l, sets, dev, (const uint8_t *)cells, 0, n, mode, st, status, n, use);
}

}  // namespace

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs(Cell *recovered_cells, KZGProof *recovered_proofs, const uint64_t *cell_indices, const Cell *cells,
                                             size_t num_cells, const KZGSettings *s) {
    return guarded("lwkzg_recover_cells_and_kzg_proofs", [&] {
        return recover_host(recovered_cells, recovered_proofs, Lists{false, cell_indices, &num_cells}, cells, 1, s, nullptr);
    });
}

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_batch(Cell *recovered_cells, KZGProof *recovered_proofs, const uint64_t *cell_indices,
                                                   const Cell *cells, size_t num_cells, size_t n, const KZGSettings *s, size_t *first_bad) {
    return guarded("lwkzg_recover_cells_and_kzg_proofs_batch", [&] {
        return recover_host(recovered_cells, recovered_proofs, Lists{false, cell_indices, &num_cells}, cells, n, s, first_bad);
    });
}

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_batch_device(void *recovered_cells_dev, void *recovered_proofs48_dev, const uint64_t *cell_indices,
                                                          const void *cells_dev, size_t num_cells, size_t n, const KZGSettings *s, void *stream,
                                                          int32_t *status_dev) {
    return guarded("lwkzg_recover_cells_and_kzg_proofs_batch_device", [&] {
        return recover_on_device(recovered_cells_dev, recovered_proofs48_dev, Lists{false, cell_indices, &num_cells}, cells_dev, n, s, stream,
                                 status_dev);
    });
}

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_columns(Cell *cells_out, KZGProof *proofs_out, const uint64_t *cell_indices, const Cell *cells,
                                                     size_t num_cells, size_t n, const uint64_t *columns, size_t num_columns,
                                                     const KZGSettings *s, size_t *first_bad) {
    return guarded("lwkzg_recover_cells_and_kzg_proofs_columns", [&] {
        return recover_host(cells_out, proofs_out, Lists{false, cell_indices, &num_cells}, cells, n, s, first_bad,
                            Wanted{true, columns, num_columns});
    });
}

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_columns_device(void *cells_out_dev, void *proofs48_out_dev, const uint64_t *cell_indices,
                                                            const void *cells_dev, size_t num_cells, size_t n, const uint64_t *columns,
                                                            size_t num_columns, const KZGSettings *s, void *stream, int32_t *status_dev) {
    return guarded("lwkzg_recover_cells_and_kzg_proofs_columns_device", [&] {
        return recover_on_device(cells_out_dev, proofs48_out_dev, Lists{false, cell_indices, &num_cells}, cells_dev, n, s, stream, status_dev,
                                 Wanted{true, columns, num_columns});
    });
}

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_mixed(Cell *recovered_cells, KZGProof *recovered_proofs, const uint64_t *cell_indices,
                                                   const Cell *cells, const size_t *num_cells, size_t n, const KZGSettings *s, size_t *first_bad) {
    return guarded("lwkzg_recover_cells_and_kzg_proofs_mixed", [&] {
        return recover_host(recovered_cells, recovered_proofs, Lists{true, cell_indices, num_cells}, cells, n, s, first_bad);
    });
}

C_KZG_RET lwkzg_recover_cells_and_kzg_proofs_mixed_device(void *recovered_cells_dev, void *recovered_proofs48_dev, const uint64_t *cell_indices,
                                                          const void *cells_dev, const size_t *num_cells, size_t n, const KZGSettings *s,
                                                          void *stream, int32_t *status_dev) {
    return guarded("lwkzg_recover_cells_and_kzg_proofs_mixed_device", [&] {
        return recover_on_device(recovered_cells_dev, recovered_proofs48_dev, Lists{true, cell_indices, num_cells}, cells_dev, n, s, stream,
                                 status_dev);
    });
}

}  // extern "C"
