// cells_verify_blobs.h -- the entry of the cell proof pipelines for a caller that MAKES the items of its call: the cells, the indices and
// the grouping (cells_verify_blobs.hip: the 128 cells of whole blobs). The batch pipeline (cells_verify_api.hip)
// and the grouped one (cells_verify_groups.hip) run as they do for items that are passed in; what differs is where the items and the
// lists come from, and one status word per blob that is folded into the items' words before they come down.
#pragma once
#include "cell_groups_plan.h"
#include "cellv_bufs.h"

namespace lwk {

// the lists a grouped call keeps beside a batch's (cells_verify_groups.hip: DevSide, CellgBufs)
struct CellFrontGroupLists {
    uint32_t *item_group, *item_off, *slice_off;
    GroupSlice *slices;
};

struct CellFront {
    // ---- host side, complete before the pipeline is entered ----
    // batch: m and distinct (48 m) of `g`; nothing else of it is read.
    Grouping g;
    // grouped: item_off, row_base, dead, m_total, slices, slice_off and the first 48 m_total bytes of distinct; nothing else of it is read.
    GroupsPlan plan;
    // ---- device side: called under the context's lock with the workspace held and the call's buffers carved, before anything of the
    // call is enqueued. Enqueues on st what leaves the cells and the proofs of the n items on the device (cells / proofs: where), and
    // writes b.comm_in (the distinct commitments by row, padded with infinity encodings to n), b.idx, b.rows, b.perm_row, b.row_off,
    // b.perm_col, b.col_off and, for a grouped call (gl != nullptr), the four lists of gl ----
    virtual C_KZG_RET items(Ctx *c, hipStream_t st, const CellvBufs &b, const CellFrontGroupLists *gl, const uint8_t *&cells,
                            const uint8_t *&proofs) const = 0;
    // words[i] = bad_code for every item i of a blob that the front rejected (enqueued on st behind the validation's own words)
    virtual void fold_status(int32_t *words, int bad_code, hipStream_t st) const = 0;
    virtual ~CellFront() {}
};

// ---- the two device steps of a blob front, shared with the cell verifier's blob calls (cells_verify_async.hip; section 4t) ----
// nb device-resident blobs to their 128 cells each (cells: 256 KiB per blob) with a status word per blob: the front of the compute
// call, cells_chunks without proofs. The caller holds the context's lock and its workspace; enqueues on st, reads nothing back
C_KZG_RET launch_blob_cells(Ctx *c, uint8_t *cells, int32_t *bstatus, const uint8_t *blobs_dev, size_t nb, int mode, hipStream_t st);
// words[i] = bad_code for the 128 items of every blob whose status word is set (nothing in a mode that rejects no blob)
hipError_t launch_blob_fold_status(int32_t *words, const int32_t *bstatus, size_t nb, int mode, int bad_code, hipStream_t st);

// lwkzg_verify_cell_kzg_proof_batch / lwkzg_cell_verify_partials over the n items of `front` (n > 0)
C_KZG_RET cell_batch_front(bool *ok, uint8_t *partials, size_t n, const KZGSettings *s, hipStream_t caller, const CellFront &front);
// lwkzg_verify_cell_kzg_proof_groups / lwkzg_cell_verify_groups_partials over the n items of `front` in the g groups of item_offsets
C_KZG_RET cell_groups_front(uint8_t *ok_out, int32_t *rc_out, uint8_t *partials_out, size_t n, const uint64_t *item_offsets, size_t g,
                            const KZGSettings *s, hipStream_t caller, const CellFront &front);

}  // namespace lwk
