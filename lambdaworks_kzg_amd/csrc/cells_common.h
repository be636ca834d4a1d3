// cells_common.h -- what the EIP-7594 compute paths share (cells_api.hip, recover_api.hip): the sizes, the chunk loop behind the step
// that makes coefficients, and the driver of the host-pointer forms. The cell verifiers take kCellBytes and bad_input from here.
#pragma once
#include "cells_columns_plan.h"
#include "engine.h"

namespace lwk {

constexpr size_t kCellBytes = (size_t)kCellElems * 32;
constexpr size_t kBlobCellBytes = (size_t)kCellsPerBlob * kCellBytes;   // 256 KiB: the 128 cells of one blob
constexpr size_t kProofsPerBlob = kCellsPerBlob;
constexpr size_t kProofChunk = kMaxChunk / kProofsPerBlob;               // 8 blobs = one launch set of 1024 MSMs
constexpr size_t kCellsChunk = kMaxChunk / 2;                            // two transforms (and 256 KiB of scratch) per blob in 1024 slots
constexpr size_t kHostSlice = 64;                                        // blobs per upload / download of the host-pointer forms
static_assert(kProofChunk * kProofsPerBlob == kMaxChunk, "a chunk of blobs fills a launch set");

static_assert(kColumnsMaxChunk == kMaxChunk && kColumnsPerBlob == kProofsPerBlob && kColumnsCellsChunk == kCellsChunk &&
                  kColumnsFk20ChunkBlobs == kFk20ChunkBlobs && kColumnsMinSlice == kHostSlice,
              "cells_columns_plan.h plans in the pipeline's sizes");

inline size_t min_sz(size_t a, size_t b) { return a < b ? a : b; }

inline C_KZG_RET bad_input(int mode) { return mode_rules(mode).bad; }

// The columns a call wants: c of the 128, by default all of them -- the full calls, which reach the kernels, the
// chunks and the launches they always had. pair_scratch: the step that makes the coefficients keeps two workspace slots per blob for
// itself (the recovery)
struct ColumnsUse {
    CellColumns cols;
    uint32_t c = (uint32_t)kProofsPerBlob;
    bool pair_scratch = false;
    bool all() const { return c == kProofsPerBlob; }
};
// the list of a column call as its entry point got it (num_columns in 1 .. 128, every index below 128, strictly ascending) into u;
// false with the error text set: C_KZG_BADARGS in every mode, before any device work
bool columns_from_list(ColumnsUse &u, const uint64_t *columns, size_t num_columns, const char *call);
// what cells_columns_plan.h is asked for this call (the caller holds the context's lock, under which the engine is switched)
ColumnsCall columns_call(const Ctx *c, const ColumnsUse &u, bool cells, bool proofs);

// The device pipeline of n blobs on st, a chunk at a time (cells_columns_plan.h; the full calls: 8 blobs with proofs, 512 without); the
// caller holds the context's lock and the workspace. coefficients(off, m, stt) enqueues the step that leaves the coefficients of blobs
// off .. off + m in ws.scalars and a rejection code in stt[0 .. m) (cleared before). status: n words, 0 or the mode's rejection code;
// nullptr: ws.status takes them.
// n_call: the blobs of the whole call this is a part of (a host-pointer call comes in slices): with the settings' FK20 engine on and
// n_call at or above its threshold (n_call c >= 128 min_blobs) the proofs take that engine, in chunks of kFk20ChunkBlobs.
// use: the wanted columns; the outputs are compact, use.c cells and proofs per blob
typedef std::function<void(size_t off, size_t m, int32_t *stt)> CoefficientStep;
C_KZG_RET cells_chunks(Ctx *c, uint8_t *cells_out, uint8_t *proofs48, size_t n, int mode, hipStream_t st, int32_t *status,
                       const CoefficientStep &coefficients, size_t n_call, const ColumnsUse &use = ColumnsUse());

// Host pointers: slices of blobs go up, through run (the device pipeline of the m blobs from blob off on) and back; the outputs are
// written only when every blob is good. A full call's slice is kHostSlice blobs; a column call (use given: use->c cells and proofs per
// blob, compact) takes the plan's slice. in_end (n + 1 entries): blob b's input is bytes in_end[b] .. in_end[b + 1] of `in`, so a
// slice's upload may be ragged. no_memory takes the staging's byte count, rejected the first bad blob's index and status word
typedef std::function<C_KZG_RET(uint8_t *d_cells, uint8_t *d_proofs, const uint8_t *d_in, size_t off, size_t m, hipStream_t st, int32_t *d_status)>
    SliceRunAt;
C_KZG_RET cells_host_slices_ragged(Ctx *c, const uint8_t *in, const size_t *in_end, uint8_t *cells_out, uint8_t *proofs48, size_t n, int mode,
                                   size_t *first_bad, const char *no_memory, const char *rejected, const SliceRunAt &run,
                                   const ColumnsUse *use = nullptr);
// the same with in_bytes_per_blob input bytes for every blob
typedef std::function<C_KZG_RET(uint8_t *d_cells, uint8_t *d_proofs, const uint8_t *d_in, size_t m, hipStream_t st, int32_t *d_status)> SliceRun;
C_KZG_RET cells_host_slices(Ctx *c, const uint8_t *in, size_t in_bytes_per_blob, uint8_t *cells_out, uint8_t *proofs48, size_t n, int mode,
                            size_t *first_bad, const char *no_memory, const char *rejected, const SliceRun &run, const ColumnsUse *use = nullptr);

}  // namespace lwk
