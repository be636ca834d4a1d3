// cells_columns_plan.h -- how a call that wants c of a blob's 128 columns (lwkzg_compute_cells_and_kzg_proofs_columns*,
// lwkzg_recover_cells_and_kzg_proofs_columns*) is cut up: which engine makes its proofs, how many blobs go
// through the workspace at a time, how many workspace slots that takes and how many blobs a host-pointer call stages at once. The
// full calls are the case c = 128 and come out as they always have: 8 / 512 / 512 blobs per chunk, 128 m or 2 m slots.
// Pure functions, host only and free of HIP: tests/cells_columns_plan_check.cpp walks them under the sanitizers.
#pragma once
#include <stddef.h>

namespace lwk {

constexpr size_t kColumnsMaxChunk = 1024;                      // engine.h: kMaxChunk, the slots of one launch set (static_assert in cells_common.h)
constexpr size_t kColumnsPerBlob = 128;                        // kernels.h: kCellsPerBlob
constexpr size_t kColumnsCellsChunk = kColumnsMaxChunk / 2;    // cells_common.h: kCellsChunk
constexpr size_t kColumnsFk20ChunkBlobs = 512;                 // engine.h: kFk20ChunkBlobs
constexpr size_t kColumnsMinSlice = 64;                        // cells_common.h: kHostSlice, what the full host-pointer calls stage
// What a host-pointer column call may stage on the device at once (input, outputs and status words of one slice): 64 MiB. The full
// calls' 64 blobs stage 24.4 MiB (64 x (128 + 256 + 6) KiB); with c = 8 that many blobs would fill half a launch set of 1024 scalar
// slots, and the upload of a slice does not overlap its compute, so beyond whole launch sets a larger slice buys nothing. 64 MiB holds
// three chunks of 128 blobs at c = 8 and stays a per-call allocation of the size the full calls already make. The bound gives way in
// two places only: a slice is never less than one chunk, and never less than 64 blobs rounded up to whole chunks.
constexpr size_t kColumnsStageBytes = (size_t)64 << 20;

// what the plan is asked about: c columns (1 .. 128), which outputs, whether the step that makes the coefficients needs two workspace
// slots per blob of its own (the recovery: 256 KiB of ws.scalars2 per blob), and the settings' FK20 state
struct ColumnsCall {
    size_t c = kColumnsPerBlob;
    bool cells = true, proofs = true;
    bool pair_scratch = false;
    bool fk20_on = false;
    size_t min_blobs = 0;
};

// Engine: a call of n_call blobs brings n_call c MSMs where the full call brings 128 n_call, and min_blobs was measured as the n at which
// 128 n MSMs cost more than one FK20 pass. c = 128: n_call >= min_blobs, the full calls' rule
inline bool columns_fk20(const ColumnsCall &q, size_t n_call) {
    return q.proofs && q.fk20_on && n_call * q.c >= kColumnsPerBlob * q.min_blobs;
}

// does a blob take two slots of the workspace beside its scalar sets? (the extension's two transforms in ws.fr / ws.scalars2; the
// recovery's scratch)
inline bool columns_pair(const ColumnsCall &q) { return q.cells || q.pair_scratch; }

// Chunk: blobs per pass. MSM path with proofs: the largest m with m c <= 1024 (one launch set of scalar sets in ws.scalars2),
// m <= 1024 (the coefficients in ws.scalars) and 2 m <= 1024 where a blob takes two slots
inline size_t columns_chunk(const ColumnsCall &q, bool fk20) {
    if (fk20) return kColumnsFk20ChunkBlobs;
    if (!q.proofs) return kColumnsCellsChunk;
    size_t m = kColumnsMaxChunk / q.c;   // (c >= 1: m <= 1024)
    if (columns_pair(q) && m > kColumnsMaxChunk / 2) m = kColumnsMaxChunk / 2;
    return m;
}

// Reserve: the slots ctx_reserve is asked for, for a call (or slice) of n blobs: its largest chunk's scalar sets, coefficients and
// pairs of slots
inline size_t columns_reserve(const ColumnsCall &q, bool fk20, size_t n) {
    const size_t chunk = columns_chunk(q, fk20), m = n < chunk ? n : chunk;
    if (fk20 || !q.proofs) return 2 * m;
    const size_t sets = m * q.c, beside = columns_pair(q) ? 2 * m : m;
    return sets > beside ? sets : beside;
}

// Host slice: blobs per upload / download of a host-pointer call of n blobs that stages bytes_per_blob bytes for every blob: whole
// chunks up to kColumnsStageBytes, at least one chunk and at least 64 blobs (in whole chunks), or the whole call
inline size_t columns_host_slice(size_t chunk, size_t bytes_per_blob, size_t n) {
    size_t chunks = kColumnsStageBytes / (chunk * bytes_per_blob);
    if (chunks < 1) chunks = 1;
    if (chunks * chunk < kColumnsMinSlice) chunks = (kColumnsMinSlice + chunk - 1) / chunk;
    return n < chunks * chunk ? n : chunks * chunk;
}

}  // namespace lwk
