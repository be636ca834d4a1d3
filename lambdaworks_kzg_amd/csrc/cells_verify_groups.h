// cells_verify_groups.h -- the launches behind r of a grouped cell proof verification (cells_verify_groups.hip),
// shared by the synchronous call there and the cell verifier's grouped calls (cells_verify_async.hip; section 4r). All pointers are
// device memory, everything is enqueued on st and nothing is read back.
#pragma once
#include "cell_groups_plan.h"
#include "cells_common.h"
#include "kernels.h"

namespace lwk {

constexpr size_t kPwWords = 33;   // Fr slots of a group's power table
// bytes of the interpolant kernels' scratch (kInterpChunk groups x 128 columns x 64 coefficients = 16 MiB, whatever g)
size_t cellg_colcoef_bytes();

// a_i = r_j^(i - off_j), b_i = a_i c_(k_i) for the items of the groups with gflag[j] == 0; pw: group j's table at 33 j
void launch_cellg_scalars(const Fr *pw, const uint64_t *idx, const Fr *tw_fwd, const uint32_t *item_group, const uint32_t *item_off,
                          const uint32_t *gflag, Fr *a_mont, uint32_t *sc_a, uint32_t *sc_b, size_t n, hipStream_t st);
// every group's interpolant committed: k_cellg_columns / k_cellg_coeffs a chunk of kInterpChunk groups at a time into the context's MSM
// slots, the engine's MSM a launch set of up to kMaxChunk slots at a time; rli48[48 j]: group j's commitment, compressed. The caller
// holds the context's lock and workspace and has reserved it for min(g, kMaxChunk) slots. colcoef: cellg_colcoef_bytes()
void launch_cellg_interpolants(Ctx *c, int mode, const uint8_t *cells, const Fr *a_mont, const uint32_t *perm_col, const uint32_t *col_off,
                               const uint32_t *gflag, Fr *colcoef, uint8_t *rli48, int le, size_t g, hipStream_t st);
// the three sums of every group: one workgroup per slice on `workgroups` of them, then the fold. live: nullptr, or where the device
// keeps the number of slices that exist -- workgroups from there on leave at once (a verifier fixes `workgroups` at enqueue, before
// anybody knows the count). out96 / inf: sum 3 j + s in the layout launch_vmsm_reduce leaves
void launch_cellg_sums(const GroupSlice *slices, const uint32_t *slice_off, const uint32_t *gflag, const uint32_t *sc_a, const uint32_t *sc_b,
                       const uint32_t *sc_c, const G1Affine29 *pts_p, const int32_t *kind_p, const G1Affine29 *pts_c, const int32_t *kind_c,
                       G1Xyzz *part, uint8_t *out96, int32_t *inf, size_t workgroups, const uint32_t *live, size_t g, hipStream_t st);

}  // namespace lwk
