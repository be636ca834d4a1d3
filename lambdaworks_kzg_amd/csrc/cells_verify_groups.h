// cells_verify_groups.h -- the launches behind r of a grouped cell proof verification (cells_verify_groups.hip)
// and the buffers they work on (CellgBufs, CellgPin), shared by the synchronous call there and the cell verifier's grouped calls
// (cells_verify_async.hip; section 4r). The launches take device memory, enqueue everything on st and read nothing back.
#pragma once
#include "carve.h"
#include "cell_groups_plan.h"
#include "cells_common.h"
#include "kernels.h"

namespace lwk {

constexpr size_t kGroupUpBytes = kPwWords * sizeof(Fr) + 4;   // per group on its way up: its powers and its flag word
// bytes of the interpolant kernels' scratch (kInterpChunk groups x 128 columns x 64 coefficients = 16 MiB, whatever g)
size_t cellg_colcoef_bytes();

// ---- what a grouped call adds behind r to the buffers of a batch (cellv_bufs.h), out of the caller's Carver: the synchronous call's
// block with the context, a verifier's own. up: a call's g power tables and, right behind them, its g flag words -- one copy up
struct CellgBufs {
    uint8_t *up, *out96, *rli48;
    uint32_t *slice_off;
    GroupSlice *slices;
    G1Xyzz *part;
    int32_t *inf;
    Fr *colcoef;
    const Fr *pw() const { return (const Fr *)up; }
    const uint32_t *gflag(size_t g) const { return (const uint32_t *)(up + g * kPwWords * sizeof(Fr)); }
};
inline void cellg_carve(CellgBufs &b, Carver &cv, size_t gcap, size_t slice_cap) {
    cv.take(b.up, gcap * kGroupUpBytes);
    cv.take(b.slice_off, (3 * gcap + 1) * 4);
    cv.take(b.slices, slice_cap * sizeof(GroupSlice));
    cv.take(b.part, slice_cap * sizeof(G1Xyzz));
    cv.take(b.out96, gcap * 3 * 96);
    cv.take(b.inf, gcap * 3 * 4);
    cv.take(b.rli48, gcap * 48);
    cv.take(b.colcoef, cellg_colcoef_bytes());
}
// the pinned side of the same: powers and flags on their way up (laid out as CellgBufs::up), sums, their flags and RLIs on their way down
struct CellgPin {
    uint8_t *up, *sums, *rli48;
    int32_t *inf;
    Fr *pw() const { return (Fr *)up; }
    uint32_t *gflag(size_t g) const { return (uint32_t *)(up + g * kPwWords * sizeof(Fr)); }
};
inline void cellg_carve_pin(CellgPin &p, Carver &cv, size_t gcap) {
    cv.take(p.up, gcap * kGroupUpBytes);
    cv.take(p.sums, gcap * 3 * 96);
    cv.take(p.inf, gcap * 3 * 4);
    cv.take(p.rli48, gcap * 48);
}

// a_i = r_j^(i - off_j), b_i = a_i c_(k_i) for the items of the groups with gflag[j] == 0; pw: group j's table at 33 j
void launch_cellg_scalars(const Fr *pw, const uint64_t *idx, const Fr *tw_fwd, const uint32_t *item_group, const uint32_t *item_off,
                          const uint32_t *gflag, Fr *a_mont, uint32_t *sc_a, uint32_t *sc_b, size_t n, hipStream_t st);
// every group's interpolant committed: launch_cellv_interpolant (k_cellv_columns / k_cellv_coeffs) a chunk of kInterpChunk groups at a time into the context's MSM
// slots, the engine's MSM a launch set of up to kMaxChunk slots at a time; rli48[48 j]: group j's commitment, compressed. The caller
// holds the context's lock and workspace and has reserved it for min(g, kMaxChunk) slots. colcoef: cellg_colcoef_bytes() of scratch
void launch_cellg_interpolants(Ctx *c, int mode, const uint8_t *cells, const Fr *a_mont, const uint32_t *perm_col, const uint32_t *col_off,
                               const uint32_t *gflag, Fr *colcoef, uint8_t *rli48, int le, size_t g, hipStream_t st);
// the three sums of every group: one workgroup per slice on `workgroups` of them, then the fold. live: nullptr, or where the device
// keeps the number of slices that exist -- workgroups from there on leave at once (a verifier fixes `workgroups` at enqueue, before
// anybody knows the count). out96 / inf: sum 3 j + s in the layout launch_vmsm_reduce leaves
void launch_cellg_sums(const GroupSlice *slices, const uint32_t *slice_off, const uint32_t *gflag, const uint32_t *sc_a, const uint32_t *sc_b,
                       const uint32_t *sc_c, const G1Affine29 *pts_p, const int32_t *kind_p, const G1Affine29 *pts_c, const int32_t *kind_c,
                       G1Xyzz *part, uint8_t *out96, int32_t *inf, size_t workgroups, const uint32_t *live, size_t g, hipStream_t st);

}  // namespace lwk
