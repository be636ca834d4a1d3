// cells_verify_groups.hip -- EIP-7594 cell proof verification with one answer per GROUP of items (a column sidecar, a transaction's
// blobs): lwkzg_verify_cell_kzg_proof_groups (+ _device) and lwkzg_cell_verify_groups_partials. DESIGN.md section 4q.
//
// Group j's answer is by definition lwkzg_verify_cell_kzg_proof_batch on its items alone: its own de-duplication and row numbers, its
// own transcript header, its own r. One call, one stream, two host visits, under the context's lock:
//   host     the plan (cell_groups_plan.h): offsets checked, every range grouped by the batch call's rule, the slice table
//   device   the first visit the cell verifier runs too (cells_verify.hip: launch_cellv_first_visit) over all n items at once: digests
//            with the group-local rows, both point sets validated (the groups' distinct commitments one after the other, padded
//            with infinity encodings to n), the 2 n fault words; digests and fault words come down
//   host     every group's fault; g transcripts and g power tables on the host threads (cells_verify_host.h: groups_decide)
//   device   k_cellg_scalars (a_i = r_j^(i - off_j), b_i = a_i c_(k_i)), the row weights over the concatenated rows, the batch call's
//            k_cellv_columns / k_cellv_coeffs on a grid of (.., groups) (cells_verify.hip: the interpolant of every group into one MSM
//            slot per group, a chunk of kInterpChunk groups at a time), the engine's MSM over the slots, k_cellg_slices (one 64-lane workgroup per slice of one sum of one group: a scalar product
//            per lane, the six-level tree of cell_each.cuh) and k_cellg_fold (the slices of a sum); sums and RLIs come down
//   host     cell_batch_finish per live group on the host threads (the pairing does not re-enter them: it forks by SideTask) and the
//            answers (cells_verify_host.h: groups_answers)
// A dead (bad index) or faulty group is flagged before the second device visit and nothing there reads its points or its indices.
// Both host steps are the cell verifier's (cells_verify_async.hip) on the plan's view of the call, and the tests reach them without a
// GPU (lwkzg_cell_verifier_groups_host_steps). The buffers behind r are CellgBufs / CellgPin (cells_verify_groups.h), the verifier's too.
#include "abi_guard.h"
#include "cells_verify_blobs.h"
#include "cells_verify_groups.h"
#include "cells_verify_host.h"
#include "cellv_bufs.h"
#include "cell_interp.cuh"
#include "cell_each.cuh"
#include "knobs.h"

#include <string.h>

#include <functional>
#include <vector>

namespace lwk {

namespace {

static_assert(kPlanSliceTerms == (uint32_t)kCellElems, "a slice is one term per lane of the tree's 64-lane workgroup");
static_assert(sizeof(GroupSlice) == 16, "four words per slice on the device");

// groups per pass of the interpolant kernels: their scratch is kInterpChunk x 128 columns x 64 coefficients = 16 MiB, whatever g
constexpr size_t kInterpChunk = 64;
constexpr size_t kInterpGroupBytes = (size_t)kCellsPerBlob * kCellElems * sizeof(Fr);   // 256 KiB

// ---- behind r: a_i = r_j^(i - off_j), b_i = a_i c_(k_i) for the items of the live groups -------------------------------------------------
// pw: group j's table at 33 j (r_j^(2^k), k < 32, then 1). One lane per item and no barrier: a lane of a flagged group leaves alone, before
// its index is looked at. a_mont / sc_a / sc_b as k_cellv_scalars writes them, by the same body (cell_interp.cuh: cell_item_scalars).
__global__ __launch_bounds__(64) void k_cellg_scalars(const Fr *__restrict__ pw, const uint64_t *__restrict__ idx, const Fr *__restrict__ tw_fwd,
                                                      const uint32_t *__restrict__ item_group, const uint32_t *__restrict__ item_off,
                                                      const uint32_t *__restrict__ gflag, Fr *__restrict__ a_mont, uint32_t *__restrict__ sc_a,
                                                      uint32_t *__restrict__ sc_b, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = item_group[i];
    if (gflag[j]) return;
    cell_item_scalars(pw + kPwWords * (size_t)j, i - item_off[j], i, idx, tw_fwd, a_mont, sc_a, sc_b);
}

// ---- behind r: the three variable-base sums of every group -------------------------------------------------------------------------------
// One 64-lane workgroup per slice (cell_groups_plan.h): lane t takes term first + t of sum `sum` -- [a_i]pi_i (0), [b_i]pi_i (1) over the
// group's items, [w_q]C_q (2) over its rows -- as a scalar product over the endomorphism split, or the point at infinity where the
// term's kind says so or the slice is short; the 64 points are summed by the tree of complete additions (a repeated item gives equal
// lanes, a cancelling pair opposite ones). part[slice]: the slice's sum. A flagged group's workgroups leave whole, before the barrier.
__global__ __launch_bounds__(64) void k_cellg_slices(const GroupSlice *__restrict__ slices, const uint32_t *__restrict__ gflag,
                                                     const uint32_t *__restrict__ sc_a, const uint32_t *__restrict__ sc_b,
                                                     const uint32_t *__restrict__ sc_c, const G1Affine29 *__restrict__ pts_p,
                                                     const int32_t *__restrict__ kind_p, const G1Affine29 *__restrict__ pts_c,
                                                     const int32_t *__restrict__ kind_c, Fp beta, G1Xyzz *__restrict__ part,
                                                     const uint32_t *__restrict__ live) {
    __shared__ G1Xyzz sh[kCellElems];   // 12 KiB: the tree's points
    const uint32_t t = threadIdx.x;
    if (live && blockIdx.x >= *live) return;   // (a verifier's launch covers the most slices its call can have: section 4r)
    const GroupSlice sl = slices[blockIdx.x];
    if (gflag[sl.group]) return;
    // a lane without a term -- the slice is short, or the term's point is the point at infinity -- multiplies by zero: the product is
    // complete, and every lane runs the same 128 doublings
    Fp px = Fp::zero(), py = Fp::zero();
    uint32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};
    if (t < sl.count) {
        const size_t q = (size_t)sl.first + t;
        const bool comm = sl.sum == 2;
        if ((comm ? kind_c[q] : kind_p[q]) == 0) {
            const G1Affine29 &pt = comm ? pts_c[q] : pts_p[q];
            const uint32_t *sc = (comm ? sc_c : sl.sum == 1 ? sc_b : sc_a) + 8 * q;
            px = f29_to_fp(pt.x), py = f29_to_fp(pt.y);
#pragma unroll
            for (int w = 0; w < 4; w++) lo[w] = sc[w], hi[w] = sc[4 + w];
        }
    }
    G1Xyzz acc = glv_mul_affine_split(px, py, beta, lo, hi);
    cell_each_tree_sum(acc, sh, t);
    if (t == 0) part[blockIdx.x] = acc;
}

// One lane per (group, sum): the slices' sums added by complete additions, then affine big-endian x | y and an infinity flag in the
// layout launch_vmsm_reduce leaves (sum 3 j + s at out96 + 96 (3 j + s)). A flagged group and a sum of no slices give the flag and zeros.
__global__ __launch_bounds__(64) void k_cellg_fold(const G1Xyzz *__restrict__ part, const uint32_t *__restrict__ slice_off,
                                                   const uint32_t *__restrict__ gflag, uint8_t *__restrict__ out96, int32_t *__restrict__ inf,
                                                   uint32_t sums) {
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= sums) return;
    G1Xyzz acc = G1Xyzz::infinity();
    if (!gflag[q / 3]) {
        const uint32_t lo = slice_off[q], hi = slice_off[q + 1];
#pragma unroll 1
        for (uint32_t s = lo; s < hi; s++) acc = xyzz_add(acc, part[s]);
    }
    uint8_t *o = out96 + 96 * (size_t)q;
    if (acc.is_inf()) {
        inf[q] = 1;
        for (int k = 0; k < 96; k++) o[k] = 0;
        return;
    }
    inf[q] = 0;
    const G1Affine a = xyzz_to_affine(acc);
    uint32_t raw[12];
    fe_to_raw<FpParams>(raw, a.x);
    raw_to_be<12>(o, raw);
    fe_to_raw<FpParams>(raw, a.y);
    raw_to_be<12>(o + 48, raw);
}

}  // namespace

// ---- the launches (cells_verify_groups.h) ----------------------------------------------------------------------------------------------------
size_t cellg_colcoef_bytes() { return kInterpChunk * kInterpGroupBytes; }

void launch_cellg_scalars(const Fr *pw, const uint64_t *idx, const Fr *tw_fwd, const uint32_t *item_group, const uint32_t *item_off,
                          const uint32_t *gflag, Fr *a_mont, uint32_t *sc_a, uint32_t *sc_b, size_t n, hipStream_t st) {
    prof_launch("k_cellg_scalars", st, k_cellg_scalars, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, pw, idx, tw_fwd, item_group, item_off, gflag,
                a_mont, sc_a, sc_b, (uint32_t)n);
}

void launch_cellg_interpolants(Ctx *c, int mode, const uint8_t *cells, const Fr *a_mont, const uint32_t *perm_col, const uint32_t *col_off,
                               const uint32_t *gflag, Fr *colcoef, uint8_t *rli48, int le, size_t g, hipStream_t st) {
    for (size_t base = 0; base < g; base += kMaxChunk) {   // a launch set of MSM slots at a time
        const size_t set = min_sz(g - base, kMaxChunk);
        for (size_t off = 0; off < set; off += kInterpChunk) {
            const size_t m = min_sz(set - off, kInterpChunk);
            launch_cellv_interpolant(cells, a_mont, perm_col, col_off, c->tw_inv, colcoef, c->ws.scalars2 + 8 * (size_t)kBlobElems * off, le, st,
                                     gflag, base + off, m);
        }
        const bool lg = coefficients_to_msm_form(c, mode, set, st);
        msm_stages(c, c->ws.scalars2, rli48 + 48 * base, set, st, 0, false, lg);
    }
}

void launch_cellg_sums(const GroupSlice *slices, const uint32_t *slice_off, const uint32_t *gflag, const uint32_t *sc_a, const uint32_t *sc_b,
                       const uint32_t *sc_c, const G1Affine29 *pts_p, const int32_t *kind_p, const G1Affine29 *pts_c, const int32_t *kind_c,
                       G1Xyzz *part, uint8_t *out96, int32_t *inf, size_t workgroups, const uint32_t *live, size_t g, hipStream_t st) {
    uint32_t braw[12];
    g1_beta_raw(braw);
    const Fp beta = fe_from_raw<FpParams>(braw);
    if (workgroups) {
        prof_launch("k_cellg_slices", st, k_cellg_slices, dim3((unsigned)workgroups), dim3(kCellElems), 0, slices, gflag, sc_a, sc_b, sc_c, pts_p,
                    kind_p, pts_c, kind_c, beta, part, live);
    }
    prof_launch("k_cellg_fold", st, k_cellg_fold, dim3((unsigned)((3 * g + 63) / 64)), dim3(64), 0, (const G1Xyzz *)part, slice_off, gflag, out96,
                inf, (uint32_t)(3 * g));
}

namespace {

// ---- the device side of a call, carved out of one allocation ---------------------------------------------------------------------------------
// cap counts units: a call of n items in g groups needs max(n, g) of them. A batch's buffers without what the batch call alone runs
// behind r, a column list per group (cellv_bufs.h); what a grouped call runs there; the plan's two item lists and the fault words
struct DevSide {
    CellvBufs b;      // (carved without the batch call's own: b.out96, rli48, inf, pw, colcoef, tab_*, vm_*, partial, bsum are EMPTY -- gb has a grouped call's)
    CellgBufs gb;
    uint32_t *item_group, *item_off;
    int32_t *fault;   // 2 cap words (k_cellv_fault_words)
};

size_t carve(DevSide &b, uint8_t *base, size_t cap) {
    Carver cv(base);
    cellv_carve(b.b, cv, cap, true, false, cap);
    cellg_carve(b.gb, cv, cap, plan_max_slices(cap, cap));
    cv.take(b.item_group, cap * 4);
    cv.take(b.item_off, (cap + 1) * 4);
    cv.take(b.fault, 2 * cap * 4);
    return cv.bytes();
}

// the pinned side: what comes down and goes up, per unit
struct PinSide {
    CellgPin gp;
    uint8_t *digests;
    int32_t *fault;
};

size_t carve_pin(PinSide &p, uint8_t *base, size_t cap) {
    Carver cv(base);
    cellg_carve_pin(p.gp, cv, cap);
    cv.take(p.digests, cap * 32);
    cv.take(p.fault, 2 * cap * 4);
    return cv.bytes();
}

// grow-only, kept with the settings object: first 256 units, then doubling; no allocation in steady state (caller holds c->mu)
C_KZG_RET reserve(Ctx *c, size_t units, DevSide &b, PinSide &p) {
    if (c->cellg.cap < units) {
        size_t bytes = 0;
        C_KZG_RET rc = grow_reserve(c->cellg, units, 256, [&](size_t cap) { DevSide probe; return bytes = carve(probe, nullptr, cap); }, nullptr);
        if (rc == C_KZG_ERROR) return rc;   // the wait failed: both buffers are as they were
        if (c->cellg_pin) hipHostFree(c->cellg_pin);
        c->cellg_pin = nullptr;
        PinSide probe;
        if (rc == C_KZG_OK && hipHostMalloc((void **)&c->cellg_pin, carve_pin(probe, nullptr, c->cellg.cap)) != hipSuccess) {
            (void)hipGetLastError();
            grow_free(c->cellg);
            rc = C_KZG_MALLOC;
        }
        if (rc != C_KZG_OK) {
            set_error("verify_cell_kzg_proof_groups: no memory for a call of %zu items or groups (%zu bytes on the device)", units, bytes);
            return rc;
        }
    }
    carve(b, c->cellg.dev, c->cellg.cap);
    carve_pin(p, c->cellg_pin, c->cellg.cap);
    return C_KZG_OK;
}

template <class T>
hipError_t upload(T *dst, const std::vector<T> &src, hipStream_t st) {
    return src.empty() ? hipSuccess : hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, st);
}

// the answers (ok_out, rc_out) or the partials (partials_out, LWKZG_CELL_VERIFY_PARTIAL_BYTES per group): one code path up to the pairing.
// Host pointers are uploaded into the context's buffer; device pointers (device_inputs) are read where they are, except the commitments
// and the indices, which come down first. front (cells_verify_blobs.h): the caller makes the items, the lists and the plan itself; the
// four item arrays are not read, and offsets are the items' (checked like anybody's).
C_KZG_RET cell_groups_impl(uint8_t *ok_out, int32_t *rc_out, uint8_t *partials_out, const void *comms_v, const void *idx_v, const void *cells_v,
                           const void *proofs_v, size_t n, const uint64_t *offsets, size_t g, const KZGSettings *s, bool device_inputs,
                           hipStream_t caller, const CellFront *front = nullptr) {
    // the call-level checks: before any device work, and nothing is written
    if (!s) return C_KZG_BADARGS;
    const bool no_output = partials_out ? false : !ok_out || !rc_out;
    if (g > 0 && (no_output || !offsets)) {
        set_error("verify_cell_kzg_proof_groups: NULL argument");
        return C_KZG_BADARGS;
    }
    if (n > 0 && !front && (!comms_v || !idx_v || !cells_v || !proofs_v)) {
        set_error("verify_cell_kzg_proof_groups: NULL argument");
        return C_KZG_BADARGS;
    }
    if (n > (size_t)0x7fffffff || g > (size_t)0x3fffffff || !group_offsets_valid(offsets, g, n)) {
        set_error("verify_cell_kzg_proof_groups: group_offsets must be %zu ascending values from 0 to %zu", g + 1, n);
        return C_KZG_BADARGS;
    }
    if (g == 0) return C_KZG_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const int mode = mode_of(s);
    const int le = mode_rules(mode).le();
    if (n == 0) {   // empty groups alone: the batch call's answer to n == 0, without a context
        if (partials_out) memset(partials_out, 0, g * (size_t)LWKZG_CELL_VERIFY_PARTIAL_BYTES);
        else
            for (size_t j = 0; j < g; j++) rc_out[j] = (int32_t)C_KZG_OK, ok_out[j] = 1;
        return C_KZG_OK;
    }
    const uint8_t *comms = (const uint8_t *)comms_v, *cells = (const uint8_t *)cells_v, *proofs = (const uint8_t *)proofs_v;
    const uint64_t *idx = (const uint64_t *)idx_v;
    GroupsPlan own;
    const GroupsPlan &plan = front ? front->plan : own;
    if (!front && !device_inputs) plan_groups(own, comms, idx, n, offsets, g);
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    if (!s->g2_values) {
        set_error("KZGSettings.g2_values is NULL");
        return C_KZG_ERROR;
    }
    if (partials_out) memset(partials_out, 0, g * (size_t)LWKZG_CELL_VERIFY_PARTIAL_BYTES);
    ensure_lagrange(c, mode);
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = caller ? caller : c->stream;
    if (device_inputs) {
        std::vector<uint8_t> h_comms(48 * n);
        std::vector<uint64_t> h_idx(n);
        LWK_HIP(hipMemcpyAsync(h_comms.data(), comms, 48 * n, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipMemcpyAsync(h_idx.data(), idx, 8 * n, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipStreamSynchronize(st));
        plan_groups(own, h_comms.data(), h_idx.data(), n, offsets, g);
    }
    const auto t1 = std::chrono::steady_clock::now();
    DevSide dev;
    PinSide pin;
    C_KZG_RET rc = reserve(c, n > g ? n : g, dev, pin);
    if (rc != C_KZG_OK) return rc;
    if ((rc = ctx_reserve(c, g)) != C_KZG_OK) return rc;   // (at most one launch set of slots)
    const CellvBufs &b = dev.b;
    const CellgBufs &gb = dev.gb;
    const CellgPin &gp = pin.gp;
    WsUse wsu(c, st);
    StreamDrain drain{st};   // nothing of this call is in flight when it returns, whatever the exit
    PhaseClock clk;
    clk.begin(st);

    // ---- first visit: the batch call's digests and validation over all n items ----
    if (!front) {
        LWK_HIP(upload(b.comm_in, plan.distinct, st));
        LWK_HIP(upload(b.rows, plan.rows, st));
    }
    const uint8_t *d_cells = cells, *d_proofs = proofs;
    const uint64_t *d_idx = idx;
    if (front) {   // every list of the call at once, in front of the first visit
        const CellFrontGroupLists gl{dev.item_group, dev.item_off, gb.slice_off, gb.slices};
        if ((rc = front->items(c, st, b, &gl, d_cells, d_proofs)) != C_KZG_OK) return rc;
        d_idx = b.idx;
    } else if (!device_inputs) {
        LWK_HIP(hipMemcpyAsync(b.cells, cells, n * kCellBytes, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.proofs, proofs, 48 * n, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.idx, idx, 8 * n, hipMemcpyHostToDevice, st));
        d_cells = b.cells, d_proofs = b.proofs, d_idx = b.idx;
    }
    clk.mark(0);
    const PointSet set_p{d_proofs, b.pts_p, b.kind_p, b.canon_p, b.verdict_p}, set_c{b.comm_in, b.pts_c, b.kind_c, b.canon_c, b.verdict_c};
    LWK_HIP(launch_cellv_first_visit(d_cells, d_idx, b.rows, set_p, set_c, b.digests, dev.fault, b.status, (int)bad_input(mode), le, n, st,
                                     clk.on ? clk.ev[1] : nullptr));
    if (front) front->fold_status(dev.fault, (int)bad_input(mode), st);
    clk.mark(2);
    LWK_HIP(hipMemcpyAsync(pin.digests, b.digests, 32 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(pin.fault, dev.fault, 8 * n, hipMemcpyDeviceToHost, st));
    if (!front) {   // the lists of the second visit go up beside the first visit's kernels
        LWK_HIP(upload(b.perm_row, plan.perm_row, st));
        LWK_HIP(upload(b.row_off, plan.row_off, st));
        LWK_HIP(upload(b.perm_col, plan.perm_col, st));
        LWK_HIP(upload(b.col_off, plan.col_off, st));
        LWK_HIP(upload(dev.item_group, plan.item_group, st));
        LWK_HIP(upload(dev.item_off, plan.item_off, st));
        LWK_HIP(upload(gb.slice_off, plan.slice_off, st));
        if (!plan.slices.empty())
            LWK_HIP(hipMemcpyAsync(gb.slices, plan.slices.data(), plan.slices.size() * sizeof(GroupSlice), hipMemcpyHostToDevice, st));
    }
    LWK_HIP(hipGetLastError());
    LWK_HIP(hipStreamSynchronize(st));
    const auto t2 = std::chrono::steady_clock::now();

    // ---- the host decides every group's fault, then g transcripts and g power tables (cells_verify_host.h: the verifier's step 1 on the
    // plan's view of the call; nobody asks where in a group the fault is, so there is no first_item) ----
    std::vector<int32_t> grc(g);
    std::vector<uint32_t> r_raw(8 * g, 0);
    uint32_t *flags = gp.gflag(g);
    groups_decide(grc.data(), r_raw.data(), gp.pw(), flags, plan.item_off.data(), g, n, plan.row_base.data(), plan.dead.data(), pin.fault, nullptr,
                  pin.digests, plan.distinct.data(), mode);
    size_t n_live = 0;
    for (size_t j = 0; j < g; j++) n_live += flags[j] == 0;
    const auto t3 = std::chrono::steady_clock::now();

    // ---- second visit: never enqueued when no group is live ----
    if (n_live != 0) {
        LWK_HIP(hipMemcpyAsync(gb.up, gp.up, g * kGroupUpBytes, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemsetAsync(b.a_mont, 0, n * sizeof(Fr), st));   // (the row weights read whole rows: a flagged group's stay defined)
        clk.mark(3);
        launch_cellg_scalars(gb.pw(), d_idx, c->tw_fwd, dev.item_group, dev.item_off, gb.gflag(g), b.a_mont, b.sc_a, b.sc_b, n, st);
        launch_cellv_row_weights(b.a_mont, b.perm_row, b.row_off, b.sc_c, plan.m_total, st);
        clk.mark(4);
        launch_cellg_interpolants(c, mode, d_cells, b.a_mont, b.perm_col, b.col_off, gb.gflag(g), gb.colcoef, gb.rli48, le, g, st);
        clk.mark(5);
        launch_cellg_sums(gb.slices, gb.slice_off, gb.gflag(g), b.sc_a, b.sc_b, b.sc_c, b.pts_p, b.kind_p, b.pts_c, b.kind_c, gb.part, gb.out96,
                          gb.inf, plan.slices.size(), nullptr, g, st);
        clk.mark(6);
        LWK_HIP(hipMemcpyAsync(gp.sums, gb.out96, 3 * 96 * g, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipMemcpyAsync(gp.inf, gb.inf, 3 * 4 * g, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipMemcpyAsync(gp.rli48, gb.rli48, 48 * g, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipGetLastError());
        LWK_HIP(hipStreamSynchronize(st));
    }
    const auto t4 = std::chrono::steady_clock::now();

    // ---- the pairing of every live group on the host threads, against the caller's settings, and the answers (the verifier's step 2).
    // A call without a live group comes here too, for its flagged groups' answers and zero partials; every group's answer is written
    // before a failed finish makes the call C_KZG_ERROR ----
    groups_answers(ok_out, rc_out, partials_out, grc.data(), r_raw.data(), flags, plan.item_off.data(), g, s, mode,
                   [&](size_t j, uint8_t sums[3][96], int infs[3], uint8_t rli48[48]) {
                       sums_from_pinned(sums, infs, gp.sums + 3 * 96 * j, (const uint8_t *)(gp.inf + 3 * j));
                       memcpy(rli48, gp.rli48 + 48 * j, 48);
                       return true;
                   });
    for (size_t j = 0; j < g; j++)
        if (!flags[j] && grc[j] != (int32_t)C_KZG_OK) {
            set_error("verify_cell_kzg_proof_groups: the interpolant's commitment of group %zu is not a point", j);
            return C_KZG_ERROR;
        }
    if (n_live == 0) return C_KZG_OK;   // (no second visit, so no timing line)
    if (clk.on)
        fprintf(stderr, "[lambdaworks_kzg_amd] verify cell groups n=%zu g=%zu rows=%zu slices=%zu live=%zu: host plan %.3f ms | device: digests %.3f, "
                        "validation %.3f, scalars + row weights %.3f, interpolants + MSM %.3f, slices + fold %.3f ms | host: until the first "
                        "visit landed %.3f, transcripts + powers %.3f, second visit %.3f, pairings %.3f, total %.3f ms\n",
                n, g, plan.m_total, plan.slices.size(), n_live, wall_ms(t0, t1), clk.ms(0, 1), clk.ms(1, 2), clk.ms(3, 4), clk.ms(4, 5), clk.ms(5, 6),
                wall_ms(t1, t2), wall_ms(t2, t3), wall_ms(t3, t4), wall_ms(t4, std::chrono::steady_clock::now()),
                wall_ms(t0, std::chrono::steady_clock::now()));
    return C_KZG_OK;
}

}  // namespace

// cells_verify_blobs.h
C_KZG_RET cell_groups_front(uint8_t *ok_out, int32_t *rc_out, uint8_t *partials_out, size_t n, const uint64_t *item_offsets, size_t g,
                            const KZGSettings *s, hipStream_t caller, const CellFront &front) {
    return cell_groups_impl(ok_out, rc_out, partials_out, nullptr, nullptr, nullptr, nullptr, n, item_offsets, g, s, false, caller, &front);
}

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_verify_cell_kzg_proof_groups(uint8_t *ok_out, int32_t *rc_out, const Bytes48 *commitments, const uint64_t *cell_indices,
                                             const Cell *cells, const Bytes48 *proofs, size_t n, const uint64_t *group_offsets, size_t g,
                                             const KZGSettings *s) {
    return guarded("lwkzg_verify_cell_kzg_proof_groups", [&] {
        return cell_groups_impl(ok_out, rc_out, nullptr, commitments, cell_indices, cells, proofs, n, group_offsets, g, s, false, nullptr);
    });
}

C_KZG_RET lwkzg_verify_cell_kzg_proof_groups_device(uint8_t *ok_out, int32_t *rc_out, const void *commitments48_dev,
                                                    const void *cell_indices_dev, const void *cells_dev, const void *proofs48_dev, size_t n,
                                                    const uint64_t *group_offsets, size_t g, const KZGSettings *s, void *stream) {
    return guarded("lwkzg_verify_cell_kzg_proof_groups_device", [&] {
        return cell_groups_impl(ok_out, rc_out, nullptr, commitments48_dev, cell_indices_dev, cells_dev, proofs48_dev, n, group_offsets, g, s,
                                true, (hipStream_t)stream);
    });
}

C_KZG_RET lwkzg_cell_verify_groups_partials(uint8_t *out, const Bytes48 *commitments, const uint64_t *cell_indices, const Cell *cells,
                                            const Bytes48 *proofs, size_t n, const uint64_t *group_offsets, size_t g, const KZGSettings *s) {
    if (!out && g) return C_KZG_BADARGS;
    return guarded("lwkzg_cell_verify_groups_partials", [&] {
        return cell_groups_impl(nullptr, nullptr, out, commitments, cell_indices, cells, proofs, n, group_offsets, g, s, false, nullptr);
    });
}

}  // extern "C"
