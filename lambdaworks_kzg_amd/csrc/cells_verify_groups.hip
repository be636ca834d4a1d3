// cells_verify_groups.hip -- EIP-7594 cell proof verification with one answer per GROUP of items (a column sidecar, a transaction's
// blobs): lwkzg_verify_cell_kzg_proof_groups (+ _device) and lwkzg_cell_verify_groups_partials. DESIGN.md section 4q.
//
// Group j's answer is by definition lwkzg_verify_cell_kzg_proof_batch on its items alone: its own de-duplication and row numbers, its
// own transcript header, its own r. One call, one stream, two host visits, under the context's lock:
//   host     the plan (cell_groups_plan.h): offsets checked, every range grouped by the batch call's rule, the slice table
//   device   the batch call's own launches over all n items at once: digests with the group-local rows, both point sets validated
//            (the groups' distinct commitments one after the other, padded with infinity encodings to n); digests, status and kinds
//            come down
//   host     every group's fault; g transcripts and g power tables on the host threads
//   device   k_cellg_scalars (a_i = r_j^(i - off_j), b_i = a_i c_(k_i)), the row weights over the concatenated rows, k_cellg_columns /
//            k_cellg_coeffs (the interpolant of every group into one MSM slot per group, a chunk of kInterpChunk groups at a time), the
//            engine's MSM over the slots, k_cellg_slices (one 64-lane workgroup per slice of one sum of one group: a scalar product
//            per lane, the six-level tree of cell_each.cuh) and k_cellg_fold (the slices of a sum); sums and RLIs come down
//   host     cell_batch_finish per live group on the host threads (the pairing does not re-enter them: it forks by SideTask)
// A dead (bad index) or faulty group is flagged before the second device visit and nothing there reads its points or its indices.
#include "abi_guard.h"
#include "cells_verify_groups.h"
#include "cellv_bufs.h"
#include "cell_interp.cuh"
#include "cell_each.cuh"
#include "knobs.h"

#include <string.h>

#include <functional>
#include <vector>

namespace lwk {

void host_parallel_for(size_t n, const std::function<void(size_t)> &fn);  // sha256_host.hip: persistent workers

namespace {

#include "recover_consts.inc"   // w8192^-1 and 1/64 in Montgomery form

static_assert(kPlanSliceTerms == (uint32_t)kCellElems, "a slice is one term per lane of the tree's 64-lane workgroup");
static_assert(sizeof(GroupSlice) == 16, "four words per slice on the device");

// groups per pass of the interpolant kernels: their scratch is kInterpChunk x 128 columns x 64 coefficients = 16 MiB, whatever g
constexpr size_t kInterpChunk = 64;
constexpr size_t kInterpGroupBytes = (size_t)kCellsPerBlob * kCellElems * sizeof(Fr);   // 256 KiB

// ---- behind r: a_i = r_j^(i - off_j), b_i = a_i c_(k_i) for the items of the live groups -------------------------------------------------
// pw: group j's table at 33 j (r_j^(2^k), k < 32, then 1). One lane per item and no barrier: a lane of a flagged group leaves alone, before
// its index is looked at. a_mont / sc_a / sc_b as k_cellv_scalars writes them.
__global__ __launch_bounds__(64) void k_cellg_scalars(const Fr *__restrict__ pw, const uint64_t *__restrict__ idx, const Fr *__restrict__ tw_fwd,
                                                      const uint32_t *__restrict__ item_group, const uint32_t *__restrict__ item_off,
                                                      const uint32_t *__restrict__ gflag, Fr *__restrict__ a_mont, uint32_t *__restrict__ sc_a,
                                                      uint32_t *__restrict__ sc_b, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t j = item_group[i];
    if (gflag[j]) return;
    const Fr *tab = pw + kPwWords * (size_t)j;
    const uint32_t e = i - item_off[j];
    Fr a = tab[32];
#pragma unroll 1
    for (int k = 0; k < 32; k++) {
        if ((e >> k) == 0) break;
        if ((e >> k) & 1u) a = a * tab[k];
    }
    a_mont[i] = a;
    const Fr b = a * c_of_cell(tw_fwd, (uint32_t)idx[i]);
    uint32_t raw[8], lo[4], hi[4];
    fe_to_raw<FrParams>(raw, a);
    split_by_z2_barrett(lo, hi, raw);
#pragma unroll
    for (int q = 0; q < 4; q++) sc_a[8 * (size_t)i + q] = lo[q], sc_a[8 * (size_t)i + 4 + q] = hi[q];
    fe_to_raw<FrParams>(raw, b);
    split_by_z2_barrett(lo, hi, raw);
#pragma unroll
    for (int q = 0; q < 4; q++) sc_b[8 * (size_t)i + q] = lo[q], sc_b[8 * (size_t)i + 4 + q] = hi[q];
}

// ---- behind r: the column sums of k_cellv_columns per (column, group) ----------------------------------------------------------------------
// Workgroup (k, jj): column k of group first + jj, four waves as there. col_off: list 128 j + k of the call. colcoef[(128 jj + k) 64 + t]:
// coefficient t of the column's share of the group's interpolant (zero for a column the group did not sample). A flagged group's
// workgroups leave whole, before their first barrier; k_cellg_coeffs then reads nothing of their scratch.
__global__ __launch_bounds__(256) void k_cellg_columns(const uint4 *__restrict__ cells, const Fr *__restrict__ a_mont,
                                                       const uint32_t *__restrict__ perm_col, const uint32_t *__restrict__ col_off,
                                                       const uint32_t *__restrict__ gflag, const Fr *__restrict__ tw_inv,
                                                       Fr *__restrict__ colcoef, int le, uint32_t first) {
    __shared__ Fr part[4][kCellElems];
    __shared__ Fr buf[kCellElems];
    const uint32_t k = blockIdx.x, jj = blockIdx.y, j = first + jj, t = threadIdx.x & 63u, v = threadIdx.x >> 6;
    if (gflag[j]) return;
    Fr *out = colcoef + ((size_t)kCellsPerBlob * jj + k) * kCellElems;
    const uint32_t lo = col_off[(size_t)kCellsPerBlob * j + k], hi = col_off[(size_t)kCellsPerBlob * j + k + 1];
    if (lo == hi) {   // (the same for the whole workgroup: no barrier is left behind)
        if (v == 0) out[t] = Fr::zero();
        return;
    }
    Fr acc = Fr::zero();
#pragma unroll 1
    for (uint32_t s = lo + v; s < hi; s += 4) {
        const uint32_t i = perm_col[s];
        const uint4 *e = cells + ((size_t)kCellElems * i + t) * 2;
        Fr x;
        element_limbs(x.l, e[0], e[1], le);
        acc = acc + a_mont[i] * x;
    }
    part[v][t] = acc;
    __syncthreads();
    if (v == 0) buf[t] = (part[0][t] + part[1][t]) + (part[2][t] + part[3][t]);
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < 6; s++) {
        if (threadIdx.x < 32) cell_idft64_stage(buf, tw_inv, s, threadIdx.x);
        __syncthreads();
    }
    if (v != 0) return;
    const Fr sc = cell_coeff_twist(tw_inv, k, t, kRecInvOmega8192Mont);   // times h_k^-t / 64 (cell_interp.cuh)
    Fr c;
#pragma unroll
    for (int q = 0; q < 8; q++) c.l[q] = kRecInv64Mont[q];
    out[t] = (sc * c) * buf[t];
}

// scalar t of MSM slot jj (group first + jj): the sum of the 128 columns' coefficient t for t < 64, zero above; all 4096 zero for a
// flagged group (the engine's launch set behind this kernel takes no flag, so its slot is defined either way)
__global__ __launch_bounds__(256) void k_cellg_coeffs(const Fr *__restrict__ colcoef, const uint32_t *__restrict__ gflag, Fr *__restrict__ slots,
                                                      uint32_t first) {
    const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, jj = blockIdx.y;
    Fr acc = Fr::zero();
    if (t < (uint32_t)kCellElems && !gflag[first + jj]) {
        const Fr *cc = colcoef + (size_t)kCellsPerBlob * kCellElems * jj;
#pragma unroll 1
        for (int k = 0; k < kCellsPerBlob; k++) acc = acc + cc[kCellElems * k + t];
    }
    slots[(size_t)kBlobElems * jj + t] = acc;
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
    ProfScope p("k_cellg_scalars", st);
    hipLaunchKernelGGL(k_cellg_scalars, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, pw, idx, tw_fwd, item_group, item_off, gflag, a_mont,
                       sc_a, sc_b, (uint32_t)n);
}

void launch_cellg_interpolants(Ctx *c, int mode, const uint8_t *cells, const Fr *a_mont, const uint32_t *perm_col, const uint32_t *col_off,
                               const uint32_t *gflag, Fr *colcoef, uint8_t *rli48, int le, size_t g, hipStream_t st) {
    for (size_t base = 0; base < g; base += kMaxChunk) {   // a launch set of MSM slots at a time
        const size_t set = min_sz(g - base, kMaxChunk);
        for (size_t off = 0; off < set; off += kInterpChunk) {
            const size_t m = min_sz(set - off, kInterpChunk);
            const uint32_t first = (uint32_t)(base + off);
            {
                ProfScope p("k_cellg_columns", st);
                hipLaunchKernelGGL(k_cellg_columns, dim3(kCellsPerBlob, (unsigned)m), dim3(256), 0, st, (const uint4 *)cells, a_mont, perm_col,
                                   col_off, gflag, (const Fr *)c->tw_inv, colcoef, le, first);
            }
            ProfScope p("k_cellg_coeffs", st);
            hipLaunchKernelGGL(k_cellg_coeffs, dim3(kBlobElems / 256, (unsigned)m), dim3(256), 0, st, (const Fr *)colcoef, gflag,
                               (Fr *)c->ws.scalars2 + (size_t)kBlobElems * off, first);
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
        ProfScope p("k_cellg_slices", st);
        hipLaunchKernelGGL(k_cellg_slices, dim3((unsigned)workgroups), dim3(kCellElems), 0, st, slices, gflag, sc_a, sc_b, sc_c, pts_p, kind_p,
                           pts_c, kind_c, beta, part, live);
    }
    ProfScope p("k_cellg_fold", st);
    hipLaunchKernelGGL(k_cellg_fold, dim3((unsigned)((3 * g + 63) / 64)), dim3(64), 0, st, (const G1Xyzz *)part, slice_off, gflag, out96, inf,
                       (uint32_t)(3 * g));
}

namespace {

// ---- the device side of a call, carved out of one allocation ---------------------------------------------------------------------------------
// cap counts units: a call of n items in g groups needs max(n, g) of them
struct Bufs {
    uint8_t *cells, *proofs, *comm_in, *canon_p, *canon_c, *digests, *out96, *rli48;
    uint64_t *idx;
    uint32_t *rows, *perm_row, *row_off, *perm_col, *col_off, *verdict_p, *verdict_c, *sc_a, *sc_b, *sc_c, *item_group, *item_off, *gflag, *slice_off;
    int32_t *kind_p, *kind_c, *status, *vstatus, *inf;
    G1Affine29 *pts_p, *pts_c;
    GroupSlice *slices;
    G1Xyzz *part;
    Fr *a_mont, *pw, *colcoef;
};

size_t carve(Bufs &b, uint8_t *base, size_t cap) {
    Carver cv(base);
    const size_t slices = plan_max_slices(cap, cap);
    cv.take(b.cells, cap * kCellBytes);
    cv.take(b.proofs, cap * 48);
    cv.take(b.comm_in, cap * 48);
    cv.take(b.canon_p, cap * 48);
    cv.take(b.canon_c, cap * 48);
    cv.take(b.digests, cap * 32);
    cv.take(b.out96, cap * 3 * 96);
    cv.take(b.rli48, cap * 48);
    cv.take(b.idx, cap * 8);
    cv.take(b.rows, cap * 4);
    cv.take(b.perm_row, cap * 4);
    cv.take(b.row_off, (cap + 1) * 4);
    cv.take(b.perm_col, cap * 4);
    cv.take(b.col_off, (cap * kCellsPerBlob + 1) * 4);
    cv.take(b.verdict_p, cap * 4);
    cv.take(b.verdict_c, cap * 4);
    cv.take(b.sc_a, cap * 32);
    cv.take(b.sc_b, cap * 32);
    cv.take(b.sc_c, cap * 32);
    cv.take(b.item_group, cap * 4);
    cv.take(b.item_off, (cap + 1) * 4);
    cv.take(b.gflag, cap * 4);
    cv.take(b.slice_off, (3 * cap + 1) * 4);
    cv.take(b.kind_p, cap * 4);
    cv.take(b.kind_c, cap * 4);
    cv.take(b.status, cap * 4);
    cv.take(b.vstatus, cap * 4);
    cv.take(b.inf, cap * 3 * 4);
    cv.take(b.pts_p, cap * sizeof(G1Affine29));
    cv.take(b.pts_c, cap * sizeof(G1Affine29));
    cv.take(b.slices, slices * sizeof(GroupSlice));
    cv.take(b.part, slices * sizeof(G1Xyzz));
    cv.take(b.a_mont, cap * sizeof(Fr));
    cv.take(b.pw, cap * kPwWords * sizeof(Fr));
    cv.take(b.colcoef, kInterpChunk * kInterpGroupBytes);
    return cv.bytes();
}

// the pinned side: what comes down and goes up, per unit
struct Pin {
    uint8_t *digests, *sums, *rli48;
    int32_t *status, *kind_p, *kind_c, *inf;
    uint32_t *gflag;
    Fr *pw;
};

size_t carve_pin(Pin &p, uint8_t *base, size_t cap) {
    Carver cv(base);
    cv.take(p.digests, cap * 32);
    cv.take(p.sums, cap * 3 * 96);
    cv.take(p.rli48, cap * 48);
    cv.take(p.status, cap * 4);
    cv.take(p.kind_p, cap * 4);
    cv.take(p.kind_c, cap * 4);
    cv.take(p.inf, cap * 3 * 4);
    cv.take(p.gflag, cap * 4);
    cv.take(p.pw, cap * kPwWords * sizeof(Fr));
    return cv.bytes();
}

// grow-only, kept with the settings object: first 256 units, then doubling; no allocation in steady state (caller holds c->mu)
C_KZG_RET reserve(Ctx *c, size_t units, Bufs &b, Pin &p) {
    if (c->cellg.cap < units) {
        size_t bytes = 0;
        C_KZG_RET rc = grow_reserve(c->cellg, units, 256, [&](size_t cap) { Bufs probe; return bytes = carve(probe, nullptr, cap); }, nullptr);
        if (rc == C_KZG_ERROR) return rc;   // the wait failed: both buffers are as they were
        if (c->cellg_pin) hipHostFree(c->cellg_pin);
        c->cellg_pin = nullptr;
        Pin probe;
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
// and the indices, which come down first.
C_KZG_RET cell_groups_impl(uint8_t *ok_out, int32_t *rc_out, uint8_t *partials_out, const void *comms_v, const void *idx_v, const void *cells_v,
                           const void *proofs_v, size_t n, const uint64_t *offsets, size_t g, const KZGSettings *s, bool device_inputs,
                           hipStream_t caller) {
    // the call-level checks: before any device work, and nothing is written
    if (!s) return C_KZG_BADARGS;
    const bool no_output = partials_out ? false : !ok_out || !rc_out;
    if (g > 0 && (no_output || !offsets)) {
        set_error("verify_cell_kzg_proof_groups: NULL argument");
        return C_KZG_BADARGS;
    }
    if (n > 0 && (!comms_v || !idx_v || !cells_v || !proofs_v)) {
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
    auto answer = [&](size_t j, C_KZG_RET rc, bool ok) {
        if (partials_out) return;
        rc_out[j] = rc;
        ok_out[j] = rc == C_KZG_OK && ok ? 1 : 0;
    };
    if (n == 0) {   // empty groups alone: the batch call's answer to n == 0, without a context
        if (partials_out) memset(partials_out, 0, g * (size_t)LWKZG_CELL_VERIFY_PARTIAL_BYTES);
        for (size_t j = 0; j < g; j++) answer(j, C_KZG_OK, true);
        return C_KZG_OK;
    }
    const uint8_t *comms = (const uint8_t *)comms_v, *cells = (const uint8_t *)cells_v, *proofs = (const uint8_t *)proofs_v;
    const uint64_t *idx = (const uint64_t *)idx_v;
    GroupsPlan plan;
    if (!device_inputs) plan_groups(plan, comms, idx, n, offsets, g);
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
        plan_groups(plan, h_comms.data(), h_idx.data(), n, offsets, g);
    }
    const auto t1 = std::chrono::steady_clock::now();
    Bufs b;
    Pin pin;
    C_KZG_RET rc = reserve(c, n > g ? n : g, b, pin);
    if (rc != C_KZG_OK) return rc;
    if ((rc = ctx_reserve(c, g)) != C_KZG_OK) return rc;   // (at most one launch set of slots)
    WsUse wsu(c, st);
    StreamDrain drain{st};   // nothing of this call is in flight when it returns, whatever the exit
    PhaseClock clk;
    clk.begin(st);

    // ---- first visit: the batch call's digests and validation over all n items ----
    LWK_HIP(upload(b.comm_in, plan.distinct, st));
    LWK_HIP(upload(b.rows, plan.rows, st));
    const uint8_t *d_cells = cells, *d_proofs = proofs;
    const uint64_t *d_idx = idx;
    if (!device_inputs) {
        LWK_HIP(hipMemcpyAsync(b.cells, cells, n * kCellBytes, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.proofs, proofs, 48 * n, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.idx, idx, 8 * n, hipMemcpyHostToDevice, st));
        d_cells = b.cells, d_proofs = b.proofs, d_idx = b.idx;
    }
    LWK_HIP(hipMemsetAsync(b.status, 0, 4 * n, st));
    LWK_HIP(hipMemsetAsync(b.vstatus, 0, 4 * n, st));
    clk.mark(0);
    const int bad = (int)bad_input(mode);
    launch_cellv_digests(d_cells, d_proofs, b.rows, d_idx, b.digests, b.status, bad, le, n, st);
    clk.mark(1);
    const PointSet set_p{d_proofs, b.pts_p, b.kind_p, b.canon_p, b.verdict_p}, set_c{b.comm_in, b.pts_c, b.kind_c, b.canon_c, b.verdict_c};
    launch_decompress_points(set_p, &set_c, n, st);
    launch_subgroup_canon(set_p, &set_c, b.vstatus, bad, n, st);   // (its one word per index mixes item i and row i: the kinds tell them apart)
    clk.mark(2);
    LWK_HIP(hipMemcpyAsync(pin.digests, b.digests, 32 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(pin.status, b.status, 4 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(pin.kind_p, b.kind_p, 4 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(pin.kind_c, b.kind_c, 4 * n, hipMemcpyDeviceToHost, st));
    // the lists of the second visit go up beside the first visit's kernels
    LWK_HIP(upload(b.perm_row, plan.perm_row, st));
    LWK_HIP(upload(b.row_off, plan.row_off, st));
    LWK_HIP(upload(b.perm_col, plan.perm_col, st));
    LWK_HIP(upload(b.col_off, plan.col_off, st));
    LWK_HIP(upload(b.item_group, plan.item_group, st));
    LWK_HIP(upload(b.item_off, plan.item_off, st));
    LWK_HIP(upload(b.slice_off, plan.slice_off, st));
    if (!plan.slices.empty())
        LWK_HIP(hipMemcpyAsync(b.slices, plan.slices.data(), plan.slices.size() * sizeof(GroupSlice), hipMemcpyHostToDevice, st));
    LWK_HIP(hipGetLastError());
    LWK_HIP(hipStreamSynchronize(st));
    const auto t2 = std::chrono::steady_clock::now();

    // ---- the host decides every group's fault; a bad commitment counts for the group whose row it is ----
    std::vector<uint8_t> live(g, 0);
    size_t n_live = 0;
    for (size_t j = 0; j < g; j++) {
        const uint32_t lo = plan.item_off[j], hi = plan.item_off[j + 1];
        pin.gflag[j] = 1;
        if (lo == hi) {
            answer(j, C_KZG_OK, true);
            continue;
        }
        if (plan.dead[j]) {
            answer(j, C_KZG_BADARGS, false);
            continue;
        }
        bool fault = false;
        for (uint32_t i = lo; i < hi && !fault; i++) fault = pin.status[i] != 0 || pin.kind_p[i] == 2;
        for (uint32_t q = plan.row_base[j]; q < plan.row_base[j + 1] && !fault; q++) fault = pin.kind_c[q] == 2;
        if (fault) {
            answer(j, bad_input(mode), false);
            continue;
        }
        pin.gflag[j] = 0;
        live[j] = 1;
        n_live++;
    }
    if (n_live == 0) return C_KZG_OK;
    std::vector<uint32_t> r_raw(8 * g, 0);
    host_parallel_for(g, [&](size_t j) {
        if (!live[j]) return;
        const uint32_t lo = plan.item_off[j], cnt = plan.item_off[j + 1] - lo, rb = plan.row_base[j];
        cell_batch_challenge(&r_raw[8 * j], plan.distinct.data() + 48 * (size_t)rb, plan.row_base[j + 1] - rb, pin.digests + 32 * (size_t)lo, cnt, le);
        cell_batch_powers(pin.pw + kPwWords * j, &r_raw[8 * j]);
    });
    const auto t3 = std::chrono::steady_clock::now();

    // ---- second visit ----
    LWK_HIP(hipMemcpyAsync(b.pw, pin.pw, g * kPwWords * sizeof(Fr), hipMemcpyHostToDevice, st));
    LWK_HIP(hipMemcpyAsync(b.gflag, pin.gflag, 4 * g, hipMemcpyHostToDevice, st));
    LWK_HIP(hipMemsetAsync(b.a_mont, 0, n * sizeof(Fr), st));   // (the row weights read whole rows: a flagged group's stay defined)
    clk.mark(3);
    launch_cellg_scalars(b.pw, d_idx, c->tw_fwd, b.item_group, b.item_off, b.gflag, b.a_mont, b.sc_a, b.sc_b, n, st);
    launch_cellv_row_weights(b.a_mont, b.perm_row, b.row_off, b.sc_c, plan.m_total, st);
    clk.mark(4);
    launch_cellg_interpolants(c, mode, d_cells, b.a_mont, b.perm_col, b.col_off, b.gflag, b.colcoef, b.rli48, le, g, st);
    clk.mark(5);
    launch_cellg_sums(b.slices, b.slice_off, b.gflag, b.sc_a, b.sc_b, b.sc_c, b.pts_p, b.kind_p, b.pts_c, b.kind_c, b.part, b.out96, b.inf,
                      plan.slices.size(), nullptr, g, st);
    clk.mark(6);
    LWK_HIP(hipMemcpyAsync(pin.sums, b.out96, 3 * 96 * g, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(pin.inf, b.inf, 3 * 4 * g, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(pin.rli48, b.rli48, 48 * g, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipGetLastError());
    LWK_HIP(hipStreamSynchronize(st));
    const auto t4 = std::chrono::steady_clock::now();

    // ---- the pairing of every live group on the host threads (cell_batch_finish forks by SideTask, never by host_parallel_for) ----
    std::vector<int32_t> frc(g, (int32_t)C_KZG_OK);
    std::vector<uint8_t> fok(g, 0);
    const bool r_le = mode_rules(mode).little_endian;
    host_parallel_for(g, [&](size_t j) {
        if (!live[j]) return;
        uint8_t sums[3][96];
        int infs[3];
        for (int k = 0; k < 3; k++) {
            memcpy(sums[k], pin.sums + 96 * (3 * j + k), 96);
            infs[k] = pin.inf[3 * j + k];
        }
        uint8_t *part = partials_out ? partials_out + (size_t)LWKZG_CELL_VERIFY_PARTIAL_BYTES * j : nullptr;
        if (part) {
            if (r_le) raw_to_le<8>(part, &r_raw[8 * j]);
            else raw_to_be<8>(part, &r_raw[8 * j]);
        }
        bool ok = false;
        frc[j] = (int32_t)cell_batch_finish(partials_out ? nullptr : &ok, part ? part + 32 : nullptr, sums, infs, pin.rli48 + 48 * j, s);
        fok[j] = ok;
    });
    for (size_t j = 0; j < g; j++) {
        if (!live[j]) continue;
        if (frc[j] != (int32_t)C_KZG_OK) {
            set_error("verify_cell_kzg_proof_groups: the interpolant's commitment of group %zu is not a point", j);
            return C_KZG_ERROR;
        }
        answer(j, C_KZG_OK, fok[j] != 0);
    }
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
