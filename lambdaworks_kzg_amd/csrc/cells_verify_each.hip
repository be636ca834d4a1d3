// cells_verify_each.hip -- n independent EIP-7594 cell proof verifications in one call, each with its own answer:
// lwkzg_verify_cell_kzg_proof_each (+ _device) and lwkzg_cell_verify_each_points. DESIGN.md section 4k.
//
// For every item (C_i, k_i, cell_i, pi_i) the answer is what lwkzg_verify_cell_kzg_proof_batch gives for it as a batch of one, whose
// r^0 = 1 leaves   e(C - [I(tau)]G + [c_k]pi, G2) e(-pi, g2_values[64]) == 1,   I the interpolant of the cell on its coset.
// Every step runs on the GPU, on one stream, under the context's lock:
//   validation  both point sets, n long and index-aligned, through the two-set launches of the batch verifications; one status word
//               per item, nothing stops at a bad item
//   commit      k_celleach_commit, one wave per item: the index and the range check, the cell's 64-point inverse transform in LDS
//               (cell_interp.cuh), lane t's [I[t]]S_t over the endomorphism split (cell_each.cuh; S_t: monomial setup point t) and a
//               six-level tree over the 64 partial points -- the 64-term commitment [I(tau)]G of the item
//   combine     k_celleach_combine, one lane per item: P = C - [I(tau)]G + [c_k]pi, affine, with -pi, as the blob call's records
//   pairing     k_each_pairing (verify_each.hip) against the line tables of g2_values[0] and [64], made once per context
// The verdicts and status words come back in one copy each; the host maps a status to the batch of one's code.
#include "abi_guard.h"
#include "carve.h"
#include "cells_common.h"
#include "each.h"
#include "cell_interp.cuh"
#include "cell_each.cuh"

#include <string.h>

#include <vector>

namespace lwk {

namespace {

// the status word of an item whose index is not below 128: no C_KZG_RET, so that the host can answer C_KZG_BADARGS for it in both modes
constexpr int32_t kStatusBadIndex = 0x100;

// One wave (one workgroup) per item, lane t = element t of its cell = coefficient t of its interpolant = setup point t.
// status[i] comes in as the validation left it (0, or bad_code where a point is bad). An index that is not below 128 is decided first
// and overrides it; nothing is indexed by k before that. An element that is not below r sets bad_code. Every exit is taken by the
// whole wave. isum[i] = [I_i(tau)]G for every item whose status is still 0 at the end.
__global__ __launch_bounds__(64) void k_celleach_commit(const uint4 *__restrict__ cells, const uint64_t *__restrict__ idx,
                                                        const Fr *__restrict__ tw_inv, const G1Affine *__restrict__ setup, Fp beta,
                                                        int32_t *__restrict__ status, int bad_code, int le, G1Xyzz *__restrict__ isum) {
    __shared__ G1Xyzz sh[kCellElems];   // 12 KiB: the tree's points; the transform's 64 elements lie in its first 2 KiB before that
    Fr *buf = (Fr *)sh;
    const uint32_t t = threadIdx.x;
    const size_t i = blockIdx.x;
    const uint64_t k64 = idx[i];
    if (k64 >= (uint64_t)kCellsPerBlob) {
        if (t == 0) status[i] = kStatusBadIndex;
        return;
    }
    if (status[i] != 0) return;
    const uint32_t k = (uint32_t)k64;
    const uint4 *e = cells + ((size_t)i * kCellElems + t) * 2;
    Fr x;
    element_limbs(x.l, e[0], e[1], le);
    if (__any(raw_geq<8>(x.l, FrParams::MOD))) {
        if (t == 0) status[i] = bad_code;
        return;
    }
    buf[t] = x;
    __syncthreads();
#pragma unroll 1
    for (int s = 0; s < 6; s++) {
        if (t < 32) cell_idft64_stage(buf, tw_inv, s, t);
        __syncthreads();
    }
    // I_i[t]: times h_k^-t / 64, a canonical integer
    uint32_t coef[8];
    cell_each_coeff_raw(coef, cell_coeff_scale(tw_inv, k, t), buf[t]);
    __syncthreads();   // buf is read; the tree may write over it
    const G1Affine q = setup[t];
    G1Xyzz acc = glv_mul_affine(q.x, q.y, beta, coef);
    // the 64 partial points summed pairwise by the complete addition (cell_each.cuh)
    cell_each_tree_sum(acc, sh, t);
    if (t == 0) isum[i] = acc;
}

// One lane per item: P_i = C_i - [I_i(tau)]G + [c_k]pi_i, made affine with one inversion, and -pi_i; the flags as k_each_combine sets
// them. An item whose status is not 0 gets flags = 0 and none of its points is read.
__global__ __launch_bounds__(kEachBlock) void k_celleach_combine(const G1Affine29 *__restrict__ pts_c, const int32_t *__restrict__ kind_c,
                                                                 const G1Affine29 *__restrict__ pts_p, const int32_t *__restrict__ kind_p,
                                                                 const int32_t *__restrict__ status, const uint64_t *__restrict__ idx,
                                                                 const Fr *__restrict__ tw_fwd, const G1Xyzz *__restrict__ isum, Fp beta,
                                                                 EachPoints *__restrict__ out, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (status[i] != 0) {
        out[i].flags = 0;
        return;
    }
    const bool has_c = kind_c[i] == 0, has_pi = kind_p[i] == 0;
    Fp pix = Fp::zero(), piy = Fp::zero();
    G1Xyzz acc = G1Xyzz::infinity();
    if (has_pi) {
        pix = f29_to_fp(pts_p[i].x);
        piy = f29_to_fp(pts_p[i].y);
        uint32_t ck[8];
        cell_each_ck_raw(ck, c_of_cell(tw_fwd, (uint32_t)idx[i]));   // (status 0: the index is below 128)
        acc = glv_mul_affine(pix, piy, beta, ck);
    }
    if (has_c) acc = xyzz_madd(acc, f29_to_fp(pts_c[i].x), f29_to_fp(pts_c[i].y));
    G1Xyzz m = isum[i];
    m.y = neg(m.y);
    acc = xyzz_add(acc, m);
    EachPoints e;
    e.flags = kEachValid;
    e.px = e.py = Fp::zero();
    if (!acc.is_inf()) {
        const G1Affine a = xyzz_to_affine(acc);
        e.px = a.x;
        e.py = a.y;
        e.flags |= kEachHasP;
    }
    e.qx = pix;
    e.qy = neg(piy);
    if (has_pi) e.flags |= kEachHasPi;
    out[i] = e;
}

// the device side of a call, carved out of one allocation
struct Bufs {
    uint8_t *cells, *proofs, *comms, *canon_p, *canon_c, *ok;
    uint64_t *idx;
    uint32_t *verdict_p, *verdict_c;
    int32_t *kind_p, *kind_c, *status;
    G1Affine29 *pts_p, *pts_c;
    G1Xyzz *isum;
    EachPoints *pts;
};

size_t carve(Bufs &b, uint8_t *base, size_t cap) {
    Carver cv(base);
    cv.take(b.cells, cap * kCellBytes);
    cv.take(b.proofs, cap * 48);
    cv.take(b.comms, cap * 48);
    cv.take(b.canon_p, cap * 48);
    cv.take(b.canon_c, cap * 48);
    cv.take(b.ok, cap);
    cv.take(b.idx, cap * 8);
    cv.take(b.verdict_p, cap * 4);
    cv.take(b.verdict_c, cap * 4);
    cv.take(b.kind_p, cap * 4);
    cv.take(b.kind_c, cap * 4);
    cv.take(b.status, cap * 4);
    cv.take(b.pts_p, cap * sizeof(G1Affine29));
    cv.take(b.pts_c, cap * sizeof(G1Affine29));
    cv.take(b.isum, cap * sizeof(G1Xyzz));
    cv.take(b.pts, cap * sizeof(EachPoints));
    return cv.bytes();
}

// grow-only, kept with the settings object: first 64 items, then doubling; no allocation in steady state (caller holds c->mu)
C_KZG_RET reserve(Ctx *c, size_t n, Bufs &b) {
    C_KZG_RET rc = grow_reserve(c->celleach, n, 64, [](size_t cap) { Bufs probe; return carve(probe, nullptr, cap); },
                                "verify_cell_kzg_proof_each: no device memory for %zu cells (%zu bytes)");
    if (rc == C_KZG_OK) carve(b, c->celleach.dev, c->celleach.cap);
    return rc;
}

// flag | x 48 | y 48 of an item's P: 0 = affine, 1 = the point at infinity, 2 = the item did not reach the combine
void point_bytes(uint8_t *out97, const EachPoints &e) {
    memset(out97, 0, LWKZG_CELL_EACH_POINT_BYTES);
    if (!(e.flags & kEachValid)) {
        out97[0] = 2;
        return;
    }
    if (!(e.flags & kEachHasP)) {
        out97[0] = 1;
        return;
    }
    uint32_t raw[12];
    fe_to_raw<FpParams>(raw, e.px);
    raw_to_be<12>(out97 + 1, raw);
    fe_to_raw<FpParams>(raw, e.py);
    raw_to_be<12>(out97 + 49, raw);
}

// the verdicts and codes (ok_out, rc_out) or the points of the pairing checks (points_out): one code path up to the pairing. Host
// pointers are uploaded into the context's buffer; device pointers (device_inputs) are read where they are.
C_KZG_RET cell_each_impl(uint8_t *ok_out, int32_t *rc_out, uint8_t *points_out, const void *comms, const void *idx, const void *cells,
                         const void *proofs, size_t n, const KZGSettings *s, bool device_inputs, hipStream_t caller) {
    if (!s) return C_KZG_BADARGS;
    if (n == 0) return C_KZG_OK;
    const bool no_output = points_out ? false : !ok_out || !rc_out;
    if (no_output || !comms || !idx || !cells || !proofs) {
        set_error("verify_cell_kzg_proof_each: NULL argument");
        return C_KZG_BADARGS;
    }
    const int mode = mode_of(s);
    const int le = mode_rules(mode).le();
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    if (!s->g2_values) {
        set_error("KZGSettings.g2_values is NULL");
        return C_KZG_ERROR;
    }
    std::vector<int32_t> status(n);
    std::vector<EachPoints> h_pts(points_out ? n : 0);
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = caller ? caller : c->stream;
    Bufs b;
    C_KZG_RET rc = reserve(c, n, b);
    if (rc != C_KZG_OK) return rc;
    const PairingLine *lines = nullptr;
    if (!points_out && (rc = each_line_tables(s, 64, &c->celleach_lines, &lines)) != C_KZG_OK) return rc;
    StreamDrain drain{st};   // nothing of this call is in flight when it returns, whatever the exit
    const uint8_t *d_comms = (const uint8_t *)comms, *d_cells = (const uint8_t *)cells, *d_proofs = (const uint8_t *)proofs;
    const uint64_t *d_idx = (const uint64_t *)idx;
    if (!device_inputs) {
        LWK_HIP(hipMemcpyAsync(b.comms, comms, 48 * n, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.idx, idx, 8 * n, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.cells, cells, n * kCellBytes, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(b.proofs, proofs, 48 * n, hipMemcpyHostToDevice, st));
        d_comms = b.comms, d_idx = b.idx, d_cells = b.cells, d_proofs = b.proofs;
    }
    LWK_HIP(hipMemsetAsync(b.status, 0, 4 * n, st));
    const int bad = (int)bad_input(mode);
    const PointSet set_p{d_proofs, b.pts_p, b.kind_p, b.canon_p, b.verdict_p}, set_c{d_comms, b.pts_c, b.kind_c, b.canon_c, b.verdict_c};
    launch_decompress_points(set_p, &set_c, n, st);
    launch_subgroup_canon(set_p, &set_c, b.status, bad, n, st, false, true);
    uint32_t braw[12];
    g1_beta_raw(braw);
    const Fp beta = fe_from_raw<FpParams>(braw);
    prof_launch("k_celleach_commit", st, k_celleach_commit, dim3((unsigned)n), dim3(kCellElems), 0, (const uint4 *)d_cells, d_idx,
                (const Fr *)c->tw_inv, (const G1Affine *)c->points, beta, b.status, bad, le, b.isum);
    prof_launch("k_celleach_combine", st, k_celleach_combine, dim3(each_blocks(n)), dim3(kEachBlock), 0, (const G1Affine29 *)b.pts_c,
                (const int32_t *)b.kind_c, (const G1Affine29 *)b.pts_p, (const int32_t *)b.kind_p, (const int32_t *)b.status, d_idx,
                (const Fr *)c->tw_fwd, (const G1Xyzz *)b.isum, beta, b.pts, n);
    LWK_HIP(hipGetLastError());
    if (points_out) {
        LWK_HIP(hipMemcpyAsync(h_pts.data(), b.pts, n * sizeof(EachPoints), hipMemcpyDeviceToHost, st));
    } else {
        launch_each_pairing(b.pts, lines, b.ok, n, st);
        LWK_HIP(hipGetLastError());
        LWK_HIP(hipMemcpyAsync(ok_out, b.ok, n, hipMemcpyDeviceToHost, st));
    }
    LWK_HIP(hipMemcpyAsync(status.data(), b.status, n * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipStreamSynchronize(st));
    if (points_out) {
        for (size_t i = 0; i < n; i++) point_bytes(points_out + (size_t)LWKZG_CELL_EACH_POINT_BYTES * i, h_pts[i]);
        return C_KZG_OK;
    }
    // cells_verify_api.hip: an index that is not below 128 is C_KZG_BADARGS in both modes and decided first; a rejected point or
    // element is the mode's code
    for (size_t i = 0; i < n; i++) {
        if (status[i] == 0) {
            rc_out[i] = C_KZG_OK;
        } else {
            rc_out[i] = status[i] == kStatusBadIndex ? C_KZG_BADARGS : bad_input(mode);
            ok_out[i] = 0;
        }
    }
    return C_KZG_OK;
}

}  // namespace

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_verify_cell_kzg_proof_each(uint8_t *ok_out, int32_t *rc_out, const Bytes48 *commitments, const uint64_t *cell_indices,
                                           const Cell *cells, const Bytes48 *proofs, size_t n, const KZGSettings *s) {
    return guarded("lwkzg_verify_cell_kzg_proof_each", [&] {
        return cell_each_impl(ok_out, rc_out, nullptr, commitments, cell_indices, cells, proofs, n, s, false, nullptr);
    });
}

C_KZG_RET lwkzg_verify_cell_kzg_proof_each_device(uint8_t *ok_out, int32_t *rc_out, const void *commitments48_dev,
                                                  const void *cell_indices_dev, const void *cells_dev, const void *proofs48_dev, size_t n,
                                                  const KZGSettings *s, void *stream) {
    return guarded("lwkzg_verify_cell_kzg_proof_each_device", [&] {
        return cell_each_impl(ok_out, rc_out, nullptr, commitments48_dev, cell_indices_dev, cells_dev, proofs48_dev, n, s, true,
                              (hipStream_t)stream);
    });
}

C_KZG_RET lwkzg_cell_verify_each_points(uint8_t *out, const Bytes48 *commitments, const uint64_t *cell_indices, const Cell *cells,
                                        const Bytes48 *proofs, size_t n, const KZGSettings *s) {
    if (!out && n) return C_KZG_BADARGS;
    return guarded("lwkzg_cell_verify_each_points", [&] {
        return cell_each_impl(nullptr, nullptr, out, commitments, cell_indices, cells, proofs, n, s, false, nullptr);
    });
}

}  // extern "C"
