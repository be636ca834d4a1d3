// verify_each.hip -- n independent verifications in one call, each with its own answer: lwkzg_verify_blob_kzg_proof_each (+ _device)
// and lwkzg_verify_kzg_proof_each (+ _device) -- n verify_blob_kzg_proof / verify_kzg_proof calls (the reference's src/lib.rs:456-505, 407-453).
//
// Every step runs on the GPU, the pairing included:
//   front    the batch verification's device front for blobs (verify_prepare_device, keep = true: validation of C_i and pi_i, the
//            challenge z_i over the canonical commitment bytes, y_i = p_i(z_i), one status word per item, nothing stops at a bad item);
//            for openings the same validation and k_each_openings (z_i, y_i checked in the mode's byte order)
//   combine  k_each_combine: P_i = C_i - [y_i]G + [z_i]pi_i, affine, for every item whose status is 0 (a bad item's points are not read)
//   pairing  k_each_pairing: e(P_i, G2) e(-pi_i, [tau]G2) == 1 on fp12.cuh's tower, against the line tables of g2_values[0] and [1]
//            made once per context by the host's fixed_q_lines (pairing.hip)
// One lane per item. The verdicts and status words come back in one copy each; the host maps a status to the single call's code.
#include "abi_guard.h"
#include "each.h"
#include "knobs.h"
#include "fp12.cuh"
#include "glv.cuh"

#include <string.h>

#include <vector>

namespace lwk {

void pairing_line_table_host(const Fp2 &qx, const Fp2 &qy, Fp2 *out);  // pairing.hip
static_assert(sizeof(PairingLine) == 2 * sizeof(Fp2), "pairing_line_table_host writes lambda, c0 per line");

namespace {

// 32 bytes of a scalar in the given byte order -> raw limbs; false if not below r (reduced or rejected: the caller's)
__device__ __forceinline__ bool each_scalar(uint32_t raw[8], const uint8_t *b, bool little_endian) {
    if (little_endian) raw_from_le<8>(raw, b);
    else raw_from_be<8>(raw, b);
    return !raw_geq<8>(raw, FrParams::MOD);
}

__global__ void k_each_openings(const uint8_t *z_in, const uint8_t *y_in, uint8_t *z_out, uint8_t *y_out, int32_t *status, int bad_code,
                                int scalar_rule, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool little = scalar_rule == kScalarLeCanonical, canonical = scalar_rule != kScalarBeReduced;   // (mode_rules.h)
    bool ok = true;
    for (int k = 0; k < 2; k++) {
        const uint8_t *in = (k ? y_in : z_in) + 32 * i;
        uint8_t *out = (k ? y_out : z_out) + 32 * i;
        uint32_t raw[8];
        if (!each_scalar(raw, in, little)) {
            if (canonical) {  // c-kzg and eth: a non-canonical element is rejected (verify.hip: fr_from_bytes)
                ok = false;
                continue;
            }
            Fr f = fe_from_raw<FrParams>(raw);  // reference: reduced
            fe_to_raw<FrParams>(raw, f);
        }
        if (little) raw_to_le<8>(out, raw);
        else raw_to_be<8>(out, raw);
    }
    if (!ok) status[i] = bad_code;
}

__global__ void k_each_combine(const G1Affine29 *pts_c, const int32_t *kind_c, const G1Affine29 *pts_p, const int32_t *kind_p,
                               const int32_t *status, const uint8_t *z32, const uint8_t *y32, int le, G1Affine g, Fp beta, EachPoints *out,
                               size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (status[i] != 0) {
        out[i].flags = 0;
        return;
    }
    uint32_t z[8], y[8];
    each_scalar(z, z32 + 32 * i, le != 0);  // (canonical: the front wrote them)
    each_scalar(y, y32 + 32 * i, le != 0);
    const bool has_c = kind_c[i] == 0, has_pi = kind_p[i] == 0;
    Fp pix = Fp::zero(), piy = Fp::zero();
    if (has_pi) {
        pix = f29_to_fp(pts_p[i].x);
        piy = f29_to_fp(pts_p[i].y);
    }
    // [k]Q = [lo]Q + [hi](beta x_Q, -y_Q) for k = lo + hi z^2 < r (glv.cuh): four 128-bit scalars against -G, its image, pi and its image,
    // sharing 128 doublings
    uint32_t ylo[4], yhi[4], zlo[4], zhi[4];
    split_by_z2_barrett(ylo, yhi, y);
    split_by_z2_barrett(zlo, zhi, z);
    const Fp bx[4] = {g.x, beta * g.x, pix, beta * pix};
    const Fp by[4] = {neg(g.y), g.y, piy, neg(piy)};
    G1Xyzz acc = G1Xyzz::infinity();
#pragma unroll 1
    for (int bit = 127; bit >= 0; bit--) {
        acc = xyzz_dbl(acc);
        const uint32_t w = bit >> 5, sh = bit & 31;
        const uint32_t bits[4] = {(ylo[w] >> sh) & 1, (yhi[w] >> sh) & 1, has_pi ? (zlo[w] >> sh) & 1 : 0, has_pi ? (zhi[w] >> sh) & 1 : 0};
#pragma unroll 1
        for (int j = 0; j < 4; j++)
            if (bits[j]) acc = xyzz_madd(acc, bx[j], by[j]);
    }
    if (has_c) acc = xyzz_madd(acc, f29_to_fp(pts_c[i].x), f29_to_fp(pts_c[i].y));
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

__global__ void k_each_pairing(const EachPoints *pts, const PairingLine *lines, uint8_t *ok, size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const EachPoints e = pts[i];
    if (!(e.flags & kEachValid)) {
        ok[i] = 0;
        return;
    }
    ok[i] = pairing2_is_one(e.px, e.py, lines, (e.flags & kEachHasP) != 0, e.qx, e.qy, lines + kPairingLines, (e.flags & kEachHasPi) != 0)
                ? 1
                : 0;
}

// reference blst_fp (canonical, most-significant u64 first) -> Fp
Fp fp_of_blst(const blst_fp &v) {
    uint32_t raw[12];
    for (int k = 0; k < 6; k++) {
        raw[2 * k] = (uint32_t)v.l[5 - k];
        raw[2 * k + 1] = (uint32_t)(v.l[5 - k] >> 32);
    }
    return fe_from_raw<FpParams>(raw);
}

}  // namespace

// each.h: the line tables of g2_values[0] and [power] on the device, made at the context's first per-item verification of that kind
C_KZG_RET each_line_tables(const KZGSettings *s, int power, void **slot, const PairingLine **out) {
    if (!*slot) {
        std::vector<PairingLine> h(2 * kPairingLines);
        for (int q = 0; q < 2; q++) {
            const g2_t &p = s->g2_values[q ? power : 0];
            const Fp2 qx = {fp_of_blst(p.x.fp[0]), fp_of_blst(p.x.fp[1])}, qy = {fp_of_blst(p.y.fp[0]), fp_of_blst(p.y.fp[1])};
            pairing_line_table_host(qx, qy, (Fp2 *)&h[q * kPairingLines]);
        }
        void *d = nullptr;
        LWK_HIP(hipMalloc(&d, h.size() * sizeof(PairingLine)));
        if (hipMemcpy(d, h.data(), h.size() * sizeof(PairingLine), hipMemcpyHostToDevice) != hipSuccess) {
            hipFree(d);
            set_error("per-item verification: line table upload failed");
            return C_KZG_ERROR;
        }
        *slot = d;
    }
    *out = (const PairingLine *)*slot;
    return C_KZG_OK;
}

void launch_each_pairing(const EachPoints *pts, const PairingLine *lines, uint8_t *ok, size_t n, hipStream_t st) {
    prof_launch("k_each_pairing", st, k_each_pairing, each_blocks(n), kEachBlock, 0, pts, lines, ok, n);
}

namespace {

// inputs already on the device; blobs == nullptr: the openings form (z / y given)
C_KZG_RET verify_each_device(uint8_t *ok_out, int32_t *rc_out, Ctx *ctx, const KZGSettings *s, int mode, const uint8_t *d_blobs,
                             const uint8_t *d_comm, const uint8_t *d_proofs, const uint8_t *d_z, const uint8_t *d_y, size_t n,
                             hipStream_t caller) {
    // the single calls answer C_KZG_ERROR for an item that reaches the pairing when the setup's generator or G2 points are unusable
    // (verify.hip: setup_generator, pairing_verdict)
    G1Affine g;
    g.x = g.y = Fp::zero();
    bool setup_ok = s->g1_values && s->g2_values;
    if (setup_ok) {
        g.x = fp_of_blst(s->g1_values[0].x);
        g.y = fp_of_blst(s->g1_values[0].y);
        setup_ok = g1_on_curve(g);
    }
    VerifyBuffers vb;   // holds the context's verify scratch until the verdicts are back
    C_KZG_RET rc = d_blobs ? verify_prepare_device(ctx, d_blobs, d_comm, d_proofs, n, mode, nullptr, nullptr, nullptr, nullptr, vb, caller,
                                                   nullptr, true)
                           : verify_openings_prepare_device(ctx, d_comm, d_proofs, d_z, d_y, n, mode, vb, caller);
    if (rc != C_KZG_OK) return rc == C_KZG_MALLOC ? rc : C_KZG_ERROR;
    std::vector<int32_t> status(n);
    std::lock_guard<std::mutex> lk(ctx->mu);
    LWK_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const PairingLine *lines = nullptr;
    if (setup_ok) {
        if ((rc = each_line_tables(s, 1, &ctx->each_lines, &lines)) != C_KZG_OK) return rc;
        // per-item points and verdicts, grow-only: 64 items at first use, then doubling
        if ((rc = grow_reserve(ctx->each, n, 64, [](size_t cap) { return cap * (sizeof(EachPoints) + 1); },
                               "per-item verification: no device memory for %zu items")) != C_KZG_OK)
            return rc;
        EachPoints *pts = (EachPoints *)ctx->each.dev;
        uint8_t *d_ok = ctx->each.dev + ctx->each.cap * sizeof(EachPoints);
        uint32_t braw[12];
        g1_beta_raw(braw);
        const Fp beta = fe_from_raw<FpParams>(braw);
        k_each_combine<<<each_blocks(n), kEachBlock, 0, st>>>(vb.pts_c, vb.kind_c, vb.pts_p, vb.kind_p, vb.status_all, vb.d_rz, vb.d_r,
                                                             mode_rules(mode).le(), g, beta, pts, n);
        LWK_HIP(hipGetLastError());
        launch_each_pairing(pts, lines, d_ok, n, st);
        LWK_HIP(hipGetLastError());
        LWK_HIP(hipMemcpyAsync(ok_out, d_ok, n, hipMemcpyDeviceToHost, st));
    }
    LWK_HIP(hipMemcpyAsync(status.data(), vb.status_all, n * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipStreamSynchronize(st));
    // verify.hip: a rejected input is bad(mode) in c-kzg mode (the status word holds that code, or the blob parser's) and C_KZG_ERROR in
    // reference mode
    for (size_t i = 0; i < n; i++) {
        if (status[i] != 0) {
            rc_out[i] = mode_rules(mode).bad == C_KZG_ERROR ? C_KZG_ERROR : status[i];
            ok_out[i] = 0;
        } else if (!setup_ok) {
            rc_out[i] = C_KZG_ERROR;
            ok_out[i] = 0;
        } else {
            rc_out[i] = C_KZG_OK;
        }
    }
    return C_KZG_OK;
}

// host inputs: up to the device in one allocation, then the device path
C_KZG_RET verify_each_host(uint8_t *ok_out, int32_t *rc_out, Ctx *ctx, const KZGSettings *s, int mode, const uint8_t *blobs,
                           const uint8_t *comms, const uint8_t *proofs, const uint8_t *zs, const uint8_t *ys, size_t n) {
    const size_t blob_bytes = blobs ? n * (size_t)kBlobBytes : 0, sc_bytes = blobs ? 0 : 32 * n;
    const size_t total = blob_bytes + 96 * n + 2 * sc_bytes;
    uint8_t *d = nullptr;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        LWK_HIP(hipSetDevice(ctx->device));
    }
    if (hipMalloc((void **)&d, total) != hipSuccess) {
        (void)hipGetLastError();
        set_error("per-item verification: no device memory for %zu bytes of inputs", total);
        return C_KZG_MALLOC;
    }
    DevBlock block{d};
    uint8_t *d_blobs = blobs ? d : nullptr, *d_comm = d + blob_bytes, *d_proofs = d_comm + 48 * n;
    uint8_t *d_z = blobs ? nullptr : d_proofs + 48 * n, *d_y = blobs ? nullptr : d_z + 32 * n;
    LWK_HIP(hipMemcpy(d_comm, comms, 48 * n, hipMemcpyHostToDevice));
    LWK_HIP(hipMemcpy(d_proofs, proofs, 48 * n, hipMemcpyHostToDevice));
    if (blobs) {
        LWK_HIP(hipMemcpy(d_blobs, blobs, blob_bytes, hipMemcpyHostToDevice));
    } else {
        LWK_HIP(hipMemcpy(d_z, zs, 32 * n, hipMemcpyHostToDevice));
        LWK_HIP(hipMemcpy(d_y, ys, 32 * n, hipMemcpyHostToDevice));
    }
    return verify_each_device(ok_out, rc_out, ctx, s, mode, d_blobs, d_comm, d_proofs, d_z, d_y, n, nullptr);
}

}  // namespace

void launch_each_openings(const uint8_t *z_in, const uint8_t *y_in, uint8_t *z_out, uint8_t *y_out, int32_t *status, int bad_code,
                          int scalar_rule, size_t n, hipStream_t st) {
    k_each_openings<<<each_blocks(n), kEachBlock, 0, st>>>(z_in, y_in, z_out, y_out, status, bad_code, scalar_rule, n);
}

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_verify_blob_kzg_proof_each(uint8_t *ok_out, int32_t *rc_out, const Blob *blobs, const Bytes48 *commitments,
                                           const Bytes48 *proofs, size_t n, const KZGSettings *s) {
    return guarded("lwkzg_verify_blob_kzg_proof_each", [&]() -> C_KZG_RET {
        if (!ok_out || !rc_out || !s) return C_KZG_BADARGS;
        if (n == 0) return C_KZG_OK;
        if (!blobs || !commitments || !proofs) return C_KZG_BADARGS;
        Ctx *ctx = ctx_of(s);
        if (!ctx) return C_KZG_ERROR;
        return verify_each_host(ok_out, rc_out, ctx, s, mode_of(s), (const uint8_t *)blobs, (const uint8_t *)commitments,
                                (const uint8_t *)proofs, nullptr, nullptr, n);
    });
}

C_KZG_RET lwkzg_verify_blob_kzg_proof_each_device(uint8_t *ok_out, int32_t *rc_out, const void *blobs_dev, const void *commitments48_dev,
                                                  const void *proofs48_dev, size_t n, const KZGSettings *s, void *stream) {
    return guarded("lwkzg_verify_blob_kzg_proof_each_device", [&]() -> C_KZG_RET {
        if (!ok_out || !rc_out || !s) return C_KZG_BADARGS;
        if (n == 0) return C_KZG_OK;
        if (!blobs_dev || !commitments48_dev || !proofs48_dev) return C_KZG_BADARGS;
        Ctx *ctx = ctx_of(s);
        if (!ctx) return C_KZG_ERROR;
        return verify_each_device(ok_out, rc_out, ctx, s, mode_of(s), (const uint8_t *)blobs_dev, (const uint8_t *)commitments48_dev,
                                  (const uint8_t *)proofs48_dev, nullptr, nullptr, n, (hipStream_t)stream);
    });
}

C_KZG_RET lwkzg_verify_kzg_proof_each(uint8_t *ok_out, int32_t *rc_out, const Bytes48 *commitments, const Bytes32 *zs, const Bytes32 *ys,
                                      const Bytes48 *proofs, size_t n, const KZGSettings *s) {
    return guarded("lwkzg_verify_kzg_proof_each", [&]() -> C_KZG_RET {
        if (!ok_out || !rc_out || !s) return C_KZG_BADARGS;
        if (n == 0) return C_KZG_OK;
        if (!commitments || !zs || !ys || !proofs) return C_KZG_BADARGS;
        Ctx *ctx = ctx_of(s);
        if (!ctx) return C_KZG_ERROR;
        return verify_each_host(ok_out, rc_out, ctx, s, mode_of(s), nullptr, (const uint8_t *)commitments, (const uint8_t *)proofs,
                                (const uint8_t *)zs, (const uint8_t *)ys, n);
    });
}

C_KZG_RET lwkzg_verify_kzg_proof_each_device(uint8_t *ok_out, int32_t *rc_out, const void *commitments48_dev, const void *zs32_dev,
                                             const void *ys32_dev, const void *proofs48_dev, size_t n, const KZGSettings *s, void *stream) {
    return guarded("lwkzg_verify_kzg_proof_each_device", [&]() -> C_KZG_RET {
        if (!ok_out || !rc_out || !s) return C_KZG_BADARGS;
        if (n == 0) return C_KZG_OK;
        if (!commitments48_dev || !zs32_dev || !ys32_dev || !proofs48_dev) return C_KZG_BADARGS;
        Ctx *ctx = ctx_of(s);
        if (!ctx) return C_KZG_ERROR;
        return verify_each_device(ok_out, rc_out, ctx, s, mode_of(s), nullptr, (const uint8_t *)commitments48_dev, (const uint8_t *)proofs48_dev,
                                  (const uint8_t *)zs32_dev, (const uint8_t *)ys32_dev, n, (hipStream_t)stream);
    });
}

// test hook (host only): the 68 lines of Q's Miller loop as the device takes them, canonical big-endian lambda.c0 | lambda.c1 | c0.c0 |
// c0.c1 per line (68 x 192 bytes)
C_KZG_RET lwkzg_pairing_line_table(uint8_t *out, const uint8_t *g2_compressed) {
    if (!out || !g2_compressed) return C_KZG_BADARGS;
    Fp2 x, y;
    bool inf = false;
    if (!g2_decompress(x, y, inf, g2_compressed) || inf) return C_KZG_BADARGS;
    std::vector<PairingLine> t(kPairingLines);
    pairing_line_table_host(x, y, (Fp2 *)t.data());
    for (int k = 0; k < kPairingLines; k++) {
        const Fp v[4] = {t[k].lambda.c0, t[k].lambda.c1, t[k].c0.c0, t[k].c0.c1};
        for (int j = 0; j < 4; j++) {
            uint32_t raw[12];
            fe_to_raw<FpParams>(raw, v[j]);
            raw_to_be<12>(out + 192 * k + 48 * j, raw);
        }
    }
    return C_KZG_OK;
}

}  // extern "C"
