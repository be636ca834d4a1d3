// verify_openings.hip -- batch verification of n openings (C_i, z_i, y_i, pi_i) with one pairing check: the consensus specs'
// verify_kzg_proof_batch, the inner function of the reference's blob batch (src/lib.rs:639-692). DESIGN.md section 4p.
//
// Every piece behind the front is the blob batch's own (verify.hip: the transcript's challenge, vmsm.hip's three sums, sum r^i y_i, the
// host pairing). This file has the one kernel an opening needs in place of the blob hash and the evaluation -- k_opening_records -- and
// the C entry points of the synchronous forms; the front is verify_front.hip's verify_openings_front_device, the call from begin to
// verdict verify.hip's verify_openings_batch_full, the form that does not block verify_async.hip's lwkzg_verifier_enqueue_openings.
#include "abi_guard.h"
#include "engine.h"

#include <string.h>

namespace lwk {

namespace {

constexpr int kOpeningBlock = 64;   // one wave per workgroup: 4096 openings spread over 64 compute units

// 32 bytes of a caller's scalar, as two 16-byte words, by the mode's rule (mode_rules.h) -> its canonical bytes in the same byte order.
// false: not below r where the rule rejects that (the bytes pass through; the record of a rejected item is never hashed)
__device__ __forceinline__ bool opening_scalar(uint4 out[2], const uint4 *in, bool little, bool canonical) {
    const uint4 a = in[0], b = in[1];
    const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    uint32_t raw[8];
#pragma unroll
    for (int k = 0; k < 8; k++) raw[k] = little ? w[k] : __builtin_bswap32(w[7 - k]);
    out[0] = a;
    out[1] = b;
    if (!raw_geq<8>(raw, FrParams::MOD)) return true;   // canonical already: the caller's bytes are the record's
    if (canonical) return false;                         // c-kzg and eth: rejected (verify.hip: fr_from_bytes)
    const Fr f = fe_from_raw<FrParams>(raw);             // reference: reduced
    fe_to_raw<FrParams>(raw, f);
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = little ? raw[k] : __builtin_bswap32(raw[7 - k]);
    out[0] = make_uint4(v[0], v[1], v[2], v[3]);
    out[1] = make_uint4(v[4], v[5], v[6], v[7]);
    return true;
}

// One lane per opening: k_each_openings (z_i, y_i by the mode's rule, canonical bytes where k_vmsm_scalars and k_verify_ysum read
// them) and k_verify_records (the 160-byte record, the lowest rejected index) in one launch, every access a 16-byte one. z_out / y_out
// may be z_in / y_in: a lane has read its item before it writes it. A rejected item's point bytes are whatever the validation left;
// its record is never hashed, because the call is decided by first_bad first.
__global__ __launch_bounds__(kOpeningBlock) void k_opening_records(const uint4 *z_in, const uint4 *y_in, const uint4 *__restrict__ canon_c,
                                                                   const uint4 *__restrict__ canon_p, uint4 *z_out, uint4 *y_out,
                                                                   int32_t *__restrict__ status, int bad_code, int scalar_rule,
                                                                   uint4 *__restrict__ records, uint32_t *__restrict__ first_bad, uint32_t n) {
    const uint32_t i = blockIdx.x * kOpeningBlock + threadIdx.x;
    if (i >= n) return;
    const bool little = scalar_rule == kScalarLeCanonical, canonical = scalar_rule != kScalarBeReduced;
    uint4 z[2], y[2];
    const bool z_ok = opening_scalar(z, z_in + 2 * (size_t)i, little, canonical);
    const bool y_ok = opening_scalar(y, y_in + 2 * (size_t)i, little, canonical);
    z_out[2 * (size_t)i] = z[0];
    z_out[2 * (size_t)i + 1] = z[1];
    y_out[2 * (size_t)i] = y[0];
    y_out[2 * (size_t)i + 1] = y[1];
    const uint4 *c = canon_c + 3 * (size_t)i, *p = canon_p + 3 * (size_t)i;
    uint4 *rec = records + 10 * (size_t)i;
    rec[0] = c[0];
    rec[1] = c[1];
    rec[2] = c[2];
    rec[3] = z[0];
    rec[4] = z[1];
    rec[5] = y[0];
    rec[6] = y[1];
    rec[7] = p[0];
    rec[8] = p[1];
    rec[9] = p[2];
    bool rejected = status[i] != 0;   // the validation's verdict on C_i or pi_i
    if (!(z_ok && y_ok)) {
        status[i] = bad_code;
        rejected = true;
    }
    if (rejected) atomicMin(first_bad, i);
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

// what the three synchronous forms decide before any device work; *done: the call is answered
C_KZG_RET openings_entry(bool *done, bool *ok, const void *comm, const void *z, const void *y, const void *proofs, size_t n,
                         const KZGSettings *s, int mode, bool device_inputs) {
    *done = true;
    if (n == 0) {   // verify.hip: verify_batch_impl -- the reference answers OK with ok = false, c-kzg-4844 and the specs accept the empty batch
        if (ok) *ok = mode_rules(mode).empty_ok;
        return C_KZG_OK;
    }
    if (!comm || !z || !y || !proofs || !s) return mode_rules(mode).bad;
    if (device_inputs && !(aligned16(comm) && aligned16(z) && aligned16(y) && aligned16(proofs))) {
        set_error("openings batch: the device pointers must be 16-byte aligned");
        return C_KZG_BADARGS;
    }
    *done = false;
    return C_KZG_OK;
}

}  // namespace

void launch_opening_records(const uint8_t *z_in, const uint8_t *y_in, const uint8_t *canon_c, const uint8_t *canon_p, uint8_t *z_out,
                            uint8_t *y_out, int32_t *status, int bad_code, int scalar_rule, uint8_t *records, uint32_t *first_bad, size_t n,
                            hipStream_t st) {
    prof_launch("k_opening_records", st, k_opening_records, dim3((unsigned)((n + kOpeningBlock - 1) / kOpeningBlock)), dim3(kOpeningBlock), 0,
                (const uint4 *)z_in, (const uint4 *)y_in, (const uint4 *)canon_c, (const uint4 *)canon_p, (uint4 *)z_out, (uint4 *)y_out, status,
                bad_code, scalar_rule, (uint4 *)records, first_bad, (uint32_t)n);
}

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_verify_kzg_proof_batch(bool *ok, const Bytes48 *commitments, const Bytes32 *zs, const Bytes32 *ys, const Bytes48 *proofs,
                                       size_t n, const KZGSettings *s) {
    if (ok) *ok = false;
    return guarded("lwkzg_verify_kzg_proof_batch", [&]() -> C_KZG_RET {
        if (!ok) return C_KZG_BADARGS;
        const int mode = mode_of(s);
        bool done;
        const C_KZG_RET rc = openings_entry(&done, ok, commitments, zs, ys, proofs, n, s, mode, false);
        if (done) return rc;
        return verify_openings_batch_full(ok, nullptr, nullptr, (const uint8_t *)commitments, (const uint8_t *)zs, (const uint8_t *)ys,
                                          (const uint8_t *)proofs, n, s, mode, false, nullptr);
    });
}

C_KZG_RET lwkzg_verify_kzg_proof_batch_device(bool *ok, const void *commitments48_dev, const void *zs32_dev, const void *ys32_dev,
                                              const void *proofs48_dev, size_t n, const KZGSettings *s, void *stream) {
    if (ok) *ok = false;
    return guarded("lwkzg_verify_kzg_proof_batch_device", [&]() -> C_KZG_RET {
        if (!ok) return C_KZG_BADARGS;
        const int mode = mode_of(s);
        bool done;
        const C_KZG_RET rc = openings_entry(&done, ok, commitments48_dev, zs32_dev, ys32_dev, proofs48_dev, n, s, mode, true);
        if (done) return rc;
        return verify_openings_batch_full(ok, nullptr, nullptr, (const uint8_t *)commitments48_dev, (const uint8_t *)zs32_dev,
                                          (const uint8_t *)ys32_dev, (const uint8_t *)proofs48_dev, n, s, mode, true, (hipStream_t)stream);
    });
}

C_KZG_RET lwkzg_verify_kzg_proof_batch_partial(uint8_t r_out[32], uint8_t partial_out[LWKZG_VERIFY_PARTIAL_BYTES], const Bytes48 *commitments,
                                               const Bytes32 *zs, const Bytes32 *ys, const Bytes48 *proofs, size_t n, const KZGSettings *s) {
    return guarded("lwkzg_verify_kzg_proof_batch_partial", [&]() -> C_KZG_RET {
        if (!r_out || !partial_out) return C_KZG_BADARGS;
        const int mode = mode_of(s);
        bool done;
        const C_KZG_RET rc = openings_entry(&done, nullptr, commitments, zs, ys, proofs, n, s, mode, false);
        if (done) return rc;
        return verify_openings_batch_full(nullptr, r_out, partial_out, (const uint8_t *)commitments, (const uint8_t *)zs, (const uint8_t *)ys,
                                          (const uint8_t *)proofs, n, s, mode, false, nullptr);
    });
}

}  // extern "C"
