// device_api.hip -- the device-resident C ABI: the reserve calls and every lwkzg_*_device compute entry point (device pointers in and out,
// asynchronous on the caller's stream).
#include "abi_guard.h"
#include "async_verifier.h"

#include <string.h>

using namespace lwk;

// The entry points whose call may run on the settings' second context (pick_ctx): the settings' context and mode, the Lagrange form
// where the mode wants it, the context for this caller stream -- locked, its device selected, the workspace taken on the call's stream
// (the caller's, or the context's own) -- and body(Ctx *, int mode, hipStream_t) inside the ABI's guard: the proof pipelines size host
// vectors by their arguments.
template <class F>
static C_KZG_RET on_picked_ctx(const char *what, const KZGSettings *s, void *stream, F &&body) {
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    const int mode = mode_of(s);
    ensure_lagrange(c, mode);
    c = pick_ctx(c, (hipStream_t)stream);
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    WsUse wsu(c, st);
    return guarded(what, [&] { return body(c, mode, st); });
}

extern "C" {

// ------------------------------------------------------------------------------------------------
// device-resident entry points

// everything a device-resident call of up to max_batch blobs would otherwise allocate or synchronise for on first use: the workspace,
// the pinned staging of the host-assisted challenge paths (once, at its final size), and -- for settings that answer in c-kzg mode --
// the Lagrange form of the setup
static C_KZG_RET reserve_ctx(Ctx *c, size_t max_batch) {
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    C_KZG_RET rc = ctx_reserve(c, max_batch);
    if (rc != C_KZG_OK) return rc;
    const size_t host_n = max_batch < mid_proof_host_limit() ? max_batch : mid_proof_host_limit();
    const size_t small_n = max_batch < small_proof_host_limit() ? max_batch : small_proof_host_limit();
    if (host_n || small_n) {
        if (sph_reserve(c, host_n > small_n ? host_n : small_n, true)) {   // (no pinned memory: the calls take the GPU hash)
            SmallProofHost &h = c->sph;   // first touches of the staging happen here, not in the first call
            memset(h.blobs, 0, h.cap * (size_t)kBlobBytes);
            memset(h.dig, 0, h.cap * 32);
        }
        host_pool_warm();   // the host threads exist and have run once
        // the runtime's own first-use costs of a host function on each helper stream (its callback machinery: the first host-assisted
        // call of a process took ~6 ms longer than the second, gpurun_out r05/gpu23) are paid here too
        for (hipStream_t hs : {c->aux[0], c->aux[1], c->vstream}) stream_warm_host_fn(hs);
    }
    // a caller that announces batches of more than a chunk gets the device-side double buffer of the long host-pointer batches now (256 MiB)
    // instead of inside its first long call; the twin context never runs host-pointer batches
    if (max_batch > kMaxChunk && !c->is_twin) {
        (void)dev_stage_ready(c);
        (void)upload_stream(c);   // (the high-priority stream their uploads run on)
    }
    return C_KZG_OK;
}

C_KZG_RET lwkzg_reserve(const KZGSettings *s, size_t max_batch) {
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    ensure_lagrange(c, mode_of(s));
    C_KZG_RET rc = reserve_ctx(c, max_batch);
    if (rc == C_KZG_OK) c->reserved.store(true, std::memory_order_release);
    return rc;
}

// the same for a caller that will issue device-resident calls on `caller_streams` streams at once: with two or more the
// settings' second context (own streams and workspace over the same tables, pick_ctx) is created and reserved HERE -- workspace and
// pinned staging both --, so that the first overlapped call neither allocates nor synchronises the device
C_KZG_RET lwkzg_reserve_streams(const KZGSettings *s, size_t max_batch, int caller_streams) {
    C_KZG_RET rc = lwkzg_reserve(s, max_batch);
    if (rc != C_KZG_OK || caller_streams < 2 || twin_off()) return rc;  // LWKZG_TWIN=0: pick_ctx never uses a twin
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    Ctx *t = nullptr;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        t = c->twin.load(std::memory_order_acquire);
        if (!t) {
            if ((rc = ctx_new(&t, c)) != C_KZG_OK) return rc;
            c->twin.store(t, std::memory_order_release);
        }
    }
    return reserve_ctx(t, max_batch);
}

C_KZG_RET lwkzg_blob_to_kzg_commitment_batch_device(void *out48_dev, const void *blobs_dev, size_t n, const KZGSettings *s,
                                                    void *stream, int32_t *status_dev) {
    return on_picked_ctx("lwkzg_blob_to_kzg_commitment_batch_device", s, stream, [&](Ctx *c, int mode, hipStream_t st) {
        return commit_batch_device(c, (uint8_t *)out48_dev, (const uint8_t *)blobs_dev, n, mode, st, status_dev);
    });
}

C_KZG_RET lwkzg_compute_blob_kzg_proof_batch_device(void *out48_dev, const void *blobs_dev, const void *commitments48_dev,
                                                    size_t n, const KZGSettings *s, void *stream, int32_t *status_dev) {
    return on_picked_ctx("lwkzg_compute_blob_kzg_proof_batch_device", s, stream, [&](Ctx *c, int mode, hipStream_t st) {
        return blob_proof_batch_device(c, (uint8_t *)out48_dev, (const uint8_t *)blobs_dev, (const uint8_t *)commitments48_dev,
                                       n, mode, st, status_dev);
    });
}

C_KZG_RET lwkzg_commit_and_prove_batch_device(void *commitments48_dev, void *proofs48_dev, const void *blobs_dev, size_t n,
                                              const KZGSettings *s, void *stream, int32_t *status_dev) {
    if (!commitments48_dev || !proofs48_dev || !blobs_dev) return map_rc(C_KZG_BADARGS, mode_of(s));
    if (n == 0) return ctx_of(s) ? C_KZG_OK : C_KZG_ERROR;   // (settings that are no settings fail an empty call too)
    return on_picked_ctx("lwkzg_commit_and_prove_batch_device", s, stream, [&](Ctx *c, int mode, hipStream_t st) {
        return commit_and_prove_batch_device(c, (uint8_t *)commitments48_dev, (uint8_t *)proofs48_dev, (const uint8_t *)blobs_dev, n,
                                             mode, st, status_dev);
    });
}

// z_i = compute_challenge(blob_i, commitment_i) (src/utils.rs:120-154) for device-resident blobs, as 32 bytes in the
// mode's byte order (canonical, reduced mod r): the Fiat-Shamir kernel of the proof path, exposed so that a test can
// put its output next to hashlib's at any batch size. The commitment bytes are hashed as given (the proof path
// hashes the canonical re-compression; for canonical inputs the two are the same bytes).
C_KZG_RET lwkzg_compute_challenges_device(void *z32_dev, const void *blobs_dev, const void *commitments48_dev, size_t n,
                                          const KZGSettings *s, void *stream) {
    if (!z32_dev || !blobs_dev || !commitments48_dev) return C_KZG_BADARGS;
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    WsUse wsu(c, st);
    C_KZG_RET rc = ctx_reserve(c, n);
    if (rc != C_KZG_OK) return rc;
    CallWords cw;
    if ((rc = call_words(c, n, nullptr, cw)) != C_KZG_OK) return rc;
    const ModeRules mr = mode_rules(mode_of(s));
    const int le = mr.le();
    Fr *z = cw.z;
    launch_challenge((const uint8_t *)blobs_dev, (const uint8_t *)commitments48_dev, z, mr.hash_rule(), n, st);
    launch_fr_mont_to_bytes(z, (uint8_t *)z32_dev, le, n, st);
    return C_KZG_OK;
}

C_KZG_RET lwkzg_g1_lincomb_setup_device(void *out48_dev, const void *scalars_be_dev, size_t n_msm, const KZGSettings *s,
                                        void *stream) {
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    WsUse wsu(c, st);
    C_KZG_RET rc = ctx_reserve(c, n_msm);
    if (rc != C_KZG_OK) return rc;
    for (size_t off = 0; off < n_msm; off += kMaxChunk) {
        size_t m = n_msm - off < kMaxChunk ? n_msm - off : kMaxChunk;
        launch_parse_be_reduce((const uint8_t *)scalars_be_dev + off * (size_t)kBlobBytes, c->ws.scalars, m * kBlobElems, st);
        msm_scalars_raw_device(c, (uint8_t *)out48_dev + 48 * off, c->ws.scalars, m, st);
    }
    return C_KZG_OK;
}

// sum_k s_k * g1[k mod 4096] for n_terms = tiles * 4096 scalars (BASELINE config "2^20-point MSM, tiled
// trusted setup"): one 4096-term fixed-base MSM per tile, then one sum of the tile results.
C_KZG_RET lwkzg_g1_msm_tiled_device(void *out48_dev, const void *scalars_be_dev, size_t n_terms, const KZGSettings *s,
                                    void *stream) {
    if (n_terms == 0 || n_terms % kBlobElems != 0) {
        set_error("lwkzg_g1_msm_tiled_device: n_terms must be a positive multiple of 4096");
        return C_KZG_BADARGS;
    }
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    WsUse wsu(c, st);
    const size_t tiles = n_terms / kBlobElems;
    C_KZG_RET rc = ctx_reserve(c, tiles);
    if (rc != C_KZG_OK) return rc;
    Workspace &w = c->ws;
    G1Xyzz29 *total = w.sums + w.cap;  // the extra slot behind the per-tile sums
    for (size_t off = 0; off < tiles; off += kMaxChunk) {
        size_t m = tiles - off < kMaxChunk ? tiles - off : kMaxChunk;
        launch_parse_be_reduce((const uint8_t *)scalars_be_dev + off * (size_t)kBlobBytes, w.scalars, m * kBlobElems, st);
        launch_sum_points(msm_sums_stage(c, w.scalars, m, st), m, total, off != 0, st);
    }
    launch_finalize_compress(total, (uint8_t *)out48_dev, 1, st);
    return C_KZG_OK;
}

C_KZG_RET lwkzg_fr_ntt4096_device(void *out_dev, const void *in_dev, size_t n, int inverse, const KZGSettings *s,
                                  void *stream) {
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    WsUse wsu(c, st);
    C_KZG_RET rc = ctx_reserve(c, n);
    if (rc != C_KZG_OK) return rc;
    Workspace &w = c->ws;
    for (size_t off = 0; off < n; off += kMaxChunk) {
        size_t m = n - off < kMaxChunk ? n - off : kMaxChunk;
        const uint8_t *src = (const uint8_t *)in_dev + off * (size_t)kBlobBytes;
        uint8_t *dst = (uint8_t *)out_dev + off * (size_t)kBlobBytes;
        launch_fr_be_to_mont(src, (Fr *)w.scalars2, m * kBlobElems, st);
        launch_bitrev_permute((const Fr *)w.scalars2, w.fr, m, st);  // natural order in -> DIT wants bit-reversed
        if (inverse) {
            launch_ntt4096(w.fr, (Fr *)w.scalars, c->tw28_inv, 1, m, st);  // scaled by 4096^-1, canonical limbs out
            launch_raw_to_be(w.scalars, dst, m * kBlobElems, st);
        } else {
            launch_ntt4096(w.fr, (Fr *)w.scalars2, c->tw28_fwd, 0, m, st);
            launch_fr_mont_to_be((const Fr *)w.scalars2, dst, m * kBlobElems, st);
        }
    }
    return C_KZG_OK;
}

}  // extern "C"
