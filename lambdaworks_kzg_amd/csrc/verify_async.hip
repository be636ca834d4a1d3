// verify_async.hip -- lwkzg_verifier_*: lwkzg_verify_blob_kzg_proof_batch_device without a parked host thread.
//
// The synchronous call stops its thread twice: behind the transcript's copy (the host hashes it into r) and behind the copy of the
// three sums (the host multiplies the generator and runs the pairing). Here both pieces of host work are HOST FUNCTIONS in stream
// order (hipLaunchHostFunc, as proof_calls.hip's small_proof_host_fn), the one O(n) piece of it -- sum r^i y_i, a serial walk over n powers
// on the host -- is a kernel (k_verify_ysum), and the verdict lands in a LwkzgVerifyResult whose state word is stored last:
//
//   caller's stream --event--> context stream: per-blob pass, k_verify_records, transcript -> h_rec, status words -> h_status
//                              HOST FUNCTION 1: first_bad; r = SHA-256(transcript); 33 powers (or the skip word) -> h_pin
//                              h_pin -> vm_pw, skip word
//                              k_vmsm_scalars, k_vmsm_accumulate, k_vmsm_bucket_sums, k_vmsm_weighted   |  side stream: k_verify_ysum
//                              the three sums, their flags, sum r^i y_i -> h_pin
//                              HOST FUNCTION 2: [sum r^i y_i]G, pairing, partial -> *result, state = 1 (release), slot freed
//   caller's stream <--event-- (work enqueued behind the call sees the verdict)
//
// lwkzg_verifier_enqueue_openings is the same call for n openings (C, z, y, pi): verify_openings_front_device in place of the per-blob
// pass and k_verify_records, everything from host function 1 on unchanged.
//
// Calls on one verifier share its VerifyBuffers and run one after the other: on one context by stream order, across the settings' two
// contexts (pick_ctx) by the verifier's last_done event. The job slots and their hand-over are verifier_ring.h; what this verifier
// shares with the cells' (cells_verify_async.hip) -- the handle's head, the enqueue around enqueue_on, pending / wait / free -- is
// async_verifier.h.
#include "abi_guard.h"
#include "async_verifier.h"
#include "verify_ysum.cuh"

#include <new>

namespace lwk {

// ---- sum r^i y_i on the device -----------------------------------------------------------------------------------------------------
// A latency kernel like its neighbours in vmsm.hip: ONE workgroup of kYsumLanes lanes, lane t owns the terms i = t (mod T), a tree in
// LDS at the end, no atomics. The arithmetic and its bounds are verify_ysum.cuh's.
__global__ __launch_bounds__(kYsumLanes) void k_verify_ysum(const uint8_t *__restrict__ y32, int le, const Fr *__restrict__ pw,
                                                            uint8_t *__restrict__ out32, uint32_t n, const uint32_t *__restrict__ skip) {
    __shared__ Fr28 tab[33];
    __shared__ Fr28 part[kYsumLanes];
    if (skip && *skip) return;  // a rejected batch: its y bytes are not a transcript's (the whole workgroup, before its first barrier)
    const uint32_t t = threadIdx.x;
    if (t < 33) tab[t] = fr28_from_mont256(pw[t]);
    __syncthreads();
    part[t] = ysum_lane(tab, y32, le, t, n);
    __syncthreads();
    for (int d = kYsumLanes / 2; d >= 1; d >>= 1) {
        if (t < (uint32_t)d) part[t] = ysum_add(part[t], part[t + d]);
        __syncthreads();
    }
    if (t == 0) ysum_bytes(out32, part[0]);
}

void launch_verify_ysum(const uint8_t *y32, int le, const Fr *pw, uint8_t *out32, size_t n, hipStream_t st, const uint32_t *skip) {
    prof_launch("k_verify_ysum", st, k_verify_ysum, dim3(1), dim3(kYsumLanes), 0, y32, le, pw, out32, (uint32_t)n, skip);
}

// ---- the verifier --------------------------------------------------------------------------------------------------------------------
namespace {

constexpr uint64_t kVerifierMagic = 0x4c574b5a56524659ull;  // "LWKZVRFY"

struct Verifier : AsyncVerifier {
    VerifyBuffers vb;              // owned: device scratch, h_rec, h_pin
    int32_t *h_status = nullptr;   // hipHostMalloc, cap words: the status words beside the transcript (the rejected input's code)
    hipEvent_t ev_fork = nullptr, ev_ysum = nullptr;
    // the generator and the two G2 points of the settings, copied at creation: all the host functions ever see of them
    g1_t generator;
    g2_t g2[2];
    KZGSettings own;
    Verifier(Ctx *c, const KZGSettings *s, size_t max_blobs) : AsyncVerifier(kVerifierMagic, c, s, max_blobs) {}
    void free_own() {
        verify_buffers_free(vb);
        if (h_status) (void)hipHostFree(h_status);
        for (hipEvent_t e : {ev_fork, ev_ysum})
            if (e) (void)hipEventDestroy(e);
    }
};

// ---- the two host functions (their rules: async_verifier.h) ------------------------------------------------------------------------

// behind the transcript's copy: first_bad, r, the 33 powers (or the skip word) into the pinned block
void verifier_host_fn1(void *p) {
    AsyncJob *j = (AsyncJob *)p;
    Verifier *v = static_cast<Verifier *>(j->v);
    uint32_t skip = 1;
    try {
        memcpy(&j->first_bad, v->vb.h_rec + LWKZG_VERIFY_RECORD_BYTES * j->n, 4);
        if (j->first_bad == kNoneBad) {
            Fr pw[33];
            verify_async_challenge(((LwkzgVerifyResult *)j->res)->r, pw, v->vb.h_rec, j->n, j->mode);
            memcpy(v->vb.h_pin, pw, sizeof pw);
            skip = 0;
        } else if (j->first_bad < j->n) {
            j->code = v->h_status[j->first_bad];
        } else {
            j->failed = true;
        }
    } catch (...) {
        j->failed = true;
    }
    memcpy(v->vb.h_pin + kVmsmPinSkip, &skip, 4);
}

// behind the copy of the three sums and of sum r^i y_i: [sum r^i y_i]G, the pairing, the partial; the state word last; the slot freed
void verifier_host_fn2(void *p) {
    AsyncJob *j = (AsyncJob *)p;
    Verifier *v = static_cast<Verifier *>(j->v);
    LwkzgVerifyResult *res = (LwkzgVerifyResult *)j->res;
    C_KZG_RET rc = C_KZG_ERROR;
    bool ok = false;
    try {
        if (j->failed) {
            rc = C_KZG_ERROR;
        } else if (j->first_bad != kNoneBad) {   // as verify_prepare_device and shard_begin answer a rejected input
            rc = mode_rules(j->mode).bad == C_KZG_ERROR || j->code != kStatusBadArgs ? C_KZG_ERROR : C_KZG_BADARGS;
        } else {
            const uint8_t *pin = v->vb.h_pin;
            uint8_t sums[3][96];
            int infs[3];
            sums_from_pinned(sums, infs, pin + kVmsmPinSums, pin + kVmsmPinInfs);
            rc = verify_async_verdict(&ok, res->partial, sums, infs, pin + kVmsmPinYsum, &v->own);
        }
    } catch (...) {
        rc = C_KZG_ERROR;
    }
    res->first_bad = j->first_bad;
    complete_now(res, rc, ok && rc == C_KZG_OK);
    v->ring.release(j);   // (the verifier may be gone as soon as this returns)
}

// the workspace a call of n blobs on context c takes, as verify_front_device reserves it
C_KZG_RET reserve_for(Ctx *c, size_t n) {
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    C_KZG_RET rc = ctx_reserve(c, n < kMaxChunk ? n : kMaxChunk);
    if (rc != C_KZG_OK) return rc;
    CallWords cw;
    if ((rc = call_words(c, n, nullptr, cw)) != C_KZG_OK) return rc;
    stream_warm_host_fn(c->stream);
    return C_KZG_OK;
}

C_KZG_RET verifier_new_impl(LwkzgVerifier **out, const KZGSettings *s, size_t max_blobs) {
    if (!out) return C_KZG_BADARGS;
    *out = nullptr;
    if (!s || max_blobs == 0) return C_KZG_BADARGS;
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    if (!s->g1_values || !s->g2_values) {
        set_error("lwkzg_verifier_new: the settings have no g1_values / g2_values");
        return C_KZG_BADARGS;
    }
    Verifier *v = new (std::nothrow) Verifier(c, s, max_blobs);
    if (!v) return C_KZG_MALLOC;
    v->vb.owned = true;
    v->generator = s->g1_values[0];
    v->g2[0] = s->g2_values[0];
    v->g2[1] = s->g2_values[1];
    v->own.fs = nullptr;
    v->own.g1_values = &v->generator;
    v->own.g2_values = v->g2;
    C_KZG_RET rc = reserve_for(c, max_blobs);
    if (rc == C_KZG_OK)
        if (Ctx *t = c->twin.load(std::memory_order_acquire)) rc = reserve_for(t, max_blobs);
    if (rc == C_KZG_OK) {
        std::lock_guard<std::mutex> lk(c->mu);
        rc = verify_buffers_alloc(v->vb, max_blobs < 64 ? 64 : max_blobs);
        if (rc == C_KZG_OK) {
            const bool ok = hipHostMalloc((void **)&v->h_status, 4 * max_blobs, hipHostMallocDefault) == hipSuccess &&
                            hipEventCreateWithFlags(&v->ev_fork, hipEventDisableTiming) == hipSuccess &&
                            hipEventCreateWithFlags(&v->ev_ysum, hipEventDisableTiming) == hipSuccess &&
                            hipEventCreateWithFlags(&v->last_done, hipEventDisableTiming) == hipSuccess;
            if (!ok) {
                (void)hipGetLastError();
                set_error("lwkzg_verifier_new: no pinned memory or events for %zu blobs", max_blobs);
                rc = C_KZG_MALLOC;
            }
        }
    }
    return async_verifier_new_end(out, v, rc);
}

// everything of one call on context c, enqueued; caller holds c->mu. *hf: host functions handed to the runtime so far.
// front(c, vb, &recorded): the enqueue-only front of the call's kind -- verify_front_device for blobs, verify_openings_front_device for
// openings; both leave the transcript on its way to vb.h_rec, the canonical z / y bytes in vb.d_rz / vb.d_r and the rows of both point sets
template <class Front>
C_KZG_RET enqueue_on(Verifier *v, Ctx *c, AsyncJob *j, hipStream_t caller, int *hf, Front front) {
    LWK_HIP(hipSetDevice(c->device));
    VerifyBuffers &vb = v->vb;
    const size_t n = j->n;
    const int le = mode_rules(j->mode).le();
    hipStream_t st = c->stream, sy = c->aux[1];
    uint32_t *d_skip = (uint32_t *)(vb.vm_pw + kVmsmPwSkip);
    uint8_t *d_ysum = (uint8_t *)(vb.vm_pw + kVmsmPwYsum);
    C_KZG_RET rc = async_enqueue_head(v, c);
    if (rc != C_KZG_OK) return rc;
    bool recorded = false;
    rc = front(c, vb, &recorded);
    if (rc != C_KZG_OK) return rc;
    if (!recorded) {
        set_error("lwkzg_verifier_enqueue: the verifier's scratch has no room for the transcript");
        return C_KZG_ERROR;
    }
    LWK_HIP(hipMemcpyAsync(v->h_status, vb.status_all, 4 * n, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipLaunchHostFunc(st, verifier_host_fn1, j));
    *hf = 1;
    LWK_HIP(hipMemcpyAsync(vb.vm_pw, vb.h_pin, 33 * sizeof(Fr), hipMemcpyHostToDevice, st));
    LWK_HIP(hipMemcpyAsync(d_skip, vb.h_pin + kVmsmPinSkip, 4, hipMemcpyHostToDevice, st));
    LWK_HIP(hipEventRecord(v->ev_fork, st));
    LWK_HIP(hipStreamWaitEvent(sy, v->ev_fork, 0));
    launch_verify_ysum(vb.d_r, le, vb.vm_pw, d_ysum, n, sy, d_skip);
    LWK_HIP(hipEventRecord(v->ev_ysum, sy));
    launch_vmsm_scalars(vb.d_rz, le, vb.vm_pw, vb.sc_a, vb.sc_b, n, st, d_skip);
    launch_vmsm_accumulate(vb.sc_a, vb.sc_b, vb.tab_p, vb.kind_p, vb.tab_c, vb.kind_c, vb.vm_partial, n, st, nullptr, d_skip);
    launch_vmsm_reduce(vb.vm_partial, vb.vm_bsum, vb.d_aff, vb.d_inf, n, st, d_skip);
    LWK_HIP(hipStreamWaitEvent(st, v->ev_ysum, 0));
    LWK_HIP(hipMemcpyAsync(vb.h_pin + kVmsmPinSums, vb.d_aff, 3 * 96, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(vb.h_pin + kVmsmPinInfs, vb.d_inf, 3 * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(vb.h_pin + kVmsmPinYsum, d_ysum, 32, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipLaunchHostFunc(st, verifier_host_fn2, j));
    *hf = 2;
    return async_enqueue_tail(v, c, caller);
}

C_KZG_RET verifier_enqueue_impl(const LwkzgVerifier *handle, LwkzgVerifyResult *res, const uint8_t *blobs, const uint8_t *comm, const uint8_t *proofs,
                                size_t n, hipStream_t caller) {
    AsyncVerifier *base;
    const C_KZG_RET refused = async_enqueue_checks(&base, handle, kVerifierMagic, res, n, "lwkzg_verifier_enqueue", "blobs");
    if (refused != C_KZG_OK) return refused;
    Verifier *v = static_cast<Verifier *>(base);
    const int mode = mode_of(v->s);
    if (n == 0) {   // the reference answers OK with ok = false, c-kzg-4844 accepts the empty batch (verify.hip: verify_batch_impl)
        complete_now(res, C_KZG_OK, mode_rules(mode).empty_ok);
        return C_KZG_OK;
    }
    if (!blobs || !comm || !proofs) return async_refuse(res, C_KZG_BADARGS);
    std::lock_guard<std::mutex> enq(v->enq_mu);
    if (!vmsm_ready(v->vb)) {   // the experiment arm LWKZG_VERIFY_MSM=0: the synchronous call, complete before this returns
        v->ring.wait();
        bool ok = false;
        const C_KZG_RET rc = verify_batch_device_full(&ok, res->r, res->partial, blobs, comm, proofs, n, v->s, mode, caller);
        complete_now(res, rc, ok);
        return C_KZG_OK;
    }
    return async_enqueue(v, res, n, mode, caller, [&](Ctx *c, AsyncJob *j, int *hf) {
        return enqueue_on(v, c, j, caller, hf, [&](Ctx *cc, VerifyBuffers &vb, bool *recorded) {
            return verify_front_device(cc, blobs, comm, proofs, n, mode, vb, caller, true, false, recorded);
        });
    });
}

// lwkzg_verifier_enqueue for n openings: the same checks, the same two host functions and the same launches
// behind r; only the front differs. The verifier's capacity counts openings here.
C_KZG_RET verifier_enqueue_openings_impl(const LwkzgVerifier *handle, LwkzgVerifyResult *res, const uint8_t *comm, const uint8_t *zs,
                                         const uint8_t *ys, const uint8_t *proofs, size_t n, hipStream_t caller) {
    AsyncVerifier *base;
    const C_KZG_RET refused = async_enqueue_checks(&base, handle, kVerifierMagic, res, n, "lwkzg_verifier_enqueue_openings", "openings");
    if (refused != C_KZG_OK) return refused;
    Verifier *v = static_cast<Verifier *>(base);
    const int mode = mode_of(v->s);
    if (n == 0) {
        complete_now(res, C_KZG_OK, mode_rules(mode).empty_ok);
        return C_KZG_OK;
    }
    if (!comm || !zs || !ys || !proofs) return async_refuse(res, C_KZG_BADARGS);
    if ((((uintptr_t)comm | (uintptr_t)zs | (uintptr_t)ys | (uintptr_t)proofs) & 15u) != 0) {
        set_error("lwkzg_verifier_enqueue_openings: the device pointers must be 16-byte aligned");
        return async_refuse(res, C_KZG_BADARGS);
    }
    std::lock_guard<std::mutex> enq(v->enq_mu);
    if (!vmsm_ready(v->vb)) {   // the experiment arm LWKZG_VERIFY_MSM=0: the synchronous call, complete before this returns
        v->ring.wait();
        bool ok = false;
        const C_KZG_RET rc = verify_openings_batch_full(&ok, res->r, res->partial, comm, zs, ys, proofs, n, v->s, mode, true, caller);
        complete_now(res, rc, ok);
        return C_KZG_OK;
    }
    return async_enqueue(v, res, n, mode, caller, [&](Ctx *c, AsyncJob *j, int *hf) {
        return enqueue_on(v, c, j, caller, hf, [&](Ctx *cc, VerifyBuffers &vb, bool *recorded) {
            return verify_openings_front_device(cc, comm, proofs, zs, ys, n, mode, vb, caller, recorded);
        });
    });
}

}  // namespace

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_verifier_new(LwkzgVerifier **out, const KZGSettings *s, size_t max_blobs) {
    return guarded("lwkzg_verifier_new", [&] { return verifier_new_impl(out, s, max_blobs); });
}

C_KZG_RET lwkzg_verifier_enqueue(LwkzgVerifier *v, LwkzgVerifyResult *result, const void *blobs_dev, const void *commitments48_dev,
                                 const void *proofs48_dev, size_t n, void *stream) {
    return guarded("lwkzg_verifier_enqueue", [&] {
        return verifier_enqueue_impl(v, result, (const uint8_t *)blobs_dev, (const uint8_t *)commitments48_dev, (const uint8_t *)proofs48_dev, n,
                                     (hipStream_t)stream);
    });
}

C_KZG_RET lwkzg_verifier_enqueue_openings(LwkzgVerifier *v, LwkzgVerifyResult *result, const void *commitments48_dev, const void *zs32_dev,
                                          const void *ys32_dev, const void *proofs48_dev, size_t n, void *stream) {
    return guarded("lwkzg_verifier_enqueue_openings", [&] {
        return verifier_enqueue_openings_impl(v, result, (const uint8_t *)commitments48_dev, (const uint8_t *)zs32_dev, (const uint8_t *)ys32_dev,
                                              (const uint8_t *)proofs48_dev, n, (hipStream_t)stream);
    });
}

int lwkzg_verifier_pending(const LwkzgVerifier *v) { return async_verifier_pending(v, kVerifierMagic); }
C_KZG_RET lwkzg_verifier_wait(LwkzgVerifier *v) { return async_verifier_wait(v, kVerifierMagic); }
void lwkzg_verifier_free(LwkzgVerifier *v) { async_verifier_free<Verifier>(v, kVerifierMagic); }

C_KZG_RET lwkzg_verifier_host_steps(LwkzgVerifyResult *out, const uint8_t *records, size_t n, uint32_t first_bad, const uint8_t *sums3x97,
                                    const uint8_t *ysum32, const KZGSettings *s, int mode) {
    if (!out) return C_KZG_BADARGS;
    memset(out, 0, sizeof *out);
    out->first_bad = first_bad;
    if (!mode_known(mode)) return async_refuse(out, C_KZG_BADARGS);
    if (first_bad != kNoneBad) {   // a rejected input: the mode's code, and nothing else is read
        complete_now(out, mode_rules(mode).bad, false);
        return C_KZG_OK;
    }
    if ((!records && n) || !sums3x97 || !ysum32 || !s) return async_refuse(out, C_KZG_BADARGS);
    C_KZG_RET rc = C_KZG_ERROR;
    bool ok = false;
    try {
        Fr pw[33];
        verify_async_challenge(out->r, pw, records, n, mode);
        uint8_t sums[3][96];
        int infs[3];
        rc = sums_from_97(sums, infs, sums3x97) ? verify_async_verdict(&ok, out->partial, sums, infs, ysum32, s) : C_KZG_BADARGS;
    } catch (...) {
        rc = C_KZG_ERROR;
    }
    complete_now(out, rc, ok && rc == C_KZG_OK);
    return C_KZG_OK;
}

}  // extern "C"
