// verify_async.hip -- lwkzg_verifier_*: lwkzg_verify_blob_kzg_proof_batch_device without a parked host thread.
//
// The synchronous call stops its thread twice: behind the transcript's copy (the host hashes it into r) and behind the copy of the
// three sums (the host multiplies the generator and runs the pairing). Here both pieces of host work are HOST FUNCTIONS in stream
// order (hipLaunchHostFunc, as engine.hip's small_proof_host_fn), the one O(n) piece of it -- sum r^i y_i, a serial walk over n powers
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
// Calls on one verifier share its VerifyBuffers and run one after the other: on one context by stream order, across the settings' two
// contexts (pick_ctx) by the verifier's last_done event. The job slots and their hand-over are verifier_ring.h.
#include "abi_guard.h"
#include "engine_internal.h"
#include "verifier_ring.h"
#include "verify_ysum.cuh"

#include <string.h>

#include <memory>
#include <new>
#include <set>

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
    ProfScope p("k_verify_ysum", st);
    hipLaunchKernelGGL(k_verify_ysum, dim3(1), dim3(kYsumLanes), 0, st, y32, le, pw, out32, (uint32_t)n, skip);
}

// ---- the verifier --------------------------------------------------------------------------------------------------------------------
namespace {

constexpr uint64_t kVerifierMagic = 0x4c574b5a56524659ull;  // "LWKZVRFY"
constexpr uint32_t kNoneBad = 0xffffffffu;

struct Verifier;
struct VerifyJob {
    Verifier *v = nullptr;
    LwkzgVerifyResult *res = nullptr;
    size_t n = 0;
    int mode = 0;
    uint32_t first_bad = kNoneBad;
    int32_t code = 0;       // the rejected input's status word
    bool failed = false;    // host function 1 could not do its work
};
typedef VerifierRing<VerifyJob, LWKZG_VERIFIER_DEPTH> Ring;

struct Verifier {
    uint64_t magic = kVerifierMagic;
    Ctx *ctx = nullptr;            // the settings' primary context; a call runs there or on its twin (pick_ctx)
    uint64_t ctx_generation = 0;   // (engine.h: ctx_is_live -- the caller's KZGSettings is not read to decide that)
    const KZGSettings *s = nullptr;   // read by the enqueuing thread only, and only while the context is live (the mode)
    int device = 0;
    size_t cap = 0;
    VerifyBuffers vb;              // owned: device scratch, h_rec, h_pin
    int32_t *h_status = nullptr;   // hipHostMalloc, cap words: the status words beside the transcript (the rejected input's code)
    hipEvent_t ev_fork = nullptr, ev_ysum = nullptr, last_done = nullptr;
    Ctx *last_ctx = nullptr;       // the context whose stream recorded last_done (under enq_mu)
    // the generator and the two G2 points of the settings, copied at creation: all the host functions ever see of them
    g1_t generator;
    g2_t g2[2];
    KZGSettings own;
    std::mutex enq_mu;             // enqueues of one verifier, one at a time; never taken by a host function
    Ring ring;
};

std::mutex g_verifiers_mu;         // the set below; never taken by a host function
std::set<Verifier *> g_verifiers;

void complete_now(LwkzgVerifyResult *res, C_KZG_RET rc, bool ok) {
    res->rc = (int32_t)rc;
    res->ok = ok ? 1 : 0;
    Ring::publish(&res->state);
}

// ---- the two host functions ------------------------------------------------------------------------------------------------------
// They run on the runtime's callback thread, in stream order, and the stream does not move until they return. Rules for both:
//   - no HIP call;
//   - no lock that any thread may hold while it waits for a stream or an event: Ctx::mu and verify_mu are such locks (a synchronous
//     call holds them across hipStreamSynchronize on this very stream), as are Verifier::enq_mu and g_verifiers_mu. The ring's mutex
//     is not: nobody waits for the GPU under it;
//   - nothing thrown: a failure becomes rc = C_KZG_ERROR (the abi_guard.h pattern, without its error text);
//   - no set_error: the thread is the runtime's, its error text nobody's;
//   - the mode and n come from the job slot; the caller's KZGSettings is never read -- the generator and the G2 points were copied into
//     the verifier at creation.

// behind the transcript's copy: first_bad, r, the 33 powers (or the skip word) into the pinned block
void verifier_host_fn1(void *p) {
    VerifyJob *j = (VerifyJob *)p;
    Verifier *v = j->v;
    uint32_t skip = 1;
    try {
        memcpy(&j->first_bad, v->vb.h_rec + LWKZG_VERIFY_RECORD_BYTES * j->n, 4);
        if (j->first_bad == kNoneBad) {
            Fr pw[33];
            verify_async_challenge(j->res->r, pw, v->vb.h_rec, j->n, j->mode == LWKZG_MODE_CKZG);
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
    VerifyJob *j = (VerifyJob *)p;
    Verifier *v = j->v;
    LwkzgVerifyResult *res = j->res;
    C_KZG_RET rc = C_KZG_ERROR;
    bool ok = false;
    try {
        if (j->failed) {
            rc = C_KZG_ERROR;
        } else if (j->first_bad != kNoneBad) {   // as verify_prepare_device and shard_begin answer a rejected input
            rc = j->mode == LWKZG_MODE_REFERENCE || j->code != kStatusBadArgs ? C_KZG_ERROR : C_KZG_BADARGS;
        } else {
            const uint8_t *pin = v->vb.h_pin;
            uint8_t sums[3][96];
            int infs[3];
            for (int k = 0; k < 3; k++) {
                memcpy(sums[k], pin + kVmsmPinSums + 96 * k, 96);
                int32_t f;
                memcpy(&f, pin + kVmsmPinInfs + 4 * k, 4);
                infs[k] = f;
            }
            rc = verify_async_verdict(&ok, res->partial, sums, infs, pin + kVmsmPinYsum, &v->own);
        }
    } catch (...) {
        rc = C_KZG_ERROR;
    }
    res->first_bad = j->first_bad;
    complete_now(res, rc, ok && rc == C_KZG_OK);
    v->ring.release(j);   // (the verifier may be gone as soon as this returns)
}

void host_noop_fn(void *) {}

void verifier_destroy(Verifier *v) {
    hipSetDevice(v->device);
    hipDeviceSynchronize();   // as a shard's destructor: device memory of its own, freed whether or not the context still exists
    verify_buffers_free(v->vb);
    if (v->h_status) (void)hipHostFree(v->h_status);
    for (hipEvent_t e : {v->ev_fork, v->ev_ysum, v->last_done})
        if (e) (void)hipEventDestroy(e);
    v->magic = 0;
    delete v;
}

// the workspace a call of n blobs on context c takes, as verify_front_device reserves it
C_KZG_RET reserve_for(Ctx *c, size_t n) {
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    C_KZG_RET rc = ctx_reserve(c, n < kMaxChunk ? n : kMaxChunk);
    if (rc != C_KZG_OK) return rc;
    if (n > kMaxChunk && (rc = ws_long_reserve(c, n)) != C_KZG_OK) return rc;
    // the runtime's first-use costs of a host function on this stream are paid here, not in the first call
    if (hipLaunchHostFunc(c->stream, host_noop_fn, nullptr) != hipSuccess) (void)hipGetLastError();
    (void)hipStreamSynchronize(c->stream);
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
    Verifier *v = new (std::nothrow) Verifier();
    if (!v) return C_KZG_MALLOC;
    v->ctx = c;
    v->ctx_generation = c->generation;
    v->s = s;
    v->device = c->device;
    v->cap = max_blobs;
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
    if (rc != C_KZG_OK) {
        verifier_destroy(v);
        return rc == C_KZG_MALLOC ? C_KZG_MALLOC : C_KZG_ERROR;
    }
    {
        std::lock_guard<std::mutex> lk(g_verifiers_mu);
        g_verifiers.insert(v);
    }
    *out = (LwkzgVerifier *)v;
    return C_KZG_OK;
}

// everything of one call on context c, enqueued; caller holds c->mu. *hf: host functions handed to the runtime so far
C_KZG_RET enqueue_on(Verifier *v, Ctx *c, VerifyJob *j, const uint8_t *blobs, const uint8_t *comm, const uint8_t *proofs, hipStream_t caller,
                     int *hf) {
    LWK_HIP(hipSetDevice(c->device));
    VerifyBuffers &vb = v->vb;
    const size_t n = j->n;
    const int le = j->mode == LWKZG_MODE_CKZG;
    hipStream_t st = c->stream, sy = c->aux[1];
    uint32_t *d_skip = (uint32_t *)(vb.vm_pw + kVmsmPwSkip);
    uint8_t *d_ysum = (uint8_t *)(vb.vm_pw + kVmsmPwYsum);
    // the verifier's scratch: behind its previous call, whichever of the two contexts ran that
    if (v->last_ctx && v->last_ctx != c) LWK_HIP(hipStreamWaitEvent(st, v->last_done, 0));
    bool recorded = false;
    const C_KZG_RET rc = verify_front_device(c, blobs, comm, proofs, n, j->mode, vb, caller, true, false, &recorded);
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
    LWK_HIP(hipEventRecord(v->last_done, st));
    v->last_ctx = c;
    if (caller && caller != st) LWK_HIP(hipStreamWaitEvent(caller, v->last_done, 0));   // work behind the call sees the verdict
    return C_KZG_OK;
}

C_KZG_RET verifier_enqueue_impl(Verifier *v, LwkzgVerifyResult *res, const uint8_t *blobs, const uint8_t *comm, const uint8_t *proofs, size_t n,
                                hipStream_t caller) {
    if (!res) return C_KZG_BADARGS;
    memset(res, 0, sizeof *res);   // state = 0
    res->first_bad = kNoneBad;
    auto refuse = [&](C_KZG_RET rc) {
        complete_now(res, rc, false);
        return rc;
    };
    if (!v || v->magic != kVerifierMagic) return refuse(C_KZG_BADARGS);
    if (!ctx_is_live(v->ctx, v->ctx_generation)) {
        set_error("lwkzg_verifier_enqueue: the verifier's trusted setup is no longer loaded");
        return refuse(C_KZG_BADARGS);
    }
    if (n > v->cap) {
        set_error("lwkzg_verifier_enqueue: %zu blobs, the verifier was created for %zu", n, v->cap);
        return refuse(C_KZG_BADARGS);
    }
    const int mode = mode_of(v->s);
    if (n == 0) {   // the reference answers OK with ok = false, c-kzg-4844 accepts the empty batch (verify.hip: verify_batch_impl)
        complete_now(res, C_KZG_OK, mode == LWKZG_MODE_CKZG);
        return C_KZG_OK;
    }
    if (!blobs || !comm || !proofs) return refuse(C_KZG_BADARGS);
    std::lock_guard<std::mutex> enq(v->enq_mu);
    if (!vmsm_ready(v->vb)) {   // the experiment arm LWKZG_VERIFY_MSM=0: the synchronous call, complete before this returns
        v->ring.wait();
        bool ok = false;
        const C_KZG_RET rc = verify_batch_device_full(&ok, res->r, res->partial, blobs, comm, proofs, n, v->s, mode, caller);
        complete_now(res, rc, ok);
        return C_KZG_OK;
    }
    // while a call of this verifier is in flight the next one follows it on the same context (stream order; two verifiers kept deep then
    // stay on a context each); otherwise the settings' usual choice for a caller stream
    Ctx *c = v->last_ctx && v->ring.pending() > 0 ? v->last_ctx : pick_ctx(v->ctx, caller);
    VerifyJob *j = v->ring.acquire();   // the one place this call may wait: LWKZG_VERIFIER_DEPTH calls are in flight
    *j = VerifyJob();
    j->v = v;
    j->res = res;
    j->n = n;
    j->mode = mode;
    int hf = 0;
    C_KZG_RET rc;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        rc = enqueue_on(v, c, j, blobs, comm, proofs, caller, &hf);
        // a failing enqueue, and only that: whatever was handed to the runtime runs before the slot and the result are touched again
        if (rc != C_KZG_OK && hf) (void)hipStreamSynchronize(c->stream);
    }
    if (rc == C_KZG_OK) return C_KZG_OK;
    (void)hipGetLastError();
    if (hf < 2) {   // (behind host function 2 the result is complete and the slot free already)
        complete_now(res, C_KZG_ERROR, false);
        v->ring.release(j);
    }
    return C_KZG_ERROR;
}

}  // namespace

void verifiers_drain(const Ctx *c) {
    if (!c) return;
    std::lock_guard<std::mutex> lk(g_verifiers_mu);
    for (Verifier *v : g_verifiers)
        if (v->ctx == c) v->ring.wait();
}

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_verifier_new(LwkzgVerifier **out, const KZGSettings *s, size_t max_blobs) {
    return guarded("lwkzg_verifier_new", [&] { return verifier_new_impl(out, s, max_blobs); });
}

C_KZG_RET lwkzg_verifier_enqueue(LwkzgVerifier *v, LwkzgVerifyResult *result, const void *blobs_dev, const void *commitments48_dev,
                                 const void *proofs48_dev, size_t n, void *stream) {
    return guarded("lwkzg_verifier_enqueue", [&] {
        return verifier_enqueue_impl((Verifier *)v, result, (const uint8_t *)blobs_dev, (const uint8_t *)commitments48_dev,
                                     (const uint8_t *)proofs48_dev, n, (hipStream_t)stream);
    });
}

int lwkzg_verifier_pending(const LwkzgVerifier *v) {
    Verifier *w = (Verifier *)v;
    if (!w || w->magic != kVerifierMagic) return -1;
    return w->ring.pending();
}

C_KZG_RET lwkzg_verifier_wait(LwkzgVerifier *v) {
    Verifier *w = (Verifier *)v;
    if (!w || w->magic != kVerifierMagic) return C_KZG_BADARGS;
    w->ring.wait();
    return C_KZG_OK;
}

void lwkzg_verifier_free(LwkzgVerifier *v) {
    Verifier *w = (Verifier *)v;
    if (!w || w->magic != kVerifierMagic) return;
    w->ring.wait();
    {
        std::lock_guard<std::mutex> lk(g_verifiers_mu);
        g_verifiers.erase(w);
    }
    verifier_destroy(w);
}

C_KZG_RET lwkzg_verifier_host_steps(LwkzgVerifyResult *out, const uint8_t *records, size_t n, uint32_t first_bad, const uint8_t *sums3x97,
                                    const uint8_t *ysum32, const KZGSettings *s, int mode) {
    if (!out) return C_KZG_BADARGS;
    memset(out, 0, sizeof *out);
    out->first_bad = first_bad;
    if (mode != LWKZG_MODE_REFERENCE && mode != LWKZG_MODE_CKZG) {
        complete_now(out, C_KZG_BADARGS, false);
        return C_KZG_BADARGS;
    }
    if (first_bad != kNoneBad) {   // a rejected input: the mode's code, and nothing else is read
        complete_now(out, mode == LWKZG_MODE_REFERENCE ? C_KZG_ERROR : C_KZG_BADARGS, false);
        return C_KZG_OK;
    }
    if ((!records && n) || !sums3x97 || !ysum32 || !s) {
        complete_now(out, C_KZG_BADARGS, false);
        return C_KZG_BADARGS;
    }
    C_KZG_RET rc = C_KZG_ERROR;
    bool ok = false;
    try {
        Fr pw[33];
        verify_async_challenge(out->r, pw, records, n, mode == LWKZG_MODE_CKZG);
        uint8_t sums[3][96];
        int infs[3];
        bool well_formed = true;
        for (int k = 0; k < 3; k++) {
            const uint8_t *p = sums3x97 + 97 * k;
            infs[k] = p[0] == 1;
            well_formed = well_formed && p[0] <= 1;
            memcpy(sums[k], p + 1, 96);
        }
        rc = well_formed ? verify_async_verdict(&ok, out->partial, sums, infs, ysum32, s) : C_KZG_BADARGS;
    } catch (...) {
        rc = C_KZG_ERROR;
    }
    complete_now(out, rc, ok && rc == C_KZG_OK);
    return C_KZG_OK;
}

}  // extern "C"
