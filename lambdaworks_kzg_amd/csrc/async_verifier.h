// async_verifier.h -- what the verifiers that do not block have in common (verify_async.hip: blobs, cells_verify_async.hip: cells;
// DESIGN.md sections 4m, 4n): the head of a handle, the registry ctx_destroy drains, the checks and the skeleton of an enqueue, the
// ends of new, and pending / wait / free. A kind derives its handle from AsyncVerifier and keeps its buffers, its two host functions
// and its launches. The job slots and the protocol of a failing enqueue are verifier_ring.h (plain C++, run under ThreadSanitizer).
//
// HOST FUNCTIONS run on the runtime's callback thread, in stream order, and the stream does not move until they return. Rules:
//   - no HIP call;
//   - no lock that any thread may hold while it waits for a stream or an event: Ctx::mu and verify_mu are such locks (a synchronous
//     call holds them across hipStreamSynchronize on this very stream), as are AsyncVerifier::enq_mu and g_async_verifiers_mu. The
//     ring's mutex is not: nobody waits for the GPU under it;
//   - nothing thrown: a failure becomes rc = C_KZG_ERROR (the abi_guard.h pattern, without its error text);
//   - no set_error: the thread is the runtime's, its error text nobody's;
//   - the mode and n come from the job slot; the caller's KZGSettings is never read -- what a kind needs of it was copied into the
//     verifier at creation.
#pragma once
#include "engine_internal.h"
#include "verifier_ring.h"

#include <string.h>

#include <set>

namespace lwk {

constexpr uint32_t kNoneBad = 0xffffffffu;

struct AsyncVerifier;
struct AsyncJob {
    AsyncVerifier *v = nullptr;
    void *res = nullptr;    // the kind's result struct
    size_t n = 0;
    int mode = 0;
    uint32_t first_bad = kNoneBad, m = 0;   // (m: cells, the distinct commitments)
    int32_t code = 0;       // a rejected input's status word (blobs), a rejected batch's return code (cells)
    bool failed = false;    // host function 1 could not do its work
};
typedef VerifierRing<AsyncJob, LWKZG_VERIFIER_DEPTH> AsyncRing;

struct AsyncVerifier {
    uint64_t magic;                   // the kind's own: a handle of one kind is refused by the other kind's entry points
    Ctx *ctx;                         // the settings' primary context; a call runs there or on its twin (pick_ctx)
    uint64_t ctx_generation;          // (engine.h: ctx_is_live -- the caller's KZGSettings is not read to decide that)
    const KZGSettings *s;             // read by the enqueuing thread only, and only while the context is live (the mode)
    int device;
    size_t cap;
    hipEvent_t last_done = nullptr;
    Ctx *last_ctx = nullptr;          // the context whose stream recorded last_done (under enq_mu)
    std::mutex enq_mu;                // enqueues of one verifier, one at a time; never taken by a host function
    AsyncRing ring;
    AsyncVerifier(uint64_t kind_magic, Ctx *c, const KZGSettings *settings, size_t max_items)
        : magic(kind_magic), ctx(c), ctx_generation(c->generation), s(settings), device(c->device), cap(max_items) {}
};

inline std::mutex g_async_verifiers_mu;   // the set below; never taken by a host function
inline std::set<AsyncVerifier *> g_async_verifiers;

// the calls in flight of every verifier of this context have completed (ctx_destroy, before the context goes)
inline void async_verifiers_drain(const Ctx *c) {
    if (!c) return;
    std::lock_guard<std::mutex> lk(g_async_verifiers_mu);
    for (AsyncVerifier *v : g_async_verifiers)
        if (v->ctx == c) v->ring.wait();
}

inline AsyncVerifier *async_verifier_of(const void *handle, uint64_t magic) {
    AsyncVerifier *v = (AsyncVerifier *)handle;
    return v && v->magic == magic ? v : nullptr;
}

// the runtime's first-use costs of a host function on this stream are paid here, not in the first call that launches one
inline void host_noop_fn(void *) {}
inline void stream_warm_host_fn(hipStream_t st) {
    if (hipLaunchHostFunc(st, host_noop_fn, nullptr) != hipSuccess) (void)hipGetLastError();
    (void)hipStreamSynchronize(st);
}

// ---- new ---------------------------------------------------------------------------------------------------------------------------
// V: a kind, with free_own() for its buffers and its own events
template <class V>
void async_verifier_destroy(V *v) {
    hipSetDevice(v->device);
    hipDeviceSynchronize();   // as a shard's destructor: device memory of its own, freed whether or not the context still exists
    v->free_own();
    if (v->last_done) (void)hipEventDestroy(v->last_done);
    v->magic = 0;
    delete v;
}

// rc: how the kind's reservations and allocations went
template <class V, class Handle>
C_KZG_RET async_verifier_new_end(Handle **out, V *v, C_KZG_RET rc) {
    if (rc != C_KZG_OK) {
        async_verifier_destroy(v);
        return rc == C_KZG_MALLOC ? C_KZG_MALLOC : C_KZG_ERROR;
    }
    {
        std::lock_guard<std::mutex> lk(g_async_verifiers_mu);
        g_async_verifiers.insert(v);
    }
    *out = (Handle *)static_cast<AsyncVerifier *>(v);
    return C_KZG_OK;
}

// ---- enqueue -----------------------------------------------------------------------------------------------------------------------
// a call refused on the spot: its result is complete when the call returns
template <class Res>
C_KZG_RET async_refuse(Res *res, C_KZG_RET rc) {
    complete_now(res, rc, false);
    return rc;
}

// What every enqueue decides first. C_KZG_OK: *out is the verifier and *res is zeroed (state = 0, first_bad = none); otherwise the code
// to return, with *res complete unless it is NULL. fn, noun: of the error texts
template <class Res>
C_KZG_RET async_enqueue_checks(AsyncVerifier **out, const void *handle, uint64_t magic, Res *res, size_t n, const char *fn, const char *noun) {
    if (!res) return C_KZG_BADARGS;
    memset(res, 0, sizeof *res);   // state = 0
    res->first_bad = kNoneBad;
    AsyncVerifier *v = *out = async_verifier_of(handle, magic);
    if (v && !ctx_is_live(v->ctx, v->ctx_generation)) set_error("%s: the verifier's trusted setup is no longer loaded", fn);
    else if (v && n > v->cap) set_error("%s: %zu %s, the verifier was created for %zu", fn, n, noun, v->cap);
    else if (v) return C_KZG_OK;
    return async_refuse(res, C_KZG_BADARGS);
}

// One call of n items, enqueued; the caller holds v->enq_mu. While a call of this verifier is in flight the next one follows it on the
// same context (stream order; two verifiers kept deep then stay on a context each); otherwise the settings' usual choice for a caller
// stream. enqueue_on(c, job, &hf) runs with c->mu held, between async_enqueue_head and async_enqueue_tail.
template <class Res, class EnqueueOn>
C_KZG_RET async_enqueue(AsyncVerifier *v, Res *res, size_t n, int mode, hipStream_t caller, EnqueueOn enqueue_on) {
    Ctx *c = v->last_ctx && v->ring.pending() > 0 ? v->last_ctx : pick_ctx(v->ctx, caller);
    int rc;
    {
        std::unique_lock<std::mutex> lk(c->mu, std::defer_lock);   // taken once the call has its slot, held to the end of the protocol
        rc = ring_enqueue(
            v->ring, res, C_KZG_ERROR,
            [&](AsyncJob *j) {
                *j = AsyncJob();
                j->v = v;
                j->res = res;
                j->n = n;
                j->mode = mode;
            },
            [&](AsyncJob *j, int *hf) {
                lk.lock();
                return (int)enqueue_on(c, j, hf);
            },
            [&] { (void)hipStreamSynchronize(c->stream); });
    }
    if (rc != C_KZG_OK) (void)hipGetLastError();
    return (C_KZG_RET)rc;
}

// the verifier's scratch: behind its previous call, whichever of the two contexts ran that
inline C_KZG_RET async_enqueue_head(AsyncVerifier *v, Ctx *c) {
    if (v->last_ctx && v->last_ctx != c) LWK_HIP(hipStreamWaitEvent(c->stream, v->last_done, 0));
    return C_KZG_OK;
}

// behind host function 2: the next call's mark, and work enqueued behind the call on the caller's stream sees the verdict
inline C_KZG_RET async_enqueue_tail(AsyncVerifier *v, Ctx *c, hipStream_t caller) {
    LWK_HIP(hipEventRecord(v->last_done, c->stream));
    v->last_ctx = c;
    if (caller && caller != c->stream) LWK_HIP(hipStreamWaitEvent(caller, v->last_done, 0));
    return C_KZG_OK;
}

// ---- pending, wait, free -------------------------------------------------------------------------------------------------------------
inline int async_verifier_pending(const void *handle, uint64_t magic) {
    AsyncVerifier *v = async_verifier_of(handle, magic);
    return v ? v->ring.pending() : -1;
}

inline C_KZG_RET async_verifier_wait(const void *handle, uint64_t magic) {
    AsyncVerifier *v = async_verifier_of(handle, magic);
    if (!v) return C_KZG_BADARGS;
    v->ring.wait();
    return C_KZG_OK;
}

template <class V>
void async_verifier_free(const void *handle, uint64_t magic) {
    AsyncVerifier *v = async_verifier_of(handle, magic);
    if (!v) return;
    v->ring.wait();
    {
        std::lock_guard<std::mutex> lk(g_async_verifiers_mu);
        g_async_verifiers.erase(v);
    }
    async_verifier_destroy(static_cast<V *>(v));
}

// ---- the three sums and their flags ------------------------------------------------------------------------------------------------
// as the device sent them down: 3 x 96 bytes, 3 words
inline void sums_from_pinned(uint8_t sums[3][96], int infs[3], const uint8_t *sums288, const uint8_t *flags12) {
    memcpy(sums, sums288, 3 * 96);
    for (int k = 0; k < 3; k++) {
        int32_t f;
        memcpy(&f, flags12 + 4 * k, 4);
        infs[k] = f;
    }
}

// as the host-steps hooks take them: 3 x (flag byte, 96 bytes); false for a flag byte above 1
inline bool sums_from_97(uint8_t sums[3][96], int infs[3], const uint8_t *sums3x97) {
    bool well_formed = true;
    for (int k = 0; k < 3; k++) {
        const uint8_t *p = sums3x97 + 97 * k;
        infs[k] = p[0] == 1;
        well_formed = well_formed && p[0] <= 1;
        memcpy(sums[k], p + 1, 96);
    }
    return well_formed;
}

}  // namespace lwk
