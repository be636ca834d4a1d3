// proof_calls.hip -- the device-resident proof calls (host side, HIP runtime): blob proofs under the five schedules of plan.h, the one-pass
// commit-and-prove, proofs at given points; the pinned staging and the warmth test of their host-assisted schedules; and where a call's
// per-blob words live (call_words). The context, the workspace and the launch stages these calls are made of stay in engine.hip.
#include "carve.h"
#include "engine_internal.h"

#include <string.h>

#include <atomic>
#include <new>
#include <vector>

namespace lwk {

void sph_free(SmallProofHost &h) {
    if (h.blobs) hipHostFree(h.blobs);
    if (h.comm) hipHostFree(h.comm);
    if (h.canon) hipHostFree(h.canon);
    if (h.dig) hipHostFree(h.dig);
    if (h.code) hipHostFree(h.code);
    for (hipEvent_t e : h.chunk_done)
        if (e) hipEventDestroy(e);
    for (hipEvent_t e : h.hashed)
        if (e) hipEventDestroy(e);
    h = SmallProofHost();
}

// Up to this many blobs a device-resident blob-proof call takes its Fiat-Shamir challenges and its commitment validation from the
// host threads (0 = never). Default 64 since r05 (the GPU's validation went from 2.0 to 1.1 ms: at 128 blobs the mid-size path below takes 2.9 ms where this one
// takes 3.6, at 64 both 2.25, at 16 this one 1.2 against 1.8; gpurun_out r05/gpu14); r04's table, when the default was 128 (default engine, same box, ms per call with / without: 1 blob 0.80 / 3.62, 16: 0.87 / 3.61, 64: 1.96 / 4.29,
// 128: 3.41 / 5.05, 256: 6.43 / 6.68 -- beyond that the copy out and the host threads cost what the GPU chains did; gpurun_out r04c).
static std::atomic<int> g_last_proof_schedule{-1};   // test hook (lwkzg_last_proof_schedule): the schedule the last device-resident proof call took
int last_proof_schedule() { return g_last_proof_schedule.load(std::memory_order_relaxed); }
size_t small_proof_host_limit() {
    const size_t x = knobs().small_proof_host;
    return x > kMaxChunk ? kMaxChunk : x;
}

// at_reserve: called from lwkzg_reserve* (the place to pay for pinned memory). From inside a call (at_reserve = false) the staging
// only grows on settings objects whose owner never reserved anything -- growing means a device synchronisation and up to 64 MiB of
// hipHostMalloc, which a caller that reserved (a stream-capturing or latency-sensitive one) was promised not to meet:
// there the call takes the GPU hash path instead.
bool sph_reserve(Ctx *c, size_t n, bool at_reserve) {
    SmallProofHost &h = c->sph;
    if (h.cap >= n) return true;
    if (!at_reserve && c->primary->reserved.load(std::memory_order_acquire)) return false;
    hipDeviceSynchronize();  // a host function of an earlier call may still be reading the old buffers
    sph_free(h);
    size_t cap = 16;
    while (cap < n) cap <<= 1;
    const bool ok = hipHostMalloc((void **)&h.blobs, cap * (size_t)kBlobBytes) == hipSuccess && hipHostMalloc((void **)&h.comm, cap * 48) == hipSuccess &&
                    hipHostMalloc((void **)&h.canon, cap * 48) == hipSuccess && hipHostMalloc((void **)&h.dig, cap * 32) == hipSuccess &&
                    hipHostMalloc((void **)&h.code, cap * 4) == hipSuccess;
    bool ev_ok = ok;
    for (int k = 0; ev_ok && k < SmallProofHost::kChunks; k++)
        ev_ok = hipEventCreateWithFlags(&h.chunk_done[k], hipEventDisableTiming) == hipSuccess &&
                hipEventCreateWithFlags(&h.hashed[k], hipEventDisableTiming) == hipSuccess;
    if (!ev_ok) {
        (void)hipGetLastError();
        sph_free(h);
        return false;
    }
    h.cap = cap;
    return true;
}

// Between the small calls and the large ones: up to this many blobs the Fiat-Shamir hashing of a device-resident blob-proof call runs
// on the host threads too, but PIPELINED -- the blobs leave in chunks on a side stream and every chunk is hashed while the next one is
// on its way -- and beside the GPU's commitment validation (which stays on the GPU: 2 ms whatever the batch, where the host would need
// 0.2 ms per point per thread). 256 blobs: the challenges in ~1.6 ms instead of the hash kernel's flat 3.2.
static size_t mid_proof_chunks() {   // experiment knob: host functions (= chunks) per mid-size call, 1 .. SmallProofHost::kChunks
    const size_t x = knobs().mid_proof_chunks;
    return x < 1 ? 1 : x > (size_t)SmallProofHost::kChunks ? (size_t)SmallProofHost::kChunks : x;
}
size_t mid_proof_host_limit() {
    const size_t x = knobs().mid_proof_host;
    return x > kMaxChunk ? kMaxChunk : x;
}

// the knobs a plan depends on, clamped as the engine uses them (plan.h: PlanKnobs)
static PlanKnobs plan_knobs() {
    PlanKnobs k;
    k.small_proof_host = small_proof_host_limit();
    k.mid_proof_host = mid_proof_host_limit();
    k.mid_proof_chunks = mid_proof_chunks();
    k.mid_proof_pipe = knobs().mid_proof_pipe;
    k.mid_proof_pipe_min = knobs().mid_proof_pipe_min;
    k.mid_proof_parts = knobs().mid_proof_parts;
    k.heavy_serial = knobs().heavy_serial;
    return k;
}

static void host_warm_fn(void *) {
    try {
        host_pool_warm();
    } catch (...) {
    }
}

// Are the host threads warm? The mid-size host-assisted challenge (hashing on the host threads, pipelined with the copy out) beats
// the GPU's hash kernel only when they are: a pool that does not exist yet, or threads idle for longer than LWKZG_HOST_WARM_MS
// (default 2000; measured: up to a second of idleness costs the first two calls 0.2 ms, tools/experiments/r05_host_cold.py), make the
// call take the GPU kernel this once -- and wake the threads on the side, from a host function, so that the NEXT call finds them warm
// (a cold burst of host-assisted calls ran at 30.7k proofs/s where the GPU path does 41.5k).
static std::atomic<int64_t> g_wake_requested_ns{0};
static bool host_assist_warm() {
    const int64_t window_ns = (int64_t)(knobs().host_warm_ms < 0 ? 0 : knobs().host_warm_ms) * 1000000;
    const int64_t last = host_last_active_ns(), woken = g_wake_requested_ns.load(std::memory_order_acquire), now = host_now_ns();
    // (a wake-up that is on its way counts: the calls of a burst are enqueued within microseconds of each other, before the first one's
    // wake-up has run, and their host functions only run after the first call's GPU work -- milliseconds later, on threads that are awake)
    return (last != 0 && now - last <= window_ns) || (woken != 0 && now - woken <= window_ns);
}
// enqueue the wake-up of the host threads on a stream the call does not wait for
static void launch_host_wake(Ctx *c) {
    g_wake_requested_ns.store(host_now_ns(), std::memory_order_release);
    if (hipLaunchHostFunc(c->aux[1], host_warm_fn, nullptr) != hipSuccess) (void)hipGetLastError();
}

struct ChunkHashArgs {
    SmallProofHost *h;
    size_t first, count;
    bool be_fields;   // the mode's transcript (mode_rules.h)
};
static void chunk_midstate_host_fn(void *p) {   // the one-pass commit-and-prove: the commitment-free 2048 blocks of a chunk's hashes
    ChunkHashArgs *a = (ChunkHashArgs *)p;
    SmallProofHost &h = *a->h;
    try {
        challenge_midstates_host((uint32_t *)(h.dig + 32 * a->first), h.blobs + a->first * (size_t)kBlobBytes, a->count, a->be_fields);
    } catch (...) {
        memset(h.dig + 32 * a->first, 0, 32 * a->count);
    }
    delete a;
}
static void chunk_hash_host_fn(void *p) {
    ChunkHashArgs *a = (ChunkHashArgs *)p;
    SmallProofHost &h = *a->h;
    try {
        challenge_digests_host(h.dig + 32 * a->first, h.blobs + a->first * (size_t)kBlobBytes, h.comm + 48 * a->first, a->count, a->be_fields);
    } catch (...) {
        memset(h.dig + 32 * a->first, 0, 32 * a->count);   // (host_parallel_for does not throw; a wrong digest would show as a wrong proof, never silently)
    }
    delete a;
}

// Mid-size host-assisted hashing: the blobs leave on `sc` chunk by chunk and every chunk's host function runs on `sf` once its copy
// has landed. All argument blocks are allocated BEFORE anything is enqueued (an allocation failure returns with nothing in flight);
// if a host function cannot be launched, `join` is made to wait for everything this function has put in flight -- the side copies and
// the host functions already queued -- so that the caller can return the error without leaving work running against its buffers and
// the context's staging.
static C_KZG_RET chunk_host_functions(Ctx *c, const uint8_t *blobs, size_t n, hipStream_t sc, hipStream_t sf, hipStream_t join,
                                      void (*fn)(void *), const char *prof_name, bool be_fields, bool record_hashed = false) {
    SmallProofHost &h = c->sph;
    const size_t per = (n + mid_proof_chunks() - 1) / mid_proof_chunks();
    std::vector<ChunkHashArgs *> args;
    for (size_t first = 0; first < n; first += per) {
        ChunkHashArgs *a = new (std::nothrow) ChunkHashArgs{&h, first, n - first < per ? n - first : per, be_fields};
        if (!a) {
            for (ChunkHashArgs *b : args) delete b;
            return C_KZG_MALLOC;
        }
        args.push_back(a);
    }
    for (size_t k = 0; k < args.size(); k++) {
        const size_t first = args[k]->first, cnt = args[k]->count;
        hipError_t e = hipMemcpyAsync(h.blobs + first * (size_t)kBlobBytes, blobs + first * (size_t)kBlobBytes, cnt * (size_t)kBlobBytes,
                                      hipMemcpyDeviceToHost, sc);
        if (e == hipSuccess) e = hipEventRecord(h.chunk_done[k], sc);
        if (e == hipSuccess) e = hipStreamWaitEvent(sf, h.chunk_done[k], 0);
        bool queued = false;   // once the host function is in the queue args[k] is ITS to delete (a failing event record
                               // behind a successful launch freed it here as well -- a use-after-free in the callback, then a double free)
        if (e == hipSuccess) {
            ProfScope p(prof_name, sf);
            e = hipLaunchHostFunc(sf, fn, args[k]);
            queued = e == hipSuccess;
        }
        if (e == hipSuccess && record_hashed) e = hipEventRecord(h.hashed[k], sf);
        if (e != hipSuccess) {
            for (size_t j = queued ? k + 1 : k; j < args.size(); j++) delete args[j];
            set_error("host-assisted challenge: %s", hipGetErrorString(e));
            (void)hipGetLastError();
            if (hipEventRecord(c->ev_join[kMaxSplit - 2], sc) == hipSuccess) hipStreamWaitEvent(join, c->ev_join[kMaxSplit - 2], 0);
            if (sf != join && hipEventRecord(c->ev_join[kMaxSplit - 3], sf) == hipSuccess) hipStreamWaitEvent(join, c->ev_join[kMaxSplit - 3], 0);
            return C_KZG_ERROR;
        }
    }
    return C_KZG_OK;
}

struct SmallProofArgs {
    SmallProofHost *h;
    size_t n;
    int32_t bad;
    bool be_fields;
};

// runs on the runtime's callback thread, in stream order, between the copies out and the copies back: no HIP calls in here
static void small_proof_host_fn(void *p) {
    SmallProofArgs *a = (SmallProofArgs *)p;
    SmallProofHost &h = *a->h;
    try {
        challenge_digests_host(h.dig, h.blobs, h.comm, a->n, a->be_fields);     // compute_challenge, src/utils.rs:120-154, over the caller's commitment bytes
        std::vector<int> vrc(a->n);
        host_validate_commitments(h.comm, h.canon, vrc.data(), a->n);  // src/lib.rs:372-375: decompress + subgroup check; canonical re-compression
        for (size_t i = 0; i < a->n; i++) h.code[i] = vrc[i] == 2 ? a->bad : 0;
    } catch (...) {
        for (size_t i = 0; i < a->n; i++) h.code[i] = kStatusError;
    }
    delete a;
}

// engine_internal.h: CallWords. The long block holds z, the canonical commitment bytes, the status words and the validation's scratch of a
// call longer than one chunk (first 2 * kMaxChunk blobs, then doubling)
static size_t carve_words(CallWords &o, uint8_t *base, size_t cap) {
    Carver cv(base);
    cv.take(o.z, cap * sizeof(Fr));
    cv.take(o.canon, cap * 48);
    cv.take(o.status, cap * 4);
    cv.take(o.val_pts, cap * sizeof(G1Affine29));
    cv.take(o.val_kind, cap * 4);
    cv.take(o.val_verdict, cap * 4);
    return cv.bytes();
}
C_KZG_RET call_words(Ctx *c, size_t n, int32_t *caller_status, CallWords &out) {
    Workspace &w = c->ws;
    if (n > kMaxChunk) {
        const C_KZG_RET rc = grow_reserve(c->long_words, n, 2 * kMaxChunk, [](size_t cap) { CallWords probe; return carve_words(probe, nullptr, cap); }, nullptr);
        if (rc == C_KZG_MALLOC) set_error("proof batch of %zu blobs: out of device memory for the challenges", n);
        if (rc != C_KZG_OK) return rc;
        carve_words(out, c->long_words.dev, c->long_words.cap);
    } else {
        out = CallWords{w.status, w.z, w.canon48, w.val_pts, w.val_kind, w.val_verdict};
    }
    if (caller_status) out.status = caller_status;
    return C_KZG_OK;
}

// ---- blob proofs: the call's constants, a head per schedule of plan.h (everything in front of the MSM), one tail ------------------------
struct ProofCall {
    Ctx *c;
    uint8_t *out48;
    const uint8_t *blobs, *comm48;
    size_t n;
    int mode;
    hipStream_t st;   // (so far blob_proof_batch_device's arguments; begin() fills in the rest)
    ModeRules mr;
    int le, fs;       // the byte order of digests and outputs; what the hash kernels are told
    CallWords cw;
    bool evf;        // proof_in_evaluation_form (then the quotient's MSM runs on the Lagrange form's table)
    ProofPlan plan;
    SmallProofArgs *host_args;   // kProofSmallHost: the argument block (its host function deletes it)

    // the reservation, the status words cleared, and the plan
    C_KZG_RET begin(int32_t *status) {
        C_KZG_RET rc = ctx_reserve(c, n);
        if (rc != C_KZG_OK) return rc;
        if ((rc = call_words(c, n, status, cw)) != C_KZG_OK) return rc;
        mr = mode_rules(mode);
        le = mr.le(), fs = mr.hash_rule();
        LWK_HIP(hipMemsetAsync(cw.status, 0, n * 4, st));
        // lib.rs:372-375: the commitment is decompressed (and subgroup-checked) first. Validation (a long scalar
        // multiplication per lane) and hashing (131 KB per lane pair) are both latency chains whose run time does not depend
        // on the number of blobs (2 ms and 3.2 ms for anything from 64 blobs to one workgroup per compute unit, 16k), and independent as long as
        // the caller's bytes are the canonical encoding, which they are except for exotic encodings of infinity: ALL
        // blobs of the call are hashed optimistically from the caller's bytes on `st` while the validation stream
        // validates all commitments, then only the lanes whose canonical bytes differ are redone. A call of several chunks
        // therefore pays the two chains once, not once per chunk.
        // WHICH schedule runs in front of the MSM is a pure function of the batch, the host threads' warmth, the other context's state, the
        // table forms and the knobs (plan.h: plan_proof_call; the table is pinned by tests/test_plan_cpu.py). The engine's part: the inputs,
        // the pinned staging the host-assisted schedules need (asked for only when the plan wants it; if it cannot be had the plan is taken
        // again without it), and the launches.
        evf = proof_in_evaluation_form(c, mode);
        const bool msm_direct = evf ? c->lag.direct_table != nullptr : c->direct_table && !proof_on_lagrange(c, mode);
        const bool warm = host_assist_warm(), busy = peer_busy(c);
        const PlanKnobs pk = plan_knobs();
        plan = plan_proof_call(n, warm, busy, msm_direct, true, pk);
        const int forced = knobs().proof_schedule;   // experiment: tests/test_gpu_plan.py runs every schedule once on the same inputs
        if (forced >= 0 && forced <= kProofGpuChains && n <= kMaxChunk) {
            PlanKnobs fk = pk;
            fk.small_proof_host = forced == kProofSmallHost ? kMaxChunk : 0;
            fk.mid_proof_host = forced == kProofSmallHost || forced == kProofGpuChains ? 0 : kMaxChunk;
            fk.mid_proof_pipe = forced == kProofMidPiped;
            fk.mid_proof_pipe_min = 0;
            plan = plan_proof_call(n, forced != kProofMidCold, false, forced == kProofMidPiped ? msm_direct : false, true, fk);
        }
        if (plan.needs_staging()) {
            bool ok = sph_reserve(c, n);
            if (ok && plan.schedule == kProofSmallHost) {
                host_args = new (std::nothrow) SmallProofArgs{&c->sph, n, mr.bad_status(), mr.be_transcript};
                ok = host_args != nullptr;
            }
            if (!ok) plan = plan_proof_call(n, warm, busy, msm_direct, false, pk);
        }
        g_last_proof_schedule.store((int)plan.schedule, std::memory_order_relaxed);
        return C_KZG_OK;
    }

    // the validation of ALL the call's commitments on the validation stream, forked from the call's stream; its end is ev_join[0]. `also`:
    // further streams the head forks, made to wait for ev_fork before the validation is submitted
    C_KZG_RET fork_validation(const hipStream_t *also = nullptr, int n_also = 0) {
        LWK_HIP(hipEventRecord(c->ev_fork, st));
        LWK_HIP(hipStreamWaitEvent(c->vstream, c->ev_fork, 0));
        for (int k = 0; k < n_also; k++) LWK_HIP(hipStreamWaitEvent(also[k], c->ev_fork, 0));
        launch_validate_commitments(comm48, cw.canon, cw.status, mr.bad_status(), n, c->vstream, cw.val_pts, cw.val_kind, cw.val_verdict);
        LWK_HIP(hipEventRecord(c->ev_join[0], c->vstream));
        return C_KZG_OK;
    }

    // A small call: both chains above cost their full 2-3 ms for a handful of blobs, and the host does the same work in a tenth
    // of that (3.63 ms device-resident against 0.82 ms through the host-pointer ABI at one blob). The blobs and
    // commitments go out to pinned memory, a host function hashes and validates them on the host threads IN STREAM ORDER (the
    // call stays asynchronous), digests, verdicts and canonical bytes come back; a lane whose canonical commitment bytes differ
    // from the caller's (an exotic encoding of infinity) is rehashed on the GPU as in the large-batch path.
    C_KZG_RET head_small_host() {
        Workspace &w = c->ws;
        SmallProofHost &h = c->sph;
        LWK_HIP(hipMemcpyAsync(h.blobs, blobs, n * (size_t)kBlobBytes, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipMemcpyAsync(h.comm, comm48, n * 48, hipMemcpyDeviceToHost, st));
        {
            ProfScope p("host_challenge_and_validate", st);
            hipError_t e = hipLaunchHostFunc(st, small_proof_host_fn, host_args);
            if (e != hipSuccess) {
                delete host_args;
                set_error("hipLaunchHostFunc failed: %s", hipGetErrorString(e));
                return C_KZG_ERROR;
            }
        }
        LWK_HIP(hipMemcpyAsync(cw.status, h.code, n * 4, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(w.zbytes, h.dig, n * 32, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(cw.canon, h.canon, n * 48, hipMemcpyHostToDevice, st));
        launch_z_from_bytes(w.zbytes, cw.z, nullptr, le, n, st);  // digest -> Fr, reduced (utils.rs:148-154)
        launch_challenge(blobs, cw.canon, cw.z, fs, n, st, comm48);
        return C_KZG_OK;
    }

    // the two chains on the GPU: the validation on its side stream, the hash on the call's. `wake` (kProofMidCold): a mid-size call, host
    // threads cold: the GPU's hash kernel this once, and a nudge for the threads on the side stream
    C_KZG_RET head_gpu_chains(bool wake) {
        const C_KZG_RET rc = fork_validation();
        if (rc != C_KZG_OK) return rc;
        // (the wake-up on a stream this call does not wait for: on the validation's stream, in front of the join event, the first call of a
        // process paid for the creation of the thread pool)
        if (wake) launch_host_wake(c);
        launch_challenge(blobs, comm48, cw.z, fs, n, st);
        LWK_HIP(hipStreamWaitEvent(st, c->ev_join[0], 0));
        launch_challenge(blobs, cw.canon, cw.z, fs, n, st, comm48);
        return C_KZG_OK;
    }

    // mid-size call on a settings object whose other context is idle (a producer that alternates two caller streams hides the GPU's hash
    // behind the other call's MSM at no cost, and two calls' host hashing would queue for the same host threads: 70.9k against 49.7k
    // proofs/s at 256 blobs on two streams -- there the hash kernel stays): the validation on the GPU's side stream as in the large path; the hashing on the host threads, chunk by chunk
    // while the next chunk is still being copied out (side stream c->aux[0], one event per chunk)
    // This is the front both mid-size heads share; piped: the host functions on c->aux[1], an event behind each, else on the call's stream
    C_KZG_RET mid_host_front(bool piped) {
        const hipStream_t side[2] = {c->aux[0], c->aux[1]}, sc = side[0], sh = side[1];
        C_KZG_RET rc = fork_validation(side, piped ? 2 : 1);
        if (rc != C_KZG_OK) return rc;
        LWK_HIP(hipMemcpyAsync(c->sph.comm, comm48, n * 48, hipMemcpyDeviceToHost, sc));
        rc = chunk_host_functions(c, blobs, n, sc, piped ? sh : st, st, chunk_hash_host_fn, "host_challenge_chunk", mr.be_transcript, piped);
        if (rc != C_KZG_OK) hipStreamWaitEvent(st, c->ev_join[0], 0);   // the validation on the side stream: nothing of this call outlives `st`
        return rc;
    }

    C_KZG_RET head_mid_host() {
        Workspace &w = c->ws;
        const C_KZG_RET rc = mid_host_front(false);
        if (rc != C_KZG_OK) return rc;
        LWK_HIP(hipMemcpyAsync(w.zbytes, c->sph.dig, n * 32, hipMemcpyHostToDevice, st));
        launch_z_from_bytes(w.zbytes, cw.z, nullptr, le, n, st);  // digest -> Fr, reduced (utils.rs:148-154)
        LWK_HIP(hipStreamWaitEvent(st, c->ev_join[0], 0));
        launch_challenge(blobs, cw.canon, cw.z, fs, n, st, comm48);   // only the lanes whose canonical commitment bytes differ from the caller's
        return C_KZG_OK;
    }

    // PIPELINED when the quotient's MSM runs on a monomial direct table (r05): the host functions run on a stream of their own, the
    // first half's quotient and MSM start as soon as ITS chunks are hashed -- beside the hashing of the second half, and without
    // waiting for the validation either (2 ms flat on its side stream): the challenges are taken over the caller's commitment
    // bytes, and once the validation's canonical bytes exist a blob whose bytes were NOT canonical (a valid point in an exotic
    // encoding: infinity with stray bits) gets its challenge, quotient and MSM again in a second pass that exits at its first
    // instruction for every other blob. 256 blobs: hash 2.1 ms -> MSM 2.3 ms in series becomes 1.05 -> 1.2 || 1.05 -> 1.2.
    // (plan.h decides `piped`: the knob, a direct table under the quotient's MSM, at least mid_proof_pipe_min blobs -- 128 blobs: 3.3 ms
    // pipelined, 2.9 not --, an even number of chunks, one launch set)
    // This head finishes the call itself: no tail behind it.
    C_KZG_RET head_mid_piped() {
        Workspace &w = c->ws;
        SmallProofHost &h = c->sph;
        Fr *z = cw.z;
        const C_KZG_RET rc = mid_host_front(true);
        if (rc != C_KZG_OK) return rc;
        const size_t per = plan.per_chunk;
        // sub-batches of whole chunks, alternating between the call's stream and a second one: a sub-batch's quotient and MSM start
        // when ITS chunks are hashed, and its latency-shaped folds run beside the next sub-batch's accumulation
        // (plan.h: four measured best at 256 while the validation took 2 ms; with 1.1 ms of it two win there, 61.9k against 59.7k proofs/s; at 384 four: 66.0k against 63.7k)
        const size_t parts = plan.parts;
        const size_t cps = plan.chunks / parts;   // chunks per sub-batch
        uint32_t *differs = w.perm;   // (bucket-engine scratch, idle on a direct table: one word per blob)
        hipStream_t s2 = c->aux[2];
        LWK_HIP(hipStreamWaitEvent(s2, c->ev_fork, 0));
        for (size_t j = 0; j < parts; j++) {
            const size_t off = j * cps * per, end_ = (j + 1) * cps * per < n ? (j + 1) * cps * per : n;
            if (off >= end_) continue;
            const size_t m = end_ - off;
            hipStream_t sk = (j & 1) ? s2 : st;
            LWK_HIP(hipStreamWaitEvent(sk, h.hashed[(j + 1) * cps - 1], 0));
            LWK_HIP(hipMemcpyAsync(w.zbytes + 32 * off, h.dig + 32 * off, m * 32, hipMemcpyHostToDevice, sk));
            launch_z_from_bytes(w.zbytes + 32 * off, z + off, nullptr, le, m, sk);
            coefficients_stage(c, blobs + off * (size_t)kBlobBytes, m, mode, cw.status + off, sk, off);
            quotient_stage(c, mode, w.scalars + off * (size_t)kBlobElems * 8, z + off, w.scalars2 + off * (size_t)kBlobElems * 8, nullptr, le, m, sk);
            (void)msm_sums_stage(c, w.scalars2 + off * (size_t)kBlobElems * 8, m, sk, off, false, evf);
        }
        LWK_HIP(hipEventRecord(c->ev_join[2], s2));
        LWK_HIP(hipStreamWaitEvent(st, c->ev_join[2], 0));
        // the second pass: only the blobs whose commitment bytes were not the canonical encoding
        LWK_HIP(hipStreamWaitEvent(st, c->ev_join[0], 0));
        launch_flag_differs48(cw.canon, comm48, differs, n, st);
        launch_challenge(blobs, cw.canon, z, fs, n, st, comm48);
        quotient_stage(c, mode, w.scalars, z, w.scalars2, nullptr, le, n, st, differs);
        launch_direct_msm_only(evf ? c->lag.direct_bits : c->direct_bits, evf ? c->lag.direct_tab.win_dev : c->direct_tab.win_dev,
                               evf ? c->lag.direct_row_bytes : c->direct_row_bytes, w.scalars2, w.sums, differs, n, st);
        launch_finalize_compress(w.sums, out48, n, st);
        return C_KZG_OK;
    }

    // the ALU-bound phase: in turns with the settings' other context (engine.h: heavy_done), so that THIS call's hash
    // above ran beside the other call's MSM and the other call's next hash runs beside this one
    C_KZG_RET msm_tail() {
        Workspace &w = c->ws;
        Ctx *pr = c->primary;
        // (up to half a chunk: there the MSM is about as long as the hash and the two pipelines would phase-lock; a longer
        // MSM covers the other call's hash by itself, and taking turns only adds bubbles -- 81k against 90k proofs/s at 1024)
        const bool heavy_serial = plan.heavy_serial;
        if (heavy_serial) {
            std::lock_guard<std::mutex> hk(pr->heavy_mu);
            LWK_HIP(hipStreamWaitEvent(st, pr->heavy_done, 0));
        }
        for (size_t off = 0; off < n; off += kMaxChunk) {
            size_t m = n - off < kMaxChunk ? n - off : kMaxChunk;
            coefficients_stage(c, blobs + off * (size_t)kBlobBytes, m, mode, cw.status + off, st);
            quotient_stage(c, mode, w.scalars, cw.z + off, w.scalars2, nullptr, le, m, st);
            G1Xyzz29 *sums = msm_sums_stage(c, w.scalars2, m, st, 0, false, quotient_to_msm_form(c, mode, m, st));
            if (heavy_serial && off + kMaxChunk >= n) {  // the last accumulation is in the queue: the other context's phase may follow it
                std::lock_guard<std::mutex> hk(pr->heavy_mu);
                LWK_HIP(hipEventRecord(pr->heavy_done, st));
            }
            launch_finalize_compress(sums, out48 + 48 * off, m, st);
        }
        return C_KZG_OK;
    }
};

C_KZG_RET blob_proof_batch_device(Ctx *c, uint8_t *out48, const uint8_t *blobs, const uint8_t *comm48, size_t n, int mode,
                                  hipStream_t st, int32_t *status) {
    ProofCall p{c, out48, blobs, comm48, n, mode, st};
    C_KZG_RET rc = p.begin(status);
    if (rc != C_KZG_OK) return rc;
    switch (p.plan.schedule) {
    case kProofSmallHost: rc = p.head_small_host(); break;
    case kProofMidCold: rc = p.head_gpu_chains(true); break;
    case kProofMidHost: rc = p.head_mid_host(); break;
    case kProofMidPiped: return p.head_mid_piped();
    case kProofGpuChains: rc = p.head_gpu_chains(false); break;
    }
    return rc != C_KZG_OK ? rc : p.msm_tail();
}

// Commitment AND blob proof of every blob in one pass (what a blob producer needs: lib.rs:253-283 followed by
// lib.rs:361-404 on its own output). Two things a pair of separate calls cannot do: the 2048 blocks of the Fiat-Shamir
// hash that do not depend on the commitment (all but the last 32 bytes of the blob) run on the side stream BESIDE the
// commitment MSMs and only the last two blocks wait for the commitments (k_challenge_finish) -- the 3.3 ms hash phase
// that stands in front of a proof call's MSM disappears -- and the blob is parsed (mode C: transformed) once. The
// commitments are the library's own output: nothing to validate. Results are those of the two calls, byte for byte.
C_KZG_RET commit_and_prove_batch_device(Ctx *c, uint8_t *comm_out48, uint8_t *proof_out48, const uint8_t *blobs, size_t n, int mode,
                                        hipStream_t st, int32_t *status) {
    C_KZG_RET rc = ctx_reserve(c, n);
    if (rc != C_KZG_OK) return rc;
    CallWords cw;
    if ((rc = call_words(c, n, status, cw)) != C_KZG_OK) return rc;
    Workspace &w = c->ws;
    const ModeRules mr = mode_rules(mode);
    const int le = mr.le(), fs = mr.hash_rule();   // the byte order of digests and outputs; what the hash kernels are told
    int32_t *stt = cw.status;
    Fr *z = cw.z;
    uint32_t *mid = (uint32_t *)cw.canon;  // 32 of the 48 bytes per blob this call has no other use for
    LWK_HIP(hipMemsetAsync(stt, 0, n * 4, st));
    LWK_HIP(hipEventRecord(c->ev_fork, st));
    LWK_HIP(hipStreamWaitEvent(c->vstream, c->ev_fork, 0));
    // mid-size calls on a settings object whose other context is idle: the commitment-free part of the hashes on the host threads,
    // chunk by chunk beside the copy out (as blob_proof_batch_device does for whole hashes), instead of the 3.2 ms kernel beside the MSM
    const bool host_cold = n <= mid_proof_host_limit() && !peer_busy(c) && !host_assist_warm();
    if (host_cold) launch_host_wake(c);   // (the GPU kernel this once; the wake-up on a stream this call does not wait for)
    const bool host_mid = !host_cold && n <= mid_proof_host_limit() && !peer_busy(c) && sph_reserve(c, n);
    if (host_mid) {
        SmallProofHost &h = c->sph;
        hipStream_t sc = c->aux[0];
        LWK_HIP(hipStreamWaitEvent(sc, c->ev_fork, 0));
        {
            const C_KZG_RET rch = chunk_host_functions(c, blobs, n, sc, c->vstream, st, chunk_midstate_host_fn, "host_midstate_chunk", mr.be_transcript);
            if (rch != C_KZG_OK) return rch;   // (st has been made to wait for both side streams)
        }
        LWK_HIP(hipMemcpyAsync(mid, h.dig, n * 32, hipMemcpyHostToDevice, c->vstream));
    } else {
        launch_challenge_midstate(blobs, mid, n, c->vstream, mr.be_transcript);  // ALL blobs of the call: a latency chain, as long for 64 blobs as for 16k
    }
    LWK_HIP(hipEventRecord(c->ev_join[0], c->vstream));
    for (size_t off = 0; off < n; off += kMaxChunk) {
        const size_t m = n - off < kMaxChunk ? n - off : kMaxChunk;
        const uint8_t *b = blobs + off * (size_t)kBlobBytes;
        if (coefficients_stage(c, b, m, mode, stt + off, st)) {  // evaluations: commitment and quotient both on the Lagrange form
            msm_stages(c, w.scalars, comm_out48 + 48 * off, m, st, 0, off == 0 && !host_mid, true);
        } else if (proof_on_lagrange(c, mode)) {  // coefficients for the quotient, but the only direct table is the Lagrange one: the commitment comes from the evaluations as they stand
            if (le) launch_copy_le_check(b, (uint32_t *)w.fr, nullptr, m, st);
            else launch_copy_be_check(b, (uint32_t *)w.fr, nullptr, m, st);
            msm_stages(c, (const uint32_t *)w.fr, comm_out48 + 48 * off, m, st, 0, off == 0 && !host_mid, true);
        } else {
            msm_stages(c, w.scalars, comm_out48 + 48 * off, m, st, 0, off == 0 && !host_mid);  // the first one has the hash kernel beside it
        }
        if (off == 0) LWK_HIP(hipStreamWaitEvent(st, c->ev_join[0], 0));
        launch_challenge_finish(b, comm_out48 + 48 * off, mid + 8 * off, z + off, fs, m, st);
        quotient_stage(c, mode, w.scalars, z + off, w.scalars2, nullptr, le, m, st);
        msm_stages(c, w.scalars2, proof_out48 + 48 * off, m, st, 0, false, quotient_to_msm_form(c, mode, m, st));
    }
    return C_KZG_OK;
}

C_KZG_RET point_proof_batch_device(Ctx *c, uint8_t *proof48, uint8_t *y32, const uint8_t *blobs, const uint8_t *z32,
                                   size_t n, int mode, hipStream_t st, int32_t *status, const G1Xyzz29 **sums_out) {
    C_KZG_RET rc = ctx_reserve(c, n);
    if (rc != C_KZG_OK) return rc;
    Workspace &w = c->ws;
    const ModeRules mr = mode_rules(mode);
    const int le = mr.le();
    for (size_t off = 0; off < n; off += kMaxChunk) {
        size_t m = n - off < kMaxChunk ? n - off : kMaxChunk;
        CallWords cw;   // (of one chunk: the workspace's own arrays, nothing to reserve)
        if ((rc = call_words(c, m, status ? status + off : nullptr, cw)) != C_KZG_OK) return rc;
        int32_t *stt = cw.status;
        LWK_HIP(hipMemsetAsync(stt, 0, m * 4, st));
        coefficients_stage(c, blobs + off * (size_t)kBlobBytes, m, mode, stt, st);
        launch_z_from_bytes(z32 + 32 * off, cw.z, stt, mr.scalar_rule(), m, st);
        quotient_stage(c, mode, w.scalars, cw.z, w.scalars2, y32 + 32 * off, le, m, st);
        const bool lg = quotient_to_msm_form(c, mode, m, st);
        if (sums_out && n <= kMaxChunk) *sums_out = msm_sums_stage(c, w.scalars2, m, st, 0, false, lg);   // the caller finishes on the host
        else msm_stages(c, w.scalars2, proof48 + 48 * off, m, st, 0, false, lg);
    }
    return C_KZG_OK;
}

}  // namespace lwk
