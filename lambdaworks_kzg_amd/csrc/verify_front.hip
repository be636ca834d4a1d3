// verify_front.hip -- the front of a batch verification (host side, HIP runtime): the verify scratch, the per-blob pass over host-pointer,
// staged, long and device-resident inputs, and the three linear combinations behind it. verify.hip and verify_each.hip call it
// through engine.h.
#include "carve.h"
#include "engine_internal.h"

#include <stdio.h>
#include <string.h>

#include <vector>

namespace lwk {

// ------------------------------------------------------------------------------------------------
// verify-side helpers: host buffers in and out, kernels in between

void verify_buffers_free(VerifyBuffers &v) {
    dev_free(v.pts_c);
    dev_free(v.pts_p);
    dev_free(v.mult_c);
    dev_free(v.mult_p);
    dev_free(v.kind_c);
    dev_free(v.kind_p);
    dev_free(v.proof_in);
    dev_free(v.comm_in);
    dev_free(v.canon_dev);
    dev_free(v.status_all);
    dev_free(v.verdict_c);
    dev_free(v.verdict_p);
    dev_free(v.d_r);
    dev_free(v.d_rz);
    dev_free(v.d_aff);
    dev_free(v.d_part);
    dev_free(v.d_inf);
    dev_free(v.vm_base);
    dev_free(v.d_rec);
    if (v.h_rec) {
        (void)hipHostFree(v.h_rec);
        v.h_rec = nullptr;
    }
    v.rec_cap = 0;
    v.tab_p = v.tab_c = nullptr;
    v.vm_tmp = v.vm_partial = v.vm_bsum = nullptr;
    v.vm_pre = nullptr;
    v.sc_a = v.sc_b = nullptr;
    v.vm_pw = nullptr;
    if (v.h_pin) {
        (void)hipHostFree(v.h_pin);
        v.h_pin = nullptr;
    }
    if (v.vm_done) {
        (void)hipEventDestroy(v.vm_done);
        v.vm_done = nullptr;
    }
}

void vs_free(Ctx *c) {
    verify_buffers_free(c->vs);
    c->vs_cap = 0;
}

// the pieces of vm_base for `cap` blobs; the byte count of the whole (base == nullptr: the size probe)
static size_t carve_vmsm(VerifyBuffers &v, uint8_t *base, size_t cap) {
    Carver cv(base);
    cv.take(v.tab_p, (size_t)kVmsmRows * cap * sizeof(G1Affine29));
    cv.take(v.tab_c, (size_t)kVmsmRows * cap * sizeof(G1Affine29));
    cv.take(v.vm_tmp, (size_t)kVmsmSteps * 2 * cap * sizeof(G1Xyzz29));
    cv.take(v.vm_pre, (size_t)kVmsmSteps * 2 * cap * sizeof(F29<2>));
    cv.take(v.sc_a, 32 * cap);
    cv.take(v.sc_b, 32 * cap);
    cv.take(v.vm_partial, 3 * vmsm_max_slices(cap) * 256 * sizeof(G1Xyzz29));
    cv.take(v.vm_bsum, 3 * 256 * sizeof(G1Xyzz29));
    cv.take(v.vm_pw, kVmsmPwSlots * sizeof(Fr));   // (behind the 33 powers: the skip word and sum r^i y_i of an asynchronous verification)
    return cv.bytes();
}

// device scratch of one batch verification of up to `cap` blobs
C_KZG_RET verify_buffers_alloc(VerifyBuffers &v, size_t cap) {
    const size_t nblk = lincomb3_blocks(cap);
    bool ok = hipMalloc((void **)&v.pts_c, cap * sizeof(G1Affine29)) == hipSuccess &&
              hipMalloc((void **)&v.pts_p, cap * sizeof(G1Affine29)) == hipSuccess &&
              hipMalloc((void **)&v.mult_c, 3 * cap * sizeof(G1Affine29)) == hipSuccess &&
              hipMalloc((void **)&v.mult_p, 3 * cap * sizeof(G1Affine29)) == hipSuccess &&
              hipMalloc((void **)&v.kind_c, cap * 4) == hipSuccess && hipMalloc((void **)&v.kind_p, cap * 4) == hipSuccess &&
              hipMalloc((void **)&v.proof_in, cap * 48) == hipSuccess && hipMalloc((void **)&v.d_r, cap * 32) == hipSuccess &&
              hipMalloc((void **)&v.comm_in, cap * 48) == hipSuccess && hipMalloc((void **)&v.canon_dev, 2 * cap * 48) == hipSuccess &&
              hipMalloc((void **)&v.status_all, cap * 4) == hipSuccess &&
              hipMalloc((void **)&v.verdict_c, cap * 4) == hipSuccess && hipMalloc((void **)&v.verdict_p, cap * 4) == hipSuccess &&
              hipMalloc((void **)&v.d_rz, cap * 32) == hipSuccess &&
              hipMalloc((void **)&v.d_part, (3 * nblk + 3) * sizeof(G1Xyzz29)) == hipSuccess &&
              hipMalloc((void **)&v.d_aff, 3 * 96) == hipSuccess && hipMalloc((void **)&v.d_inf, 3 * 4) == hipSuccess;
    // vmsm.hip's scratch: one allocation, 256-byte aligned pieces
    if (ok) {
        ok = hipMalloc((void **)&v.vm_base, carve_vmsm(v, nullptr, cap)) == hipSuccess &&
             hipHostMalloc((void **)&v.h_pin, kVmsmPinBytes, hipHostMallocDefault) == hipSuccess &&
             hipMalloc((void **)&v.d_rec, 160 * cap + 16) == hipSuccess &&
             hipHostMalloc((void **)&v.h_rec, 160 * cap + 16, hipHostMallocDefault) == hipSuccess &&
             hipEventCreateWithFlags(&v.vm_done, hipEventDisableTiming) == hipSuccess;
        if (ok) {
            v.rec_cap = cap;
            carve_vmsm(v, v.vm_base, cap);
        }
    }
    if (!ok) {
        (void)hipGetLastError();
        verify_buffers_free(v);
        set_error("verify scratch for %zu blobs: out of device memory", cap);
        return C_KZG_MALLOC;
    }
    return C_KZG_OK;
}

// a verification that runs on the context's scratch (under verify_mu) sees it through its own VerifyBuffers
static void verify_buffers_lend(VerifyBuffers &vb, const VerifyBuffers &v) {
    vb.mult_c = v.mult_c; vb.mult_p = v.mult_p;
    vb.pts_c = v.pts_c; vb.pts_p = v.pts_p; vb.kind_c = v.kind_c; vb.kind_p = v.kind_p; vb.proof_in = v.proof_in;
    vb.d_r = v.d_r; vb.d_rz = v.d_rz; vb.d_aff = v.d_aff; vb.d_part = v.d_part; vb.d_inf = v.d_inf;
    vb.comm_in = v.comm_in; vb.canon_dev = v.canon_dev; vb.status_all = v.status_all; vb.verdict_c = v.verdict_c; vb.verdict_p = v.verdict_p;
    vb.vm_base = nullptr;   // (not this object's to free)
    vb.tab_p = v.tab_p; vb.tab_c = v.tab_c; vb.vm_tmp = v.vm_tmp; vb.vm_pre = v.vm_pre; vb.sc_a = v.sc_a; vb.sc_b = v.sc_b;
    vb.vm_partial = v.vm_partial; vb.vm_bsum = v.vm_bsum; vb.vm_pw = v.vm_pw; vb.h_pin = v.h_pin; vb.vm_done = v.vm_done;
    vb.d_rec = v.d_rec; vb.h_rec = v.h_rec; vb.rec_cap = v.rec_cap;
}

// the rows of both point sets for the linear combinations, on `st` (needs the decompressed points, not the subgroup verdicts):
// vmsm.hip's 32 byte-spaced rows per point, or (LWKZG_VERIFY_MSM=0) r05's three 32-bit-spaced multiples
static void launch_verify_rows(VerifyBuffers &vb, size_t n, hipStream_t st, bool apart) {
    if (knobs().verify_msm)
        launch_vmsm_multiples2(vb.pts_p, vb.kind_p, vb.tab_p, vb.pts_c, vb.kind_c, vb.tab_c, vb.vm_tmp, vb.vm_pre, n, st, apart);
    else
        launch_point_multiples(vb.pts_p, vb.kind_p, vb.mult_p, n, st, vb.pts_c, vb.kind_c, vb.mult_c);
}

// grow-only verify scratch for n blobs; the caller holds verify_mu
static C_KZG_RET vs_reserve(Ctx *c, size_t n) {
    if (c->vs_cap >= n) return C_KZG_OK;
    LWK_HIP(hipDeviceSynchronize());  // the validation / multiples streams included
    vs_free(c);
    size_t cap = 64;
    while (cap < n) cap <<= 1;
    C_KZG_RET rc = verify_buffers_alloc(c->vs, cap);
    if (rc != C_KZG_OK) return rc;
    c->vs_cap = cap;
    return C_KZG_OK;
}

// the device scratch a verification of n blobs runs on. vb.owned: the caller's VerifyBuffers brings its own (allocated on first use);
// otherwise the context's grow-only scratch is lent out (the caller holds verify_mu)
static C_KZG_RET verify_buffers_take(Ctx *c, VerifyBuffers &vb, size_t n) {
    if (vb.owned) {
        if (!vb.pts_c) {
            C_KZG_RET rcv = verify_buffers_alloc(vb, n < 64 ? 64 : n);
            if (rcv != C_KZG_OK) return rcv;
        }
    } else {
        C_KZG_RET rcv = vs_reserve(c, n);
        if (rcv != C_KZG_OK) return rcv;
        verify_buffers_lend(vb, c->vs);
    }
    return C_KZG_OK;
}

// ---- long host-pointer verifications, r06 second form: the device-resident pipeline behind an upload --------------------------------------
// verify_prepare_long below hashes every blob on the host threads, slice by slice beside the upload -- and on a host whose container gets
// ~32 hardware threads that is the longest stage of its pipeline: 1.78 ms of SHA-256 per 512-blob slice against 1.2 ms of upload, 4096 blobs
// in 16 ms of which the upload is 9.6 (profiles/r06_experiments.md section 9). Here ALL blobs go into one device buffer (537 MB for 4096 of the 288 GB), in
// slices on a copy stream, and the hashing is SHARED: the head of the batch is hashed by the GPU's kernel slice by slice as it lands (a
// 3.2 ms latency chain per launch whatever its size, hidden behind the uploads still to come), the tail by the host threads from the
// caller's memory, starting at once (their share is what they hash in 0.8 of the upload time at their measured rate). y = p(z) is then
// read straight from the uploaded blobs (k_eval_quotient_from_blobs / its evaluation-form twin: no coefficient slots to recycle).
// Reference mode and c-kzg mode on the Lagrange form; other forms, no memory for the buffer, or LWKZG_HOST_STAGE=0 (experiment): the
// sliced form below. `taken` says which. Caller holds c->mu.
static C_KZG_RET verify_prepare_staged(Ctx *c, const uint8_t *blobs, const uint8_t *comm48, const uint8_t *proofs48, size_t n, int mode,
                                       uint8_t *z32, uint8_t *y32, uint8_t *canon_c, uint8_t *canon_p, VerifyBuffers &vb, bool &taken) {
    taken = false;
    const ModeRules mr = mode_rules(mode);
    const int le = mr.le(), fs = mr.hash_rule();   // the byte order of digests and outputs; what the hash kernels are told
    const bool evf = proof_in_evaluation_form(c, mode);
    if (!knobs().host_stage || !(!mr.evaluation_form || evf) || n > ((size_t)1 << 17)) return C_KZG_OK;
    if (grow_reserve(c->vblobs, n, 2 * kMaxChunk, [](size_t cap) { return cap * (size_t)kBlobBytes; }, nullptr) != C_KZG_OK) return C_KZG_OK;
    uint8_t *d_all = c->vblobs.dev;
    CallWords cw;   // (the long block: only batches of more than a chunk come here)
    C_KZG_RET rc = call_words(c, n, nullptr, cw);
    if (rc != C_KZG_OK) return rc;
    taken = true;
    const int bad = mr.bad_status();
    // Four streams are at work at once here, and the runtime multiplexes a process's streams onto four hardware queues: a copy that shares
    // its queue with the validation kernels or with a 3.1 ms hash launch simply waits for them (uploads on aux[3]: 15.9 instead of 13.1 ms;
    // which side streams collide depends on what else the process has created). The uploads therefore get a HIGH-PRIORITY stream of their
    // own -- the runtime keeps a queue per priority level -- and every choice of hash stream then measures the same
    // (profiles/r06_experiments.md section 9). LWKZG_STAGE_STREAMS=c,h (experiment) puts them on side streams instead.
    hipStream_t st = c->stream, sv = c->vstream, sc = upload_stream(c), sh = c->aux[knobs().stage_streams[1]];
    Fr *z = cw.z;
    // who hashes what, and when the head's launches go out: plan.h: plan_staged_verification (pure; tests/test_plan_cpu.py pins its table)
    const StagedSplit split = plan_staged_verification(n, host_hash_rate());
    const size_t slice = split.slice, n_gpu = split.n_gpu, n_host = split.n_host, every = split.every;
    if (knobs().timing)
        fprintf(stderr, "[lambdaworks_kzg_amd] staged verification of %zu blobs: the GPU hashes the first %zu (a launch per %zu slices of %zu), the host threads the last %zu (they hashed %.1f GB/s lately)\n",
                n, n_gpu, every, slice, n_host, host_hash_rate() * 1e-9);
    std::vector<uint8_t> dig(32 * (n_host ? n_host : 1));
    SideTask hasher;   // joined by its destructor on every exit (digests assume canonical commitment bytes; the comparison below confirms or refutes that)
    if (n_host) hasher.start([&, n_gpu, n_host]() { challenge_digests_host(dig.data(), blobs + n_gpu * (size_t)kBlobBytes, comm48 + 48 * n_gpu, n_host, mr.be_transcript); });
    // up-front validation of every commitment (main stream) and every proof (validation stream), the rows of the linear combinations behind them
    LWK_HIP(hipMemcpyAsync(vb.comm_in, comm48, n * 48, hipMemcpyHostToDevice, st));
    LWK_HIP(hipMemsetAsync(vb.status_all, 0, n * 4, st));
    LWK_HIP(hipEventRecord(c->ev_fork, st));
    LWK_HIP(hipStreamWaitEvent(sv, c->ev_fork, 0));
    LWK_HIP(hipStreamWaitEvent(sc, c->ev_fork, 0));
    LWK_HIP(hipStreamWaitEvent(sh, c->ev_fork, 0));
    LWK_HIP(hipMemcpyAsync(vb.proof_in, proofs48, n * 48, hipMemcpyHostToDevice, sv));
    launch_validate_commitments(vb.proof_in, vb.canon_dev + 48 * n, vb.status_all, bad, n, sv, vb.pts_p, vb.kind_p, vb.verdict_p);
    launch_validate_commitments(vb.comm_in, vb.canon_dev, vb.status_all, bad, n, st, vb.pts_c, vb.kind_c, vb.verdict_c);
    LWK_HIP(hipEventRecord(c->ev_join[kMaxSplit - 2], st));
    LWK_HIP(hipStreamWaitEvent(sv, c->ev_join[kMaxSplit - 2], 0));
    launch_verify_rows(vb, n, sv, false);
    LWK_HIP(hipEventRecord(c->ev_join[kMaxSplit - 1], sv));
    // the uploads (this thread is inside a blocking pageable copy most of the time) and, behind each slice of the head, its hash
    size_t hashed = 0, landed = 0;   // slices
    for (size_t off = 0; off < n; off += slice) {
        const size_t m = n - off < slice ? n - off : slice;
        LWK_HIP(hipMemcpyAsync(d_all + off * (size_t)kBlobBytes, blobs + off * (size_t)kBlobBytes, m * (size_t)kBlobBytes, hipMemcpyHostToDevice, sc));
        if (off < n_gpu) {
            landed++;
            if (split.launch_after(landed)) {
                const size_t lo = hashed * slice, cnt = (landed - hashed) * slice;
                LWK_HIP(hipEventRecord(c->ev_join[3], sc));
                LWK_HIP(hipStreamWaitEvent(sh, c->ev_join[3], 0));
                launch_challenge(d_all + lo * (size_t)kBlobBytes, vb.comm_in + 48 * lo, z + lo, fs, cnt, sh);
                hashed = landed;
            }
        }
    }
    LWK_HIP(hipEventRecord(c->ev_join[3], sc));
    LWK_HIP(hipStreamWaitEvent(sh, c->ev_join[3], 0));          // every blob is on the device
    LWK_HIP(hipStreamWaitEvent(st, c->ev_join[kMaxSplit - 1], 0));   // the validation's canonical bytes and verdicts
    LWK_HIP(hipMemcpyAsync(canon_c, vb.canon_dev, n * 48, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(canon_p, vb.canon_dev + 48 * n, n * 48, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipEventRecord(c->ev_join[kMaxSplit - 2], st));
    LWK_HIP(hipStreamSynchronize(st));
    LWK_HIP(hipStreamWaitEvent(sh, c->ev_join[kMaxSplit - 2], 0));
    hasher.join();
    // the head: redo the challenges of blobs whose commitment bytes were not canonical (exits at once otherwise)
    if (n_gpu) launch_challenge(d_all, vb.canon_dev, z, fs, n_gpu, sh, vb.comm_in);
    // the tail: the host's digests, unless a commitment among them was not in its canonical encoding
    if (n_host) {
        if (memcmp(canon_c + 48 * n_gpu, comm48 + 48 * n_gpu, 48 * n_host) == 0) {
            LWK_HIP(hipMemcpyAsync(vb.d_rz + 32 * n_gpu, dig.data(), 32 * n_host, hipMemcpyHostToDevice, sh));
            launch_z_from_bytes(vb.d_rz + 32 * n_gpu, z + n_gpu, nullptr, le, n_host, sh);
        } else {
            launch_challenge(d_all + n_gpu * (size_t)kBlobBytes, vb.canon_dev + 48 * n_gpu, z + n_gpu, fs, n_host, sh);
        }
    }
    if (evf) launch_eval_y_from_blobs_evalform(d_all, z, c->tw28_fwd + kBlobElems / 2, vb.d_r, vb.status_all, n, sh, le);
    else launch_eval_y_from_blobs_be(d_all, z, vb.d_r, n, sh);
    launch_fr_mont_to_bytes(z, vb.d_rz, le, n, sh);
    LWK_HIP(hipEventRecord(c->ev_join[3], sh));
    LWK_HIP(hipStreamWaitEvent(st, c->ev_join[3], 0));
    LWK_HIP(hipMemcpyAsync(z32, vb.d_rz, n * 32, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(y32, vb.d_r, n * 32, hipMemcpyDeviceToHost, st));
    return first_status(c, vb.status_all, n, st);
}

// Batches longer than one chunk (1024 blobs). All 2n points are validated ONCE up front (two launches side by side; the kernel is a 2 ms
// latency chain whatever n is), and the blobs then go through in slices that alternate between the two halves of the
// workspace and two streams: while the GPU parses / evaluates one slice, this thread is already inside the (blocking,
// pageable) H2D copy of the next and the host threads hash it. A slot is finished (digests uploaded, y = p(z)
// evaluated, z and y copied back, statuses checked) right before it is reused, and at the end. Caller holds c->mu.
static C_KZG_RET verify_prepare_long(Ctx *c, const uint8_t *blobs, const uint8_t *comm48, const uint8_t *proofs48, size_t n,
                                     int mode, uint8_t *z32, uint8_t *y32, uint8_t *canon_c, uint8_t *canon_p,
                                     VerifyBuffers &vb) {
    const ModeRules mr = mode_rules(mode);
    const int le = mr.le(), fs = mr.hash_rule();   // the byte order of digests and outputs; what the hash kernels are told
    const int bad = mr.bad_status();
    hipStream_t st = c->stream, sv = c->vstream;
    const bool piped = n >= kMaxChunk;
    const size_t step = piped ? kMaxChunk / 2 : n;
    C_KZG_RET rcw = ctx_reserve(c, n < kMaxChunk ? n : kMaxChunk);
    if (rcw != C_KZG_OK) return rcw;
    Workspace &w = c->ws;

    // up-front validation of every commitment (main stream) and every proof (validation stream)
    LWK_HIP(hipMemcpyAsync(vb.comm_in, comm48, n * 48, hipMemcpyHostToDevice, st));
    LWK_HIP(hipMemsetAsync(vb.status_all, 0, n * 4, st));
    LWK_HIP(hipEventRecord(c->ev_fork, st));
    LWK_HIP(hipStreamWaitEvent(sv, c->ev_fork, 0));
    LWK_HIP(hipMemcpyAsync(vb.proof_in, proofs48, n * 48, hipMemcpyHostToDevice, sv));
    launch_validate_commitments(vb.proof_in, vb.canon_dev + 48 * n, vb.status_all, bad, n, sv, vb.pts_p, vb.kind_p, vb.verdict_p);
    launch_validate_commitments(vb.comm_in, vb.canon_dev, vb.status_all, bad, n, st, vb.pts_c, vb.kind_c, vb.verdict_c);
    LWK_HIP(hipEventRecord(c->ev_join[kMaxSplit - 2], st));
    LWK_HIP(hipStreamWaitEvent(sv, c->ev_join[kMaxSplit - 2], 0));
    launch_verify_rows(vb, n, sv, false);  // for the linear combinations; needs the points of both sets and no scalar
    LWK_HIP(hipEventRecord(c->ev_join[kMaxSplit - 1], sv));
    LWK_HIP(hipStreamWaitEvent(st, c->ev_join[kMaxSplit - 1], 0));
    // the canonical bytes come back the first time the host needs them: a device-to-host copy into pageable memory
    // blocks this thread until the stream has reached it, and the first slices should be on their way by then
    bool validated = false;
    auto fetch_canon = [&]() -> C_KZG_RET {
        if (validated) return C_KZG_OK;
        LWK_HIP(hipMemcpyAsync(canon_c, vb.canon_dev, n * 48, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipMemcpyAsync(canon_p, vb.canon_dev + 48 * n, n * 48, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipStreamSynchronize(st));
        validated = true;
        return C_KZG_OK;
    };

    struct Slot {
        bool used = false;
        size_t off = 0, m = 0, base = 0;
        hipStream_t sk = nullptr;
        const uint8_t *hb = nullptr, *hc = nullptr;
        std::vector<uint8_t> dig;
        SideTask hasher;  // joined by its destructor
    } slots[2];

    auto begin = [&](Slot &s, size_t off, size_t m, int idx) -> C_KZG_RET {
        s.used = true;
        s.off = off;
        s.m = m;
        s.base = piped ? (size_t)idx * step : 0;
        s.sk = c->aux[idx];
        s.hb = blobs + off * (size_t)kBlobBytes;
        s.hc = comm48 + 48 * off;
        s.dig.resize(32 * m);
        Slot *sp = &s;  // digests assume the caller's commitment bytes are canonical; finish() confirms or refutes that
        uint8_t *d_blobs = w.blobs + s.base * (size_t)kBlobBytes;
        const bool be_fields = mr.be_transcript;
        s.hasher.start([sp, be_fields]() { challenge_digests_host(sp->dig.data(), sp->hb, sp->hc, sp->m, be_fields); });
        LWK_HIP(hipMemcpyAsync(d_blobs, s.hb, m * (size_t)kBlobBytes, hipMemcpyHostToDevice, s.sk));
        // (the parser's verdicts go beside the validation's, as in the device-resident form: both only ever write failure codes)
        coefficients_stage(c, d_blobs, m, mode, vb.status_all + off, s.sk, s.base);
        return C_KZG_OK;
    };

    auto finish = [&](Slot &s) -> C_KZG_RET {
        if (!s.used) return C_KZG_OK;
        s.used = false;
        const size_t base = s.base, off = s.off, m = s.m;
        hipStream_t sk = s.sk;
        s.hasher.join();
        {
            C_KZG_RET rcf = fetch_canon();
            if (rcf != C_KZG_OK) return rcf;
        }
        Fr *d_z = w.z + base;
        uint8_t *d_zb = w.zbytes + 32 * base, *d_yb = w.ybytes + 32 * base;
        if (memcmp(canon_c + 48 * off, s.hc, m * 48) == 0) {
            LWK_HIP(hipMemcpyAsync(d_zb, s.dig.data(), m * 32, hipMemcpyHostToDevice, sk));
            launch_z_from_bytes(d_zb, d_z, nullptr, le, m, sk);
        } else {  // a non-canonical (or invalid) encoding in this slice: hash the canonical bytes on the GPU
            launch_challenge(w.blobs + base * (size_t)kBlobBytes, vb.canon_dev + 48 * off, d_z, fs, m, sk);
        }
        quotient_stage(c, mode, w.scalars + base * (size_t)kBlobElems * 8, d_z, nullptr /* y only */, d_yb, le, m,
                             sk);
        launch_fr_mont_to_bytes(d_z, d_zb, le, m, sk);
        // r06: z and y of ALL slices collect on the device (the linear combinations' scalar buffers, idle until then; k_vmsm_scalars reads z
        // from there) and come back in one copy each at the end -- r05 copied them to pageable memory slice by slice and fetched the
        // slice's verdicts, two blocking round trips per slice on the submitting thread
        LWK_HIP(hipMemcpyAsync(vb.d_rz + 32 * off, d_zb, m * 32, hipMemcpyDeviceToDevice, sk));
        LWK_HIP(hipMemcpyAsync(vb.d_r + 32 * off, d_yb, m * 32, hipMemcpyDeviceToDevice, sk));
        return C_KZG_OK;
    };

    // the slice streams start after the caller's earlier work on the main stream
    LWK_HIP(hipStreamWaitEvent(c->aux[0], c->ev_fork, 0));
    LWK_HIP(hipStreamWaitEvent(c->aux[1], c->ev_fork, 0));
    int k = 0;
    C_KZG_RET rc_all = C_KZG_OK;
    for (size_t off = 0; off < n && rc_all == C_KZG_OK; off += step, k++) {
        const size_t m = n - off < step ? n - off : step;
        Slot &s = slots[piped ? (k & 1) : 0];
        rc_all = finish(s);  // the slot's previous occupant, if any
        if (rc_all == C_KZG_OK) rc_all = begin(s, off, m, piped ? (k & 1) : 0);
    }
    for (int j = 0; j < 2; j++) {  // drain in submission order
        C_KZG_RET rc = finish(slots[piped ? ((k + j) & 1) : j]);
        if (rc_all == C_KZG_OK) rc_all = rc;
    }
    hipStreamSynchronize(c->aux[0]);
    hipStreamSynchronize(c->aux[1]);
    {
        C_KZG_RET rcf = fetch_canon();
        if (rcf != C_KZG_OK) return rcf;
    }
    if (rc_all != C_KZG_OK) return rc_all;
    LWK_HIP(hipMemcpyAsync(z32, vb.d_rz, n * 32, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(y32, vb.d_r, n * 32, hipMemcpyDeviceToHost, st));
    return first_status(c, vb.status_all, n, st);  // the validation's verdicts and the parser's: the lowest rejected index of the batch
}

// Everything per blob of a batch verification, in one pass over the blobs: validate C_i and pi_i (keeping the
// decompressed points on the device for the linear combinations), z_i = challenge(blob_i, C_i), y_i = p_i(z_i).
// The Fiat-Shamir digests are computed by host threads while the GPU validates and parses (the blobs are host
// memory here); the GPU hash is the fallback for non-canonical commitment encodings.
C_KZG_RET verify_prepare_host(Ctx *c, const uint8_t *blobs, const uint8_t *comm48, const uint8_t *proofs48, size_t n,
                              int mode, uint8_t *z32, uint8_t *y32, uint8_t *canon_c, uint8_t *canon_p, VerifyBuffers &vb,
                              const uint8_t *trusted_canon_c) {
    // vb.owned: the caller's VerifyBuffers brings device scratch of its own (a shard of a sharded verification, which
    // outlives this call and may coexist with others on the same settings object); otherwise the context's scratch is
    // lent out under verify_mu, released when the caller's VerifyBuffers goes away
    if (!vb.owned) vb.hold = std::unique_lock<std::mutex>(c->verify_mu);
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    const ModeRules mr = mode_rules(mode);
    const int le = mr.le(), fs = mr.hash_rule();   // the byte order of digests and outputs; what the hash kernels are told
    const int bad = mr.bad_status();
    hipStream_t st = c->stream;
    WsUse wsu(c, st);
    // No exit of this function may leave a validation / multiples kernel running on the side streams against scratch
    // that the next verification (or vs_reserve) is about to reuse: an early error return drains them.
    struct SideDrain {
        Ctx *c;
        bool armed = true;
        ~SideDrain() {
            if (!armed) return;
            hipStreamSynchronize(c->vstream);
            hipStreamSynchronize(c->aux[0]);
            hipStreamSynchronize(c->aux[1]);
            for (int k = 2; k < kMaxSplit; k++) hipStreamSynchronize(c->aux[k]);   // (verify_prepare_staged: its copy and hash streams)
            if (c->prio_copy) hipStreamSynchronize(c->prio_copy);
        }
    } drain{c};
    const C_KZG_RET rcv = verify_buffers_take(c, vb, n);
    if (rcv != C_KZG_OK) return rcv;
    if (n > kMaxChunk && proofs48 && !trusted_canon_c) {  // up to one chunk the single pass below is ~1 ms shorter
        bool taken = false;
        C_KZG_RET rcs = verify_prepare_staged(c, blobs, comm48, proofs48, n, mode, z32, y32, canon_c, canon_p, vb, taken);
        if (taken || rcs != C_KZG_OK) {
            if (rcs == C_KZG_OK) drain.armed = false;   // every side stream was joined into the main stream
            return rcs;
        }
        return verify_prepare_long(c, blobs, comm48, proofs48, n, mode, z32, y32, canon_c, canon_p, vb);
    }
    std::vector<uint8_t> dig(32 * (n < kMaxChunk ? n : kMaxChunk));
    for (size_t off = 0; off < n; off += kMaxChunk) {
        size_t m = n - off < kMaxChunk ? n - off : kMaxChunk;
        C_KZG_RET rc = ctx_reserve(c, m);
        if (rc != C_KZG_OK) return rc;
        Workspace &w = c->ws;
        const uint8_t *hb = blobs + off * (size_t)kBlobBytes, *hc = comm48 + 48 * off;
        // the Fiat-Shamir digests only need host memory: host threads start on them now, beside the pageable H2D copy
        // (which blocks this thread for milliseconds) and the GPU's validation / parsing. They assume the caller's
        // commitment bytes are canonical; the comparison below confirms or refutes that.
        const uint8_t *hash_comm = trusted_canon_c ? trusted_canon_c + 48 * off : hc;
        const bool hash_beside = m > 64;  // a few blobs: hashing takes microseconds, a thread and its contention do not pay
        SideTask hasher;  // joined by its destructor on every exit
        if (hash_beside) hasher.start([&, hash_comm]() { challenge_digests_host(dig.data(), hb, hash_comm, m, mr.be_transcript); });
        LWK_HIP(hipMemcpyAsync(w.comm48, hc, m * 48, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemsetAsync(w.status, 0, m * 4, st));
        // up to 64 blobs: both point sets are validated on the host threads (0.2 ms per point per thread against a 2 ms
        // latency-shaped kernel) and the decompressed points uploaded in the form the kernel would have left
        const bool host_validate = !trusted_canon_c && n <= host_small_batch_limit();
        if (proofs48 && !host_validate) {
            // Both point sets are validated on streams of their own, started before the blobs go up (the copy blocks
            // this thread for milliseconds): decompression + subgroup test, then the multiples the linear combinations
            // will want, are a ~3 ms latency chain per set that nothing on the main stream should queue behind. Both
            // validations only ever write the same failure code into status.
            // The validation is split in two launches here (square root; subgroup test + canonical bytes), and the
            // multiples run on a fourth stream beside the second one. (off == 0: longer batches take the path above.)
            hipStream_t sa = c->vstream, sc = c->aux[0], sm = c->aux[1];
            LWK_HIP(hipEventRecord(c->ev_fork, st));
            LWK_HIP(hipStreamWaitEvent(sa, c->ev_fork, 0));
            LWK_HIP(hipMemcpyAsync(vb.proof_in, proofs48, m * 48, hipMemcpyHostToDevice, sa));
            const PointSet set_p{vb.proof_in, vb.pts_p, vb.kind_p, w.out48, vb.verdict_p}, set_c{w.comm48, vb.pts_c, vb.kind_c, w.canon48, vb.verdict_c};
            launch_decompress_points(set_p, nullptr, m, sa);
            LWK_HIP(hipEventRecord(c->ev_join[4], sa));
            launch_subgroup_canon(set_p, nullptr, w.status, bad, m, sa);
            LWK_HIP(hipEventRecord(c->ev_join[0], sa));
            LWK_HIP(hipStreamWaitEvent(sc, c->ev_fork, 0));
            launch_decompress_points(set_c, nullptr, m, sc);
            LWK_HIP(hipEventRecord(c->ev_join[5], sc));
            launch_subgroup_canon(set_c, nullptr, w.status, bad, m, sc);
            LWK_HIP(hipEventRecord(c->ev_join[1], sc));
            LWK_HIP(hipStreamWaitEvent(sm, c->ev_join[4], 0));
            LWK_HIP(hipStreamWaitEvent(sm, c->ev_join[5], 0));
            launch_verify_rows(vb, m, sm, false);
            LWK_HIP(hipEventRecord(c->ev_join[2], sm));
        }
        LWK_HIP(hipMemcpyAsync(w.blobs, hb, m * (size_t)kBlobBytes, hipMemcpyHostToDevice, st));
        coefficients_stage(c, w.blobs, m, mode, w.status, st);
        if (trusted_canon_c) {
            // the caller decompressed (and so validated) the commitments itself and hands over their canonical bytes:
            // no 2 ms validation kernel on the single-blob path
            memcpy(canon_c + 48 * off, trusted_canon_c + 48 * off, m * 48);
            hc = trusted_canon_c + 48 * off;
        } else if (!host_validate && !proofs48) {
            launch_validate_commitments(w.comm48, w.canon48, w.status, bad, m, st, vb.pts_c + off, vb.kind_c + off, vb.verdict_c + off);
        }
        std::vector<int32_t> h_code(m, bad), h_kind;
        std::vector<G1Affine29> h_aff;
        if (host_validate) {
            const size_t np = proofs48 ? 2 * m : m;
            std::vector<int> vrc(np);
            h_aff.resize(np);
            h_kind.resize(np);
            host_validate_commitments(hc, canon_c + 48 * off, vrc.data(), m, h_aff.data());
            if (proofs48) host_validate_commitments(proofs48 + 48 * off, canon_p + 48 * off, vrc.data() + m, m, h_aff.data() + m);
            for (size_t i = 0; i < np; i++) {
                h_kind[i] = vrc[i];
                if (vrc[i] == 2) LWK_HIP(hipMemcpyAsync(w.status + (i % m), &h_code[i % m], 4, hipMemcpyHostToDevice, st));
            }
            if (proofs48) {  // the linear combinations of so few points run on the host threads as well
                vb.h_aff = std::move(h_aff);
                vb.h_kind = std::move(h_kind);
            }
        }
        if (proofs48 && !host_validate) {
            LWK_HIP(hipStreamWaitEvent(st, c->ev_join[0], 0));
            LWK_HIP(hipStreamWaitEvent(st, c->ev_join[1], 0));
        }
        if (hash_beside) hasher.join();
        else challenge_digests_host(dig.data(), hb, hash_comm, m, mr.be_transcript);
        // device-to-host copies into pageable memory block this thread until the stream has reached them, so the
        // canonical bytes are fetched only after every launch above has been submitted
        if (!trusted_canon_c && !host_validate)
            LWK_HIP(hipMemcpyAsync(canon_c + 48 * off, w.canon48, m * 48, hipMemcpyDeviceToHost, st));
        if (proofs48 && !host_validate) LWK_HIP(hipMemcpyAsync(canon_p + 48 * off, w.out48, m * 48, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipStreamSynchronize(st));
        if (memcmp(canon_c + 48 * off, hc, m * 48) == 0) {
            LWK_HIP(hipMemcpyAsync(w.zbytes, dig.data(), m * 32, hipMemcpyHostToDevice, st));
            launch_z_from_bytes(w.zbytes, w.z, nullptr, le, m, st);
        } else {
            if (host_validate) LWK_HIP(hipMemcpyAsync(w.canon48, canon_c + 48 * off, m * 48, hipMemcpyHostToDevice, st));
            launch_challenge(w.blobs, w.canon48, w.z, fs, m, st);
        }
        quotient_stage(c, mode, w.scalars, w.z, nullptr /* a verification wants y = p(z) only */, w.ybytes, le, m, st);
        launch_fr_mont_to_bytes(w.z, w.zbytes, le, m, st);
        if (proofs48 && !host_validate)  // k_vmsm_scalars reads the z bytes where the device-resident form leaves them
            LWK_HIP(hipMemcpyAsync(vb.d_rz + 32 * off, w.zbytes, m * 32, hipMemcpyDeviceToDevice, st));
        LWK_HIP(hipMemcpyAsync(z32 + 32 * off, w.zbytes, m * 32, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipMemcpyAsync(y32 + 32 * off, w.ybytes, m * 32, hipMemcpyDeviceToHost, st));
        rc = first_status(c, w.status, m, st);
        if (rc != C_KZG_OK) return rc;
        if (proofs48 && !host_validate)  // the linear combinations (main stream, later) read the multiples
            LWK_HIP(hipStreamWaitEvent(st, c->ev_join[2], 0));
    }
    drain.armed = false;  // everything on the side streams has been joined into the main stream
    return C_KZG_OK;
}

// The same per-blob pass for a batch that is ALREADY on the device (lwkzg_verify_blob_kzg_proof_batch_device,
// lwkzg_verify_shard_begin_device; /root/reference/src/lib.rs:525-614, 639-692): nothing crosses PCIe but the 160-byte records. Both point sets are
// validated on side streams (decompression, subgroup test, canonical bytes, the multiples the linear combinations want) while the main
// stream hashes ALL blobs in one launch over the caller's commitment bytes; where the validation's canonical bytes differ from the
// caller's (a valid point in a non-canonical encoding) that blob's challenge is taken again over the canonical ones -- a launch that
// exits at once otherwise. Then chunk by chunk: parse, y = p(z). `caller`: the stream the inputs were produced on (may be null).
//
// verify_front_device is the ENQUEUE half of that and waits for nothing: the per-blob pass and, where the caller wants the transcript and
// the scratch has room for it (*recorded), k_verify_records and the ONE copy into vb.h_rec. verify_prepare_device is that plus the wait;
// an asynchronous verifier (verify_async.hip) is that plus two host functions in stream order. Caller holds c->mu (and verify_mu unless
// vb.owned) and has selected the device.
C_KZG_RET verify_front_device(Ctx *c, const uint8_t *d_blobs, const uint8_t *d_comm, const uint8_t *d_proofs, size_t n, int mode,
                              VerifyBuffers &vb, hipStream_t caller, bool want_records, bool keep, bool *recorded) {
    *recorded = false;
    const ModeRules mr = mode_rules(mode);
    const int le = mr.le(), fs = mr.hash_rule();   // the byte order of digests and outputs; what the hash kernels are told
    const int bad = mr.bad_status();
    hipStream_t st = c->stream, sv = c->vstream, sc = c->aux[0];
    if (caller && caller != st) {  // the inputs are whatever the caller's stream has produced by now
        LWK_HIP(hipEventRecord(c->ev_join[3], caller));
        LWK_HIP(hipStreamWaitEvent(st, c->ev_join[3], 0));
    }
    WsUse wsu(c, st);
    struct SideDrain {
        Ctx *c;
        bool armed = true;
        ~SideDrain() {
            if (!armed) return;
            hipStreamSynchronize(c->vstream);
            hipStreamSynchronize(c->aux[0]);
        }
    } drain{c};
    const C_KZG_RET rcv = verify_buffers_take(c, vb, n);
    if (rcv != C_KZG_OK) return rcv;
    C_KZG_RET rc = ctx_reserve(c, n < kMaxChunk ? n : kMaxChunk);
    if (rc != C_KZG_OK) return rc;
    CallWords cw;
    if ((rc = call_words(c, n, nullptr, cw)) != C_KZG_OK) return rc;
    Workspace &w = c->ws;
    Fr *z = cw.z;
    LWK_HIP(hipMemsetAsync(vb.status_all, 0, n * 4, st));
    LWK_HIP(hipEventRecord(c->ev_fork, st));
    LWK_HIP(hipStreamWaitEvent(sv, c->ev_fork, 0));
    LWK_HIP(hipStreamWaitEvent(sc, c->ev_fork, 0));
    // Beside the hash (64 blobs per workgroup, one workgroup per compute unit: 3.2 ms whatever n is) the validation and the rows of the
    // linear combinations are latency chains of a few hundred waves, and r05 lost 2 ms to where the dispatcher put them: on the hash's
    // own compute units, four of its waves per SIMD-quad at a raised priority (k_decompress_points 0.43 -> 1.3 ms, k_subgroup_coop_asm
    // 0.67 -> 1.8 ms; profiles/r06_verify_b4096_device_timeline_r05_code.txt). `apart`: every such launch carries an LDS footprint that
    // cannot share a compute unit with a hash workgroup (or with each other), as long as the hash leaves half the chip free.
    const bool apart = n <= kVerifyApartMax;
    const bool fused = knobs().verify_fused || knobs().verify_msm;
    // Up to 8192 blobs (the hash on at most half the compute units) the hash is submitted FIRST and takes its compute units; the padded
    // validation workgroups then fill the others, a compute unit each, and queue among themselves where those run out -- submitted first,
    // they would take the whole chip and the hash would wait for them (8192 blobs: the hash 7.6 ms behind 256 exclusive decompression
    // workgroups; profiles/r06_experiments.md section 3). LWKZG_VERIFY_ORDER=1 (experiment) is the other order.
    const bool hash_first = fused ? (apart != (knobs().verify_order != 0)) : knobs().verify_order != 0;
    if (hash_first) launch_challenge(d_blobs, d_comm, z, fs, n, st);
    if (fused) {   // r06: ONE launch per kernel over both point sets; the rows start as soon as the points are decompressed
        const PointSet set_p{d_proofs, vb.pts_p, vb.kind_p, vb.canon_dev + 48 * n, vb.verdict_p}, set_c{d_comm, vb.pts_c, vb.kind_c, vb.canon_dev, vb.verdict_c};
        launch_decompress_points(set_p, &set_c, n, sv, apart);
        LWK_HIP(hipEventRecord(c->ev_join[2], sv));
        launch_subgroup_canon(set_p, &set_c, vb.status_all, bad, n, sv, apart);
        LWK_HIP(hipEventRecord(c->ev_join[0], sv));
        LWK_HIP(hipStreamWaitEvent(sc, c->ev_join[2], 0));
        launch_verify_rows(vb, n, sc, apart);
        LWK_HIP(hipEventRecord(c->ev_join[1], sc));
    } else {       // r05's arrangement (LWKZG_VERIFY_FUSED=0 with LWKZG_VERIFY_MSM=0): a side stream per point set
        launch_validate_commitments(d_proofs, vb.canon_dev + 48 * n, vb.status_all, bad, n, sv, vb.pts_p, vb.kind_p, vb.verdict_p);
        launch_point_multiples(vb.pts_p, vb.kind_p, vb.mult_p, n, sv);
        LWK_HIP(hipEventRecord(c->ev_join[0], sv));
        launch_validate_commitments(d_comm, vb.canon_dev, vb.status_all, bad, n, sc, vb.pts_c, vb.kind_c, vb.verdict_c);
        launch_point_multiples(vb.pts_c, vb.kind_c, vb.mult_c, n, sc);
        LWK_HIP(hipEventRecord(c->ev_join[1], sc));
    }
    if (!apart && fused) {
        // More than half the chip's compute units would hold a hash workgroup: the footprints cannot keep anything apart any more, and a
        // hash workgroup is as slow as the slowest of its four barrier-coupled waves -- 16384 blobs: the hash 7.8 ms with the validation's
        // waves among its own, 3.2 ms alone (profiles/r06_experiments.md section 3). The validation and the rows (~1.7 ms on the whole
        // chip) therefore go first and the hash follows them.
        LWK_HIP(hipStreamWaitEvent(st, c->ev_join[0], 0));
        LWK_HIP(hipStreamWaitEvent(st, c->ev_join[1], 0));
    }
    if (!hash_first) launch_challenge(d_blobs, d_comm, z, fs, n, st);
    LWK_HIP(hipStreamWaitEvent(st, c->ev_join[0], 0));
    LWK_HIP(hipStreamWaitEvent(st, c->ev_join[1], 0));
    drain.armed = false;  // both side streams are joined into the main stream from here on
    launch_challenge(d_blobs, vb.canon_dev, z, fs, n, st, d_comm);  // only the blobs whose commitment bytes were not canonical
    // chunk by chunk with no host round trip in between: y and z bytes of ALL blobs collect in the linear combinations' scalar
    // buffers (idle until lincomb3), the parser's verdicts beside the validation's
    if (!mr.evaluation_form) {   // the blobs are already on the device and a reference-mode parse cannot fail: one launch reads them as they are
        launch_eval_y_from_blobs_be(d_blobs, z, vb.d_r, n, st);
        launch_fr_mont_to_bytes(z, vb.d_rz, le, n, st);
    } else if (proof_in_evaluation_form(c, mode)) {   // c-kzg on the Lagrange form: the blob's elements ARE the evaluations; range check in the same launch
        launch_eval_y_from_blobs_evalform(d_blobs, z, c->tw28_fwd + kBlobElems / 2, vb.d_r, vb.status_all, n, st, le);
        launch_fr_mont_to_bytes(z, vb.d_rz, le, n, st);
    } else {
        for (size_t off = 0; off < n; off += kMaxChunk) {
            const size_t m = n - off < kMaxChunk ? n - off : kMaxChunk;
            coefficients_stage(c, d_blobs + off * (size_t)kBlobBytes, m, mode, vb.status_all + off, st);
            quotient_stage(c, mode, w.scalars, z + off, nullptr /* y only */, vb.d_r + 32 * off, le, m, st);
            launch_fr_mont_to_bytes(z + off, vb.d_rz + 32 * off, le, m, st);
        }
    }
    if (keep) return C_KZG_OK;   // per-item verification (verify_each.hip) reads the statuses, z and y where they are
    if (want_records && vb.d_rec && vb.h_rec && vb.rec_cap >= n) {
        // r06: the transcript C | z | y | pi per blob assembled by a kernel and ONE copy into pinned memory, the lowest rejected index in its
        // last word -- where r05 made four copies into pageable vectors, a fifth for the status words, and the host interleaved
        uint32_t *d_flag = (uint32_t *)(vb.d_rec + 160 * n);
        LWK_HIP(hipMemsetAsync(d_flag, 0xff, 4, st));
        launch_verify_records(vb.canon_dev, vb.d_rz, vb.d_r, vb.canon_dev + 48 * n, vb.status_all, vb.d_rec, d_flag, n, st);
        LWK_HIP(hipMemcpyAsync(vb.h_rec, vb.d_rec, 160 * n + 4, hipMemcpyDeviceToHost, st));
        *recorded = true;
    }
    return C_KZG_OK;
}

C_KZG_RET verify_prepare_device(Ctx *c, const uint8_t *d_blobs, const uint8_t *d_comm, const uint8_t *d_proofs, size_t n, int mode,
                                uint8_t *z32, uint8_t *y32, uint8_t *canon_c, uint8_t *canon_p, VerifyBuffers &vb, hipStream_t caller,
                                uint8_t *records_out, bool keep) {
    if (!vb.owned) vb.hold = std::unique_lock<std::mutex>(c->verify_mu);
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    bool recorded = false;
    const C_KZG_RET rc = verify_front_device(c, d_blobs, d_comm, d_proofs, n, mode, vb, caller, records_out != nullptr, keep, &recorded);
    if (rc != C_KZG_OK || keep) return rc;
    if (recorded) {
        LWK_HIP(hipStreamSynchronize(st));
        uint32_t first_bad;
        memcpy(&first_bad, vb.h_rec + 160 * n, 4);
        if (first_bad != 0xffffffffu) {
            int32_t code = 0;
            LWK_HIP(hipMemcpy(&code, vb.status_all + first_bad, 4, hipMemcpyDeviceToHost));
            set_error("input %zu rejected (status %d)", (size_t)first_bad, code);
            return (C_KZG_RET)code;
        }
        memcpy(records_out, vb.h_rec, 160 * n);
        return C_KZG_OK;
    }
    LWK_HIP(hipMemcpyAsync(canon_c, vb.canon_dev, n * 48, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(canon_p, vb.canon_dev + 48 * n, n * 48, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(z32, vb.d_rz, n * 32, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(y32, vb.d_r, n * 32, hipMemcpyDeviceToHost, st));
    return first_status(c, vb.status_all, n, st);  // the validation's verdicts and the parser's
}

C_KZG_RET verify_openings_prepare_device(Ctx *c, const uint8_t *d_comm, const uint8_t *d_proofs, const uint8_t *d_z, const uint8_t *d_y,
                                         size_t n, int mode, VerifyBuffers &vb, hipStream_t caller) {
    vb.hold = std::unique_lock<std::mutex>(c->verify_mu);
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    const ModeRules mr = mode_rules(mode);
    const int bad = mr.bad_status();
    hipStream_t st = c->stream;
    if (caller && caller != st) {  // the inputs are whatever the caller's stream has produced by now
        LWK_HIP(hipEventRecord(c->ev_join[3], caller));
        LWK_HIP(hipStreamWaitEvent(st, c->ev_join[3], 0));
    }
    WsUse wsu(c, st);
    C_KZG_RET rc = vs_reserve(c, n);
    if (rc != C_KZG_OK) return rc;
    verify_buffers_lend(vb, c->vs);
    LWK_HIP(hipMemsetAsync(vb.status_all, 0, n * 4, st));
    const PointSet set_p{d_proofs, vb.pts_p, vb.kind_p, vb.canon_dev + 48 * n, vb.verdict_p}, set_c{d_comm, vb.pts_c, vb.kind_c, vb.canon_dev, vb.verdict_c};
    launch_decompress_points(set_p, &set_c, n, st);
    launch_subgroup_canon(set_p, &set_c, vb.status_all, bad, n, st, false, true);
    launch_each_openings(d_z, d_y, vb.d_rz, vb.d_r, vb.status_all, bad, mr.scalar_rule(), n, st);
    LWK_HIP(hipGetLastError());
    return C_KZG_OK;
}

// ---- a batch of openings -------------------------------------------------------------------------------------------
// verify_front_device without the blob: no hash and no evaluation, so nothing on the main stream until the validation is through, and
// no hash to keep apart from -- but the subgroup test and the rows, which run beside each other, keep their LDS footprints.
//
//   main stream   status words, first-bad word cleared ........ k_opening_records, transcript -> h_rec [ev_join[4]] .. joins the rows
//   vstream       k_decompress_points (both sets) [ev_join[2]], subgroup test + canonical bytes (both sets) [ev_join[0]]
//   aux[0]                                         ........... the rows of both sets [ev_join[1]]
//
// Enqueue-only; caller holds c->mu (and verify_mu unless vb.owned) and has selected the device. ev_join[4] marks the transcript's arrival,
// so that a synchronous caller can hash it while the rows are still being built.
C_KZG_RET verify_openings_front_device(Ctx *c, const uint8_t *d_comm, const uint8_t *d_proofs, const uint8_t *d_z, const uint8_t *d_y,
                                       size_t n, int mode, VerifyBuffers &vb, hipStream_t caller, bool *recorded) {
    *recorded = false;
    const ModeRules mr = mode_rules(mode);
    const int bad = mr.bad_status();
    hipStream_t st = c->stream, sv = c->vstream, sc = c->aux[0];
    if (caller && caller != st) {  // the inputs are whatever the caller's stream has produced by now
        LWK_HIP(hipEventRecord(c->ev_join[3], caller));
        LWK_HIP(hipStreamWaitEvent(st, c->ev_join[3], 0));
    }
    struct SideDrain {
        Ctx *c;
        bool armed = true;
        ~SideDrain() {
            if (!armed) return;
            hipStreamSynchronize(c->vstream);
            hipStreamSynchronize(c->aux[0]);
        }
    } drain{c};
    const C_KZG_RET rcv = verify_buffers_take(c, vb, n);
    if (rcv != C_KZG_OK) return rcv;
    if (!(vb.d_rec && vb.h_rec && vb.rec_cap >= n)) {
        set_error("openings batch: the verify scratch has no room for a transcript of %zu records", n);
        return C_KZG_ERROR;
    }
    uint32_t *d_flag = (uint32_t *)(vb.d_rec + 160 * n);
    LWK_HIP(hipMemsetAsync(vb.status_all, 0, n * 4, st));
    LWK_HIP(hipMemsetAsync(d_flag, 0xff, 4, st));
    LWK_HIP(hipEventRecord(c->ev_fork, st));
    LWK_HIP(hipStreamWaitEvent(sv, c->ev_fork, 0));
    LWK_HIP(hipStreamWaitEvent(sc, c->ev_fork, 0));
    const PointSet set_p{d_proofs, vb.pts_p, vb.kind_p, vb.canon_dev + 48 * n, vb.verdict_p}, set_c{d_comm, vb.pts_c, vb.kind_c, vb.canon_dev, vb.verdict_c};
    // No hash runs beside these launches, but the subgroup test and the rows run beside EACH OTHER: up to kVerifyApartMax all three keep
    // the LDS footprints of the blob path, which no two of their workgroups can share a compute unit under (4096 openings:
    // k_vmsm_multiples 1.63 -> 1.25 ms, the call 3.4 -> 3.0 ms; a footprint on the rows alone changes nothing)
    const bool apart = n <= kVerifyApartMax;
    launch_decompress_points(set_p, &set_c, n, sv, apart);
    LWK_HIP(hipEventRecord(c->ev_join[2], sv));
    launch_subgroup_canon(set_p, &set_c, vb.status_all, bad, n, sv, apart);
    LWK_HIP(hipEventRecord(c->ev_join[0], sv));
    LWK_HIP(hipStreamWaitEvent(sc, c->ev_join[2], 0));
    launch_verify_rows(vb, n, sc, apart);
    LWK_HIP(hipEventRecord(c->ev_join[1], sc));
    LWK_HIP(hipStreamWaitEvent(st, c->ev_join[0], 0));
    launch_opening_records(d_z, d_y, vb.canon_dev, vb.canon_dev + 48 * n, vb.d_rz, vb.d_r, vb.status_all, bad, mr.scalar_rule(), vb.d_rec, d_flag,
                           n, st);
    LWK_HIP(hipMemcpyAsync(vb.h_rec, vb.d_rec, 160 * n + 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipEventRecord(c->ev_join[4], st));
    LWK_HIP(hipStreamWaitEvent(st, c->ev_join[1], 0));
    drain.armed = false;  // both side streams are joined into the main stream from here on
    LWK_HIP(hipGetLastError());
    *recorded = true;
    return C_KZG_OK;
}

C_KZG_RET verify_openings_prepare(Ctx *c, const uint8_t *comm, const uint8_t *proofs, const uint8_t *z, const uint8_t *y, size_t n, int mode,
                                  VerifyBuffers &vb, bool device_inputs, hipStream_t caller, uint8_t *records_out) {
    if (!vb.owned) vb.hold = std::unique_lock<std::mutex>(c->verify_mu);
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (!device_inputs) {
        // host memory: 160 bytes per item into the scratch the front runs on -- the points where a host-pointer blob batch puts them,
        // z and y where k_opening_records leaves their canonical bytes (it works in place)
        const C_KZG_RET rcv = verify_buffers_take(c, vb, n);
        if (rcv != C_KZG_OK) return rcv;
        LWK_HIP(hipMemcpyAsync(vb.comm_in, comm, 48 * n, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(vb.proof_in, proofs, 48 * n, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(vb.d_rz, z, 32 * n, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(vb.d_r, y, 32 * n, hipMemcpyHostToDevice, st));
        comm = vb.comm_in;
        proofs = vb.proof_in;
        z = vb.d_rz;
        y = vb.d_r;
        caller = nullptr;
    }
    bool recorded = false;
    const C_KZG_RET rc = verify_openings_front_device(c, comm, proofs, z, y, n, mode, vb, caller, &recorded);
    if (rc != C_KZG_OK) return rc;
    LWK_HIP(hipEventSynchronize(c->ev_join[4]));   // the transcript has landed; the rows may still be on their way
    uint32_t first_bad;
    memcpy(&first_bad, vb.h_rec + 160 * n, 4);
    if (first_bad != 0xffffffffu) {
        int32_t code = 0;
        if (first_bad >= n) {
            set_error("openings batch: the device reported a rejected index %zu of %zu", (size_t)first_bad, n);
            return C_KZG_ERROR;
        }
        LWK_HIP(hipMemcpyAsync(&code, vb.status_all + first_bad, 4, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipStreamSynchronize(st));   // (the rows included: nothing of this call is running when it returns)
        set_error("opening %zu rejected (status %d)", (size_t)first_bad, code);
        return (C_KZG_RET)code;
    }
    memcpy(records_out, vb.h_rec, 160 * n);
    return C_KZG_OK;
}

// sums[0] = sum r_i pi_i, sums[1] = sum r_i z_i pi_i, sums[2] = sum r_i C_i on the points verify_prepare_host kept
C_KZG_RET lincomb3_device_host(Ctx *c, VerifyBuffers &vb, const uint8_t *sc_r, const uint8_t *sc_rz, size_t n,
                               uint8_t sums[3][96], int infs[3]) {
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    const size_t nblk = lincomb3_blocks(n);
    if (!(vb.hold.owns_lock() || vb.owned) || !vb.d_r) {
        set_error("lincomb3_device_host: called without a prepared verification");
        return C_KZG_ERROR;
    }
    uint8_t *d_r = vb.d_r, *d_rz = vb.d_rz, *d_aff = vb.d_aff;
    G1Xyzz29 *d_part = vb.d_part;
    int32_t *d_inf = vb.d_inf;
    uint8_t h_aff[3 * 96];
    int32_t h_inf[3];
    bool ok = true;
    if (ok) ok = hipMemcpyAsync(d_r, sc_r, 32 * n, hipMemcpyHostToDevice, st) == hipSuccess &&
                 hipMemcpyAsync(d_rz, sc_rz, 32 * n, hipMemcpyHostToDevice, st) == hipSuccess;
    if (ok) {
        launch_lincomb3(vb.pts_p, vb.kind_p, vb.mult_p, vb.pts_c, vb.kind_c, vb.mult_c, d_r, d_rz, d_part, n, st);
        G1Xyzz29 *totals = d_part + 3 * nblk;
        for (int k = 0; k < 3; k++) launch_sum_points(d_part + k * nblk, nblk, totals + k, 0, st);
        launch_xyzz29_to_affine_be(totals, d_aff, d_inf, 3, st);
        ok = hipMemcpyAsync(h_aff, d_aff, sizeof h_aff, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipMemcpyAsync(h_inf, d_inf, sizeof h_inf, hipMemcpyDeviceToHost, st) == hipSuccess &&
             hipStreamSynchronize(st) == hipSuccess;
    }
    if (!ok) {
        set_error("lincomb3_device_host: device work failed: %s", hipGetErrorString(hipGetLastError()));
        return C_KZG_ERROR;
    }
    for (int k = 0; k < 3; k++) {
        memcpy(sums[k], h_aff + 96 * k, 96);
        infs[k] = h_inf[k];
    }
    return C_KZG_OK;
}

bool vmsm_ready(const VerifyBuffers &vb) { return knobs().verify_msm && vb.tab_p && vb.h_pin && vb.vm_done; }

// The three sums from r alone (vmsm.hip): everything is enqueued on the context's stream and the results travel to the pinned block by
// themselves; the caller (verify.hip: shard_partial) computes its host share meanwhile and collects with vmsm_finish.
C_KZG_RET vmsm_begin(Ctx *c, VerifyBuffers &vb, const Fr *pw33, int le, size_t n) {
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    hipStream_t st = c->stream;
    if (!(vb.hold.owns_lock() || vb.owned) || !vmsm_ready(vb) || !vb.d_rz) {
        set_error("vmsm_begin: called without a prepared verification");
        return C_KZG_ERROR;
    }
    memcpy(vb.h_pin, pw33, 33 * sizeof(Fr));
    LWK_HIP(hipMemcpyAsync(vb.vm_pw, vb.h_pin, 33 * sizeof(Fr), hipMemcpyHostToDevice, st));
    launch_vmsm_scalars(vb.d_rz, le, vb.vm_pw, vb.sc_a, vb.sc_b, n, st);
    launch_vmsm_accumulate(vb.sc_a, vb.sc_b, vb.tab_p, vb.kind_p, vb.tab_c, vb.kind_c, vb.vm_partial, n, st);
    launch_vmsm_reduce(vb.vm_partial, vb.vm_bsum, vb.d_aff, vb.d_inf, n, st);
    LWK_HIP(hipMemcpyAsync(vb.h_pin + 33 * sizeof(Fr), vb.d_aff, 3 * 96, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(vb.h_pin + 33 * sizeof(Fr) + 3 * 96, vb.d_inf, 3 * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipEventRecord(vb.vm_done, st));
    return C_KZG_OK;
}

C_KZG_RET vmsm_finish(Ctx *c, VerifyBuffers &vb, uint8_t sums[3][96], int infs[3]) {
    LWK_HIP(hipSetDevice(c->device));
    if (hipEventSynchronize(vb.vm_done) != hipSuccess) {
        set_error("vmsm_finish: device work failed: %s", hipGetErrorString(hipGetLastError()));
        return C_KZG_ERROR;
    }
    const uint8_t *res = vb.h_pin + 33 * sizeof(Fr);
    for (int k = 0; k < 3; k++) {
        memcpy(sums[k], res + 96 * k, 96);
        int32_t f;
        memcpy(&f, res + 3 * 96 + 4 * k, 4);
        infs[k] = f;
    }
    return C_KZG_OK;
}

}  // namespace lwk
