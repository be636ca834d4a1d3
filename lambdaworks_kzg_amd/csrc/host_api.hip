// host_api.hip -- the host-pointer batch ABI: commitments, blob proofs and point proofs of host-memory batches (one launch set, slices on
// two streams, or the staged whole-chunk schedule), the coalescing fronts of the single-blob symbols, and the reference's own symbols.
#include "abi_guard.h"
#include "engine_internal.h"

#include <stdio.h>
#include <string.h>

#include <chrono>
#include <functional>
#include <new>
#include <vector>

namespace lwk {

// ------------------------------------------------------------------------------------------------
// host-pointer entry points

// maps per-blob status words to one return code; first_bad gets the first offender
static C_KZG_RET collect_status(Ctx *c, const int32_t *d_status, size_t n, size_t base, size_t *first_bad) {
    std::vector<int32_t> h(n);
    LWK_HIP(hipMemcpyAsync(h.data(), d_status, n * 4, hipMemcpyDeviceToHost, c->stream));
    LWK_HIP(hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < n; i++)
        if (h[i] != 0) {
            if (first_bad) *first_bad = base + i;
            set_error("blob %zu rejected (status %d)", base + i, h[i]);
            return (C_KZG_RET)h[i];
        }
    return C_KZG_OK;
}

// In reference mode every failure is C_KZG_ERROR (lib.rs:263,267,272,...).
C_KZG_RET map_rc(C_KZG_RET rc, int mode) {
    if (rc == C_KZG_OK) return rc;
    if (mode_rules(mode).bad == C_KZG_ERROR) return C_KZG_ERROR;
    return rc;
}

// Slice schedule of the long host batches: 512 blobs at a time (one half of the workspace), but the first two slices are
// 128 + 384, so that the GPU is at work after a quarter of the first upload (512 commitments 6.4 instead of 7.1 ms; 1024
// on a direct table 11.9 instead of 12.8 ms, 85.7k instead of 80.2k ops/s through the host ABI). On the bucket engine a
// batch of a whole chunk or more keeps whole slices: its small launches cost what the earlier start gains.
static size_t slice_len(size_t k, size_t remaining, size_t n, bool direct) {
    const size_t first_env = knobs().slice0;  // experiment: length of the first slice
    const size_t first = first_env ? first_env : kMaxChunk / 8;
    size_t want = kMaxChunk / 2;
    if ((n < kMaxChunk || direct || first_env) && k < 2 && first < kMaxChunk / 2) want = k == 0 ? first : kMaxChunk / 2 - first;
    return remaining < want ? remaining : want;
}

// ------------------------------------------------------------------------------------------------
// Coalescing front of blob_to_kzg_commitment (engine.h: Combiner). Contract matched: concurrent callers on one
// KZGSettings, /root/reference/src/lib.rs:253-283 + SURVEY 8b "Threading".

// LWKZG_COALESCE=0: single-blob calls are not merged with concurrent ones
static bool coalesce_singles() {
    return knobs().coalesce;
}

static bool combiner_init(Ctx *c) {
    Combiner &cb = c->comb;
    std::lock_guard<std::mutex> lk(cb.init_m);
    if (cb.ready || cb.failed) return cb.ready;
    hipSetDevice(c->device);
    bool ok = hipHostMalloc((void **)&cb.pinned_blobs, kCombineSlots * (size_t)kBlobBytes, hipHostMallocDefault) == hipSuccess;
    for (int k = 0; k < kCombineLanes && ok; k++)
        ok = hipHostMalloc((void **)&cb.pinned_out[k], kCombineMaxBatch * sizeof(G1Xyzz29), hipHostMallocDefault) == hipSuccess &&
             hipHostMalloc((void **)&cb.pinned_status[k], kCombineMaxBatch * 4, hipHostMallocDefault) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        cb.failed = true;  // callers fall back to one launch set each
        return false;
    }
    {
        std::lock_guard<std::mutex> fl(cb.front.m);
        cb.front.add_slots((int)kCombineSlots);
    }
    cb.ready = true;
    return true;
}

// one launch set for `batch` (all of one mode) on lane `lane`; fills every request's rc and output
static void combine_run(Ctx *c, int lane, const std::vector<CombineReq *> &batch, bool plain = false) {
    Combiner &cb = c->comb;
    const size_t n = batch.size();
    const int mode = batch[0]->mode;
    const size_t lo = (size_t)lane * kCombineMaxBatch;  // this lane's slice of the workspace
    hipStream_t sk = c->aux[lane];
    const bool host_finish = n <= host_finish_limit();
    bool zero_copy = false;
    uint32_t *redo_flag = nullptr;
    C_KZG_RET rc = C_KZG_OK;
    {
        std::lock_guard<std::mutex> lk(c->mu);  // enqueue only: the wait below happens outside
        bool ok = hipSetDevice(c->device) == hipSuccess;
        if (ok) {
            rc = ctx_reserve(c, kCombineLanes * kCombineMaxBatch);
            ok = rc == C_KZG_OK;
        }
        if (ok) {
            WsLaneUse use(c, lane);
            Workspace &w = c->ws;
            uint8_t *d_blobs = w.blobs + lo * (size_t)kBlobBytes;
            // ONE blob -- the reference's call shape (src/lib.rs:253-283) -- moves no buffer at all (r06): the parse kernel reads the blob from
            // its pinned staging slot across the link, the cooperative kernel's last wave stores the sum into pinned memory, and in
            // reference mode, where a blob cannot be rejected, no verdict is cleared or fetched. A kernel trace of r05's call showed the
            // 118 us kernel among 57 us of copies, fills and the gaps between them (profiles/r06_experiments.md section 7).
            zero_copy = n == 1 && host_finish && !plain && knobs().zero_copy && (c->direct_table != nullptr || c->lag.direct_table != nullptr);
            if (zero_copy) d_blobs = cb.pinned_blobs + (size_t)batch[0]->slot * kBlobBytes;
            // ... and in reference mode on the cooperative kernel two more launches go: the fill of the hand-off counters (the parse kernel
            // clears them on its way) and the second pass that exits at once on honest data (the redo flag is a pinned word this thread
            // looks at after its one synchronisation; a flagged call -- P = +-Q inside a quad: chosen scalars only -- is repeated the long way)
            uint32_t ctr_words = 0;
            if (zero_copy && mode_rules(mode).parse_cannot_fail() && c->direct_table) ctr_words = direct_one_blob_counter_words(c->direct_bits);
            if (ctr_words) {
                redo_flag = (uint32_t *)&cb.pinned_status[lane][1];
                *redo_flag = 0;
            }
            for (size_t i = 0; i < n && ok && !zero_copy; i++)
                ok = hipMemcpyAsync(d_blobs + i * (size_t)kBlobBytes, cb.pinned_blobs + (size_t)batch[i]->slot * kBlobBytes, kBlobBytes,
                                    hipMemcpyHostToDevice, sk) == hipSuccess;
            const bool verdicts = !(zero_copy && mode_rules(mode).parse_cannot_fail());
            if (verdicts) ok = ok && hipMemsetAsync(w.status + lo, 0, n * 4, sk) == hipSuccess;
            else cb.pinned_status[lane][0] = 0;
            if (ok) {
                uint32_t *ctr0 = w.bucket_start + lo * (size_t)(kNumBuckets + 1) + 1;   // (msm_sums_stage: redo flags at bstart, the counters behind them)
                const bool lg = coefficients_stage(c, d_blobs, n, mode, w.status + lo, sk, lo, true, redo_flag ? ctr0 : nullptr, ctr_words);
                if (zero_copy) {
                    (void)msm_sums_stage(c, w.scalars + lo * (size_t)kBlobElems * 8, n, sk, lo, false, lg, (G1Xyzz29 *)cb.pinned_out[lane], redo_flag);
                } else if (host_finish) {  // the sums come back as they are; inversion and compression below, on this thread
                    const G1Xyzz29 *sums = msm_sums_stage(c, w.scalars + lo * (size_t)kBlobElems * 8, n, sk, lo, false, lg);
                    ok = hipMemcpyAsync(cb.pinned_out[lane], sums, n * sizeof(G1Xyzz29), hipMemcpyDeviceToHost, sk) == hipSuccess;
                } else {
                    msm_stages(c, w.scalars + lo * (size_t)kBlobElems * 8, w.out48 + 48 * lo, n, sk, lo, false, lg);
                    ok = hipMemcpyAsync(cb.pinned_out[lane], w.out48 + 48 * lo, n * 48, hipMemcpyDeviceToHost, sk) == hipSuccess;
                }
                if (verdicts) ok = ok && hipMemcpyAsync(cb.pinned_status[lane], w.status + lo, n * 4, hipMemcpyDeviceToHost, sk) == hipSuccess;
            }
        }
        if (!ok && rc == C_KZG_OK) {
            set_error("blob_to_kzg_commitment (coalesced): %s", hipGetErrorString(hipGetLastError()));
            rc = C_KZG_ERROR;
        }
    }
    if (rc == C_KZG_OK && hipStreamSynchronize(sk) != hipSuccess) {
        set_error("blob_to_kzg_commitment (coalesced): %s", hipGetErrorString(hipGetLastError()));
        rc = C_KZG_ERROR;
    }
    if (rc == C_KZG_OK && redo_flag && *redo_flag != 0) return combine_run(c, lane, batch, true);   // the complete-branches pass, the long way
    for (size_t i = 0; i < n; i++) {
        CombineReq *r = batch[i];
        if (rc != C_KZG_OK) {
            r->rc = rc;
        } else if (cb.pinned_status[lane][i] != 0) {
            r->rc = (int)map_rc((C_KZG_RET)cb.pinned_status[lane][i], mode);
        } else {
            if (host_finish) host_finish_compress(r->out48, ((const G1Xyzz29 *)cb.pinned_out[lane])[i]);
            else memcpy(r->out48, cb.pinned_out[lane] + 48 * i, 48);
            r->rc = C_KZG_OK;
        }
    }
}

// blob_to_kzg_commitment for one blob, merged with whatever other callers are waiting. Returns false when the front is
// unavailable (no pinned memory): the caller then takes the plain path.
static bool combine_commit(Ctx *c, uint8_t *out48, const uint8_t *blob, int mode, C_KZG_RET *rc_out) {
    Combiner &cb = c->comb;
    if (!combiner_init(c)) return false;
    CombineReq req;
    req.mode = mode;
    req.out48 = out48;
    // front.h: every caller stages its own blob (in parallel), the first to find a free lane leads everything queued
    const int rc = cb.front.submit(
        req, kCombineMaxBatch, (int)C_KZG_MALLOC,
        [&](int slot) { memcpy(cb.pinned_blobs + (size_t)slot * kBlobBytes, blob, kBlobBytes); },
        [&](int lane, const std::vector<CombineReq *> &batch) { combine_run(c, lane, batch); });
    *rc_out = (C_KZG_RET)rc;
    return true;
}

namespace {

struct ResBlock {  // a piece of the context's result block (host_res_block) carved into 256-byte aligned pieces
    uint8_t *base = nullptr;
    size_t used = 0, cap = 0;
    static size_t pad(size_t b) { return (b + 255) & ~(size_t)255; }
    bool alloc(Ctx *c, size_t bytes) {
        cap = bytes;
        base = host_res_block(c, bytes);
        return base != nullptr;
    }
    uint8_t *take(size_t bytes) {
        uint8_t *p = base + used;
        used += pad(bytes);
        return p;
    }
};

C_KZG_RET scan_status(const std::vector<int32_t> &h_status, size_t *first_bad, int mode) {
    for (size_t i = 0; i < h_status.size(); i++)
        if (h_status[i] != 0) {
            if (first_bad) *first_bad = i;
            set_error("blob %zu rejected (status %d)", i, h_status[i]);
            return map_rc((C_KZG_RET)h_status[i], mode);
        }
    return C_KZG_OK;
}

}  // namespace

// (the host-pointer entry points allocate host vectors: nothing may unwind across the C ABI -- the exported symbols wrap these)
static C_KZG_RET commitment_batch_impl(KZGCommitment *out, const Blob *blobs, size_t n, const KZGSettings *s, size_t *first_bad) {
    const int mode = mode_of(s);
    if (!out || !blobs) return map_rc(C_KZG_BADARGS, mode);
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    ensure_lagrange(c, mode);
    if (n == 1) {  // the reference's symbol: merged with the other callers of the moment
        C_KZG_RET rc1;
        uint8_t tmp[48];
        if (coalesce_singles() && combine_commit(c, tmp, (const uint8_t *)blobs, mode, &rc1)) {
            if (rc1 == C_KZG_OK) memcpy(out, tmp, 48);
            else if (first_bad) *first_bad = 0;
            if (rc1 != C_KZG_OK && !get_error()[0]) set_error("blob 0 rejected");
            return rc1;
        }
    }
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    WsUse wsu(c, c->stream);
    // (the bucket engine overlaps the tails of its own sub-batches inside commit_batch_device, which a lone 512-blob slice
    // would forgo: it takes the single pass up to a whole chunk)
    if (n < 512 || (!c->direct_table && n <= kMaxChunk)) {  // one launch set, results and verdicts back in one go
        C_KZG_RET rc = ctx_reserve(c, n);
        if (rc != C_KZG_OK) return rc;
        Workspace &w = c->ws;
        LWK_HIP(hipMemcpyAsync(w.blobs, blobs, n * (size_t)kBlobBytes, hipMemcpyHostToDevice, c->stream));
        if (n <= host_finish_limit()) {   // a handful of results: the sums come back as they are, inversion and compression on this thread
            LWK_HIP(hipMemsetAsync(w.status, 0, n * 4, c->stream));
            const bool lg = coefficients_stage(c, w.blobs, n, mode, w.status, c->stream, 0, true);
            const G1Xyzz29 *d_sums = msm_sums_stage(c, w.scalars, n, c->stream, 0, false, lg);
            std::vector<G1Xyzz29> h_sums(n);
            LWK_HIP(hipMemcpyAsync(h_sums.data(), d_sums, n * sizeof(G1Xyzz29), hipMemcpyDeviceToHost, c->stream));
            rc = collect_status(c, w.status, n, 0, first_bad);
            if (rc != C_KZG_OK) return map_rc(rc, mode);
            for (size_t i = 0; i < n; i++) host_finish_compress(out[i].bytes, h_sums[i]);
            return C_KZG_OK;
        }
        rc = commit_batch_device(c, w.out48, w.blobs, n, mode, c->stream, w.status);
        if (rc != C_KZG_OK) return rc;
        std::vector<uint8_t> h_out(n * 48);
        LWK_HIP(hipMemcpyAsync(h_out.data(), w.out48, n * 48, hipMemcpyDeviceToHost, c->stream));
        rc = collect_status(c, w.status, n, 0, first_bad);
        if (rc != C_KZG_OK) return map_rc(rc, mode);
        memcpy(out, h_out.data(), n * 48);
        return C_KZG_OK;
    }
    // Long batches stream through in slices of 512 blobs: slice k uses half k mod 2 of the workspace and stream
    // k mod 2, so the pageable H2D copy of a slice (which blocks this thread while it is staged) runs beside the GPU's
    // work on the previous one, a half is only reused by the stream that used it last (stream order is the only
    // synchronisation needed), and nothing waits for the host until every slice has been submitted.
    constexpr size_t kSlice = kMaxChunk / 2;
    C_KZG_RET rc = ctx_reserve(c, kMaxChunk);
    if (rc != C_KZG_OK) return rc;
    Workspace &w = c->ws;
    std::vector<int32_t> h_status(n);
    // results and verdicts of all slices stay on the device until the end: a D2H copy into pageable memory would make
    // this thread wait for the slice it belongs to
    uint8_t *d_out_all = host_res_block(c, ResBlock::pad(n * 48) + n * 4);
    if (!d_out_all) {
        set_error("lwkzg_blob_to_kzg_commitment_batch: out of device memory for %zu results", n);
        return C_KZG_MALLOC;
    }
    int32_t *d_status_all = (int32_t *)(d_out_all + ResBlock::pad(n * 48));
    LWK_HIP(hipEventRecord(c->ev_fork, c->stream));
    if (n > kMaxChunk && dev_stage_ready(c)) {   // (up to one chunk r05's 128 + 384 + 512 slices measure better: 81.9k against 79.9k ops/s at 1024 blobs)
        // r06 (engine.h: DevStage): the slices are uploaded into a device-side double buffer on a copy stream and go through the
        // device-resident pipeline itself -- whole chunks, one compute stream -- while the next one is on its way
        hipStream_t st = c->stream;
        LWK_HIP(hipStreamWaitEvent(upload_stream(c), c->ev_fork, 0));
        size_t k = 0;
        for (size_t off = 0, cnt = 0; off < n; off += cnt, k++) {
            cnt = stage_slice_len(k, n - off);
            uint8_t *d_blobs = nullptr;
            const auto tu0 = std::chrono::steady_clock::now();
            rc = stage_upload(c, k, (const uint8_t *)(blobs + off), cnt, st, &d_blobs);
            if (knobs().timing)
                fprintf(stderr, "[lambdaworks_kzg_amd] staged commitments: slice %zu (%zu blobs) upload call %.2f ms\n", k, cnt,
                        std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tu0).count());
            if (rc == C_KZG_OK) rc = commit_batch_device(c, d_out_all + 48 * off, d_blobs, cnt, mode, st, d_status_all + off);
            if (rc == C_KZG_OK) rc = stage_parsed(c, k, st);   // (behind the whole slice: the bucket engine's sub-batches parse on streams of their own)
            if (rc != C_KZG_OK) {
                hipStreamSynchronize(upload_stream(c));
                hipStreamSynchronize(st);
                return rc;
            }
        }
        LWK_HIP(hipMemcpyAsync((uint8_t *)out, d_out_all, n * 48, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipMemcpyAsync(h_status.data(), d_status_all, n * 4, hipMemcpyDeviceToHost, st));
        LWK_HIP(hipStreamSynchronize(st));
        return scan_status(h_status, first_bad, mode);
    }
    LWK_HIP(hipStreamWaitEvent(c->aux[0], c->ev_fork, 0));
    LWK_HIP(hipStreamWaitEvent(c->aux[1], c->ev_fork, 0));
    size_t k = 0;
    for (size_t off = 0, cnt = 0; off < n; off += cnt, k++) {
        cnt = slice_len(k, n - off, n, c->direct_table != nullptr || c->lag.direct_table != nullptr);
        const size_t lo = (k % 2) * kSlice;
        hipStream_t sk = c->aux[k & 1];
        uint8_t *d_blobs = w.blobs + lo * (size_t)kBlobBytes;
        LWK_HIP(hipMemcpyAsync(d_blobs, (const uint8_t *)(blobs + off), cnt * (size_t)kBlobBytes, hipMemcpyHostToDevice, sk));
        LWK_HIP(hipMemsetAsync(d_status_all + off, 0, cnt * 4, sk));
        const bool lg = coefficients_stage(c, d_blobs, cnt, mode, d_status_all + off, sk, lo, true);
        msm_stages(c, w.scalars + lo * (size_t)kBlobElems * 8, d_out_all + 48 * off, cnt, sk, lo, false, lg);
    }
    for (int j = 0; j < 2; j++) {
        LWK_HIP(hipEventRecord(c->ev_join[j], c->aux[j]));
        LWK_HIP(hipStreamWaitEvent(c->stream, c->ev_join[j], 0));
    }
    LWK_HIP(hipMemcpyAsync((uint8_t *)out, d_out_all, n * 48, hipMemcpyDeviceToHost, c->stream));
    LWK_HIP(hipMemcpyAsync(h_status.data(), d_status_all, n * 4, hipMemcpyDeviceToHost, c->stream));
    LWK_HIP(hipStreamSynchronize(c->stream));
    return scan_status(h_status, first_bad, mode);
}

// ------------------------------------------------------------------------------------------------
// Long host batches of proofs (512 blobs and up) stream through in slices of 512 blobs, like the commitments above:
// slice k uses half k mod 2 of the workspace on stream k mod 2, so the pageable H2D copy of slice k + 1 (which blocks
// this thread while it is staged) runs beside the GPU's work on slice k. Results and verdicts of all slices stay on
// the device until the end. The caller holds c->mu.

namespace {

C_KZG_RET point_proofs_sliced(Ctx *c, uint8_t *proofs_out, uint8_t *ys_out, const uint8_t *blobs, const uint8_t *zs, size_t n,
                              int mode, size_t *first_bad) {
    constexpr size_t kSlice = kMaxChunk / 2;
    const ModeRules mr = mode_rules(mode);
    const int le = mr.le();
    C_KZG_RET rc = ctx_reserve(c, kMaxChunk);
    if (rc != C_KZG_OK) return rc;
    Workspace &w = c->ws;
    ResBlock blk;
    if (!blk.alloc(c, ResBlock::pad(n * 48) + 2 * ResBlock::pad(n * 32) + ResBlock::pad(n * 4))) {
        set_error("lwkzg_compute_kzg_proof_batch: out of device memory for %zu results", n);
        return C_KZG_MALLOC;
    }
    uint8_t *d_out = blk.take(n * 48), *d_y = blk.take(n * 32), *d_z = blk.take(n * 32);
    int32_t *d_status = (int32_t *)blk.take(n * 4);
    std::vector<int32_t> h_status(n);
    hipStream_t st = c->stream;
    LWK_HIP(hipMemcpyAsync(d_z, zs, n * 32, hipMemcpyHostToDevice, st));
    LWK_HIP(hipMemsetAsync(d_status, 0, n * 4, st));
    LWK_HIP(hipEventRecord(c->ev_fork, st));
    // (r06: the staged whole-chunk schedule of the commitments -- engine.h: DevStage -- measured 3 % SLOWER here, 88.6k against 91.2k proofs/s at
    // 4096 blobs: on two streams the evaluation, fold and finalize of one slice run beside the other slice's MSM; profiles/r06_experiments.md section 6)
    LWK_HIP(hipStreamWaitEvent(c->aux[0], c->ev_fork, 0));
    LWK_HIP(hipStreamWaitEvent(c->aux[1], c->ev_fork, 0));
    size_t k = 0;
    for (size_t off = 0, cnt = 0; off < n; off += cnt, k++) {
        cnt = slice_len(k, n - off, n, c->direct_table != nullptr || c->lag.direct_table != nullptr);
        const size_t lo = (k % 2) * kSlice, so = lo * (size_t)kBlobElems * 8;
        hipStream_t sk = c->aux[k & 1];
        uint8_t *d_blobs = w.blobs + lo * (size_t)kBlobBytes;
        LWK_HIP(hipMemcpyAsync(d_blobs, blobs + off * (size_t)kBlobBytes, cnt * (size_t)kBlobBytes, hipMemcpyHostToDevice, sk));
        coefficients_stage(c, d_blobs, cnt, mode, d_status + off, sk, lo);
        launch_z_from_bytes(d_z + 32 * off, w.z + lo, d_status + off, mr.scalar_rule(), cnt, sk);
        quotient_stage(c, mode, w.scalars + so, w.z + lo, w.scalars2 + so, d_y + 32 * off, le, cnt, sk);
        msm_stages(c, w.scalars2 + so, d_out + 48 * off, cnt, sk, lo, false, quotient_to_msm_form(c, mode, cnt, sk, lo));
    }
    for (int j = 0; j < 2; j++) {
        LWK_HIP(hipEventRecord(c->ev_join[j], c->aux[j]));
        LWK_HIP(hipStreamWaitEvent(st, c->ev_join[j], 0));
    }
    std::vector<uint8_t> h_out(n * 48), h_y(n * 32);  // the caller's buffers are only written on success
    LWK_HIP(hipMemcpyAsync(h_out.data(), d_out, n * 48, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(h_y.data(), d_y, n * 32, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(h_status.data(), d_status, n * 4, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipStreamSynchronize(st));
    rc = scan_status(h_status, first_bad, mode);
    if (rc != C_KZG_OK) return rc;
    memcpy(proofs_out, h_out.data(), n * 48);
    memcpy(ys_out, h_y.data(), n * 32);
    return C_KZG_OK;
}

// compute_blob_kzg_proof for a long batch: every commitment is validated once up front on the validation stream (the
// kernel is a ~2 ms latency chain whatever n is); the host threads hash slice k (the digests assume the caller's
// commitment bytes are canonical) while it is copied; the canonical bytes decide per slice between those digests and
// the GPU hash over the canonical encoding.
C_KZG_RET blob_proofs_sliced(Ctx *c, uint8_t *out, const uint8_t *blobs, const uint8_t *comm48, size_t n, int mode,
                             size_t *first_bad) {
    constexpr size_t kSlice = kMaxChunk / 2;
    const ModeRules mr = mode_rules(mode);
    const int le = mr.le();
    C_KZG_RET rc = ctx_reserve(c, kMaxChunk);
    if (rc != C_KZG_OK) return rc;
    Workspace &w = c->ws;
    ResBlock blk;
    if (!blk.alloc(c, 3 * ResBlock::pad(n * 48) + ResBlock::pad(n * 32) + ResBlock::pad(n * 4))) {
        set_error("lwkzg_compute_blob_kzg_proof_batch: out of device memory for %zu results", n);
        return C_KZG_MALLOC;
    }
    const bool timing = knobs().timing;  // phase wall-clock to stderr
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    const auto t0 = now();
    uint8_t *d_out = blk.take(n * 48), *d_comm = blk.take(n * 48), *d_canon = blk.take(n * 48);
    uint8_t *d_dig = blk.take(n * 32);
    int32_t *d_status = (int32_t *)blk.take(n * 4);
    std::vector<int32_t> h_status(n);
    std::vector<uint8_t> h_canon(n * 48), h_dig(n * 32);
    hipStream_t st = c->stream, sv = c->vstream;
    LWK_HIP(hipMemsetAsync(d_status, 0, n * 4, st));
    LWK_HIP(hipEventRecord(c->ev_fork, st));
    LWK_HIP(hipStreamWaitEvent(sv, c->ev_fork, 0));
    LWK_HIP(hipStreamWaitEvent(c->aux[0], c->ev_fork, 0));
    LWK_HIP(hipStreamWaitEvent(c->aux[1], c->ev_fork, 0));
    LWK_HIP(hipMemcpyAsync(d_comm, comm48, n * 48, hipMemcpyHostToDevice, sv));
    launch_validate_commitments(d_comm, d_canon, d_status, mr.bad_status(), n, sv);  // lib.rs:372-375
    LWK_HIP(hipEventRecord(c->ev_join[kMaxSplit - 1], sv));
    bool validated = false;
    // (r06: slices on two streams stay -- the staged whole-chunk schedule of the commitments measured 84.9k against 88.1k proofs/s here)
    size_t k = 0;
    for (size_t off = 0, cnt = 0; off < n; off += cnt, k++) {
        cnt = slice_len(k, n - off, n, c->direct_table != nullptr || c->lag.direct_table != nullptr);
        const size_t lo = (k % 2) * kSlice, so = lo * (size_t)kBlobElems * 8;
        hipStream_t sk = c->aux[k & 1];
        uint8_t *d_blobs = w.blobs + lo * (size_t)kBlobBytes;
        const uint8_t *hb = blobs + off * (size_t)kBlobBytes, *hc = comm48 + 48 * off;
        uint8_t *dig = h_dig.data() + 32 * off;
        // the host threads hash the slice (the digests assume canonical commitment bytes) beside its upload, which blocks this thread while
        // the runtime stages it
        const bool be_fields = mr.be_transcript;
        SideTask hasher([=]() { challenge_digests_host(dig, hb, hc, cnt, be_fields); });
        const auto ta = now();
        LWK_HIP(hipMemcpyAsync(d_blobs, hb, cnt * (size_t)kBlobBytes, hipMemcpyHostToDevice, sk));
        const auto tb = now();
        coefficients_stage(c, d_blobs, cnt, mode, d_status + off, sk, lo);
        hasher.join();
        const auto tc = now();
        if (timing) fprintf(stderr, "[blob_proofs_sliced] slice %zu at %.2f ms: h2d %.2f ms, hash wait %.2f ms\n", k, ms(t0, ta), ms(ta, tb), ms(tb, tc));
        if (!validated) {
            // A device-to-host copy into pageable memory blocks this thread until the stream has reached it, so the
            // canonical bytes are only fetched here, after the first slice has been submitted. From here on they are
            // on the host, and the slice streams may read d_canon.
            LWK_HIP(hipMemcpyAsync(h_canon.data(), d_canon, n * 48, hipMemcpyDeviceToHost, sv));
            LWK_HIP(hipStreamSynchronize(sv));
            validated = true;
        }
        if (memcmp(h_canon.data() + 48 * off, hc, cnt * 48) == 0) {
            LWK_HIP(hipMemcpyAsync(d_dig + 32 * off, dig, cnt * 32, hipMemcpyHostToDevice, sk));
            launch_z_from_bytes(d_dig + 32 * off, w.z + lo, nullptr, le, cnt, sk);  // digest -> Fr, reduced (utils.rs:148-154)
        } else {  // a non-canonical (or invalid) encoding in this slice: hash the canonical bytes on the GPU
            launch_challenge(d_blobs, d_canon + 48 * off, w.z + lo, mr.hash_rule(), cnt, sk);
        }
        quotient_stage(c, mode, w.scalars + so, w.z + lo, w.scalars2 + so, nullptr, le, cnt, sk);
        msm_stages(c, w.scalars2 + so, d_out + 48 * off, cnt, sk, lo, false, quotient_to_msm_form(c, mode, cnt, sk, lo));
    }
    for (int j = 0; j < 2; j++) {
        LWK_HIP(hipEventRecord(c->ev_join[j], c->aux[j]));
        LWK_HIP(hipStreamWaitEvent(st, c->ev_join[j], 0));
    }
    LWK_HIP(hipStreamWaitEvent(st, c->ev_join[kMaxSplit - 1], 0));
    std::vector<uint8_t> h_out(n * 48);
    LWK_HIP(hipMemcpyAsync(h_out.data(), d_out, n * 48, hipMemcpyDeviceToHost, st));
    LWK_HIP(hipMemcpyAsync(h_status.data(), d_status, n * 4, hipMemcpyDeviceToHost, st));
    const auto td = now();
    LWK_HIP(hipStreamSynchronize(st));
    if (timing) fprintf(stderr, "[blob_proofs_sliced] n=%zu: submitted at %.2f ms, drained at %.2f ms\n", n, ms(t0, td), ms(t0, now()));
    rc = scan_status(h_status, first_bad, mode);
    if (rc != C_KZG_OK) return rc;
    memcpy(out, h_out.data(), n * 48);
    return C_KZG_OK;
}

}  // namespace

// compute_blob_kzg_proof of ONE blob in reference mode on a direct table -- the reference's own call shape (src/lib.rs:361-404) -- with
// nothing on its critical path that need not be there (r06; r05: 0.32-0.35 ms, of which the host's validation of the commitment, 0.2 ms
// of one thread, sat between the enqueue and the wait, LONGER than the GPU's whole chain behind the digest). Here the commitment is
// validated on a thread of its own from the first instruction on; the parse kernel runs beside this thread's hashing (and clears the
// cooperative kernel's hand-off counters on its way); the digest is read by k_z_from_bytes from pinned memory, the sum is stored into
// pinned memory by the MSM's last wave, the redo flag is a pinned word: no copy of a result, no fill, no second-pass launch, no verdict
// word (a reference-mode parse cannot fail; the validation's verdict is this process's own). Anything irregular -- an invalid or
// non-canonically encoded commitment, P = +-Q inside a quad, no pinned memory -- returns kOneBlobFallback and the caller takes the
// general path, which owns the error codes. (An int, not a C_KZG_RET: 100 is not a value of that enumeration, and loading it into one was
// undefined behaviour that the host-UBSan run of the GPU suite caught.) Caller holds c->mu and the workspace.
static const int kOneBlobFallback = 100;   // (not a value of the ABI: internal)
static int blob_proof_one_host(Ctx *c, uint8_t *out48, const uint8_t *blob, const uint8_t *comm48, int mode) {
    if (!mode_rules(mode).parse_cannot_fail() || !c->direct_table || !knobs().zero_copy || peer_busy(c)) return kOneBlobFallback;
    const uint32_t ctr_words = direct_one_blob_counter_words(c->direct_bits);
    if (!ctr_words) return kOneBlobFallback;
    if (!c->one_pin && hipHostMalloc((void **)&c->one_pin, 4096, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        c->one_pin = nullptr;
        return kOneBlobFallback;
    }
    if (ctx_reserve(c, 1) != C_KZG_OK) return kOneBlobFallback;
    Workspace &w = c->ws;
    hipStream_t st = c->stream;
    G1Xyzz29 *p_sum = (G1Xyzz29 *)c->one_pin;
    uint32_t *p_redo = (uint32_t *)(c->one_pin + 256);
    uint8_t *p_dig = c->one_pin + 320;
    *p_redo = 0;
    uint8_t canon[48];
    int vrc = 2;
    SideTask validator([&]() { vrc = host_validate_commitment(comm48, canon); });   // lib.rs:372-375, beside everything below
    LWK_HIP(hipMemcpyAsync(w.blobs, blob, kBlobBytes, hipMemcpyHostToDevice, st));
    (void)coefficients_stage(c, w.blobs, 1, mode, w.status, st, 0, false, w.bucket_start + 1, ctr_words);
    challenge_digests_host(p_dig, blob, comm48, 1);   // on this thread, beside the upload and the parse (assumes canonical commitment bytes)
    launch_z_from_bytes(p_dig, w.z, nullptr, 0, 1, st);   // digest -> Fr, reduced (utils.rs:148-154); read across the link
    quotient_stage(c, mode, w.scalars, w.z, w.scalars2, nullptr, 0, 1, st);
    (void)msm_sums_stage(c, w.scalars2, 1, st, 0, false, quotient_to_msm_form(c, mode, 1, st), p_sum, p_redo);
    validator.join();
    LWK_HIP(hipStreamSynchronize(st));
    if (vrc != 0 || memcmp(canon, comm48, 48) != 0 || *p_redo != 0) return kOneBlobFallback;   // (vrc 1: infinity -- canonical c0 00.. only; keep it simple)
    host_finish_compress(out48, *p_sum);
    return C_KZG_OK;
}

static C_KZG_RET blob_proof_batch_host(Ctx *c, KZGProof *out, const Blob *blobs, const Bytes48 *commitments, size_t n, int mode,
                                       size_t *first_bad) {
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    WsUse wsu(c, c->stream);
    if (n >= kMaxChunk / 2)
        return blob_proofs_sliced(c, (uint8_t *)out, (const uint8_t *)blobs, (const uint8_t *)commitments, n, mode, first_bad);
    if (n == 1) {
        const int r1 = blob_proof_one_host(c, (uint8_t *)out, (const uint8_t *)blobs, (const uint8_t *)commitments, mode);
        if (r1 != kOneBlobFallback) return (C_KZG_RET)r1;
    }
    for (size_t off = 0; off < n; off += kMaxChunk) {
        size_t m = n - off < kMaxChunk ? n - off : kMaxChunk;
        C_KZG_RET rc = ctx_reserve(c, m);
        if (rc != C_KZG_OK) return rc;
        Workspace &w = c->ws;
        hipStream_t st = c->stream;
        const ModeRules mr = mode_rules(mode);
    const int le = mr.le();
        const uint8_t *h_blobs = (const uint8_t *)(blobs + off), *h_comm = (const uint8_t *)(commitments + off);
        // host threads start hashing at once (the blobs are in host memory here; one GPU lane would need ~7 ms per
        // 131 KB message, a core with SHA extensions ~0.1 ms) and run beside the pageable H2D copy, which blocks
        // this thread for a few milliseconds. The digests assume the caller's commitment bytes are the canonical
        // encoding; the validation's re-compression confirms or refutes that below.
        std::vector<uint8_t> h_canon(m * 48), h_dig(m * 32);
        SideTask hasher([&]() { challenge_digests_host(h_dig.data(), h_blobs, h_comm, m, mr.be_transcript); });
        LWK_HIP(hipMemcpyAsync(w.blobs, h_blobs, m * (size_t)kBlobBytes, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemcpyAsync(w.comm48, h_comm, m * 48, hipMemcpyHostToDevice, st));
        LWK_HIP(hipMemsetAsync(w.status, 0, m * 4, st));
        // Validate the commitments (lib.rs:372-375): a long serial scalar multiplication per point whose verdict and
        // canonical bytes are only needed at the very end. Up to 64 points: on the host threads while the GPU works
        // (~0.2 ms each on the 64-bit host field, against a 2 ms latency-shaped kernel). A batch: on the GPU, on an
        // auxiliary stream beside everything else.
        const bool host_validate = m <= host_small_batch_limit();
        std::vector<int32_t> h_code(m, mr.bad_status());
        if (!host_validate) {
            LWK_HIP(hipEventRecord(c->ev_fork, st));
            LWK_HIP(hipStreamWaitEvent(c->vstream, c->ev_fork, 0));
            launch_validate_commitments(w.comm48, w.canon48, w.status, mr.bad_status(), m, c->vstream, w.val_pts, w.val_kind, w.val_verdict);
            LWK_HIP(hipEventRecord(c->ev_join[0], c->vstream));
        }
        // GPU, main stream: parse the blobs, then the digests as soon as the host threads have them
        coefficients_stage(c, w.blobs, m, mode, w.status, st);
        hasher.join();
        LWK_HIP(hipMemcpyAsync(w.zbytes, h_dig.data(), m * 32, hipMemcpyHostToDevice, st));
        launch_z_from_bytes(w.zbytes, w.z, nullptr, le, m, st);  // digest -> Fr, reduced (utils.rs:148-154)
        quotient_stage(c, mode, w.scalars, w.z, w.scalars2, nullptr, le, m, st);
        const bool hf = m <= host_finish_limit();  // a small call: inversion and compression on this thread, at the end
        const G1Xyzz29 *d_sums = nullptr;
        auto quotient_msm = [&]() {
            const bool lg = quotient_to_msm_form(c, mode, m, st);
            if (hf) d_sums = msm_sums_stage(c, w.scalars2, m, st, 0, false, lg);
            else msm_stages(c, w.scalars2, w.out48, m, st, 0, false, lg);
        };
        quotient_msm();
        if (host_validate) {
            // after the hashing (both want every host thread) and after the GPU has been given everything that needs only the
            // digests: the verdicts are read at the very end, and 0.2 ms of host work per point now runs beside the quotient's MSM
            std::vector<int> vrc(m);
            host_validate_commitments(h_comm, h_canon.data(), vrc.data(), m);
            for (size_t i = 0; i < m; i++)
                if (vrc[i] == 2) LWK_HIP(hipMemcpyAsync(w.status + i, &h_code[i], 4, hipMemcpyHostToDevice, st));
        }
        if (!host_validate) {
            // (a device-to-host copy into pageable memory blocks this thread until the stream has reached it: the
            // canonical bytes are fetched only now that everything else has been submitted)
            LWK_HIP(hipStreamWaitEvent(st, c->ev_join[0], 0));
            LWK_HIP(hipMemcpyAsync(h_canon.data(), w.canon48, m * 48, hipMemcpyDeviceToHost, st));
        }
        LWK_HIP(hipStreamSynchronize(st));
        if (memcmp(h_canon.data(), h_comm, m * 48) != 0) {
            // a non-canonical but valid encoding somewhere in the chunk (or an invalid point, reported through
            // status): redo the chunk with the hash taken over the canonical bytes on the GPU
            if (host_validate) LWK_HIP(hipMemcpyAsync(w.canon48, h_canon.data(), m * 48, hipMemcpyHostToDevice, st));
            launch_challenge(w.blobs, w.canon48, w.z, mr.hash_rule(), m, st);
            coefficients_stage(c, w.blobs, m, mode, w.status, st);  // (the first attempt's forward transform may have used them as scratch)
            quotient_stage(c, mode, w.scalars, w.z, w.scalars2, nullptr, le, m, st);
            quotient_msm();
        }
        std::vector<uint8_t> h_out(m * 48);
        std::vector<G1Xyzz29> h_sums(hf ? m : 0);
        if (hf) LWK_HIP(hipMemcpyAsync(h_sums.data(), d_sums, m * sizeof(G1Xyzz29), hipMemcpyDeviceToHost, c->stream));
        else LWK_HIP(hipMemcpyAsync(h_out.data(), w.out48, m * 48, hipMemcpyDeviceToHost, c->stream));
        rc = collect_status(c, w.status, m, off, first_bad);
        if (rc != C_KZG_OK) return map_rc(rc, mode);
        for (size_t i = 0; i < h_sums.size(); i++) host_finish_compress(h_out.data() + 48 * i, h_sums[i]);
        memcpy(out + off, h_out.data(), m * 48);
    }
    return C_KZG_OK;
}

static C_KZG_RET point_proof_batch_host(Ctx *c, KZGProof *proofs_out, Bytes32 *ys_out, const Blob *blobs, const Bytes32 *zs, size_t n,
                                        int mode, size_t *first_bad) {
    std::lock_guard<std::mutex> lk(c->mu);
    LWK_HIP(hipSetDevice(c->device));
    WsUse wsu(c, c->stream);
    if (n >= kMaxChunk / 2)
        return point_proofs_sliced(c, (uint8_t *)proofs_out, (uint8_t *)ys_out, (const uint8_t *)blobs, (const uint8_t *)zs, n, mode,
                                   first_bad);
    for (size_t off = 0; off < n; off += kMaxChunk) {
        size_t m = n - off < kMaxChunk ? n - off : kMaxChunk;
        C_KZG_RET rc = ctx_reserve(c, m);
        if (rc != C_KZG_OK) return rc;
        Workspace &w = c->ws;
        LWK_HIP(hipMemcpyAsync(w.blobs, blobs + off, m * (size_t)kBlobBytes, hipMemcpyHostToDevice, c->stream));
        LWK_HIP(hipMemcpyAsync(w.zbytes, zs + off, m * 32, hipMemcpyHostToDevice, c->stream));
        const bool hf = m <= host_finish_limit();  // a small call: inversion and compression on this thread
        const G1Xyzz29 *d_sums = nullptr;
        rc = point_proof_batch_device(c, w.out48, w.ybytes, w.blobs, w.zbytes, m, mode, c->stream, w.status, hf ? &d_sums : nullptr);
        if (rc != C_KZG_OK) return rc;
        std::vector<uint8_t> h_out(m * 48), h_y(m * 32);
        std::vector<G1Xyzz29> h_sums(hf ? m : 0);
        if (hf) LWK_HIP(hipMemcpyAsync(h_sums.data(), d_sums, m * sizeof(G1Xyzz29), hipMemcpyDeviceToHost, c->stream));
        else LWK_HIP(hipMemcpyAsync(h_out.data(), w.out48, m * 48, hipMemcpyDeviceToHost, c->stream));
        LWK_HIP(hipMemcpyAsync(h_y.data(), w.ybytes, m * 32, hipMemcpyDeviceToHost, c->stream));
        rc = collect_status(c, w.status, m, off, first_bad);
        if (rc != C_KZG_OK) return map_rc(rc, mode);
        for (size_t i = 0; i < h_sums.size(); i++) host_finish_compress(h_out.data() + 48 * i, h_sums[i]);
        memcpy(proofs_out + off, h_out.data(), m * 48);
        memcpy(ys_out + off, h_y.data(), m * 32);
    }
    return C_KZG_OK;
}

// Concurrent callers of compute_blob_kzg_proof / compute_kzg_proof (one blob per call, as a block builder issues them):
// whoever arrives while no batch is being run becomes the leader of everything queued in its mode (<= 64) and hands it to
// `run`, which answers every member; the others wait for their bytes (front.h: LeaderFront). A `run` that throws (the
// leader's host vectors: std::bad_alloc) answers every member with C_KZG_MALLOC instead of unwinding across the C ABI.
static C_KZG_RET front_run(ProofFront &pf, ProofReq &req, const std::function<void(const std::vector<ProofReq *> &)> &run) {
    return (C_KZG_RET)pf.submit(req, kCombineMaxBatch, (int)C_KZG_MALLOC, run);
}

// The leader copies the blobs and commitments into contiguous host arrays and runs them as ONE host-pointer batch (host
// threads hash, one launch set). If the batch fails (an invalid commitment somewhere in it), every member is redone on
// its own, so each caller gets exactly the return code a lone call would have given.
static C_KZG_RET combine_blob_proof(Ctx *c, KZGProof *out, const Blob *blob, const Bytes48 *commitment, int mode) {
    ProofReq req;
    req.blob = (const uint8_t *)blob;
    req.second = (const uint8_t *)commitment;
    req.out = (uint8_t *)out;
    req.mode = mode;
    return front_run(c->blob_proof_front, req, [c, mode](const std::vector<ProofReq *> &batch) {
        auto alone = [c, mode](ProofReq *r) {
            r->rc = blob_proof_batch_host(c, (KZGProof *)r->out, (const Blob *)r->blob, (const Bytes48 *)r->second, 1, mode, nullptr);
        };
        const size_t m = batch.size();
        if (m == 1) return alone(batch[0]);
        std::vector<uint8_t> hb(m * (size_t)kBlobBytes), hc(m * 48), ho(m * 48);
        for (size_t i = 0; i < m; i++) {
            memcpy(&hb[i * (size_t)kBlobBytes], batch[i]->blob, kBlobBytes);
            memcpy(&hc[48 * i], batch[i]->second, 48);
        }
        C_KZG_RET rc = blob_proof_batch_host(c, (KZGProof *)ho.data(), (const Blob *)hb.data(), (const Bytes48 *)hc.data(), m, mode, nullptr);
        for (size_t i = 0; i < m; i++) {
            if (rc != C_KZG_OK) {  // somebody's input was rejected: everyone gets the verdict of a call of their own
                alone(batch[i]);
                continue;
            }
            memcpy(batch[i]->out, &ho[48 * i], 48);
            batch[i]->rc = C_KZG_OK;
        }
    });
}

// compute_kzg_proof the same way: blobs and evaluation points side by side, proofs and y values back.
static C_KZG_RET combine_point_proof(Ctx *c, KZGProof *proof_out, Bytes32 *y_out, const Blob *blob, const Bytes32 *z, int mode) {
    ProofReq req;
    req.blob = (const uint8_t *)blob;
    req.second = (const uint8_t *)z;
    req.out = (uint8_t *)proof_out;
    req.y_out = (uint8_t *)y_out;
    req.mode = mode;
    return front_run(c->point_proof_front, req, [c, mode](const std::vector<ProofReq *> &batch) {
        auto alone = [c, mode](ProofReq *r) {
            r->rc = point_proof_batch_host(c, (KZGProof *)r->out, (Bytes32 *)r->y_out, (const Blob *)r->blob, (const Bytes32 *)r->second, 1,
                                           mode, nullptr);
        };
        const size_t m = batch.size();
        if (m == 1) return alone(batch[0]);
        std::vector<uint8_t> hb(m * (size_t)kBlobBytes), hz(m * 32), ho(m * 48), hy(m * 32);
        for (size_t i = 0; i < m; i++) {
            memcpy(&hb[i * (size_t)kBlobBytes], batch[i]->blob, kBlobBytes);
            memcpy(&hz[32 * i], batch[i]->second, 32);
        }
        C_KZG_RET rc = point_proof_batch_host(c, (KZGProof *)ho.data(), (Bytes32 *)hy.data(), (const Blob *)hb.data(),
                                              (const Bytes32 *)hz.data(), m, mode, nullptr);
        for (size_t i = 0; i < m; i++) {
            if (rc != C_KZG_OK) {
                alone(batch[i]);
                continue;
            }
            memcpy(batch[i]->out, &ho[48 * i], 48);
            memcpy(batch[i]->y_out, &hy[32 * i], 32);
            batch[i]->rc = C_KZG_OK;
        }
    });
}

static C_KZG_RET blob_proof_batch_impl(KZGProof *out, const Blob *blobs, const Bytes48 *commitments, size_t n, const KZGSettings *s,
                                       size_t *first_bad) {
    const int mode = mode_of(s);
    if (!out || !blobs || !commitments) return map_rc(C_KZG_BADARGS, mode);
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    ensure_lagrange(c, mode);
    if (n == 1) {  // the reference's symbol: merged with the other callers of the moment
        if (coalesce_singles()) {
            C_KZG_RET rc1 = combine_blob_proof(c, out, blobs, commitments, mode);
            if (rc1 != C_KZG_OK) {
                if (first_bad) *first_bad = 0;
                if (!get_error()[0]) set_error("blob 0 rejected");
            }
            return rc1;
        }
    }
    return blob_proof_batch_host(c, out, blobs, commitments, n, mode, first_bad);
}

static C_KZG_RET point_proof_batch_impl(KZGProof *proofs_out, Bytes32 *ys_out, const Blob *blobs, const Bytes32 *zs, size_t n,
                                        const KZGSettings *s, size_t *first_bad) {
    const int mode = mode_of(s);
    if (!proofs_out || !ys_out || !blobs || !zs) return map_rc(C_KZG_BADARGS, mode);
    Ctx *c = ctx_of(s);
    if (!c) return C_KZG_ERROR;
    ensure_lagrange(c, mode);
    if (n == 1 && coalesce_singles()) {  // the reference's symbol: merged with the other callers of the moment
        C_KZG_RET rc1 = combine_point_proof(c, proofs_out, ys_out, blobs, zs, mode);
        if (rc1 != C_KZG_OK) {
            if (first_bad) *first_bad = 0;
            if (!get_error()[0]) set_error("blob 0 rejected");
        }
        return rc1;
    }
    return point_proof_batch_host(c, proofs_out, ys_out, blobs, zs, n, mode, first_bad);
}

}  // namespace lwk

using namespace lwk;

extern "C" {

C_KZG_RET lwkzg_blob_to_kzg_commitment_batch(KZGCommitment *out, const Blob *blobs, size_t n, const KZGSettings *s, size_t *first_bad) {
    return guarded("lwkzg_blob_to_kzg_commitment_batch", [&] { return commitment_batch_impl(out, blobs, n, s, first_bad); });
}
C_KZG_RET lwkzg_compute_blob_kzg_proof_batch(KZGProof *out, const Blob *blobs, const Bytes48 *commitments, size_t n,
                                             const KZGSettings *s, size_t *first_bad) {
    return guarded("lwkzg_compute_blob_kzg_proof_batch", [&] { return blob_proof_batch_impl(out, blobs, commitments, n, s, first_bad); });
}
C_KZG_RET lwkzg_compute_kzg_proof_batch(KZGProof *proofs_out, Bytes32 *ys_out, const Blob *blobs, const Bytes32 *zs, size_t n,
                                        const KZGSettings *s, size_t *first_bad) {
    return guarded("lwkzg_compute_kzg_proof_batch", [&] { return point_proof_batch_impl(proofs_out, ys_out, blobs, zs, n, s, first_bad); });
}

C_KZG_RET blob_to_kzg_commitment(KZGCommitment *out, const Blob *blob, const KZGSettings *s) {
    return lwkzg_blob_to_kzg_commitment_batch(out, blob, 1, s, nullptr);
}

C_KZG_RET compute_kzg_proof(KZGProof *proof_out, Bytes32 *y_out, const Blob *blob, const Bytes32 *z_bytes,
                            const KZGSettings *s) {
    return lwkzg_compute_kzg_proof_batch(proof_out, y_out, blob, z_bytes, 1, s, nullptr);
}

C_KZG_RET compute_blob_kzg_proof(KZGProof *out, const Blob *blob, const Bytes48 *commitment_bytes, const KZGSettings *s) {
    return lwkzg_compute_blob_kzg_proof_batch(out, blob, commitment_bytes, 1, s, nullptr);
}

}  // extern "C"
